"""SparseMatrixConvolver (include/fftconv.h): one FFTConvolver instance per
listed (output, input) pair in lockstep, output o the sum of the instances
listed for it.  Reference: per output the f64 sum of oracle FFTConvolver
instances fed the same call lengths (matrix_sp_ref.SparseSummedOracle;
tests/test_matrix_sp_ref.py holds it within 1e-6 of f64 direct convolution on
these patterns), tolerance common.REL_TOL.  The contract's order of summation is
pinned bitwise: every output against a dense MatrixConvolver holding that
output's pairs alone, and a pattern split by outputs against the whole."""
import functools

import numpy as np
import pytest
import torch

import oracle as oracle_module
from common import REL_TOL, assert_close, max_rel_err
from matrix_paths import parts
from matrix_ref import RAGGED_64, RAGGED_256
from matrix_sp_ref import (BITWISE, PATTERN_1, PATTERN_256, SparseSummedOracle, direct, from_rows, make, rows_of,
                           sp_blocks, sp_len)

pytestmark = pytest.mark.gpu

I1, O1 = 5, 4  # PATTERN_1's matrix


@functools.lru_cache(maxsize=None)
def _case(seed, pairs, I, O, B, L, lengths):
    """(h, x, sparse summed-oracle output, oracle state after every call);
    computed once per case, shared, never written to"""
    h, x = make(seed, pairs, I, L, sum(lengths))
    ref = SparseSummedOracle(oracle_module, pairs, h, I, O, B, L)
    ys, states, pos = [], [], 0
    for n in lengths:
        ys.append(ref.process(x[:, pos:pos + n]))
        states.append(ref.state())
        pos += n
    y = np.concatenate(ys, axis=1)
    for a in (h, x, y):
        a.setflags(write=False)
    return h, x, y, tuple(states)


def _init(amd, pairs, h, I, O, B, L):
    return amd.SparseMatrixConvolver.init(pairs, h, I, O, B, L)


def _run(conv, x, lengths, states=None):
    out, pos = [], 0
    for k, n in enumerate(lengths):
        out.append(conv.process(x[:, pos:pos + n]))
        if states is not None:
            assert conv.state() == states[k], (k, conv.state(), states[k])
        pos += n
    return np.concatenate(out, axis=1)


def _check_outputs(y, ref, pairs, what):
    """within tolerance of the reference; an output without pairs is exactly zero"""
    assert np.isfinite(y).all(), what
    for o, row in enumerate(rows_of(pairs, ref.shape[0])):
        if row:
            print(f"{what} output {o}: max_rel_err {max_rel_err(y[o], ref[o]):.3e}")
            assert np.abs(y[o]).max() > 0, f"{what} output {o}"
            assert_close(y[o], ref[o], what=f"{what} output {o}")
        else:
            assert not y[o].any() and not ref[o].any(), f"{what}: output {o} has no pair"


def test_full_blocks(amd):
    """I 5, O 4, B 64, L 1000 (S 16), o0 <- all, o1 <- {2}, o2 <- {}, o3 <-
    {0, 4}: 40 one-block calls."""
    B, L = 64, 1000
    pairs = tuple(PATTERN_1)
    h, x, ref, states = _case(31, pairs, I1, O1, B, L, (B,) * 40)
    conv = _init(amd, pairs, h, I1, O1, B, L)
    assert (conv.inputs, conv.outputs, conv.pairs, conv.block_size, conv.seg_count) == (I1, O1, 8, B, 16)
    y = _run(conv, x, (B,) * 40, states)
    _check_outputs(y, ref, pairs, "summed oracle")
    assert not y[2].any()
    _check_outputs(y, direct(oracle_module, x, pairs, h, O1), pairs, "direct")


@pytest.mark.parametrize("pairs,I,O,B,L,lengths", [
    (tuple(PATTERN_1), I1, O1, 64, 1000, tuple(RAGGED_64)),
    (tuple(PATTERN_256), 3, 2, 256, 1500, tuple(RAGGED_256))], ids=["B64", "B256"])
def test_ragged_calls(amd, pairs, I, O, B, L, lengths):
    """Calls that start and end anywhere: the input buffer, the kept
    pre_multiplied sum, and calls that span several blocks."""
    h, x, ref, states = _case(32, pairs, I, O, B, L, lengths)
    conv = _init(amd, pairs, h, I, O, B, L)
    y = _run(conv, x, lengths, states)
    _check_outputs(y, ref, pairs, "summed oracle")


@functools.lru_cache(maxsize=None)
def _bitwise_case(name):
    """(shape, pairs, h, x, sparse output) of a bitwise shape, run once with
    the automatic load policy"""
    import fftconv_amd as amd

    s = next(s for s in BITWISE if s.name == name)
    pairs = from_rows(s.cols)
    L, n = sp_len(s), sp_blocks(s) * s.B
    h, x = make(33, pairs, s.I, L, n)
    conv = _init(amd, pairs, h, s.I, len(s.cols), s.B, L)
    assert (conv.block_size, conv.seg_count, conv.pairs) == (s.B, s.S, len(pairs))
    for o, cols in enumerate(s.cols):
        assert conv.output_parts(o) == parts(len(cols), s.S), (name, o)
    y = conv.process(x)
    assert conv.state() == (-sp_blocks(s) % s.S, s.S, 0)
    for a in (h, x, y):
        a.setflags(write=False)
    return s, pairs, h, x, y


@pytest.mark.parametrize("name", [s.name for s in BITWISE])
def test_bitwise_against_dense(amd, name):
    """Property 1: S + 3 full blocks, L = S * B - 3; output o equals, bit for
    bit, the single output of a dense MatrixConvolver with k_o inputs that
    holds h[pair e] and is fed x[i_e] in list order.  One dropped, doubled or
    misplaced row, a part left out, or a row taken from another input's delay
    line moves bits."""
    s, pairs, h, x, y = _bitwise_case(name)
    L = sp_len(s)
    assert np.isfinite(y).all()
    for o, row in enumerate(rows_of(pairs, len(s.cols))):
        ns, cols = [n for n, _ in row], [i for _, i in row]
        dense = amd.MatrixConvolver.init(h[ns][None], s.B, L)
        assert dense.mac_parts == parts(len(cols), s.S)  # (the sparse handle's P_o: asserted in _bitwise_case)
        yd = dense.process(x[cols])
        assert np.abs(yd).max() > 0
        assert np.array_equal(y[o], yd[0]), f"{name} output {o} (k = {len(cols)}) differs from its dense matrix"
    _check_outputs(y, direct(oracle_module, x, pairs, h, len(s.cols)), pairs, f"{name} direct")


def _update_sequence(pairs, I, B, L):
    """tests/test_gpu_matrix.py's _update_sequence over the listed pairs:
    update at a block boundary (700 samples: P_0 2 -> 1), mid-block, a shrink
    to 130 samples while current >= 3, a zero-length response; then two
    updates back to back and 10 blocks"""
    rng = np.random.default_rng(37)
    N = len(pairs)
    h0, x = make(37, pairs, I, L, 60 * B)
    mk = lambda n: (rng.uniform(-1, 1, (N, n)) / np.sqrt(max(n, 1))).astype(np.float32)
    return h0, x, [("run", (B,) * 5), ("update", mk(700)), ("run", (B,) * 3 + (20,)), ("update", mk(L)),
                   ("run", (44,) + (B,) * 4), ("need_current", 3), ("update", mk(130)),
                   ("run", (B, 10, 54, B, 2 * B, B)), ("update", mk(0)), ("run", (B, 30)),
                   ("need_active", 0), ("update", mk(400)), ("update", mk(L)), ("run", (B,) * 10)]


def test_update(amd):
    B, L = 64, 1000
    pairs = PATTERN_1
    h0, x, seq = _update_sequence(pairs, I1, B, L)
    ref = SparseSummedOracle(oracle_module, pairs, h0, I1, O1, B, L)
    conv = _init(amd, pairs, h0, I1, O1, B, L)
    dev = _init(amd, pairs, h0, I1, O1, B, L)
    ks = [len(r) for r in rows_of(pairs, O1)]
    pos = 0
    for kind, arg in seq:
        if kind == "update":
            ref.update(arg)
            conv.update(arg)
            d = torch.from_numpy(arg).to("cuda:0")
            dev.update_device(d.data_ptr(), arg.shape[1], arg.shape[1], 0)
            dev.synchronize()
            assert conv.state() == dev.state() == ref.state()
            for o, k in enumerate(ks):
                assert conv.output_parts(o) == dev.output_parts(o) == parts(k, ref.state()[1]), o
        elif kind == "need_current":
            assert ref.state()[0] >= arg, ref.state()
        elif kind == "need_active":
            assert ref.state()[1] == arg, ref.state()
        else:
            for n in arg:
                blk = x[:, pos:pos + n]
                r = ref.process(blk)
                y = conv.process(blk)
                yd = dev.process(blk)
                assert conv.state() == ref.state()
                assert np.array_equal(y, yd), "update_device differs from update"
                if ref.state()[1] == 0:
                    assert not y.any() and not r.any()
                else:
                    _check_outputs(y, r, pairs, f"after update, samples {pos}..{pos + n}")
                pos += n
    assert ref.state()[1] == 16


def test_reset_and_clone(amd):
    B, L = 64, 1000
    pairs = tuple(PATTERN_1)
    lengths = tuple(RAGGED_64[:11])
    h, x, ref, states = _case(32, pairs, I1, O1, B, L, tuple(RAGGED_64))
    n = sum(lengths)
    conv = _init(amd, pairs, h, I1, O1, B, L)
    _run(conv, x[:, 500:], (64, 64, 17))
    conv.reset()
    assert conv.state() == (0, 16, 0)
    fresh = _init(amd, pairs, h, I1, O1, B, L)
    y = _run(conv, x[:, :n], lengths)
    assert np.array_equal(y, _run(fresh, x[:, :n], lengths))
    _check_outputs(y, ref[:, :n], pairs, "after reset")
    # (the 11 calls end mid-block: fill != 0)
    assert conv.state()[2] != 0
    twin = conv.clone()
    assert twin.state() == conv.state()
    assert (twin.inputs, twin.outputs, twin.pairs) == (I1, O1, len(pairs))
    assert [twin.output_parts(o) for o in range(O1)] == [conv.output_parts(o) for o in range(O1)]
    rest = tuple(RAGGED_64[11:])
    ya = _run(conv, x[:, n:], rest)
    yb = _run(twin, x[:, n:], rest)
    assert np.array_equal(ya, yb)
    _check_outputs(ya, ref[:, n:], pairs, "after clone")


@pytest.mark.parametrize("n,K", [(64, 30), (40, 30)])
def test_process_device_steps(amd, n, K):
    """30 steps of a block and 30 steps of 40 samples at B = 64, on a torch
    side stream with padded rows: bit-identical to the separate calls."""
    B, L = 64, 1000
    pairs = PATTERN_1
    h, x = make(38, pairs, I1, L, K * n)
    dev = torch.device("cuda:0")
    pad_in, pad_out = n + 5, n + 3
    xs = np.zeros((K, I1, pad_in), np.float32)
    xs[:, :, :n] = x.reshape(I1, K, n).transpose(1, 0, 2)
    xd = torch.from_numpy(xs).to(dev)
    s = torch.cuda.Stream(dev)
    a = _init(amd, pairs, h, I1, O1, B, L)
    b = _init(amd, pairs, h, I1, O1, B, L)
    ya = torch.full((K, O1, pad_out), -7.0, device=dev)
    yb = torch.full((K, O1, pad_out), -7.0, device=dev)
    s.wait_stream(torch.cuda.current_stream())
    a.process_device_steps(xd.data_ptr(), pad_in, I1 * pad_in, ya.data_ptr(), pad_out, O1 * pad_out, n, K,
                           s.cuda_stream)
    for k in range(K):
        b.process_device(xd[k].data_ptr(), pad_in, yb[k].data_ptr(), pad_out, n, s.cuda_stream)
    s.synchronize()
    assert a.state() == b.state()
    ya_h, yb_h = ya.cpu().numpy(), yb.cpu().numpy()
    assert np.array_equal(ya_h, yb_h)
    assert (ya_h[:, :, n:] == -7.0).all()  # (the padding is untouched)
    y = ya_h[:, :, :n].transpose(1, 0, 2).reshape(O1, K * n)
    ref = SparseSummedOracle(oracle_module, pairs, h, I1, O1, B, L).run(x, (n,) * K)
    _check_outputs(y, ref, pairs, "device steps")


def test_output_sharding_bitwise(amd):
    """Property 2: outputs {0, 1} and {2, 3} of PATTERN_1 on two handles
    against one handle."""
    B, L = 64, 1000
    pairs = PATTERN_1
    h, x = make(39, pairs, I1, L, 40 * B)
    whole = _init(amd, pairs, h, I1, O1, B, L)
    sel_lo = [n for n, (o, _) in enumerate(pairs) if o < 2]
    sel_hi = [n for n, (o, _) in enumerate(pairs) if o >= 2]
    lo = _init(amd, [pairs[n] for n in sel_lo], h[sel_lo], I1, 2, B, L)
    hi = _init(amd, [(pairs[n][0] - 2, pairs[n][1]) for n in sel_hi], h[sel_hi], I1, 2, B, L)
    assert [whole.output_parts(o) for o in range(4)] == [lo.output_parts(0), lo.output_parts(1), hi.output_parts(0),
                                                         hi.output_parts(1)]
    yw = _run(whole, x, (B,) * 40)
    ys = np.concatenate([_run(lo, x, (B,) * 40), _run(hi, x, (B,) * 40)], axis=0)
    assert np.isfinite(yw).all() and np.abs(yw[[0, 1, 3]]).max() > 0 and not yw[2].any()
    assert np.array_equal(yw, ys)


@pytest.mark.parametrize("name", ["groups", "spt2"])
def test_load_policy(amd, name):
    """Bit 1 of fftconv_set_kernel_variant selects matrix_sp_a_kernel<...,
    true> (nontemporal H loads; automatic only above 256 MiB of H) or the
    plain instantiation, at a shape with row groups (G = 4) and one with
    SPT = 2: the same bits as each other and as the automatic policy."""
    s, pairs, h, x, y_auto = _bitwise_case(name)
    ys = []
    for v in (2, 0):
        amd.set_kernel_variant(v)
        try:
            conv = _init(amd, pairs, h, s.I, len(s.cols), s.B, sp_len(s))
            ys.append(conv.process(x))
        finally:
            amd.set_kernel_variant(-1)
    assert amd.get_kernel_variant() == -1
    for y in ys:
        assert np.abs(y).max() > 0
    assert np.array_equal(ys[0], ys[1])
    assert np.array_equal(ys[0], y_auto)


def test_wide_diagonal(amd):
    """I = O = 2048, pairs (o, o), B 32, L 64, 6 blocks: 2048 pairs where the
    dense form holds 4.2 M.  Per channel against numpy's f64 direct
    convolution."""
    C, B, L, nb = 2048, 32, 64, 6
    rng = np.random.default_rng(40)
    h = (rng.uniform(-1, 1, (C, L)) / np.sqrt(L)).astype(np.float32)
    x = rng.uniform(-1, 1, (C, nb * B)).astype(np.float32)
    conv = _init(amd, [(o, o) for o in range(C)], h, C, C, B, L)
    assert (conv.pairs, conv.inputs, conv.outputs, conv.seg_count) == (C, C, C, 2)
    assert conv.output_parts(0) == conv.output_parts(C - 1) == 1
    y = np.concatenate([conv.process(x[:, k * B:(k + 1) * B]) for k in range(nb)], axis=1)
    assert conv.state() == (0, 2, 0)
    ref = np.stack([np.convolve(x[c].astype(np.float64), h[c].astype(np.float64))[:nb * B] for c in range(C)])
    assert np.isfinite(y).all()
    err = np.abs(y - ref).max(axis=1) / np.abs(ref).max(axis=1)
    print(f"wide diagonal: worst channel {err.argmax()} max_rel_err {err.max():.3e}")
    assert (err <= REL_TOL).all(), (int(err.argmax()), float(err.max()))


def test_errors(amd):
    B, L = 64, 100
    pairs = [(0, 0), (0, 1), (1, 1)]
    h, x = make(41, pairs, 2, L, 64)
    init = amd.SparseMatrixConvolver.init
    for bad in ([(0, 1), (0, 0), (1, 1)],      # unsorted within an output
                [(1, 1), (0, 0), (0, 1)],      # unsorted outputs
                [(0, 0), (0, 0), (1, 1)],      # a duplicate pair
                [(0, 0), (0, 2), (1, 1)],      # pair_in >= inputs
                [(0, 0), (0, 1), (2, 1)]):     # pair_out >= outputs
        with pytest.raises(amd.ConvolutionPanic):
            init(bad, h, 2, 2, B, L)
    with pytest.raises(amd.ConvolutionPanic):
        init([], np.zeros((0, L), np.float32), 2, 2, B, L)           # pairs == 0
    with pytest.raises(amd.ConvolutionPanic):
        init(pairs, h, 2, 2, B, L - 1)                               # response_len > max_response_length
    with pytest.raises(amd.ConvolutionPanic):
        init(pairs, h, 0, 2, B, L)                                   # inputs == 0 (every pair out of range)
    for bad in (16, 16384):
        with pytest.raises(amd.DeviceError, match="block size"):
            init(pairs, h, 2, 2, bad, L)
    conv = init(pairs, h, 2, 2, B, L)
    with pytest.raises(amd.ConvolutionPanic):
        conv.process(x[:, :10], out_len=11)                          # input_len < output_len
    with pytest.raises(amd.ConvolutionPanic):
        conv.update(np.zeros((3, L + 1), np.float32))                # response_len > max_response_length
    assert conv.state() == (0, 2, 0)
    y = conv.process(x, out_len=32)                                  # (the handle keeps working)
    assert y.shape == (2, 32) and np.abs(y).max() > 0
    assert_close(y, direct(oracle_module, x[:, :32], pairs, h, 2), what="after a failed update")
