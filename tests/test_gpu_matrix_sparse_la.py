"""SparseMatrixLookaheadConvolver (include/fftconv.h): the SparseMatrixConvolver's
definition with the MatrixLookaheadConvolver's far-row windows.  Reference:
matrix_sp_ref.SparseSummedOracle fed the same call lengths and f64 direct
convolution, tolerance common.REL_TOL.  The scheme's own contract is bitwise:
(1) a run served from windows equals the same run with set_windows(0), whatever
the anchor phase, the grouping of calls or the load policy; (2) output o equals
the single output of a dense MatrixLookaheadConvolver with k_o inputs; (3) a
pattern split by outputs over two handles computes the same bits.
tests/test_matrix_sp_la_ref.py proves on the CPU what each shape is there for."""
import functools

import numpy as np
import pytest
import torch

import oracle as oracle_module
from common import REL_TOL, assert_close
from matrix_la_ref import Q
from matrix_ref import RAGGED_64
from matrix_sp_la_ref import (MAIN, NEAR_SPLIT, SHAPE_32, SHAPE_256, SHAPE_512, SHAPES, anchors, far_parts,
                              near_parts, shape_len, shape_pairs)
from matrix_sp_ref import SparseSummedOracle, direct, from_rows, make

pytestmark = pytest.mark.gpu

FULL_100 = (64,) * 100


def _case(seed, shape, lengths, L=None):
    """(pairs, h, x, summed-oracle output, oracle state after every call);
    computed once per case, shared, never written to"""
    return _case_of(seed, shape.name, lengths, L)


@functools.lru_cache(maxsize=None)
def _case_of(seed, name, lengths, L):
    shape = next(s for s in SHAPES if s.name == name)
    pairs = shape_pairs(shape)
    L = shape_len(shape) if L is None else L
    h, x = make(seed, pairs, shape.I, L, sum(lengths))
    ref = SparseSummedOracle(oracle_module, pairs, h, shape.I, len(shape.cols), shape.B, L)
    ys, states, pos = [], [], 0
    for n in lengths:
        ys.append(ref.process(x[:, pos:pos + n]))
        states.append(ref.state())
        pos += n
    y = np.concatenate(ys, axis=1)
    for a in (h, x, y):
        a.setflags(write=False)
    return pairs, h, x, y, tuple(states)


def _run(conv, x, lengths, states=None, anchors=None):
    out, pos = [], 0
    for k, n in enumerate(lengths):
        if anchors is not None:
            anchors.append(conv.anchors())
        out.append(conv.process(x[:, pos:pos + n]))
        if states is not None:
            assert conv.state() == states[k], (k, conv.state(), states[k])
        pos += n
    return np.concatenate(out, axis=1)


def _check_outputs(y, ref, cols, what):
    assert np.isfinite(y).all(), what
    for o, c in enumerate(cols):
        if c:
            assert np.abs(y[o]).max() > 0, (what, o)
            assert_close(y[o], ref[o], what=f"{what} output {o}")
        else:
            assert not y[o].any() and not ref[o].any(), (what, o)


def _init(amd, shape, h, windows=True, L=None, pairs=None, outputs=None):
    conv = amd.SparseMatrixLookaheadConvolver.init(shape_pairs(shape) if pairs is None else pairs, h, shape.I,
                                                   len(shape.cols) if outputs is None else outputs, shape.B,
                                                   shape_len(shape) if L is None else L)
    conv.set_windows(windows)
    return conv


def test_main_shape_full_blocks(amd):
    """I 7, O 10, B 64, L 2560 (S 40), 100 one-block calls: pair counts 6, 1, 0,
    2, 3, 4, ... with one to three far parts, two outputs in anchor classes 0 and
    1, the delay line wraps twice."""
    s = MAIN
    pairs, h, x, ref, states = _case(71, s, FULL_100)
    ks = [len(c) for c in s.cols]
    conv = _init(amd, s, h)
    assert amd.SparseMatrixLookaheadConvolver.period() == Q
    assert (conv.inputs, conv.outputs, conv.pairs, conv.block_size, conv.seg_count) == (7, 10, len(pairs), 64, 40)
    assert [conv.near_parts(o) for o in range(10)] == [near_parts(k, 40) for k in ks]
    assert [conv.far_parts(o) for o in range(10)] == [far_parts(k, 40) for k in ks]
    assert [conv.far_parts(o) for o in range(6)] == [3, 1, 0, 1, 2, 2]
    assert conv.near_parts(10) == conv.far_parts(10) == 0
    seen = []
    y = _run(conv, x, FULL_100, states, seen)
    assert seen == [anchors(t, ks, 40, 0) for t in range(100)]
    assert seen[:Q] == [2, 2, 0, 1, 1, 1, 1, 1]  # (class 2 holds the output without pairs only)
    _check_outputs(y, ref, s.cols, "summed oracle")
    _check_outputs(y, direct(oracle_module, x, pairs, h, 10), s.cols, "direct")


def test_main_shape_ragged_calls(amd):
    """Calls that start and end anywhere: a window row is consumed by the chunk
    that starts a block, the kept pre_multiplied sum serves the rest."""
    s = MAIN
    lengths = tuple(RAGGED_64)
    pairs, h, x, ref, states = _case(72, s, lengths)
    seen = []
    y = _run(_init(amd, s, h), x, lengths, states, seen)
    assert max(seen) > 0
    _check_outputs(y, ref, s.cols, "ragged, summed oracle")
    full = _init(amd, s, h, windows=False)
    assert np.array_equal(y, _run(full, x, lengths, states)), "windows differ from full sums"


@pytest.mark.parametrize("shape,blocks", [(SHAPE_32, 30), (SHAPE_256, 45), (SHAPE_512, 12)],
                         ids=["B32", "B256", "B512"])
def test_block_sizes(amd, shape, blocks):
    """B 32 (sixteen row groups), B 256 (two), B 512 (one group, the largest
    block): full blocks, then two calls that split a block; windows against full
    sums bitwise."""
    B = shape.B
    lengths = (B,) * blocks + (B - 24, 24)
    pairs, h, x, ref, states = _case(73, shape, lengths)
    conv = _init(amd, shape, h)
    assert [conv.far_parts(o) for o in range(3)] == [far_parts(len(c), shape.S) for c in shape.cols]
    seen = []
    y = _run(conv, x, lengths, states, seen)
    assert max(seen) > 0
    _check_outputs(y, ref, shape.cols, f"B={B}")
    full = _init(amd, shape, h, windows=False)
    off = []
    assert np.array_equal(y, _run(full, x, lengths, anchors=off)), "windows differ from full sums"
    assert not any(off)


@pytest.mark.parametrize("shape,blocks", [(MAIN, 60), (NEAR_SPLIT, 30)], ids=["main", "near-split"])
def test_outputs_equal_the_dense_lookahead_matrix_bitwise(amd, shape, blocks):
    """Property 2: output o against a dense MatrixLookaheadConvolver with k_o
    inputs and ONE output (which anchors on t = 0 (mod Q), not on o) that holds
    h[pair e] and is fed x[i_e]; the output without pairs is all zeros."""
    B, L = shape.B, shape_len(shape)
    lengths = (B,) * blocks + (B - 17, 17, B)
    pairs, h, x, _, _ = _case(74, shape, lengths)
    y = _run(_init(amd, shape, h), x, lengths)
    n = 0
    for o, cols in enumerate(shape.cols):
        if not cols:
            assert not y[o].any()
            continue
        dense = amd.MatrixLookaheadConvolver.init(h[n:n + len(cols)][None], B, L)
        assert dense.near_parts == near_parts(len(cols), shape.S) and dense.far_parts == far_parts(len(cols), shape.S)
        yd = _run(dense, x[cols], lengths)
        assert np.abs(yd).max() > 0
        assert np.array_equal(y[o], yd[0]), f"output {o} ({len(cols)} pairs) differs from the dense lookahead matrix"
        n += len(cols)
    assert n == len(pairs)


def test_update_sequence_windows_equal_full_sums(amd):
    """An update at a block boundary, one mid-block, a shrink to 12 segments
    while current >= 20 (current >= active: no anchors until it is back
    inside), a zero-length response, a full-length one, then a reset.  Three
    handles: windows, windows through update_device, full sums -- bitwise equal
    after every call, within tolerance of the summed oracle."""
    s = MAIN
    B, L, O = s.B, shape_len(s), len(s.cols)
    pairs = shape_pairs(s)
    N = len(pairs)
    rng = np.random.default_rng(75)
    h0, x = make(75, pairs, s.I, L, 112 * B)
    mk = lambda n: (rng.uniform(-1, 1, (N, n)) / np.sqrt(max(n, 1))).astype(np.float32)
    ref = SparseSummedOracle(oracle_module, pairs, h0, s.I, O, B, L)
    win, dev, full = (_init(amd, s, h0, w) for w in (True, True, False))
    pos = 0
    seen = {"anchors": 0, "outside": 0}

    def run(calls, what):
        nonlocal pos
        for n in calls:
            blk = x[:, pos:pos + n]
            cur, act, fill = ref.state()
            if act and cur >= act and fill == 0:
                seen["outside"] += 1
                assert win.anchors() == 0
            seen["anchors"] += win.anchors()
            assert full.anchors() == 0
            r = ref.process(blk)
            y, yf, yd = win.process(blk), full.process(blk), dev.process(blk)
            assert win.state() == dev.state() == full.state() == ref.state()
            assert np.array_equal(y, yf), f"{what}: windows differ from full sums at {pos}"
            assert np.array_equal(y, yd), f"{what}: update_device differs at {pos}"
            if ref.state()[1] == 0:
                assert not y.any() and not r.any()
            else:
                _check_outputs(y, r, s.cols, f"{what}, samples {pos}..{pos + n}")
            pos += n

    def update(hn):
        ref.update(hn)
        win.update(hn)
        full.update(hn)
        d = torch.from_numpy(hn).to("cuda:0")
        dev.update_device(d.data_ptr(), hn.shape[1], hn.shape[1], 0)
        dev.synchronize()
        assert win.state() == dev.state() == full.state() == ref.state()

    run((B,) * 12, "init")
    update(mk(L - 100))                      # at a block boundary, mid-window for every output
    run((B,) * 9 + (20,), "boundary update")
    update(mk(L))                            # mid-block
    run((44,) + (B,) * 22, "mid-block update")  # (the delay line wraps: current 18 -> 36)
    assert ref.state()[0] >= 20
    update(mk(12 * B - 10))                  # shrink: current >= active = 12 > Q
    assert [win.far_parts(o) for o in range(O)] == [far_parts(len(c), 12) for c in s.cols]
    run((B, 10, 54, B, 2 * B) + (B,) * 25, "shrink")
    assert seen["outside"] >= 3 and ref.state()[0] < 12
    before = seen["anchors"]
    run((B,) * 10, "shrunk, inside")
    assert seen["anchors"] > before
    update(mk(0))
    run((B, 30), "no response")
    update(mk(L))
    run((34,) + (B,) * 12, "full length again")
    run((20,), "into a block")                # the reset drops a block in progress
    for c in (win, dev, full):
        c.reset()
    ref.reset()
    assert win.state() == ref.state()
    run((B,) * 11, "after reset")
    assert pos <= x.shape[1]


def test_update_pairs_equals_update(amd):
    """update_pairs against update(R') on a twin, bit for bit, at a block
    boundary and mid-window / mid-block; the windows of every output are dropped
    (a stale window of a touched output would show here).  A pair that is not
    listed raises and leaves the handle unchanged."""
    s = MAIN
    B, L, O = s.B, shape_len(s), len(s.cols)
    pairs = shape_pairs(s)
    h, x = make(76, pairs, s.I, L, 70 * B)
    a, b, full = _init(amd, s, h), _init(amd, s, h), _init(amd, s, h, windows=False)
    pos = 0

    def both(calls):
        nonlocal pos
        for n in calls:
            blk = x[:, pos:pos + n]
            ya, yb, yf = a.process(blk), b.process(blk), full.process(blk)
            pos += n
            assert a.state() == b.state() == full.state()
            assert np.array_equal(ya, yb) and np.array_equal(ya, yf), pos
            assert np.abs(ya[0]).max() > 0 and not ya[2].any()

    both((B,) * 19)                          # block 19 next: every output is inside a window
    lst = [(0, 3), (4, 2), (8, 4)]
    rows = make(176, lst, 1, L - 5, 1)[0]
    R = h.copy()
    for p, row in zip(lst, rows):
        R[pairs.index(p)] = 0
        R[pairs.index(p), :L - 5] = row
    a.update_pairs(lst, rows)
    b.update(R)
    full.update(R)
    both((B,) * 11 + (30,))                  # mid-block next
    lst = [(3, 0), (9, 4)]
    rows = make(177, lst, 1, L, 1)[0]
    R = R.copy()
    for p, row in zip(lst, rows):
        R[pairs.index(p)] = row
    d = torch.from_numpy(rows).to("cuda:0")
    a.update_pairs_device(lst, d.data_ptr(), L, L, 0)
    a.synchronize()
    b.update(R)
    full.update(R)
    both((34,) + (B,) * 12)
    for bad in ([(2, 0)], [(1, 0)], [(0, 6)], [(0, 1), (3, 1)]):
        with pytest.raises(amd.ConvolutionPanic, match="is not in the pattern"):
            a.update_pairs(bad, rows[:len(bad)])
    with pytest.raises(amd.ConvolutionPanic):
        a.update_pairs([(3, 4), (3, 0)], rows)   # not ascending
    assert a.state() == b.state()
    both((B,) * 10)                          # the handle is unchanged: windows and overlap kept


def test_switching_windows_mid_run(amd):
    s = MAIN
    B = s.B
    pairs, h, x, ref, states = _case(71, s, FULL_100)
    full = _init(amd, s, h, windows=False)
    off = []
    yf = _run(full, x, FULL_100, states, off)
    assert not any(off)
    yw = _run(_init(amd, s, h), x, FULL_100)
    assert np.abs(yw).max() > 0
    assert np.array_equal(yw, yf)
    # off after 21 blocks, on again after 40
    sw = _init(amd, s, h)
    ys = [_run(sw, x[:, :21 * B], (B,) * 21)]
    sw.set_windows(False)
    assert sw.anchors() == 0
    ys.append(_run(sw, x[:, 21 * B:40 * B], (B,) * 19))
    sw.set_windows(True)
    assert sw.anchors() > 0
    ys.append(_run(sw, x[:, 40 * B:], (B,) * 60))
    assert np.array_equal(np.concatenate(ys, axis=1), yf)


def test_output_sharding_bitwise(amd):
    """Outputs 0..4 and 5..9 on two handles against one handle: output 5 anchors
    on t = 5 (mod Q) in the whole matrix and on t = 0 in the shard."""
    s = MAIN
    B, L = s.B, shape_len(s)
    pairs, h, x, ref, _ = _case(71, s, FULL_100)
    n_lo = sum(len(c) for c in s.cols[:5])
    whole = _init(amd, s, h)
    lo = _init(amd, s, h[:n_lo], pairs=from_rows(s.cols[:5]), outputs=5)
    hi = _init(amd, s, h[n_lo:], pairs=from_rows(s.cols[5:]), outputs=5)
    assert [whole.far_parts(o) for o in range(10)] == [lo.far_parts(o) for o in range(5)] + \
        [hi.far_parts(o) for o in range(5)]
    lengths = (B,) * 30 + (17, 47) + (B,) * 10
    n = sum(lengths)
    yw = _run(whole, x[:, :n], lengths)
    ys = np.concatenate([_run(lo, x[:, :n], lengths), _run(hi, x[:, :n], lengths)], axis=0)
    _check_outputs(yw, ref[:, :n], s.cols, "whole")
    assert np.array_equal(yw, ys)


@pytest.mark.parametrize("n,K", [(64, 30), (40, 30)])
def test_process_device_steps(amd, n, K):
    """30 steps of a block and of 40 samples on a torch side stream with padded
    rows, against separate process_device calls and host process: the same bits."""
    s = MAIN
    I, O = s.I, len(s.cols)
    pairs, h, x, _, _ = _case(71, s, FULL_100)
    x = x[:, :K * n]
    dev = torch.device("cuda:0")
    pad_in, pad_out = n + 5, n + 3
    xs = np.zeros((K, I, pad_in), np.float32)
    xs[:, :, :n] = x.reshape(I, K, n).transpose(1, 0, 2)
    xd = torch.from_numpy(xs).to(dev)
    st = torch.cuda.Stream(dev)
    a, b = _init(amd, s, h), _init(amd, s, h)
    ya = torch.full((K, O, pad_out), -7.0, device=dev)
    yb = torch.full((K, O, pad_out), -7.0, device=dev)
    st.wait_stream(torch.cuda.current_stream())
    a.process_device_steps(xd.data_ptr(), pad_in, I * pad_in, ya.data_ptr(), pad_out, O * pad_out, n, K,
                           st.cuda_stream)
    for k in range(K):
        b.process_device(xd[k].data_ptr(), pad_in, yb[k].data_ptr(), pad_out, n, st.cuda_stream)
    st.synchronize()
    assert a.state() == b.state()
    ya_h, yb_h = ya.cpu().numpy(), yb.cpu().numpy()
    assert np.array_equal(ya_h, yb_h)
    assert (ya_h[:, :, n:] == -7.0).all()  # (the padding is untouched)
    y = ya_h[:, :, :n].transpose(1, 0, 2).reshape(O, K * n)
    assert np.array_equal(y, _run(_init(amd, s, h), x, (n,) * K))
    _check_outputs(y, direct(oracle_module, x, pairs, h, O), s.cols, "device steps")


def test_clone_mid_window_and_reset(amd):
    """A clone taken after 21 blocks and 17 samples: every output is inside a
    window, a block is in progress.  It carries the windows, the plan and the
    block count.  reset: the same bits as a fresh handle."""
    s = MAIN
    B = s.B
    pairs, h, x, ref, _ = _case(71, s, FULL_100)
    first = (B,) * 21 + (17,)
    n = sum(first)
    conv = _init(amd, s, h)
    _run(conv, x[:, :n], first)
    twin = conv.clone()
    assert twin.state() == conv.state() and twin.anchors() == conv.anchors()
    assert [twin.far_parts(o) for o in range(10)] == [conv.far_parts(o) for o in range(10)]
    rest = (47,) + (B,) * 30
    m = sum(rest)
    seen = []
    ya = _run(conv, x[:, n:n + m], rest)
    yb = _run(twin, x[:, n:n + m], rest, anchors=seen)
    assert max(seen) > 0
    assert np.array_equal(ya, yb)
    _check_outputs(ya, ref[:, n:n + m], s.cols, "after clone")
    conv.reset()
    assert conv.state() == (0, 40, 0)
    fresh = _init(amd, s, h)
    assert np.array_equal(_run(conv, x[:, :20 * B], (B,) * 20), _run(fresh, x[:, :20 * B], (B,) * 20))


@pytest.mark.parametrize("shape", [MAIN, SHAPE_256], ids=["B64", "B256"])
def test_nontemporal_instantiation(amd, shape):
    """matrix_sp_la_a_kernel<..., true> through the kernel-variant knob: bitwise
    equal to the plain-load instantiation."""
    B = shape.B
    pairs = shape_pairs(shape)
    h, x = make(77, pairs, shape.I, shape_len(shape), 30 * B)
    ys = []
    for v in (2, 0):
        amd.set_kernel_variant(v)
        try:
            ys.append(_run(_init(amd, shape, h), x, (B,) * 30))
        finally:
            amd.set_kernel_variant(-1)
    assert np.abs(ys[0]).max() > 0
    assert np.array_equal(ys[0], ys[1])
    _check_outputs(ys[0], direct(oracle_module, x, pairs, h, len(shape.cols)), shape.cols, "nontemporal")


@pytest.mark.parametrize("segs", [1, 5, 8, 9])
def test_few_segments(amd, segs):
    """active <= Q runs near rows only (far_parts == 0, nothing anchors); 9
    segments have one far row per pair."""
    s = MAIN
    B, O = s.B, len(s.cols)
    L = segs * B
    lengths = (B,) * 20 + (30, 34)
    pairs, h, x, ref, states = _case(78, s, lengths, L)
    conv = _init(amd, s, h, L=L)
    assert [conv.far_parts(o) for o in range(O)] == [1 if segs > Q and c else 0 for c in s.cols]
    seen = []
    y = _run(conv, x, lengths, states, seen)
    assert (max(seen) > 0) == (segs > Q)
    _check_outputs(y, ref, s.cols, f"{segs} segments")
    full = _init(amd, s, h, windows=False, L=L)
    assert np.array_equal(y, _run(full, x, lengths))


def test_non_finite_sample_leaves(amd):
    """A NaN in input 1 at block 5 (B 64, L 1280, S 20): from sample nan_idx +
    (S + 2) * B on, outputs are finite and within tolerance of f64 direct
    convolution with that sample set to 0 -- no window keeps it longer than the
    delay line does."""
    I, O, B, L, S = 3, 3, 64, 1280, 20
    pairs = from_rows([[0, 1], [1, 2], [2]])
    h, x = make(79, pairs, I, L, 60 * B)
    nan_idx = 5 * B + 10
    xn = x.copy()
    xn[1, nan_idx] = np.nan
    conv = amd.SparseMatrixLookaheadConvolver.init(pairs, h, I, O, B, L)
    y = _run(conv, xn, (B,) * 60)
    x0 = x.copy()
    x0[1, nan_idx] = 0.0
    ref = direct(oracle_module, x0, pairs, h, O)
    first = nan_idx + (S + 2) * B
    assert not np.isfinite(y[:2, nan_idx:first]).all()
    assert np.isfinite(y[2]).all()  # (output 2 does not read input 1)
    assert np.isfinite(y[:, first:]).all()
    assert np.abs(y[:, first:] - ref[:, first:]).max() <= REL_TOL * np.abs(ref).max()
    assert conv.state() == (0, S, 0)


def test_against_the_sparse_matrix(amd):
    """The same pattern on a SparseMatrixConvolver: equal within REL_TOL (another
    order of summation, so not bitwise)."""
    s = MAIN
    lengths = tuple(RAGGED_64)
    pairs, h, x, ref, _ = _case(72, s, lengths)
    y = _run(_init(amd, s, h), x, lengths)
    sp = amd.SparseMatrixConvolver.init(pairs, h, s.I, len(s.cols), s.B, shape_len(s))
    _check_outputs(y, _run(sp, x, lengths), s.cols, "SparseMatrixConvolver")


def test_errors(amd):
    cls = amd.SparseMatrixLookaheadConvolver
    pairs = [(0, 0), (0, 1), (1, 1)]
    h, x = make(80, pairs, 2, 100, 64)
    for bad in (16, 1024, 8192):
        with pytest.raises(amd.DeviceError, match="block size"):
            cls.init(pairs, h, 2, 2, bad, 100)
    with pytest.raises(amd.DeviceError, match="SparseMatrixConvolver"):
        cls.init(pairs, h, 2, 2, 1024, 100)
    for bad in ([(0, 1), (0, 0), (1, 1)], [(0, 0), (0, 0), (1, 1)], [(0, 0), (0, 2), (1, 1)], [(0, 0), (0, 1), (2, 1)]):
        with pytest.raises(amd.ConvolutionPanic):
            cls.init(bad, h, 2, 2, 64, 100)                        # unsorted, repeated, out of range
    with pytest.raises(amd.ConvolutionPanic):
        cls.init([], np.zeros((0, 100), np.float32), 2, 2, 64, 100)   # zero pairs
    with pytest.raises(amd.ConvolutionPanic):
        cls.init(pairs, h, 2, 2, 64, 99)                            # response_len > max_response_length
    conv = cls.init(pairs, h, 2, 2, 64, 100)
    with pytest.raises(amd.ConvolutionPanic):
        conv.process(x[:, :10], out_len=11)                         # input_len < output_len
    with pytest.raises(amd.ConvolutionPanic):
        conv.update(np.zeros((3, 101), np.float32))
    assert conv.state() == (0, 2, 0)
    assert conv.process(x, out_len=32).shape == (2, 32)
