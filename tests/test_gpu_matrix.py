"""MatrixConvolver (include/fftconv.h): y[o] = sum_i x[i] * h[o][i] as
inputs x outputs FFTConvolver instances in lockstep.  Reference: per output the
f64 sum over i of oracle FFTConvolver instances fed the same call lengths
(matrix_ref.SummedOracle; tests/test_matrix_ref.py puts it 1.6e-7 to 3.3e-7
from f64 direct convolution on these shapes), tolerance common.REL_TOL.  The
path shapes (matrix_paths.SHAPES) are compared with f64 direct convolution."""
import functools

import numpy as np
import pytest
import torch

import oracle as oracle_module
from common import REL_TOL, assert_close, max_rel_err
from matrix_paths import CAPPED, SHAPES, capped_lengths, parts, shape_blocks, shape_id, shape_len, walk
from matrix_ref import RAGGED_64, RAGGED_256, BlockModel, SummedOracle, direct, make

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(seed, I, O, B, L, lengths):
    """(h, x, summed-oracle output, oracle state after every call); computed
    once per shape, shared, never written to"""
    h, x = make(seed, I, O, L, sum(lengths))
    ref = SummedOracle(oracle_module, h, B, L)
    ys, states, pos = [], [], 0
    for n in lengths:
        ys.append(ref.process(x[:, pos:pos + n]))
        states.append(ref.state())
        pos += n
    y = np.concatenate(ys, axis=1)
    for a in (h, x, y):
        a.setflags(write=False)
    return h, x, y, tuple(states)


def _run(conv, x, lengths, states=None):
    out, pos = [], 0
    for k, n in enumerate(lengths):
        out.append(conv.process(x[:, pos:pos + n]))
        if states is not None:
            assert conv.state() == states[k], (k, conv.state(), states[k])
        pos += n
    return np.concatenate(out, axis=1)


def _check_outputs(y, ref, what):
    for o in range(ref.shape[0]):
        assert_close(y[o], ref[o], what=f"{what} output {o}")


def test_full_blocks(amd):
    """I=3, O=2, B=64, L=1000 (S=16), 40 one-block calls."""
    I, O, B, L = 3, 2, 64, 1000
    h, x, ref, states = _case(11, I, O, B, L, (B,) * 40)
    conv = amd.MatrixConvolver.init(h, B, L)
    assert (conv.inputs, conv.outputs, conv.block_size, conv.seg_count) == (I, O, B, 16)
    y = _run(conv, x, (B,) * 40, states)
    _check_outputs(y, ref, "summed oracle")
    _check_outputs(y, direct(oracle_module, x, h), "direct")


@pytest.mark.parametrize("I,O,B,L,lengths", [(3, 2, 64, 1000, tuple(RAGGED_64)), (2, 2, 256, 1500, tuple(RAGGED_256))])
def test_ragged_calls(amd, I, O, B, L, lengths):
    """Calls that start and end anywhere: the input buffer, the kept
    pre_multiplied sum, and calls that span several blocks."""
    h, x, ref, states = _case(12, I, O, B, L, lengths)
    conv = amd.MatrixConvolver.init(h, B, L)
    y = _run(conv, x, lengths, states)
    _check_outputs(y, ref, "summed oracle")


@pytest.mark.parametrize("B", [32, 128, 512, 2048, 8192])
def test_block_sizes(amd, B):
    """The limits (32, 8192: the two-buffer LDS is full), the first 512-thread
    size (2048) and sizes between: 5 full blocks, then calls of B - 24 and 24."""
    L = 3 * B + 5
    lengths = (B,) * 5 + (B - 24, 24)
    h, x, ref, states = _case(13, 2, 2, B, L, lengths)
    conv = amd.MatrixConvolver.init(h, B, L)
    assert conv.seg_count == 4
    y = _run(conv, x, lengths, states)
    _check_outputs(y, ref, f"B={B}")


def test_split_rows(amd):
    """I=4, O=2, B=32, L=4096 (S=128): 508 rows per output in 8 parts, 140
    blocks so the delay line wraps; I=1, O=2, B=64, L=200: 3 rows, one part."""
    h, x, ref, states = _case(14, 4, 2, 32, 4096, (32,) * 140)
    conv = amd.MatrixConvolver.init(h, 32, 4096)
    assert conv.mac_parts >= 2
    y = conv.process(x)
    assert conv.state() == states[-1]
    _check_outputs(y, ref, "split")
    h, x, ref, states = _case(15, 1, 2, 64, 200, (64,) * 10)
    conv = amd.MatrixConvolver.init(h, 64, 200)
    assert conv.mac_parts == 1
    _check_outputs(_run(conv, x, (64,) * 10, states), ref, "one part")


def test_output_sharding_bitwise(amd):
    """Outputs do not depend on the number of outputs: one handle against two
    handles holding outputs 0..2 and 3..5."""
    I, O, B, L = 3, 6, 64, 2000
    h, x = make(16, I, O, L, 40 * B)
    whole = amd.MatrixConvolver.init(h, B, L)
    lo = amd.MatrixConvolver.init(h[:3], B, L)
    hi = amd.MatrixConvolver.init(h[3:], B, L)
    assert whole.mac_parts == lo.mac_parts == hi.mac_parts
    yw = _run(whole, x, (B,) * 40)
    ys = np.concatenate([_run(lo, x, (B,) * 40), _run(hi, x, (B,) * 40)], axis=0)
    assert np.isfinite(yw).all() and np.abs(yw).max() > 0
    assert np.array_equal(yw, ys)


def _update_sequence(I, O, B, L):
    """(kind, payload) steps: update at a block boundary, mid-block, a shrink
    to 130 samples while current >= 3, then a zero-length response"""
    rng = np.random.default_rng(17)
    h0, x = make(17, I, O, L, 60 * B)
    mk = lambda n: (rng.uniform(-1, 1, (O, I, n)) / np.sqrt(max(n, 1))).astype(np.float32)
    return h0, x, [("run", (B,) * 5), ("update", mk(700)), ("run", (B,) * 3 + (20,)), ("update", mk(L)),
                   ("run", (44,) + (B,) * 4), ("need_current", 3), ("update", mk(130)),
                   ("run", (B, 10, 54, B, 2 * B, B)), ("update", mk(0)), ("run", (B, 30))]


def test_update(amd):
    I, O, B, L = 3, 2, 64, 1000
    h0, x, seq = _update_sequence(I, O, B, L)
    ref = SummedOracle(oracle_module, h0, B, L)
    conv = amd.MatrixConvolver.init(h0, B, L)
    dev = amd.MatrixConvolver.init(h0, B, L)
    pos = 0
    for kind, arg in seq:
        if kind == "update":
            ref.update(arg)
            conv.update(arg)
            d = torch.from_numpy(arg).to("cuda:0")
            dev.update_device(d.data_ptr(), arg.shape[2], arg.shape[2], 0)
            dev.synchronize()
            assert conv.state() == dev.state() == ref.state()
        elif kind == "need_current":
            assert ref.state()[0] >= arg, ref.state()
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
                    _check_outputs(y, r, f"after update, samples {pos}..{pos + n}")
                pos += n
    assert ref.state()[1] == 0


def test_reset_and_clone(amd):
    I, O, B, L = 3, 2, 64, 1000
    lengths = tuple(RAGGED_64[:11])
    h, x, ref, states = _case(12, I, O, B, L, tuple(RAGGED_64))
    n = sum(lengths)
    conv = amd.MatrixConvolver.init(h, B, L)
    _run(conv, x[:, 500:], (64, 64, 17))
    conv.reset()
    assert conv.state() == (0, 16, 0)
    fresh = amd.MatrixConvolver.init(h, B, L)
    y = _run(conv, x[:, :n], lengths)
    assert np.array_equal(y, _run(fresh, x[:, :n], lengths))
    _check_outputs(y, ref[:, :n], "after reset")
    # (the 11 calls end mid-block: fill != 0)
    assert conv.state()[2] != 0
    twin = conv.clone()
    assert twin.state() == conv.state()
    rest = tuple(RAGGED_64[11:])
    ya = _run(conv, x[:, n:], rest)
    yb = _run(twin, x[:, n:], rest)
    assert np.array_equal(ya, yb)
    _check_outputs(ya, ref[:, n:], "after clone")


@pytest.mark.parametrize("n,K", [(64, 30), (40, 30)])
def test_process_device_steps(amd, n, K):
    """30 steps of a block and 30 steps of 40 samples at B = 64, on a torch
    side stream with padded rows; a consumer on that stream reads the result
    without a host synchronisation."""
    I, O, B, L = 3, 2, 64, 1000
    h, x = make(18, I, O, L, K * n)
    dev = torch.device("cuda:0")
    pad_in, pad_out = n + 5, n + 3
    xs = np.zeros((K, I, pad_in), np.float32)
    xs[:, :, :n] = x.reshape(I, K, n).transpose(1, 0, 2)
    xd = torch.from_numpy(xs).to(dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream())
    a = amd.MatrixConvolver.init(h, B, L)
    b = amd.MatrixConvolver.init(h, B, L)
    ya = torch.full((K, O, pad_out), -7.0, device=dev)
    yb = torch.full((K, O, pad_out), -7.0, device=dev)
    s.wait_stream(torch.cuda.current_stream())
    a.process_device_steps(xd.data_ptr(), pad_in, I * pad_in, ya.data_ptr(), pad_out, O * pad_out, n, K,
                           s.cuda_stream)
    with torch.cuda.stream(s):
        doubled = ya * 2.0  # (ordered by the stream alone)
    for k in range(K):
        b.process_device(xd[k].data_ptr(), pad_in, yb[k].data_ptr(), pad_out, n, s.cuda_stream)
    s.synchronize()
    assert a.state() == b.state()
    ya_h, yb_h = ya.cpu().numpy(), yb.cpu().numpy()
    assert np.array_equal(ya_h, yb_h)
    assert np.array_equal(doubled.cpu().numpy(), ya_h * 2.0)
    assert (ya_h[:, :, n:] == -7.0).all()  # (the padding is untouched)
    y = ya_h[:, :, :n].transpose(1, 0, 2).reshape(O, K * n)
    ref = SummedOracle(oracle_module, h, B, L).run(x, (n,) * K)
    _check_outputs(y, ref, "device steps")


def test_non_finite_sample_leaves(amd):
    """A NaN in input 1 at block 5 (I=2, O=2, B=64, L=500, S=8): from sample
    nan_idx + (S + 2) * B on, outputs are finite and within tolerance of f64
    direct convolution with that sample set to 0."""
    I, O, B, L, S = 2, 2, 64, 500, 8
    h, x = make(19, I, O, L, 30 * B)
    nan_idx = 5 * B + 10
    xn = x.copy()
    xn[1, nan_idx] = np.nan
    conv = amd.MatrixConvolver.init(h, B, L)
    y = _run(conv, xn, (B,) * 30)
    x0 = x.copy()
    x0[1, nan_idx] = 0.0
    ref = direct(oracle_module, x0, h)
    first = nan_idx + (S + 2) * B
    assert np.isfinite(y[:, first:]).all()
    peak = np.abs(ref).max()
    assert np.abs(y[:, first:] - ref[:, first:]).max() <= REL_TOL * peak
    assert conv.state() == (S - 30 % S if 30 % S else 0, S, 0)


def test_errors(amd):
    h, x = make(20, 2, 2, 100, 64)
    with pytest.raises(amd.ConvolutionPanic):
        amd.MatrixConvolver.init(h, 64, 99)                       # response_len > max_response_length
    with pytest.raises(amd.ConvolutionPanic):
        amd.MatrixConvolver.init(np.zeros((2, 0, 8), np.float32), 64, 8)   # inputs == 0
    with pytest.raises(amd.ConvolutionPanic):
        amd.MatrixConvolver.init(np.zeros((0, 2, 8), np.float32), 64, 8)   # outputs == 0
    for bad in (16, 16384):
        with pytest.raises(amd.DeviceError, match="block size"):
            amd.MatrixConvolver.init(h, bad, 100)
    conv = amd.MatrixConvolver.init(h, 64, 100)
    with pytest.raises(amd.ConvolutionPanic):
        conv.process(x[:, :10], out_len=11)                       # input_len < output_len
    with pytest.raises(amd.ConvolutionPanic):
        conv.update(np.zeros((2, 2, 101), np.float32))
    assert conv.state() == (0, 2, 0)
    assert conv.process(x, out_len=32).shape == (2, 32)


# ---------------------------------------------------------------------------
# Path coverage (matrix_paths): shapes at which matrix_row_walk's unrolled loop, its
# hand-over to the tail loop, several parts at every block size, the P cap and
# matrix_b_kernel's chunked sums run; tests/test_matrix_ref.py proves on the
# CPU that each shape reaches the path it is listed for.
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _direct_case(seed, I, O, L, n):
    """(h, x, f64 direct convolution); computed once per shape, never written to"""
    h, x = make(seed, I, O, L, n)
    ref = direct(oracle_module, x, h)
    for a in (h, x, ref):
        a.setflags(write=False)
    return h, x, ref


def _check_ref(y, ref, what):
    """finite, non-zero (unless the reference is), within tolerance; prints the
    error so a run shows how much of REL_TOL each shape uses"""
    assert np.isfinite(y).all(), what
    assert np.abs(y).max() > 0 or not ref.any(), what
    print(f"{what}: max_rel_err {max_rel_err(y, ref):.3e}")
    _check_outputs(y, ref, what)


@pytest.mark.parametrize("s", SHAPES, ids=shape_id)
def test_paths(amd, s):
    """S + 3 full blocks of every path shape in one call against f64 direct
    convolution: the delay line wraps, every MAC row contributes.  One
    dropped, doubled or misplaced row of R moves an output by about
    max|ref| / sqrt(R) (1 % at R = 8220), a part left out of the finish
    kernel's sum by sqrt(1 / P): both far above REL_TOL."""
    L, n = shape_len(s), shape_blocks(s) * s.B
    h, x, ref = _direct_case(21, s.I, s.O, L, n)
    conv = amd.MatrixConvolver.init(h, s.B, L)
    assert (conv.block_size, conv.seg_count) == (s.B, s.S)
    assert conv.mac_parts == walk(s.B, s.I, s.S).P
    y = conv.process(x)
    assert conv.state() == (-shape_blocks(s) % s.S, s.S, 0)
    _check_ref(y, ref, shape_id(s))


@pytest.mark.parametrize("s", CAPPED, ids=shape_id)
def test_paths_ragged_capped(amd, s):
    """The two shapes at the P cap (64 parts, more than 64 rows each): one
    call of S blocks, then calls that start and end anywhere -- the kept
    pre_multiplied sum of 64 parts."""
    lengths = capped_lengths(s)
    h, x, ref, states = _case(22, s.I, s.O, s.B, shape_len(s), lengths)
    conv = amd.MatrixConvolver.init(h, s.B, shape_len(s))
    assert conv.mac_parts == 64
    y = _run(conv, x, lengths, states)
    _check_ref(y, ref, "ragged " + shape_id(s))


def test_update_changes_parts(amd):
    """Updates that change P (B 32, I 4, O 2, S 128; `part` is sized for
    P = 8): 68 blocks (current 60), update to 40 segments (P = 3, current >=
    active) and 45 blocks, back to the full length (P = 8) and 130 blocks, 20
    samples (one segment, no MAC rows) and 3 blocks, length 0 and one call.
    A second handle follows through update_device."""
    I, O, B, L = 4, 2, 32, 4096
    rng = np.random.default_rng(23)
    h0, x = make(23, I, O, L, (68 + 45 + 130 + 3 + 1) * B)
    mk = lambda n: (rng.uniform(-1, 1, (O, I, n)) / np.sqrt(max(n, 1))).astype(np.float32)
    ref = SummedOracle(oracle_module, h0, B, L)
    conv = amd.MatrixConvolver.init(h0, B, L)
    dev = amd.MatrixConvolver.init(h0, B, L)
    assert conv.mac_parts == dev.mac_parts == 8
    pos = 0

    def run(calls, what):
        nonlocal pos
        for n in calls:
            blk = x[:, pos:pos + n]
            r = ref.process(blk)
            y = conv.process(blk)
            yd = dev.process(blk)
            assert conv.state() == dev.state() == ref.state()
            assert np.array_equal(y, yd), "update_device differs from update"
            if ref.state()[1] == 0:
                assert not y.any() and not r.any()
            else:
                _check_ref(y, r, f"{what}, samples {pos}..{pos + n}")
            pos += n

    def update(hn, P):
        ref.update(hn)
        conv.update(hn)
        d = torch.from_numpy(hn).to("cuda:0")
        dev.update_device(d.data_ptr(), hn.shape[2], hn.shape[2], 0)
        dev.synchronize()
        assert conv.state() == dev.state() == ref.state()
        assert conv.mac_parts == dev.mac_parts == P == parts(I, ref.state()[1])

    run((B,) * 4 + (64 * B,), "P = 8")
    assert ref.state()[0] >= 60
    update(mk(40 * B - 5), 3)
    assert ref.state()[0] >= ref.state()[1] == 40
    run((B,) * 25 + (20 * B,), "P = 3")
    assert ref.state()[0] < 40  # (current came back inside the active segments)
    update(mk(L), 8)
    run((B,) * 2 + (128 * B,), "P = 8 again")
    update(mk(20), 1)
    run((B,) * 3, "one segment")
    update(mk(0), 1)
    run((B,), "no response")
    assert ref.state()[1] == 0 and pos == x.shape[1]


def test_many_pairs(amd):
    """More than 32768 (o, i) pairs (I = 2, O = 16400, B 64, L 100, S 2; H is
    33 MiB): the IR transform runs in two slabs of pairs.  Four one-block
    calls, an update to a new response, two more blocks, against the f64
    block model (matrix_ref.BlockModel, validated in tests/test_matrix_ref.py);
    the outputs of the second slab (o >= 16384) are asserted on their own."""
    I, O, B, L = 2, 16400, 64, 100
    rng = np.random.default_rng(24)
    mk = lambda: (rng.uniform(-1, 1, (O, I, L)) / np.sqrt(L)).astype(np.float32)
    h, h2 = mk(), mk()
    x = rng.uniform(-1, 1, (I, 6 * B)).astype(np.float32)
    assert O * I > 32768
    ref = BlockModel(h, B, L)
    conv = amd.MatrixConvolver.init(h, B, L)
    assert (conv.seg_count, conv.mac_parts) == (2, 1)

    def blocks(ks, what):
        for k in ks:
            blk = x[:, k * B:(k + 1) * B]
            r = ref.process_block(blk)
            y = conv.process(blk)
            assert np.isfinite(y).all() and np.abs(y[16384:]).max() > 0
            peak = np.abs(r).max()
            e_lo = np.abs(y[:16384] - r[:16384]).max() / peak
            e_hi = np.abs(y[16384:] - r[16384:]).max() / peak
            print(f"many pairs {what} block {k}: first slab {e_lo:.3e}, second slab {e_hi:.3e}")
            assert e_hi <= REL_TOL, f"{what} block {k}: second slab of pairs (outputs >= 16384) {e_hi:.3e}"
            assert e_lo <= REL_TOL, f"{what} block {k}: first slab of pairs {e_lo:.3e}"

    blocks(range(4), "init")
    # (the block model itself, on outputs of both slabs, against f64 direct convolution)
    sel = [0, 16383, 16384, 16399]
    m = BlockModel(h[sel], B, L)
    ym = np.concatenate([m.process_block(x[:, k * B:(k + 1) * B]) for k in range(4)], axis=1)
    assert max_rel_err(ym, direct(oracle_module, x[:, :4 * B], h[sel])) <= 1e-12
    ref.update(h2)
    conv.update(h2)
    blocks(range(4, 6), "after update")
    assert conv.state() == (0, 2, 0)


def test_zero_length_response_device(amd):
    """process_device with no active segment (update to length 0): exactly n
    zeros per output row of a padded output, the padding and the state
    untouched."""
    I, O, B, L, n = 3, 2, 64, 100, 40
    h, x = make(25, I, O, L, 3 * B + 17)
    conv = amd.MatrixConvolver.init(h, B, L)
    y = _run(conv, x, (B, B, B, 17))
    assert np.abs(y).max() > 0
    conv.update(np.zeros((O, I, 0), np.float32))
    state = conv.state()
    assert state == (1, 0, 17)
    dev = torch.device("cuda:0")
    xd = torch.ones((I, n + 5), device=dev)
    yd = torch.full((O, n + 3), -7.0, device=dev)
    conv.process_device(xd.data_ptr(), n + 5, yd.data_ptr(), n + 3, n)
    conv.synchronize()
    torch.cuda.synchronize()
    out = yd.cpu().numpy()
    assert (out[:, :n] == 0.0).all()
    assert (out[:, n:] == -7.0).all()
    assert conv.state() == state


@pytest.mark.parametrize("s", [s for s in SHAPES if (s.B, s.I) in ((128, 11), (1024, 5))], ids=shape_id)
def test_nontemporal_instantiation(amd, s):
    """matrix_a_kernel<..., true> (nontemporal H loads; chosen automatically
    only above 256 MiB of H) through the kernel-variant knob, at a shape with
    row groups (G = 4) and one with SPT = 2: bitwise equal to the plain-load
    instantiation and within tolerance of f64 direct convolution."""
    L, n = shape_len(s), shape_blocks(s) * s.B
    h, x, ref = _direct_case(21, s.I, s.O, L, n)
    ys = []
    for v in (2, 0):
        amd.set_kernel_variant(v)
        try:
            conv = amd.MatrixConvolver.init(h, s.B, L)
            ys.append(conv.process(x))
        finally:
            amd.set_kernel_variant(-1)
    for y, what in zip(ys, ("nontemporal", "plain")):
        _check_ref(y, ref, f"{what} {shape_id(s)}")
        assert np.abs(y).max() > 0
    assert np.array_equal(ys[0], ys[1])


# ---- the host paths every matrix handle type shares -------------------------
_SH_I, _SH_O, _SH_B, _SH_L, _SH_N = 2, 3, 32, 100, 20  # calls of 20 samples: every call ends mid-block
_SH_PAIRS = [(o, i) for o in range(_SH_O) for i in range(_SH_I)]  # the full pattern, in the dense order


def _shared_handle(amd, kind, h):
    rows = h.reshape(_SH_O * _SH_I, -1)
    dense = lambda: amd.MatrixConvolver.init(h, _SH_B, _SH_L)
    sparse = lambda: amd.SparseMatrixConvolver.init(_SH_PAIRS, rows, _SH_I, _SH_O, _SH_B, _SH_L)
    if kind == "matrix":
        return dense()
    if kind == "matrix_sparse":
        return sparse()
    if kind == "matrix_lookahead":
        return amd.MatrixLookaheadConvolver.init(h, _SH_B, _SH_L)
    if kind == "matrix_sparse_lookahead":
        return amd.SparseMatrixLookaheadConvolver.init(_SH_PAIRS, rows, _SH_I, _SH_O, _SH_B, _SH_L)
    if kind == "matrix_crossfade":  # max_buffer_size 20: the two convolvers' blocks end inside a call
        return amd.MatrixCrossfadeConvolver.new(dense(), _SH_L, _SH_N, _SH_L)
    if kind == "matrix_sparse_crossfade":
        return amd.SparseMatrixCrossfadeConvolver.new(sparse(), _SH_L, _SH_N, _SH_L)
    assert kind == "matrix_twostage"
    return amd.MatrixTwoStageConvolver.init(h, _SH_B, _SH_L)


@functools.lru_cache(maxsize=None)
def _shared_case():
    h, x = make(31, _SH_I, _SH_O, _SH_L, 6 * _SH_N)
    ref = direct(oracle_module, x, h)
    for a in (h, x, ref):
        a.setflags(write=False)
    return h, x, ref


# the dense handle whose output a sparse one over the full pattern repeats bit for bit
_SH_DENSE_OF = {"matrix_sparse": "matrix", "matrix_sparse_lookahead": "matrix_lookahead",
                "matrix_sparse_crossfade": "matrix_crossfade"}


@pytest.mark.parametrize("kind", ["matrix", "matrix_lookahead", "matrix_sparse", "matrix_sparse_lookahead",
                                  "matrix_crossfade", "matrix_sparse_crossfade", "matrix_twostage"])
def test_shared_host_paths(amd, kind):
    """The host code all seven matrix handle types run through one definition
    (the block walk, process(), clone, the zero-length cases), at I = 2, O = 3,
    B = 32, IR length 100, calls of 20 samples; the sparse types over the full
    pattern, so the dense type's output is theirs bit for bit.
      - a zero-length process() is a no-op (not for the crossfaded types: the
        reference advances both convolvers by max_buffer_size whatever the
        output length is, test_gpu_matrix_xf.test_errors_and_init_form);
      - clone() taken mid-block continues bit-identically to the original;
      - update() to a zero-length response, then process_device: exact zeros
        are written, the rest of the output buffer and state() are untouched
        (the crossfaded types once the fade has ended; they and the two-stage
        matrix have no state(), and the two-stage update is todo!() in the
        reference: test_gpu_matrix_ts.test_errors)."""
    h, x, ref = _shared_case()
    n, I, O = _SH_N, _SH_I, _SH_O
    crossfaded = kind.endswith("crossfade")
    has_state = not crossfaded and kind != "matrix_twostage"
    conv = _shared_handle(amd, kind, h)
    dense = _shared_handle(amd, _SH_DENSE_OF[kind], h) if kind in _SH_DENSE_OF else None

    def calls(c, first, count):
        return np.concatenate([c.process(x[:, k * n:(k + 1) * n]) for k in range(first, first + count)], axis=1)

    y0 = calls(conv, 0, 3)
    if has_state:
        assert conv.state() == (3, 4, 3 * n % _SH_B)  # one block completed of 4 segments, mid-block
    if not crossfaded:
        state = conv.state() if has_state else None
        assert conv.process(x[:, :0]).shape == (O, 0)
        if has_state:
            assert conv.state() == state
    twin = conv.clone()
    if has_state:
        assert twin.state() == conv.state() and conv.state()[2] != 0
    ya = calls(conv, 3, 3)
    yb = calls(twin, 3, 3)
    assert np.array_equal(ya, yb), "the clone differs from the original"
    y = np.concatenate([y0, ya], axis=1)
    _check_outputs(y, ref, kind)
    if dense is not None:
        assert np.array_equal(y, calls(dense, 0, 6)), "sparse over the full pattern differs from dense"

    if kind == "matrix_twostage":
        return
    empty = np.zeros((O * I, 0) if kind in _SH_DENSE_OF else (O, I, 0), np.float32)
    conv.update(empty)
    if crossfaded:
        for _ in range(2 * _SH_L // n + 2):  # the fade of L samples and the hold, with room
            conv.process(x[:, :n])
        assert not conv.is_crossfading()
    state = conv.state() if has_state else None
    if has_state:
        assert state[1] == 0
    dev = torch.device("cuda:0")
    xd = torch.ones((I, n), device=dev)
    yd = torch.full((O, n + 3), -7.0, device=dev)
    conv.process_device(xd.data_ptr(), n, yd.data_ptr(), n + 3, n)
    conv.synchronize()
    torch.cuda.synchronize()
    out = yd.cpu().numpy()
    assert (out[:, :n] == 0.0).all()
    assert (out[:, n:] == -7.0).all()
    if has_state:
        assert conv.state() == state
