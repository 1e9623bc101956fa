"""MatrixLookaheadConvolver (include/fftconv.h): the MatrixConvolver's
definition with far-row windows.  Reference: matrix_ref.SummedOracle fed the
same call lengths and f64 direct convolution, tolerance common.REL_TOL.  The
scheme's own contract is bitwise: a run served from windows equals the same run
with set_windows(0) (every block sums all its rows), whatever the anchor phase,
the split by outputs, the grouping of calls or the load policy.
tests/test_matrix_la_ref.py proves on the CPU what each shape is there for."""
import functools

import numpy as np
import pytest
import torch

import oracle as oracle_module
from common import REL_TOL, assert_close
from matrix_la_ref import MAIN, Q, SHAPE_32, SHAPE_256, far_parts, near_parts
from matrix_ref import RAGGED_64, SummedOracle, direct, make

pytestmark = pytest.mark.gpu

FULL_100 = (64,) * 100


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


def _check_outputs(y, ref, what):
    assert np.isfinite(y).all() and np.abs(y).max() > 0, what
    for o in range(ref.shape[0]):
        assert_close(y[o], ref[o], what=f"{what} output {o}")


def _init(amd, h, B, L, windows=True):
    conv = amd.MatrixLookaheadConvolver.init(h, B, L)
    conv.set_windows(windows)
    return conv


def test_main_shape_full_blocks(amd):
    """I 3, O 10, B 64, L 2560 (S 40), 100 one-block calls: 96 far rows in two
    parts, two outputs per anchor slot, the delay line wraps twice."""
    I, O, B, L = MAIN
    h, x, ref, states = _case(51, I, O, B, L, FULL_100)
    conv = amd.MatrixLookaheadConvolver.init(h, B, L)
    assert amd.MatrixLookaheadConvolver.period() == Q
    assert (conv.inputs, conv.outputs, conv.block_size, conv.seg_count) == (I, O, B, 40)
    assert (conv.near_parts, conv.far_parts) == (near_parts(I, 40), far_parts(I, 40)) == (1, 2)
    anchors = []
    y = _run(conv, x, FULL_100, states, anchors)
    # block t anchors the outputs o = t (mod Q): two of them for t % Q < 2, else one
    assert anchors == [2 if t % Q < O - Q else 1 for t in range(100)]
    _check_outputs(y, ref, "summed oracle")
    _check_outputs(y, direct(oracle_module, x, h), "direct")


def test_main_shape_ragged_calls(amd):
    """Calls that start and end anywhere: a window row is consumed by the chunk
    that starts a block, the kept pre_multiplied sum serves the rest."""
    I, O, B, L = MAIN
    lengths = tuple(RAGGED_64)
    h, x, ref, states = _case(52, I, O, B, L, lengths)
    conv = amd.MatrixLookaheadConvolver.init(h, B, L)
    anchors = []
    y = _run(conv, x, lengths, states, anchors)
    assert max(anchors) > 0
    _check_outputs(y, ref, "ragged, summed oracle")
    full = _init(amd, h, B, L, windows=False)
    assert np.array_equal(y, _run(full, x, lengths, states)), "windows differ from full sums"


@pytest.mark.parametrize("shape,blocks", [(SHAPE_256, 45), (SHAPE_32, 30), ((2, 3, 512, 512 * 12), 12)],
                         ids=["B256", "B32", "B512"])
def test_block_sizes(amd, shape, blocks):
    """B 256 (two row groups), B 32 (sixteen), B 512 (one group, the largest
    block): full blocks, then two calls that split a block; windows against full
    sums bitwise."""
    I, O, B, L = shape
    lengths = (B,) * blocks + (B - 24, 24)
    h, x, ref, states = _case(53, I, O, B, L, lengths)
    conv = amd.MatrixLookaheadConvolver.init(h, B, L)
    assert conv.far_parts == far_parts(I, L // B) == 1
    anchors = []
    y = _run(conv, x, lengths, states, anchors)
    assert max(anchors) > 0
    _check_outputs(y, ref, f"B={B}")
    full = _init(amd, h, B, L, windows=False)
    assert full.anchors() == 0
    assert np.array_equal(y, _run(full, x, lengths)), "windows differ from full sums"


def test_windows_equal_full_sums_bitwise(amd):
    I, O, B, L = MAIN
    h, x, ref, states = _case(51, I, O, B, L, FULL_100)
    full = _init(amd, h, B, L, windows=False)
    anchors = []
    yf = _run(full, x, FULL_100, states, anchors)
    assert not any(anchors)
    yw = _run(amd.MatrixLookaheadConvolver.init(h, B, L), x, FULL_100)
    assert np.abs(yw).max() > 0
    assert np.array_equal(yw, yf)
    # switching mid-run: off after 21 blocks, on again after 40
    sw = amd.MatrixLookaheadConvolver.init(h, B, L)
    ys = [_run(sw, x[:, :21 * B], (B,) * 21)]
    sw.set_windows(False)
    assert sw.anchors() == 0
    ys.append(_run(sw, x[:, 21 * B:40 * B], (B,) * 19))
    sw.set_windows(True)
    assert sw.anchors() > 0
    ys.append(_run(sw, x[:, 40 * B:], (B,) * 60))
    assert np.array_equal(np.concatenate(ys, axis=1), yf)


def test_update_sequence_windows_equal_full_sums(amd):
    """An update at a block boundary, one mid-block, a shrink to 12 segments
    while current >= 20 (current >= active: no anchors until it is back
    inside), a zero-length response, a full-length one, then a reset.  Three
    handles: windows, windows through update_device, full sums -- bitwise equal
    after every call, within tolerance of the summed oracle."""
    I, O, B, L = MAIN
    rng = np.random.default_rng(54)
    h0, x = make(54, I, O, L, 112 * B)
    mk = lambda n: (rng.uniform(-1, 1, (O, I, n)) / np.sqrt(max(n, 1))).astype(np.float32)
    ref = SummedOracle(oracle_module, h0, B, L)
    win, dev, full = (_init(amd, h0, B, L, w) for w in (True, True, False))
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
            r = ref.process(blk)
            y, yf, yd = win.process(blk), full.process(blk), dev.process(blk)
            assert win.state() == dev.state() == full.state() == ref.state()
            assert np.array_equal(y, yf), f"{what}: windows differ from full sums at {pos}"
            assert np.array_equal(y, yd), f"{what}: update_device differs at {pos}"
            if ref.state()[1] == 0:
                assert not y.any() and not r.any()
            else:
                _check_outputs(y, r, f"{what}, samples {pos}..{pos + n}")
            pos += n

    def update(hn):
        ref.update(hn)
        win.update(hn)
        full.update(hn)
        d = torch.from_numpy(hn).to("cuda:0")
        dev.update_device(d.data_ptr(), hn.shape[2], hn.shape[2], 0)
        dev.synchronize()
        assert win.state() == dev.state() == full.state() == ref.state()

    run((B,) * 12, "init")
    update(mk(L - 100))                      # at a block boundary, mid-window for every output
    run((B,) * 9 + (20,), "boundary update")
    update(mk(L))                            # mid-block
    run((44,) + (B,) * 22, "mid-block update")  # (the delay line wraps: current 18 -> 36)
    assert ref.state()[0] >= 20
    update(mk(12 * B - 10))                  # shrink: current >= active = 12 > Q
    assert win.far_parts == far_parts(I, 12) == 1
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


def test_output_sharding_bitwise(amd):
    """Outputs 0..4 and 5..9 on two handles against one handle: output 5 anchors
    on t = 5 (mod Q) in the whole matrix and on t = 0 in the shard."""
    I, O, B, L = MAIN
    h, x, ref, _ = _case(51, I, O, B, L, FULL_100)
    whole = amd.MatrixLookaheadConvolver.init(h, B, L)
    lo = amd.MatrixLookaheadConvolver.init(h[:5], B, L)
    hi = amd.MatrixLookaheadConvolver.init(h[5:], B, L)
    assert (whole.near_parts, whole.far_parts) == (lo.near_parts, lo.far_parts) == (hi.near_parts, hi.far_parts)
    lengths = (B,) * 30 + (17, 47) + (B,) * 10
    n = sum(lengths)
    yw = _run(whole, x[:, :n], lengths)
    ys = np.concatenate([_run(lo, x[:, :n], lengths), _run(hi, x[:, :n], lengths)], axis=0)
    _check_outputs(yw, ref[:, :n], "whole")
    assert np.array_equal(yw, ys)


@pytest.mark.parametrize("n,K", [(64, 30), (40, 30)])
def test_process_device_steps(amd, n, K):
    """30 steps of a block and of 40 samples on a torch side stream with padded
    rows, against separate process_device calls: the same bits."""
    I, O, B, L = MAIN
    h, x, _, _ = _case(51, I, O, B, L, FULL_100)
    x = x[:, :K * n]
    dev = torch.device("cuda:0")
    pad_in, pad_out = n + 5, n + 3
    xs = np.zeros((K, I, pad_in), np.float32)
    xs[:, :, :n] = x.reshape(I, K, n).transpose(1, 0, 2)
    xd = torch.from_numpy(xs).to(dev)
    s = torch.cuda.Stream(dev)
    a = amd.MatrixLookaheadConvolver.init(h, B, L)
    b = amd.MatrixLookaheadConvolver.init(h, B, L)
    ya = torch.full((K, O, pad_out), -7.0, device=dev)
    yb = torch.full((K, O, pad_out), -7.0, device=dev)
    s.wait_stream(torch.cuda.current_stream())
    a.process_device_steps(xd.data_ptr(), pad_in, I * pad_in, ya.data_ptr(), pad_out, O * pad_out, n, K,
                           s.cuda_stream)
    for k in range(K):
        b.process_device(xd[k].data_ptr(), pad_in, yb[k].data_ptr(), pad_out, n, s.cuda_stream)
    s.synchronize()
    assert a.state() == b.state()
    ya_h, yb_h = ya.cpu().numpy(), yb.cpu().numpy()
    assert np.array_equal(ya_h, yb_h)
    assert (ya_h[:, :, n:] == -7.0).all()  # (the padding is untouched)
    y = ya_h[:, :, :n].transpose(1, 0, 2).reshape(O, K * n)
    host = amd.MatrixLookaheadConvolver.init(h, B, L)
    assert np.array_equal(y, _run(host, x, (n,) * K))
    _check_outputs(y, direct(oracle_module, x, h), "device steps")


def test_clone_mid_window(amd):
    """A clone taken after 21 blocks and 17 samples: every output is inside a
    window (outputs 0..7 at different depths, 8 and 9 sharing slots 0 and 1), a
    block is in progress.  It carries the windows and the block count."""
    I, O, B, L = MAIN
    h, x, ref, _ = _case(51, I, O, B, L, FULL_100)
    first = (B,) * 21 + (17,)
    n = sum(first)
    conv = amd.MatrixLookaheadConvolver.init(h, B, L)
    _run(conv, x[:, :n], first)
    twin = conv.clone()
    assert twin.state() == conv.state() and twin.anchors() == conv.anchors()
    rest = (47,) + (B,) * 30
    m = sum(rest)
    anchors = []
    ya = _run(conv, x[:, n:n + m], rest)
    yb = _run(twin, x[:, n:n + m], rest, anchors=anchors)
    assert max(anchors) > 0
    assert np.array_equal(ya, yb)
    _check_outputs(ya, ref[:, n:n + m], "after clone")
    # reset: the same bits as a fresh handle
    conv.reset()
    assert conv.state() == (0, 40, 0)
    fresh = amd.MatrixLookaheadConvolver.init(h, B, L)
    assert np.array_equal(_run(conv, x[:, :20 * B], (B,) * 20), _run(fresh, x[:, :20 * B], (B,) * 20))


@pytest.mark.parametrize("shape", [MAIN, SHAPE_256], ids=["B64", "B256"])
def test_nontemporal_instantiation(amd, shape):
    """matrix_la_a_kernel<..., true> through the kernel-variant knob: bitwise
    equal to the plain-load instantiation."""
    I, O, B, L = shape
    h, x = make(55, I, O, L, 30 * B)
    ys = []
    for v in (2, 0):
        amd.set_kernel_variant(v)
        try:
            ys.append(_run(amd.MatrixLookaheadConvolver.init(h, B, L), x, (B,) * 30))
        finally:
            amd.set_kernel_variant(-1)
    assert np.abs(ys[0]).max() > 0
    assert np.array_equal(ys[0], ys[1])
    _check_outputs(ys[0], direct(oracle_module, x, h), "nontemporal")


@pytest.mark.parametrize("segs", [1, 5, 8, 9])
def test_few_segments(amd, segs):
    """active <= Q runs near rows only (far_parts == 0, nothing anchors); 9
    segments have one far row per input."""
    I, O, B = 3, 10, 64
    L = segs * B
    lengths = (B,) * 20 + (30, 34)
    h, x, ref, states = _case(56, I, O, B, L, lengths)
    conv = amd.MatrixLookaheadConvolver.init(h, B, L)
    assert conv.far_parts == (0 if segs <= Q else 1)
    anchors = []
    y = _run(conv, x, lengths, states, anchors)
    assert (max(anchors) > 0) == (segs > Q)
    _check_outputs(y, ref, f"{segs} segments")
    full = _init(amd, h, B, L, windows=False)
    assert np.array_equal(y, _run(full, x, lengths))


def test_non_finite_sample_leaves(amd):
    """A NaN in input 1 at block 5 (I 2, O 3, B 64, L 1280, S 20): from sample
    nan_idx + (S + 2) * B on, outputs are finite and within tolerance of f64
    direct convolution with that sample set to 0 -- no window keeps it longer
    than the delay line does."""
    I, O, B, L, S = 2, 3, 64, 1280, 20
    h, x = make(57, I, O, L, 60 * B)
    nan_idx = 5 * B + 10
    xn = x.copy()
    xn[1, nan_idx] = np.nan
    conv = amd.MatrixLookaheadConvolver.init(h, B, L)
    y = _run(conv, xn, (B,) * 60)
    x0 = x.copy()
    x0[1, nan_idx] = 0.0
    ref = direct(oracle_module, x0, h)
    first = nan_idx + (S + 2) * B
    assert not np.isfinite(y[:, nan_idx:first]).all()
    assert np.isfinite(y[:, first:]).all()
    assert np.abs(y[:, first:] - ref[:, first:]).max() <= REL_TOL * np.abs(ref).max()
    assert conv.state() == (0, S, 0)


def test_errors(amd):
    h, x = make(58, 2, 2, 100, 64)
    with pytest.raises(amd.ConvolutionPanic):
        amd.MatrixLookaheadConvolver.init(h, 64, 99)                       # response_len > max_response_length
    with pytest.raises(amd.ConvolutionPanic):
        amd.MatrixLookaheadConvolver.init(np.zeros((2, 0, 8), np.float32), 64, 8)   # inputs == 0
    with pytest.raises(amd.ConvolutionPanic):
        amd.MatrixLookaheadConvolver.init(np.zeros((0, 2, 8), np.float32), 64, 8)   # outputs == 0
    for bad in (16, 1024, 8192):
        with pytest.raises(amd.DeviceError, match="block size"):
            amd.MatrixLookaheadConvolver.init(h, bad, 100)
    conv = amd.MatrixLookaheadConvolver.init(h, 64, 100)
    with pytest.raises(amd.ConvolutionPanic):
        conv.process(x[:, :10], out_len=11)                       # input_len < output_len
    with pytest.raises(amd.ConvolutionPanic):
        conv.update(np.zeros((2, 2, 101), np.float32))
    assert conv.state() == (0, 2, 0)
    assert conv.process(x, out_len=32).shape == (2, 32)
