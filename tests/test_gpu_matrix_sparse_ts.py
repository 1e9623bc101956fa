"""SparseMatrixTwoStageConvolver (include/fftconv.h): one TwoStageFFTConvolver
instance per listed (output, input) pair in lockstep -- head, tail0 and tail as
sparse matrices over one pattern, the tail buffers summed per output.
Reference: matrix_sp_ts_ref.SparseSummedTwoStageOracle, per output the f64 sum
of the oracle TwoStageFFTConvolver instances listed for it, fed the same calls
(tests/test_matrix_sp_ts_ref.py checks it against f64 direct convolution);
tolerance common.REL_TOL on max|got - ref| / max|ref| per output, an output
without pairs exactly zero.  path(n): 0 = composition, 1 = fused.  The shapes
and what each is there for: matrix_sp_ts_ref.SHAPES."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle as oracle_module
from common import assert_close
from matrix_sp_ref import make
from matrix_sp_ts_ref import SHAPES, SparseSummedTwoStageOracle, pairs_of
from matrix_ts_ref import RAGGED

pytestmark = pytest.mark.gpu


class Scenario:
    """A shape of the table, its responses and input and a list of call
    lengths; the reference output is computed once and never written to."""

    def __init__(self, seed, name, lengths=None):
        self.name = name
        s = SHAPES[name]
        self.I, self.O, self.cols, self.head, self.L, self.T, self.segs = s.I, s.O, s.cols, s.head, s.L, s.T, s.segs
        self.pairs = pairs_of(s)
        self.lengths = [self.head] * s.calls if lengths is None else list(lengths)
        self.h, self.x = make(seed, self.pairs, self.I, self.L, sum(self.lengths))
        self.ref = SparseSummedTwoStageOracle(oracle_module, self.pairs, self.h, self.I, self.O, self.head,
                                              self.L).run(self.x, self.lengths)
        for a in (self.h, self.x, self.ref):
            a.setflags(write=False)

    def handle(self, amd, fused=True):
        conv = amd.SparseMatrixTwoStageConvolver.init(self.pairs, self.h, self.I, self.O, self.head, self.L)
        assert (conv.inputs, conv.outputs, conv.pairs) == (self.I, self.O, len(self.pairs))
        assert conv.tail_block_size == self.T
        if not fused:
            conv.set_fused(False)
        return conv

    def check(self, got, what, ref=None):
        ref = self.ref if ref is None else ref
        assert got.shape == ref.shape and np.isfinite(got).all()
        for o, cs in enumerate(self.cols):
            if cs:
                assert_close(got[o], ref[o], what=f"{what} output {o}")
            else:
                assert not got[o].any() and not ref[o].any(), f"{what}: output {o} has no pairs"


def drive(conv, x, lengths):
    """(outputs [O][sum(lengths)], path(n) before every call)"""
    ys, paths, pos = [], [], 0
    for n in lengths:
        paths.append(conv.path(n))
        ys.append(conv.process(x[:, pos:pos + n]))
        pos += n
    return np.concatenate(ys, axis=1), paths


@functools.lru_cache(maxsize=None)
def scenario(name):
    if name == "ragged":
        return Scenario(82, "three-stage", RAGGED)
    if name == "clone":   # 11 aligned calls, 20 samples into block 12, then past the end of two periods
        return Scenario(83, "three-stage", [64] * 11 + [20, 44] + [64] * 16)
    return Scenario(81, name)


_runs = {}


def gpu_run(amd, name, fused=True):
    """the scenario on a fresh handle, once per (scenario, fused)"""
    if (name, fused) not in _runs:
        sc = scenario(name)
        _runs[name, fused] = drive(sc.handle(amd, fused), sc.x, sc.lengths)
    return _runs[name, fused]


@pytest.mark.parametrize("name", list(SHAPES))
def test_aligned_calls(amd, name):
    sc = scenario(name)
    y, paths = gpu_run(amd, name)
    sc.check(y, name)
    assert paths == [1 if sc.segs[1] is not None else 0] * len(sc.lengths), paths
    if sc.segs[2] is not None:  # the tail's contribution is in the run: samples past 2T
        assert y.shape[1] > 2 * sc.T


@pytest.mark.parametrize("name", list(SHAPES))
def test_composition_equals_fused_bitwise(amd, name):
    sc = scenario(name)
    y, _ = gpu_run(amd, name)
    yc, pc = gpu_run(amd, name, fused=False)
    assert set(pc) == {0}
    sc.check(yc, f"{name} composition")
    assert np.array_equal(y, yc), (name, float(np.abs(y - yc).max()))


@pytest.mark.parametrize("name", ["three-stage", "split", "wide", "unrolled64"])
def test_each_output_equals_dense_twostage_bitwise(amd, name):
    """output o against the single output of a dense MatrixTwoStageConvolver
    with k_o inputs that holds h[pair e] and is fed x[i_e] in list order, the
    same calls; on the fused path and again on the composition path"""
    sc = scenario(name)
    n0 = 0
    for o, cs in enumerate(sc.cols):
        k = len(cs)
        if k:
            hd = np.ascontiguousarray(sc.h[n0:n0 + k][None])          # [1][k_o][L]
            xd = np.ascontiguousarray(sc.x[cs])
            for fused in (True, False):
                y, _ = gpu_run(amd, name, fused)
                dense = amd.MatrixTwoStageConvolver.init(hd, sc.head, sc.L)
                if not fused:
                    dense.set_fused(False)
                yd, paths = drive(dense, xd, sc.lengths)
                assert set(paths) == {1 if fused else 0}
                assert np.array_equal(yd[0], y[o]), (name, o, fused, float(np.abs(yd[0] - y[o]).max()))
        n0 += k
    assert n0 == len(sc.pairs)


def test_ragged(amd):
    sc = scenario("ragged")
    y, paths = gpu_run(amd, "ragged")
    sc.check(y, "ragged")
    total, want = 0, []
    for n in sc.lengths:  # aligned: a whole head block on a block boundary (64 divides T)
        want.append(1 if n == 64 and total % 64 == 0 else 0)
        total += n
    assert paths == want, (paths, want)
    assert 0 < sum(want) < len(want) and want[:4] == [1, 0, 0, 0]
    yc, pc = gpu_run(amd, "ragged", fused=False)
    assert set(pc) == {0}
    assert np.array_equal(y, yc), float(np.abs(y - yc).max())


def test_device_steps_equal_separate_calls(amd):
    """process_device_steps over 24 calls against 24 process_device calls, both
    on a stream that is not torch's default one: the same bits, and the bits
    of the host calls."""
    sc = scenario("three-stage")
    y, _ = gpu_run(amd, "three-stage")
    B, K, n = sc.head, 24, sc.x.shape[1]
    xd = torch.from_numpy(sc.x.copy()).to("cuda:0")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    outs = []
    for steps in (True, False):
        conv = sc.handle(amd)
        yd = torch.zeros((sc.O, K * B), dtype=torch.float32, device="cuda:0")
        s.wait_stream(torch.cuda.current_stream())
        if steps:
            conv.process_device_steps(xd.data_ptr(), n, B, yd.data_ptr(), K * B, B, B, K, s.cuda_stream)
        else:
            for k in range(K):
                conv.process_device(xd.data_ptr() + 4 * k * B, n, yd.data_ptr() + 4 * k * B, K * B, B, s.cuda_stream)
        s.synchronize()
        outs.append(yd.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0], y[:, :K * B])


def test_output_sharding_bitwise(amd):
    """the wide pattern as one handle against one handle per output that holds
    that output's pairs alone (outputs = 1, the same I: the inputs no pair reads
    are accepted and ignored)"""
    sc = scenario("wide")
    y, _ = gpu_run(amd, "wide")
    n0 = 0
    for o, cs in enumerate(sc.cols):
        conv = amd.SparseMatrixTwoStageConvolver.init([(0, i) for i in cs], sc.h[n0:n0 + len(cs)], sc.I, 1, sc.head,
                                                      sc.L)
        yo, paths = drive(conv, sc.x, sc.lengths)
        assert set(paths) == {1}
        assert np.array_equal(yo[0], y[o]), o
        n0 += len(cs)


def test_clone_mid_period_and_mid_block(amd):
    sc = scenario("clone")
    done = 12  # 11 aligned calls and a call of 20
    conv = sc.handle(amd)
    first, _ = drive(conv, sc.x, sc.lengths[:done])
    twin = conv.clone()
    assert (twin.inputs, twin.outputs, twin.pairs, twin.tail_block_size) == (sc.I, sc.O, len(sc.pairs), sc.T)
    at = sum(sc.lengths[:done])
    rest = sc.lengths[done:]
    assert conv.path(rest[0]) == twin.path(rest[0]) == 0 and conv.path(64) == 0
    ya, pa = drive(conv, sc.x[:, at:], rest)    # only the original advances ...
    yb, pb = drive(twin, sc.x[:, at:], rest)    # ... and the clone still continues from the cloning point
    assert pa == pb and pa[1:] == [1] * (len(rest) - 1), (pa, pb)
    assert np.array_equal(ya, yb)
    assert sum(sc.lengths) > 3 * sc.T           # past two period ends after the cloning point
    sc.check(np.concatenate([first, ya], axis=1), "original")
    sc.check(np.concatenate([first, yb], axis=1), "clone")
    # a clone of a composition handle stays on the composition path
    conv.set_fused(False)
    assert conv.clone().path(64) == 0 and conv.path(64) == 0 and twin.path(64) == 1


def test_reset(amd):
    """a ragged prefix, reset, then the aligned run: the bits of a fresh handle"""
    sc = scenario("three-stage")
    y, _ = gpu_run(amd, "three-stage")
    conv = sc.handle(amd)
    prefix = RAGGED[:13]
    assert sum(prefix) % sc.head != 0 and sum(prefix) > sc.T  # mid-block, past a period end
    drive(conv, sc.x, prefix)
    conv.reset()
    again, paths = drive(conv, sc.x, sc.lengths)
    assert set(paths) == {1}
    assert np.array_equal(again, y)


def raw_init(amd, pairs, h, inputs, outputs, block, max_len):
    """fftconv_matrix_sparse_twostage_init itself, past the mirror's checks: (handle or None, last error)"""
    po = np.ascontiguousarray([p[0] for p in pairs], dtype=np.uint32)
    pi = np.ascontiguousarray([p[1] for p in pairs], dtype=np.uint32)
    u32p, fp = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_float)
    hh = amd.lib().fftconv_matrix_sparse_twostage_init(0, inputs, outputs, len(pairs), po.ctypes.data_as(u32p),
                                                       pi.ctypes.data_as(u32p), h.ctypes.data_as(fp), h.shape[1],
                                                       h.shape[1], block, max_len)
    assert not hh
    return amd.last_error()


def test_errors(amd):
    sc = scenario("three-stage")
    y, _ = gpu_run(amd, "three-stage")
    conv = sc.handle(amd)
    first, _ = drive(conv, sc.x, sc.lengths[:3])
    with pytest.raises(amd.NotImplementedInReference):
        conv.update(sc.h)
    with pytest.raises(amd.ConvolutionPanic):
        conv.process(np.zeros((sc.I, sc.head + 1), np.float32))
    rest, _ = drive(conv, sc.x[:, 3 * sc.head:], sc.lengths[3:12])
    assert np.array_equal(np.concatenate([first, rest], axis=1), y[:, :12 * sc.head])  # the handle was unchanged
    init = amd.SparseMatrixTwoStageConvolver.init
    h1 = np.zeros((1, 16), np.float32)
    with pytest.raises(amd.DeviceError, match="tail block size 16384 exceeds 8192"):
        init([(0, 0)], h1, 1, 1, 512, 262144)
    assert init([(0, 0)], h1, 1, 1, 64, 262144).tail_block_size == 4096
    assert init([(0, 0)], h1, 1, 1, 256, 262144).tail_block_size == 8192
    with pytest.raises(amd.DeviceError, match="block size 16 outside"):
        init([(0, 0)], h1, 1, 1, 16, 100)
    with pytest.raises(amd.ConvolutionPanic, match="at least one pair"):
        init([], np.zeros((0, 16), np.float32), 2, 2, 64, 100)                  # an empty pair list
    with pytest.raises(amd.ConvolutionPanic, match="out of range"):
        init([(0, 0), (1, 2)], np.zeros((2, 16), np.float32), 2, 2, 64, 100)    # input 2 of 2
    with pytest.raises(amd.ConvolutionPanic, match="out of range"):
        init([(0, 0), (2, 0)], np.zeros((2, 16), np.float32), 2, 2, 64, 100)    # output 2 of 2
    h2 = np.zeros((2, 16), np.float32)
    with pytest.raises(ValueError, match="strictly ascending"):                # the mirror's own check ...
        init([(1, 0), (0, 0)], h2, 2, 2, 64, 100)
    for bad in ([(1, 0), (0, 0)], [(0, 1), (0, 0)], [(0, 0), (0, 0)]):           # ... and the library's
        assert "not strictly ascending" in raw_init(amd, bad, h2, 2, 2, 64, 100)
    with pytest.raises(amd.ConvolutionPanic, match="max_response_length"):
        init([(0, 0)], np.zeros((1, 101), np.float32), 1, 1, 64, 100)           # response_len > L


def test_head_block_that_does_not_divide_T(amd):
    """head 48, L 3000, T 512: a one-pair handle fed 48-sample calls until one
    fails returns the statuses of the one-channel TwoStageFFTConvolver fed the
    same calls (tail_input runs past its end, src/fft_convolver.rs:459-460),
    and its successful outputs are within tolerance of that handle's."""
    head, L = 48, 3000
    h, x = make(84, [(0, 0)], 1, L, 12 * head)
    conv = amd.SparseMatrixTwoStageConvolver.init([(0, 0)], h, 1, 1, head, L)
    ref = amd.TwoStageFFTConvolver.init(h[0], head, L)
    assert conv.tail_block_size == ref.tail_block_size == 512

    def statuses(handle, feed):
        out, ys = [], []
        for k in range(12):
            assert conv.path(head) == 0
            try:
                ys.append(feed(handle, x[:, k * head:(k + 1) * head]))
                out.append("ok")
            except amd.ConvolutionPanic:
                out.append("panic")
                break
        return out, ys

    sa, ya = statuses(conv, lambda c, v: c.process(v)[0])
    sb, yb = statuses(ref, lambda c, v: c.process(v[0]))
    assert sa == sb and sa[-1] == "panic" and len(sa) == 11, (sa, sb)   # 10 * 48 = 480, 480 + 48 > 512
    assert_close(np.concatenate(ya), np.concatenate(yb), what="head 48")
