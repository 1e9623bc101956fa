"""MatrixCrossfadeConvolver (include/fftconv.h): inputs x outputs
CrossfadeConvolver<FFTConvolver> instances in lockstep, the mix applied to the
per-output sums.  Reference: matrix_xf_ref.SummedCrossfadeOracle -- per output
the f64 sum of oracle CrossfadeConvolver instances fed the same calls and
updates (tests/test_matrix_xf_ref.py puts the device's order of operations
6.7e-8 to 7.7e-8 from it); tolerance common.REL_TOL on max|got - ref| /
max|ref| per output, and is_crossfading after every call.  path(): 0 =
composition, 1 = fused with both convolvers live, 2 = fused with one idle."""
import functools

import numpy as np
import pytest
import torch

import oracle as oracle_module
from common import assert_close
from matrix_ref import make
from matrix_xf_ref import SummedCrossfadeOracle, calls, run_script

pytestmark = pytest.mark.gpu


class Scenario:
    """A geometry, its responses and input, and a script of updates and calls;
    the reference outputs are computed once and never written to."""

    def __init__(self, seed, I, O, B, L, mbs, fade, build, mrl=None):
        self.I, self.O, self.B, self.L, self.mbs, self.fade = I, O, B, L, mbs, fade
        self.mrl = L if mrl is None else mrl
        mk = lambda k, n=L: make(seed + k, I, O, n, 1)[0]
        self.script = build(mk)
        ncalls = sum(1 for kind, _ in self.script if kind == "call")
        self.h, self.x = make(seed, I, O, L, ncalls * mbs)
        ref = SummedCrossfadeOracle(oracle_module, self.h, B, L, max_response_length=self.mrl, max_buffer_size=mbs,
                                    crossfade_samples=fade)
        self.ref, self.flags = run_script(ref, self.x, self.script, mbs, panic=oracle_module.OraclePanic)
        for a in [self.h, self.x] + self.ref:
            a.setflags(write=False)

    def handle(self, amd, fused=True):
        conv = amd.MatrixCrossfadeConvolver.new(amd.MatrixConvolver.init(self.h, self.B, self.L), self.mrl, self.mbs,
                                                self.fade)
        assert (conv.inputs, conv.outputs, conv.max_buffer_size) == (self.I, self.O, self.mbs)
        if not fused:
            conv.set_fused(False)
        return conv

    def drive(self, amd, conv):
        """(outputs of every call, is_crossfading after every call, path() before every call)"""
        paths = []
        ys, flags = run_script(conv, self.x, self.script, self.mbs, panic=amd.ConvolutionPanic,
                               before_call=lambda k: paths.append(conv.path()))
        return ys, flags, paths

    def check(self, ys, flags, what):
        assert flags == self.flags, (what, flags, self.flags)
        assert [y.shape for y in ys] == [r.shape for r in self.ref]
        got, ref = np.concatenate(ys, axis=1), np.concatenate(self.ref, axis=1)
        assert np.isfinite(got).all()
        for o in range(self.O):
            assert_close(got[o], ref[o], what=f"{what} output {o}")


@functools.lru_cache(maxsize=None)
def scenario(name):
    if name == "fade":      # 1: hold, fade and reached across one-block calls, then back towards A
        return Scenario(31, 3, 2, 64, 1000, 64, 96, lambda mk: calls(20, 64) + [("update", mk(1))] + calls(12, 64) +
                        [("update", mk(2))] + calls(8, 64))
    if name == "ragged":    # 2: swaps land mid-block, output_len 100 and 37, the state advances by 100
        alt = lambda n: [("call", 100 if k % 2 == 0 else 37) for k in range(n)]
        return Scenario(32, 3, 2, 64, 1000, 100, 250, lambda mk: alt(9) + [("update", mk(1))] + alt(9) +
                        [("update", mk(2))] + alt(6))
    if name == "pending":   # 3: two updates during one fade, one too long for the stored response (600)
        return Scenario(33, 3, 2, 64, 1000, 64, 96, lambda mk: calls(5, 64) + [("update", mk(1))] + calls(1, 64) +
                        [("update", mk(2, 500)), ("update_panics", mk(3, 700)), ("update", mk(4, 600))] +
                        calls(12, 64), mrl=600)
    if name == "split":     # 4: S = 128, P >= 2; a swap at block 100, and one after A has idled for 133 > S + 2 blocks
        return Scenario(34, 4, 2, 32, 4096, 32, 40, lambda mk: calls(100, 32) + [("update", mk(1))] + calls(136, 32) +
                        [("update", mk(2))] + calls(12, 32))
    if name == "one-part":  # 4: 3 rows per output, one part
        return Scenario(35, 1, 2, 64, 200, 64, 50, lambda mk: calls(6, 64) + [("update", mk(1))] + calls(8, 64))
    if name == "out-of-step":  # 7: an update to 300 samples changes B's active_seg_count for good
        return Scenario(36, 3, 2, 64, 1000, 64, 96, lambda mk: calls(4, 64) + [("update", mk(1, 300))] + calls(6, 64) +
                        [("update", mk(2, 300))] + calls(6, 64) + [("update", mk(3))] + calls(6, 64))
    if name == "empty":     # 7: an all-pairs empty response: that convolver's output is zero, its state freezes
        return Scenario(37, 3, 2, 64, 1000, 64, 96, lambda mk: calls(4, 64) + [("update", mk(1, 0))] + calls(6, 64) +
                        [("update", mk(2))] + calls(6, 64) + [("update", mk(3))] + calls(6, 64))
    if name.startswith("B"):   # 5: a swap after 3 blocks, a fade of B + 7 samples, calls of B - 24 and 24 at the end
        B = int(name[1:])
        return Scenario(38, 2, 2, B, 3 * B + 5, B, B + 7, lambda mk: calls(3, B) + [("update", mk(1))] + calls(4, B) +
                        [("call", B - 24), ("call", 24)])
    raise KeyError(name)


_runs = {}


def gpu_run(amd, name, fused=True):
    """the scenario on a fresh handle, once per (scenario, fused)"""
    if (name, fused) not in _runs:
        sc = scenario(name)
        _runs[name, fused] = sc.drive(amd, sc.handle(amd, fused))
    return _runs[name, fused]


def test_fade_across_calls(amd):
    sc = scenario("fade")
    ys, flags, paths = gpu_run(amd, "fade")
    sc.check(ys, flags, "fade")
    assert any(flags) and not flags[-1]
    assert paths[:20] == [2] * 20, paths          # before the first update: B idle
    assert paths[20:23] == [1, 1, 1], paths       # hold, fade, and the call in which the fade completes
    assert paths[23:32] == [2] * 9, paths         # reached B: A idle
    assert paths[32] == 1 and paths[-1] == 2, paths


def test_ragged(amd):
    sc = scenario("ragged")
    ys, flags, paths = gpu_run(amd, "ragged")
    sc.check(ys, flags, "ragged")
    assert set(paths) == {1, 2} and paths[9] == 1, paths


def test_pending(amd):
    """The second stored update overwrites the first, a longer one panics and
    changes nothing, the swap is applied by the first process() after the fade
    (path() already counts it); the stored response has 600 samples, so that
    swap ends the in-step state."""
    sc = scenario("pending")
    assert sc.flags[5:8] == [True, True, False] and sc.flags[8], sc.flags
    ys, flags, paths = gpu_run(amd, "pending")
    sc.check(ys, flags, "pending")
    assert paths[:8] == [2] * 5 + [1] * 3, paths
    assert paths[8:] == [0] * (len(paths) - 8), paths


def test_split_rows_and_wrap(amd):
    for name in ("split", "one-part"):
        sc = scenario(name)
        ys, flags, paths = gpu_run(amd, name)
        sc.check(ys, flags, name)
        assert set(paths) == {1, 2}, paths
    conv = amd.MatrixConvolver.init(scenario("split").h, 32, 4096)
    assert conv.mac_parts >= 2 and conv.seg_count == 128


@pytest.mark.parametrize("B", [32, 128, 512, 2048, 8192])
def test_block_sizes(amd, B):
    """Every supported block size runs fused (fftconv.h: the finish kernel
    needs no more LDS than the plain matrix's)."""
    sc = scenario(f"B{B}")
    ys, flags, paths = sc.drive(amd, sc.handle(amd))
    sc.check(ys, flags, f"B={B}")
    assert flags[3:6] == [True, True, False], flags
    assert paths == [2] * 3 + [1] * 3 + [2] * 3, paths


@pytest.mark.parametrize("name", ["fade", "ragged", "split"])
def test_fused_equals_composition_bitwise(amd, name):
    ys, flags, paths = gpu_run(amd, name)
    yc, fc, pc = gpu_run(amd, name, fused=False)
    assert set(pc) == {0} and set(paths) == {1, 2}
    assert flags == fc
    for k, (u, v) in enumerate(zip(ys, yc)):
        assert np.array_equal(u, v), (name, k, paths[k], float(np.abs(u - v).max()))


@pytest.mark.parametrize("name", ["fade", "ragged"])
def test_device_steps_equal_separate_calls(amd, name):
    """process_device_steps over the calls between two updates against the
    host calls, fused and composition: the same bits."""
    sc = scenario(name)
    ys, _, _ = gpu_run(amd, name)
    m = sc.mbs
    xd = torch.from_numpy(sc.x.copy()).to("cuda:0")
    for fused in (True, False):
        conv = sc.handle(amd, fused)
        k = 0
        while k < len(sc.script):
            kind, arg = sc.script[k]
            if kind == "update":
                conv.update(arg)
                k += 1
                continue
            run = 1  # consecutive calls of one output length
            while k + run < len(sc.script) and sc.script[k + run] == (kind, arg):
                run += 1
            c0 = sum(1 for s in sc.script[:k] if s[0] == "call")
            yd = torch.zeros((sc.O, run * m), dtype=torch.float32, device="cuda:0")
            conv.process_device_steps(xd.data_ptr() + 4 * c0 * m, sc.x.shape[1], m, yd.data_ptr(), run * m, m, arg, run, 0)
            got = yd.cpu().numpy().reshape(sc.O, run, m)
            for j in range(run):
                assert np.array_equal(got[:, j, :arg], ys[c0 + j]), (name, fused, c0 + j)
                assert not got[:, j, arg:].any()
            k += run


def test_clone_mid_fade(amd):
    sc = scenario("fade")
    ys, _, _ = gpu_run(amd, "fade")
    conv = sc.handle(amd)
    head, rest = sc.script[:23], sc.script[23:]  # 20 calls, the update, the hold call and one call of the fade
    run_script(conv, sc.x, head, sc.mbs)
    twin = conv.clone()
    assert conv.is_crossfading() and twin.is_crossfading() and twin.path() == conv.path() == 1
    done = sum(1 for s in head if s[0] == "call")
    for h in (conv, twin):
        out, _ = run_script(h, sc.x[:, done * sc.mbs:], rest, sc.mbs)
        for k, y in enumerate(out):
            assert np.array_equal(y, ys[done + k]), k


@pytest.mark.parametrize("name", ["out-of-step", "empty"])
def test_out_of_step(amd, name):
    sc = scenario(name)
    ys, flags, paths = gpu_run(amd, name)
    sc.check(ys, flags, name)
    assert paths[:4] == [2] * 4 and set(paths[4:]) == {0}, paths


def test_output_sharding_bitwise(amd):
    """One handle of 6 outputs against two handles of outputs 0..2 and 3..5,
    through a fade."""
    I, O, B, L = 3, 6, 64, 2000
    h, x = make(39, I, O, L, 16 * B)
    h2, _ = make(40, I, O, L, 1)
    script = calls(5, B) + [("update", None)] + calls(11, B)
    outs = []
    for lo, hi in ((0, 6), (0, 3), (3, 6)):
        conv = amd.MatrixCrossfadeConvolver.new(amd.MatrixConvolver.init(h[lo:hi], B, L), L, B, 3 * B + 11)
        sub = [(k, h2[lo:hi]) if k == "update" else (k, a) for k, a in script]
        ys, flags = run_script(conv, x, sub, B)
        assert flags[5] and not flags[-1]
        outs.append(np.concatenate(ys, axis=1))
    assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0
    assert np.array_equal(outs[0], np.concatenate(outs[1:], axis=0))


def test_errors_and_init_form(amd):
    I, O, B, L = 2, 2, 64, 300
    h, x = make(41, I, O, L, 14 * B)
    h2, _ = make(42, I, O, L, 1)
    conv = amd.MatrixCrossfadeConvolver.init(h, B, L)
    assert conv.max_buffer_size == B and conv.path() == 2 and not conv.is_crossfading()
    with pytest.raises(amd.NotImplementedInReference):
        conv.reset()
    with pytest.raises(amd.ConvolutionPanic):
        conv.process(x[:, :B - 1], B - 1)
    with pytest.raises(amd.ConvolutionPanic):
        conv.process(x[:, :B + 1], B + 1)
    # the init form: the fade takes response_len = 300 samples, the hold min(64, 300)
    script = calls(6, B) + [("update", h2)] + calls(8, B)
    ref = SummedCrossfadeOracle(oracle_module, h, B, L)
    yr, fr = run_script(ref, x, script, B)
    ys, flags = run_script(conv, x, script, B)
    assert fr == [False] * 6 + [True] * 5 + [False] * 3
    assert flags == fr
    got, want = np.concatenate(ys, axis=1), np.concatenate(yr, axis=1)
    for o in range(O):
        assert_close(got[o], want[o], what=f"init form output {o}")
