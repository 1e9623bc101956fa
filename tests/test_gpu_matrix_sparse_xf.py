"""SparseMatrixCrossfadeConvolver (include/fftconv.h): one
CrossfadeConvolver<FFTConvolver> instance per listed pair in lockstep, the mix
applied to the per-output sums.  Reference:
matrix_sp_xf_ref.SparseSummedCrossfadeOracle -- per output the f64 sum of the
oracle instances listed for it, fed the same calls and updates; tolerance
common.REL_TOL on max|got - ref| / max|ref| per output, is_crossfading after
every call, path() before every call (0 = composition, 1 = fused with both
convolvers live, 2 = fused with one idle).  The bitwise contracts: fused equals
composition, output o equals a dense MatrixCrossfadeConvolver over its k_o
pairs, update_pairs equals update(R'), process_device_steps equals the separate
calls, a clone continues identically, a pattern split by outputs gives the
same rows.  The shapes' walk properties are asserted on the CPU by
tests/test_matrix_sp_xf_ref.py."""
import functools

import numpy as np
import pytest
import torch

import oracle as oracle_module
from common import assert_close
from matrix_sp_ref import PATTERN_1, PATTERN_256, make, rows_of
from matrix_sp_xf_ref import SparseSummedCrossfadeOracle
from matrix_xf_ref import calls, run_script

pytestmark = pytest.mark.gpu


def new_handle(amd, pattern, h, I, O, B, L, mrl, mbs, fade, fused=True):
    conv = amd.SparseMatrixCrossfadeConvolver.new(amd.SparseMatrixConvolver.init(pattern, h, I, O, B, L), mrl, mbs, fade)
    assert (conv.inputs, conv.outputs, conv.pairs, conv.max_buffer_size) == (I, O, len(pattern), mbs)
    if not fused:
        conv.set_fused(False)
    return conv


class Scenario:
    """A pattern, its responses and input, and a script of updates and calls;
    the reference outputs are computed once and never written to."""

    def __init__(self, seed, pattern, I, O, B, L, mbs, fade, build, mrl=None):
        self.pattern, self.I, self.O, self.B, self.L, self.mbs, self.fade = pattern, I, O, B, L, mbs, fade
        self.mrl = L if mrl is None else mrl
        mk = lambda k, n=L: make(seed + k, pattern, I, n, 1)[0]
        self.script = build(mk)
        ncalls = sum(1 for kind, _ in self.script if kind == "call")
        self.h, self.x = make(seed, pattern, I, L, ncalls * mbs)
        ref = SparseSummedCrossfadeOracle(oracle_module, pattern, self.h, I, O, B, L, max_response_length=self.mrl,
                                          max_buffer_size=mbs, crossfade_samples=fade)
        self.ref, self.flags = run_script(ref, self.x, self.script, mbs, panic=oracle_module.OraclePanic)
        for a in [self.h, self.x] + self.ref:
            a.setflags(write=False)

    def handle(self, amd, fused=True):
        return new_handle(amd, self.pattern, self.h, self.I, self.O, self.B, self.L, self.mrl, self.mbs, self.fade, fused)

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
        for o, row in enumerate(rows_of(self.pattern, self.O)):
            if not row:
                assert not got[o].any(), f"{what}: output {o} has no pairs and is not zero"


MAIN = (PATTERN_1, 5, 4, 128, 2045)  # pattern, I, O, B, L (S 16)


@functools.lru_cache(maxsize=None)
def scenario(name):
    B = 128
    if name == "fade":      # 1: hold, fade and reached across one-block calls, then back towards A
        return Scenario(31, *MAIN, B, 3 * B // 2, lambda mk: calls(20, B) + [("update", mk(1))] + calls(12, B) +
                        [("update", mk(2))] + calls(8, B))
    if name == "ragged":    # 2: swaps land mid-block, output_len 200 and 75, the state advances by 200
        alt = lambda n: [("call", 200 if k % 2 == 0 else 75) for k in range(n)]
        return Scenario(32, *MAIN, 200, 500, lambda mk: alt(9) + [("update", mk(1))] + alt(9) +
                        [("update", mk(2))] + alt(6))
    if name == "pending":   # 3: two updates during one fade, one too long for the stored response (1200)
        return Scenario(33, *MAIN, B, 3 * B // 2, lambda mk: calls(5, B) + [("update", mk(1))] + calls(1, B) +
                        [("update", mk(2, 1000)), ("update_panics", mk(3, 1400)), ("update", mk(4, 1200))] +
                        calls(12, B), mrl=1200)
    if name == "split":     # 4: S 128, parts 10, 2, 1, 4; the second swap after A has idled for 133 > S + 2 blocks
        return Scenario(34, PATTERN_1, 5, 4, 32, 4096, 32, 40, lambda mk: calls(100, 32) + [("update", mk(1))] +
                        calls(136, 32) + [("update", mk(2))] + calls(12, 32))
    if name == "out-of-step":  # 10: an update to 300 samples changes B's active_seg_count for good
        return Scenario(36, *MAIN, B, 3 * B // 2, lambda mk: calls(4, B) + [("update", mk(1, 300))] + calls(6, B) +
                        [("update", mk(2, 300))] + calls(6, B) + [("update", mk(3))] + calls(6, B))
    if name == "empty":     # 10: an all-pairs empty response: that convolver's output is zero, its state freezes
        return Scenario(37, *MAIN, B, 3 * B // 2, lambda mk: calls(4, B) + [("update", mk(1, 0))] + calls(6, B) +
                        [("update", mk(2))] + calls(6, B) + [("update", mk(3))] + calls(6, B))
    if name.startswith("B"):   # 5: a swap after 3 blocks, a fade of B + 7 samples, calls of B - 24 and 24 at the end
        B, S = (int(v) for v in name[1:].split("-S"))
        L = 3 * B + 5 if S == 4 else S * B - 3
        return Scenario(38, PATTERN_256, 3, 2, B, L, B, B + 7, lambda mk: calls(3, B) + [("update", mk(1))] +
                        calls(4, B) + [("call", B - 24), ("call", 24)])
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
    for y in ys:
        assert not y[2].any()                     # the output without pairs, inside the fade too


def test_ragged(amd):
    sc = scenario("ragged")
    ys, flags, paths = gpu_run(amd, "ragged")
    sc.check(ys, flags, "ragged")
    assert set(paths) == {1, 2} and paths[9] == 1, paths


def test_pending(amd):
    """The second stored update overwrites the first, a longer one panics and
    changes nothing, the swap is applied by the first process() after the fade
    (path() already counts it); the stored response has 1200 samples, so that
    swap ends the in-step state."""
    sc = scenario("pending")
    assert sc.flags[5:8] == [True, True, False] and sc.flags[8], sc.flags
    ys, flags, paths = gpu_run(amd, "pending")
    sc.check(ys, flags, "pending")
    assert paths[:8] == [2] * 5 + [1] * 3, paths
    assert paths[8:] == [0] * (len(paths) - 8), paths


def test_split_rows_and_wrap(amd):
    sc = scenario("split")
    ys, flags, paths = gpu_run(amd, "split")
    sc.check(ys, flags, "split")
    assert set(paths) == {1, 2}, paths
    conv = amd.SparseMatrixConvolver.init(PATTERN_1, sc.h, 5, 4, 32, 4096)
    assert [conv.output_parts(o) for o in range(4)] == [10, 2, 1, 4] and conv.seg_count == 128


@pytest.mark.parametrize("name", ["B32-S4", "B128-S4", "B512-S4", "B2048-S4", "B4096-S4", "B8192-S4", "B512-S8"])
def test_block_sizes(amd, name):
    """Every supported block size runs fused; B 2048, 4096 and 8192 run the
    unrolled loop at two, four and eight slots per thread, B 512 with S 8 at
    one slot per thread without row groups."""
    sc = scenario(name)
    ys, flags, paths = sc.drive(amd, sc.handle(amd))
    sc.check(ys, flags, name)
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


@pytest.mark.parametrize("name", ["fade", "ragged", "split"])
def test_bitwise_against_the_dense_crossfade(amd, name):
    """Output o is, call by call, the single output of a dense
    MatrixCrossfadeConvolver with k_o inputs holding h[pair e], fed x[i_e]."""
    sc = scenario(name)
    ys, flags, _ = gpu_run(amd, name)
    for o, row in enumerate(rows_of(sc.pattern, sc.O)):
        if not row:
            continue
        ns, cols = [n for n, _ in row], [i for _, i in row]
        sub = lambda h: np.ascontiguousarray(np.asarray(h)[ns][None])  # [1][k_o][len]
        dense = amd.MatrixCrossfadeConvolver.new(amd.MatrixConvolver.init(sub(sc.h), sc.B, sc.L), sc.mrl, sc.mbs, sc.fade)
        script = [(kind, sub(arg)) if kind == "update" else (kind, arg) for kind, arg in sc.script]
        yd, fd = run_script(dense, np.ascontiguousarray(sc.x[cols]), script, sc.mbs)
        assert fd == flags
        for k, (u, v) in enumerate(zip(ys, yd)):
            assert np.array_equal(u[o], v[0]), (name, o, k, float(np.abs(u[o] - v[0]).max()))


@pytest.mark.parametrize("name", ["out-of-step", "empty"])
def test_out_of_step(amd, name):
    sc = scenario(name)
    ys, flags, paths = gpu_run(amd, name)
    sc.check(ys, flags, name)
    assert paths[:4] == [2] * 4 and set(paths[4:]) == {0}, paths


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
    assert (twin.inputs, twin.outputs, twin.pairs) == (conv.inputs, conv.outputs, conv.pairs)
    done = sum(1 for s in head if s[0] == "call")
    for h in (conv, twin):
        out, _ = run_script(h, sc.x[:, done * sc.mbs:], rest, sc.mbs)
        for k, y in enumerate(out):
            assert np.array_equal(y, ys[done + k]), k


def test_output_sharding_bitwise(amd):
    """One handle of PATTERN_1 against two handles of outputs 0..1 and 2..3,
    through a fade."""
    I, O, B, L = 5, 4, 128, 2045
    h, x = make(39, PATTERN_1, I, L, 16 * B)
    h2, _ = make(40, PATTERN_1, I, L, 1)
    script = calls(5, B) + [("update", None)] + calls(11, B)
    outs = []
    for lo, hi in ((0, 4), (0, 2), (2, 4)):
        ns = [n for n, (o, _) in enumerate(PATTERN_1) if lo <= o < hi]
        pat = [(PATTERN_1[n][0] - lo, PATTERN_1[n][1]) for n in ns]
        conv = new_handle(amd, pat, h[ns], I, hi - lo, B, L, L, B, 3 * B + 11)
        sub = [(k, h2[ns]) if k == "update" else (k, a) for k, a in script]
        ys, flags = run_script(conv, x, sub, B)
        assert flags[5] and not flags[-1]
        outs.append(np.concatenate(ys, axis=1))
    assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0
    assert np.array_equal(outs[0], np.concatenate(outs[1:], axis=0))


def test_init_form(amd):
    """The init form: the fade takes response_len = 300 samples, the hold min(64, 300)."""
    I, O, B, L = 5, 4, 64, 300
    h, x = make(41, PATTERN_1, I, L, 14 * B)
    h2, _ = make(42, PATTERN_1, I, L, 1)
    conv = amd.SparseMatrixCrossfadeConvolver.init(PATTERN_1, h, I, O, B, L)
    assert conv.max_buffer_size == B and conv.path() == 2 and not conv.is_crossfading()
    assert (conv.inputs, conv.outputs, conv.pairs) == (I, O, len(PATTERN_1))
    script = calls(6, B) + [("update", h2)] + calls(8, B)
    ref = SparseSummedCrossfadeOracle(oracle_module, PATTERN_1, h, I, O, B, L)
    yr, fr = run_script(ref, x, script, B)
    ys, flags = run_script(conv, x, script, B)
    assert fr == [False] * 6 + [True] * 5 + [False] * 3
    assert flags == fr
    got, want = np.concatenate(ys, axis=1), np.concatenate(yr, axis=1)
    for o in range(O):
        assert_close(got[o], want[o], what=f"init form output {o}")
    assert not got[2].any()


# ---- update_pairs equals update(R') -------------------------------------------

def pad(a, n):
    a = np.asarray(a, np.float32)
    out = np.zeros(a.shape[:-1] + (n,), np.float32)
    out[..., :a.shape[-1]] = a
    return out


class Pair:
    """The update_pairs handle, its update(R') twin, the oracle and the host
    model of the base set (the pending stored response, else the responses of
    the convolver the crossfader targets), driven in lockstep."""

    def __init__(self, amd, seed, ncalls, B=128, L=2045, mbs=None, fade=None, mrl=None, fused=True, pattern=PATTERN_1,
                 I=5, O=4):
        self.amd, self.pattern, self.I, self.O, self.B, self.L = amd, pattern, I, O, B, L
        self.mbs = B if mbs is None else mbs
        self.mrl = L if mrl is None else mrl
        fade = B + 7 if fade is None else fade
        self.seed, self.N = seed, len(pattern)
        self.h, self.x = make(seed, pattern, I, L, ncalls * self.mbs)
        self.conv, self.twin = (new_handle(amd, pattern, self.h, I, O, B, L, self.mrl, self.mbs, fade, fused)
                                for _ in range(2))
        self.ref = SparseSummedCrossfadeOracle(oracle_module, pattern, self.h, I, O, B, L, max_response_length=self.mrl,
                                               max_buffer_size=self.mbs, crossfade_samples=fade)
        self.cur, self.pending = self.h.copy(), None
        self.pos = 0
        self.got, self.want, self.paths = [], [], []
        assert self.conv.diff_pairs() == 0 and self.conv.last_patch() == (0, 0)

    def rows(self, k, n, length=None):
        """n fresh response rows"""
        length = self.L if length is None else length
        return make(self.seed + 100 + k, [(0, 0)] * n, 1, length, 1)[0]

    def _whole(self, R):
        fading = self.twin.is_crossfading()
        self.twin.update(R)
        self.ref.update(R)
        if fading:
            self.pending = pad(R, self.mrl)
        else:
            self.cur, self.pending = np.asarray(R, np.float32).copy(), None

    def whole(self, R):
        self.conv.update(R)
        self._whole(R)

    def r_prime(self, pairs, rows):
        base = self.pending if self.pending is not None else self.cur
        R = base.copy()
        for p, row in zip(pairs, rows):
            R[self.pattern.index(tuple(p))] = pad(row, R.shape[1])
        return R

    def partial(self, pairs, rows, how=None):
        """update_pairs on the handle (or how(conv)), update(R') on the twin and the oracle"""
        R = self.r_prime(pairs, rows)
        if how is None:
            self.conv.update_pairs(pairs, rows)
        else:
            how(self.conv)
        self._whole(R)
        return R

    def call(self, out_len=None, n=1):
        for _ in range(n):
            assert self.conv.path() == self.twin.path(), (len(self.got), self.conv.path(), self.twin.path())
            self.paths.append(self.conv.path())
            if self.pending is not None and not self.twin.is_crossfading():
                self.cur, self.pending = self.pending, None  # applied by this process()
            xs = self.x[:, self.pos:self.pos + self.mbs]
            self.pos += self.mbs
            y, yt = self.conv.process(xs, out_len), self.twin.process(xs, out_len)
            assert np.array_equal(y, yt), f"call {len(self.got)}: update_pairs differs from update(R')"
            self.got.append(y)
            self.want.append(self.ref.process(xs, out_len))
            assert self.conv.is_crossfading() == self.twin.is_crossfading() == self.ref.is_crossfading()

    def through_fade(self):
        """calls until the fade under way has ended, and one more"""
        n = 0
        while self.twin.is_crossfading():
            self.call()
            n += 1
            assert n < 64
        self.call()

    def finish(self, what):
        got, want = np.concatenate(self.got, axis=1), np.concatenate(self.want, axis=1)
        assert np.isfinite(got).all()
        for o in range(self.O):
            assert_close(got[o], want[o], what=f"{what} output {o}")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composition"])
def test_update_pairs_idle_swaps_and_bookkeeping(amd, fused):
    """8: idle swaps; last_patch is {n, 0} after init, a second list copies the
    first list's pairs minus its own, a whole update gives {N, 0}, then {n, N - n};
    a shorter response_len is zero-padded; update_input / update_output."""
    p = Pair(amd, 51, 40, fused=fused)
    N = p.N
    p.call(n=3)
    p.partial([(0, 1), (1, 2)], p.rows(1, 2))
    assert p.conv.last_patch() == (2, 0) and p.conv.diff_pairs() == 2 and p.conv.is_crossfading()
    p.through_fade()
    p.call(n=2)
    p.partial([(0, 1), (3, 4)], p.rows(2, 2, 1500))  # shorter rows: zero-padded to 2045
    assert p.conv.last_patch() == (2, 1) and p.conv.diff_pairs() == 2
    p.through_fade()
    p.whole(make(152, PATTERN_1, 5, 2045, 1)[0])
    assert p.conv.last_patch() == (N, 0) and p.conv.diff_pairs() == N
    p.through_fade()
    p.partial([(0, 0), (3, 0)], p.rows(3, 2))
    assert p.conv.last_patch() == (2, N - 2) and p.conv.diff_pairs() == 2
    p.through_fade()
    r = p.rows(4, 2)   # input 0 is read by outputs 0 and 3
    p.partial([(0, 0), (3, 0)], r, how=lambda c: c.update_input(0, r))
    assert p.conv.last_patch() == (2, 0)
    p.through_fade()
    r = p.rows(5, 5)   # output 0 lists five pairs
    p.partial([(0, i) for i in range(5)], r, how=lambda c: c.update_output(0, r))
    assert p.conv.last_patch() == (5, 1) and p.conv.diff_pairs() == 5  # (copied: (3, 0) of the list before)
    p.through_fade()
    p.finish("idle swaps")
    assert set(p.paths) == ({1, 2} if fused else {0}), p.paths


def pending_pair(amd, seed, mrl=None):
    # B 128, S 16, a fade of 3 calls after a hold of one
    p = Pair(amd, seed, 24, fade=300, mrl=mrl)
    p.call(n=2)
    p.partial([(0, 0)], p.rows(0, 1))
    p.call()
    assert p.conv.is_crossfading()
    return p


def after_pending(p, what):
    """the pending response is applied by the first process() after the fade, and path() says so beforehand"""
    n = 0
    while p.twin.is_crossfading():
        p.call()
        n += 1
        assert n < 64
    assert p.conv.path() == p.twin.path() == 1, (p.conv.path(), p.twin.path())  # (the pending swap counted)
    p.call()
    assert p.conv.is_crossfading()
    p.through_fade()
    p.call(n=2)
    p.finish(what)


def test_pending_two_partials_share_a_pair(amd):
    p = pending_pair(amd, 54)
    p.partial([(0, 1), (3, 4)], p.rows(1, 2))
    assert p.conv.last_patch() == (1, 0)  # (nothing applied yet)
    p.call()
    p.partial([(1, 2), (3, 4)], p.rows(2, 2, 1500))  # (3, 4) again, shorter: the later rows win
    after_pending(p, "two partials")
    assert p.conv.diff_pairs() == 3 and p.conv.last_patch() == (3, 1)


def test_pending_whole_then_partial(amd):
    p = pending_pair(amd, 55)
    p.whole(make(155, PATTERN_1, 5, 2045, 1)[0])
    p.partial([(0, 2), (1, 2)], p.rows(1, 2))
    after_pending(p, "whole then partial")
    assert p.conv.diff_pairs() == p.N and p.conv.last_patch() == (p.N, 0)


def test_pending_shared_whole_then_partial(amd):
    """a whole response given once for every pair (stride 0) is expanded before it is patched"""
    p = pending_pair(amd, 56)
    one = p.rows(7, 1)[0]
    R = np.broadcast_to(one, (p.N, p.L)).copy()
    rc = p.amd.lib().fftconv_matrix_sparse_crossfade_update(p.conv._h, one.ctypes.data_as(p.amd._fp), p.L, 0)
    assert rc == 0
    p._whole(R)
    p.partial([(1, 2)], p.rows(1, 1))
    after_pending(p, "shared whole then partial")


def test_pending_partial_then_whole(amd):
    p = pending_pair(amd, 57)
    p.partial([(0, 2), (1, 2)], p.rows(1, 2))
    p.whole(make(157, PATTERN_1, 5, 2045, 1)[0])
    after_pending(p, "partial then whole")
    assert p.conv.diff_pairs() == p.N and p.conv.last_patch() == (p.N, 0)


def test_pending_unsupported_length(amd):
    """The stored length gives another active segment count than the base
    convolver's: FFTCONV_E_UNSUPPORTED, and the handle goes on as a twin that
    never received the call."""
    p = pending_pair(amd, 59, mrl=200)  # ceil(200 / 128) = 2, the convolvers have 16 active segments
    with pytest.raises(amd.DeviceError, match=r"status -3"):
        p.conv.update_pairs([(0, 1)], p.rows(1, 1, 200))
    p.through_fade()
    p.call(n=3)
    p.finish("unsupported")


def test_device_variant(amd):
    """Rows from a torch tensor with stride > len, on a non-default stream, a shorter len that is zero-padded."""
    p = Pair(amd, 60, 20)
    p.call(n=3)
    pairs, n, stride = [(0, 2), (1, 2), (3, 0)], 1000, 1536
    rows = p.rows(1, 3, n)
    t = torch.zeros((3, stride), dtype=torch.float32, device="cuda")
    t[:, :n] = torch.from_numpy(rows).cuda()
    t[:, n:] = 7.0  # (never read)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    p.partial(pairs, rows, how=lambda c: c.update_pairs_device(pairs, t.data_ptr(), n, stride, s.cuda_stream))
    assert p.conv.last_patch() == (3, 0)
    p.call()
    # during the fade: the rows go to the stored response
    p.partial(pairs[:2], rows[:2], how=lambda c: c.update_pairs_device(pairs[:2], t.data_ptr(), n, stride, s.cuda_stream))
    p.through_fade()
    p.through_fade()
    p.finish("device rows")
    s.synchronize()


def test_partial_swap_changes_the_active_segment_count(amd):
    """A partial swap that changes the target convolver's active_seg_count
    rebuilds its plan: after a whole update to 300 samples (B: 16 -> 3) a
    partial swap takes A from 16 to 3; after a whole update back to the full
    length (B: 3 -> 16) a partial swap at full length takes A from 3 to 16."""
    p = Pair(amd, 63, 30)
    p.call(n=2)
    p.whole(make(163, PATTERN_1, 5, 300, 1)[0])
    p.through_fade()
    p.partial([(0, 3), (3, 4)], p.rows(1, 2, 300))      # A: 16 -> 3 active segments
    assert p.conv.last_patch() == (2, p.N - 2)
    p.through_fade()
    p.call(n=2)
    p.whole(make(164, PATTERN_1, 5, 2045, 1)[0])        # B: 3 -> 16
    p.through_fade()
    p.partial([(0, 0), (1, 2)], p.rows(2, 2))           # A: 3 -> 16, at the full length
    assert p.conv.last_patch() == (2, p.N - 2)
    p.through_fade()
    p.call(n=3)
    p.finish("active change")
    assert p.paths[:2] == [2, 2] and set(p.paths[2:]) == {0}, p.paths  # (out of step from the first update on)


def test_errors_leave_the_handle_unchanged(amd):
    """9: a pair absent from the pattern, a pair in the pair-less output, a
    descending, a repeated and an out-of-range list, len > len', reset and the
    process lengths raise and change nothing; an empty list is update(base)."""
    p = Pair(amd, 61, 20)
    p.call(n=2)
    p.partial([(0, 1)], p.rows(1, 1, 1500))
    p.through_fade()
    r = p.rows(2, 2, 1500)
    for pairs in ([(0, 1), (1, 0)], [(1, 1)], [(2, 0)], [(0, 1), (2, 4)]):
        with pytest.raises(amd.ConvolutionPanic, match="is not in the pattern"):
            p.conv.update_pairs(pairs, r[:len(pairs)])
    for pairs in ([(3, 0), (0, 1)], [(0, 1), (0, 1)], [(0, 5)], [(4, 0)], [(0, 2), (0, 1)]):
        with pytest.raises(amd.ConvolutionPanic):
            p.conv.update_pairs(pairs, r[:len(pairs)])
    with pytest.raises(amd.NotImplementedInReference):
        p.conv.reset()
    with pytest.raises(amd.ConvolutionPanic):
        p.conv.process(p.x[:, :p.mbs - 1], p.mbs - 1)
    with pytest.raises(amd.ConvolutionPanic):
        p.conv.process(p.x[:, :p.mbs + 1], p.mbs + 1)
    assert not p.conv.is_crossfading() and p.conv.diff_pairs() == 1 and p.conv.last_patch() == (1, 0)
    p.call(n=2)
    # after a whole update of 1500 samples len' = 1500
    p.whole(make(161, PATTERN_1, 5, 1500, 1)[0])
    p.through_fade()
    with pytest.raises(amd.ConvolutionPanic):
        p.conv.update_pairs([(0, 0)], p.rows(3, 1, 1501))
    assert not p.conv.is_crossfading() and p.conv.diff_pairs() == p.N
    p.call(n=2)
    p.partial([], np.zeros((0, 0), np.float32))
    assert p.conv.is_crossfading() and p.conv.last_patch() == (0, p.N) and p.conv.diff_pairs() == 0
    p.through_fade()
    p.finish("errors")


def test_clone_with_a_partial_update_pending(amd):
    """12: a clone taken with a partial update pending and D non-empty continues bit-identically."""
    p = pending_pair(amd, 62)
    p.partial([(0, 1), (3, 4)], p.rows(1, 2))
    assert p.conv.diff_pairs() == 1
    c = p.conv.clone()
    assert c.diff_pairs() == 1 and c.last_patch() == p.conv.last_patch()
    pos = p.pos
    for _ in range(10):
        assert c.path() == p.conv.path()
        p.call()
        y = c.process(p.x[:, pos:pos + p.mbs])
        pos += p.mbs
        assert np.array_equal(y, p.got[-1])
        assert c.is_crossfading() == p.conv.is_crossfading()
        assert c.diff_pairs() == p.conv.diff_pairs() and c.last_patch() == p.conv.last_patch()
    assert p.conv.last_patch() == (2, 1)
    p.finish("clone")
