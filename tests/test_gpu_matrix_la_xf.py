"""MatrixLookaheadCrossfadeConvolver (include/fftconv.h): the
MatrixCrossfadeConvolver's definition over two MatrixLookaheadConvolvers.
Reference: matrix_xf_ref.SummedCrossfadeOracle fed the same calls and updates,
tolerance common.REL_TOL on max|got - ref| / max|ref| per output (4j and 4n put
the device's order of operations 7.7e-8 and 2.9e-7 from their references), and
is_crossfading after every call.  Everything else is bitwise: fused against
composition, windows against full sums, the handle against a
MatrixLookaheadConvolver, steps, clones, shards, update_pairs against update,
the load policy, poisoned buffers.  The scenarios are matrix_la_xf_ref's;
tests/test_matrix_la_xf_ref.py proves on the CPU what each is there for, and its
model gives the expected path() and anchors() sequences."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle as oracle_module
from common import assert_close
from matrix_la_ref import MAIN, Q
from matrix_la_xf_ref import SCENARIOS, model
from matrix_ref import make
from matrix_xf_ref import SummedCrossfadeOracle, calls, run_script

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "matrix_la_xf_poison_worker.py")
CHILD_TIMEOUT = 240  # seconds, as tests/test_gpu_poison.py: a cold process, three handles, 242 calls

MAIN_SCRIPTS = ("fade", "ragged", "pending", "long-idle")
BLOCK_SIZES = ("B32", "B128", "B256", "B512")
FEW_SEGMENTS = ("S1", "S2", "S8", "S9")
OUT_OF_STEP = ("out-of-step", "empty")
ALL = MAIN_SCRIPTS + BLOCK_SIZES + FEW_SEGMENTS + OUT_OF_STEP


class Scenario:
    """A geometry, its responses and input, and a script of updates and calls;
    the reference outputs are computed once and never written to."""

    def __init__(self, name):
        seed, (I, O, B, L), mbs, fade, build, mrl = SCENARIOS[name]
        self.I, self.O, self.B, self.L, self.mbs, self.fade = I, O, B, L, mbs, fade
        self.mrl = L if mrl is None else mrl
        self.script = build(lambda k, n=L: make(seed + k, I, O, n, 1)[0])
        self.ncalls = sum(1 for kind, _ in self.script if kind == "call")
        self.h, self.x = make(seed, I, O, L, self.ncalls * mbs)
        ref = SummedCrossfadeOracle(oracle_module, self.h, B, L, max_response_length=self.mrl, max_buffer_size=mbs,
                                    crossfade_samples=fade)
        self.ref, self.flags = run_script(ref, self.x, self.script, mbs, panic=oracle_module.OraclePanic)
        for a in [self.h, self.x] + self.ref:
            a.setflags(write=False)

    def handle(self, amd, fused=True, windows=True):
        conv = amd.MatrixLookaheadCrossfadeConvolver.new(amd.MatrixLookaheadConvolver.init(self.h, self.B, self.L),
                                                         self.mrl, self.mbs, self.fade)
        assert (conv.inputs, conv.outputs, conv.max_buffer_size) == (self.I, self.O, self.mbs)
        if not fused:
            conv.set_fused(False)
        if not windows:
            conv.set_windows(False)
        return conv

    def drive(self, amd, conv):
        """(outputs of every call, is_crossfading after every call, path() before
        every call, (anchors(0), anchors(1)) before every call)"""
        paths, anchors = [], []

        def before(k):
            paths.append(conv.path())
            anchors.append((conv.anchors(0), conv.anchors(1)))

        ys, flags = run_script(conv, self.x, self.script, self.mbs, panic=amd.ConvolutionPanic, before_call=before)
        return ys, flags, paths, anchors

    def check(self, ys, flags, what):
        assert flags == self.flags, (what, flags, self.flags)
        assert [y.shape for y in ys] == [r.shape for r in self.ref]
        got, ref = np.concatenate(ys, axis=1), np.concatenate(self.ref, axis=1)
        assert np.isfinite(got).all() and np.abs(got).max() > 0
        for o in range(self.O):
            assert_close(got[o], ref[o], what=f"{what} output {o}")


@functools.lru_cache(maxsize=None)
def scenario(name):
    return Scenario(name)


_runs = {}


def gpu_run(amd, name, fused=True, windows=True):
    """the scenario on a fresh handle, once per (scenario, fused, windows)"""
    key = (name, fused, windows)
    if key not in _runs:
        sc = scenario(name)
        _runs[key] = sc.drive(amd, sc.handle(amd, fused, windows))
    return _runs[key]


def same_bits(ys, yc, what):
    assert len(ys) == len(yc)
    for k, (u, v) in enumerate(zip(ys, yc)):
        assert np.array_equal(u, v), (what, k, float(np.abs(u - v).max()))


# ---- 1: oracle parity ---------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_oracle_parity(amd, name):
    sc = scenario(name)
    ys, flags, _, _ = gpu_run(amd, name)
    sc.check(ys, flags, name)
    assert any(flags) and not flags[-1]


# ---- 2: paths -----------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_paths(amd, name):
    _, _, paths, _ = gpu_run(amd, name)
    assert paths == model(name).paths, (name, paths)
    if name == "fade":   # 64 hold + 1536 fade samples: 25 one-block calls with both convolvers live
        assert paths == [2] * 20 + [1] * 25 + [2] * 15 + [1] * 25 + [2] * 5, paths
    elif name == "pending":
        assert paths == [2] * 5 + [1] * 3 + [0] * 10, paths
    elif name in OUT_OF_STEP:
        assert paths[:4] == [2] * 4 and set(paths[4:]) == {0}, paths
    else:
        assert set(paths) == {1, 2}, paths
    _, _, pc, _ = gpu_run(amd, name, fused=False)
    assert set(pc) == {0}


# ---- 3: windows actually run ---------------------------------------------------
def test_windows_run(amd):
    """One-block calls, so call k is block k: anchors(h, c) before call k is the
    number of outputs the model has anchoring in block k for a live convolver,
    and 0 for an idle one."""
    _, _, paths, anchors = gpu_run(amd, "fade")
    m = model("fade")
    want = [[0, 0] for _ in paths]
    for r in m.blocks:
        want[r["t"]][r["c"]] = sum(1 for x in r["roles"] if x == "anchor")
    assert [list(a) for a in anchors] == want
    # both convolvers anchor in the same launch somewhere inside the long fade
    assert any(a > 0 and b > 0 and p == 1 for (a, b), p in zip(anchors, paths))
    # an idle convolver reports 0: B before the first update, A after the first fade
    assert all(b == 0 for (a, b) in anchors[:20]) and all(a > 0 for (a, b) in anchors[:20])
    assert all(a == 0 for (a, b) in anchors[45:60]) and all(b > 0 for (a, b) in anchors[45:60])
    # right after the swap the new convolver has no valid window to read: for Q - 1 blocks some of its outputs
    # sum in full beside the anchors it makes, from then on every output is served or anchors
    new = [r for r in m.blocks if r["c"] == 1 and 20 <= r["t"] < 45]
    assert all("full" in r["roles"] for r in new[:Q - 1]) and not any("full" in r["roles"] for r in new[Q - 1:])


# ---- 4: fused equals composition ------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_fused_equals_composition_bitwise(amd, name):
    ys, flags, _, _ = gpu_run(amd, name)
    yc, fc, _, _ = gpu_run(amd, name, fused=False)
    assert flags == fc
    same_bits(ys, yc, name)


# ---- 5: windows equal full sums -------------------------------------------------
@pytest.mark.parametrize("name", ["fade", "ragged", "long-idle"])
def test_windows_equal_full_sums_bitwise(amd, name):
    ys, flags, paths, _ = gpu_run(amd, name)
    yf, ff, pf, af = gpu_run(amd, name, windows=False)
    assert (flags, paths) == (ff, pf) and not any(a or b for a, b in af)
    same_bits(ys, yf, name)


# ---- 6, 7: against the MatrixLookaheadConvolver ---------------------------------
def test_never_updated_handle_is_the_lookahead_matrix(amd):
    I, O, B, L = MAIN
    mbs = 100
    script = [("call", 100 if k % 3 else 37) for k in range(24)]
    h, x = make(70, I, O, L, len(script) * mbs)
    plain = amd.MatrixLookaheadConvolver.init(h, B, L)
    conv = amd.MatrixLookaheadCrossfadeConvolver.new(plain, L, mbs, 500)
    ys, flags = run_script(conv, x, script, mbs)
    assert not any(flags) and conv.path() == 2
    for k, (_, n) in enumerate(script):
        want = plain.process(x[:, k * mbs:(k + 1) * mbs])
        assert np.array_equal(ys[k], want[:, :n]), k
    assert np.abs(ys[-1]).max() > 0


@pytest.mark.parametrize("name", ["fade", "ragged"])
def test_after_a_fade_it_is_the_updated_lookahead_matrix(amd, name):
    """Once a fade has ended every later sample is the target convolver's: a
    MatrixLookaheadConvolver that got the same update at the same call boundary
    ("fade": on a block boundary, "ragged": mid-block)."""
    sc = scenario(name)
    ys, flags, _, _ = gpu_run(amd, name)
    plain = amd.MatrixLookaheadConvolver.init(sc.h, sc.B, sc.L)
    k, fading, updates, compared = 0, False, 0, 0
    for kind, arg in sc.script:
        if kind == "update":
            plain.update(arg)
            fading, updates = True, updates + 1
            continue
        want = plain.process(sc.x[:, k * sc.mbs:(k + 1) * sc.mbs])
        if not fading:   # (no fade yet, or it ended in an earlier call)
            assert np.array_equal(ys[k], want[:, :arg]), (name, k)
            compared += updates > 0
        fading = flags[k]
        k += 1
    assert compared >= 10 and updates == 2
    if name == "ragged":
        assert (9 * sc.mbs) % sc.B and (39 * sc.mbs) % sc.B   # both swaps land mid-block


# ---- 8: steps -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fade", "ragged"])
def test_device_steps_equal_separate_calls(amd, name):
    sc = scenario(name)
    ys, _, _, _ = gpu_run(amd, name)
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


# ---- 9: clone -------------------------------------------------------------------
def test_clone_mid_fade_and_mid_window(amd):
    """After 20 calls, the update and 12 calls of the fade: A is served from
    windows, B has anchored some outputs and sums others in full."""
    sc = scenario("fade")
    ys, _, _, anchors = gpu_run(amd, "fade")
    conv = sc.handle(amd)
    head, rest = sc.script[:33], sc.script[33:]
    run_script(conv, sc.x, head, sc.mbs)
    twin = conv.clone()
    assert conv.is_crossfading() and twin.is_crossfading() and twin.path() == conv.path() == 1
    assert (twin.anchors(0), twin.anchors(1)) == (conv.anchors(0), conv.anchors(1)) == anchors[32]
    done = sum(1 for s in head if s[0] == "call")
    for h in (conv, twin):
        out, _ = run_script(h, sc.x[:, done * sc.mbs:], rest, sc.mbs)
        same_bits(out, ys[done:], "clone")


# ---- 10: sharding -----------------------------------------------------------------
def test_output_sharding_bitwise(amd):
    """One handle of 10 outputs against two of outputs 0..2 and 3..9: output 3
    anchors on t = 3 (mod Q) in the whole matrix and on t = 0 in its shard."""
    I, O, B, L = MAIN
    h, x = make(71, I, O, L, 46 * B)
    h2, _ = make(72, I, O, L, 1)
    script = calls(12, B) + [("update", None)] + calls(34, B)
    outs = []
    for lo, hi in ((0, 10), (0, 3), (3, 10)):
        conv = amd.MatrixLookaheadCrossfadeConvolver.new(amd.MatrixLookaheadConvolver.init(h[lo:hi], B, L), L, B, 12 * B + 11)
        sub = [(k, h2[lo:hi]) if k == "update" else (k, a) for k, a in script]
        ys, flags = run_script(conv, x, sub, B)
        assert flags[12] and not flags[-1]
        outs.append(np.concatenate(ys, axis=1))
    assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0
    assert np.array_equal(outs[0], np.concatenate(outs[1:], axis=0))


# ---- 11: update_pairs ---------------------------------------------------------------
def test_update_pairs_equal_update_bitwise(amd):
    """update_pairs(list, rows), update_input and update_output against
    update(R') on a second handle: the same bits in every call, through three
    fades; last_patch() = (listed, copied = |D minus the list|)."""
    I, O, B, L = MAIN
    fade, per = 10 * B, 16
    h, x = make(73, I, O, L, 4 * per * B)
    new, _ = make(74, I, O, L, 1)
    new2, _ = make(75, I, O, L - 40, 1)
    mk = lambda: amd.MatrixLookaheadCrossfadeConvolver.new(amd.MatrixLookaheadConvolver.init(h, B, L), L, B, fade)
    a, b = mk(), mk()
    pos = [0]

    def run(n):
        for _ in range(n):
            blk = x[:, pos[0]:pos[0] + B]
            ya, yb = a.process(blk), b.process(blk)
            assert np.array_equal(ya, yb), pos[0] // B
            assert a.is_crossfading() == b.is_crossfading() and a.path() == b.path() != 0
            assert (a.anchors(0), a.anchors(1)) == (b.anchors(0), b.anchors(1))
            pos[0] += B
        assert np.abs(ya).max() > 0

    run(per)
    assert b.diff_pairs() == 0 and b.last_patch() == (0, 0)
    held = h.copy()
    pairs = [(0, 1), (3, 0), (3, 2), (9, 2)]
    rows = np.stack([new[o, i] for o, i in pairs])
    for (o, i), r in zip(pairs, rows):
        held[o, i] = r
    a.update(held)
    b.update_pairs(pairs, rows)
    assert a.last_patch() == (I * O, 0) and b.last_patch() == (4, 0) and b.diff_pairs() == 4
    run(per)
    assert not b.is_crossfading()
    # every pair that reads input 1, at a shorter length: zero-padded to the held set's
    rows = np.stack([new2[o, 1] for o in range(O)])
    held = held.copy()
    held[:, 1, :] = 0
    held[:, 1, :L - 40] = rows
    a.update(held)
    b.update_input(1, rows)
    assert b.last_patch() == (O, 3) and b.diff_pairs() == O
    run(per)
    rows = np.stack([new[9, i] for i in range(I)])
    held = held.copy()
    held[9] = rows
    a.update(held)
    b.update_output(9, rows)
    assert b.last_patch() == (I, O - 1) and b.diff_pairs() == I
    run(per)
    # the errors of the dense crossfade's update_pairs: the handle is unchanged
    for bad in ([(1, 0), (0, 0)], [(0, 0), (0, 0)], [(O, 0)], [(0, I)]):
        with pytest.raises(amd.ConvolutionPanic):
            b.update_pairs(bad, np.zeros((len(bad), 8), np.float32))
    with pytest.raises(amd.ConvolutionPanic):
        b.update_pairs([(0, 0)], np.zeros((1, L + 1), np.float32))
    assert not b.is_crossfading() and b.diff_pairs() == I


# ---- 12: nontemporal H ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["long-idle", "B256"])
def test_nontemporal_instantiation(amd, name):
    """matrix_la_xf_a_kernel<..., true> through the kernel-variant knob: the same bits."""
    sc = scenario(name)
    ys, flags, paths, _ = gpu_run(amd, name)
    outs = []
    for v in (2, 0):
        amd.set_kernel_variant(v)
        try:
            outs.append(sc.drive(amd, sc.handle(amd)))
        finally:
            amd.set_kernel_variant(-1)
    for yv, fv, pv, _ in outs:
        assert (fv, pv) == (flags, paths)
        same_bits(yv, ys, name)


# ---- 13: poisoned buffers -----------------------------------------------------------------
def _child(out, poison):
    """(records by name, failure or None) of one worker run"""
    env = dict(os.environ, FFTCONV_POISON_ALLOC=poison)
    p = subprocess.Popen([sys.executable, WORKER, out], env=env, stderr=subprocess.PIPE, text=True)
    try:
        _, err = p.communicate(timeout=CHILD_TIMEOUT)
        failure = None if p.returncode == 0 else f"exit status {p.returncode}"
    except subprocess.TimeoutExpired:
        p.kill()
        _, err = p.communicate()
        failure = f"no end after {CHILD_TIMEOUT} s"
    recs = {}
    if os.path.exists(out):
        with open(out) as f:
            recs = {r["name"]: r for r in map(json.loads, f)}
    if failure:
        failure = f"the worker with FFTCONV_POISON_ALLOC={poison} ended with {failure} after {list(recs)}\n{err[-2000:]}"
    return recs, failure


def test_poisoned_buffers(amd, tmp_path):
    """"fade", "ragged" and "long-idle" in a child with clean allocations, then in
    one whose every new buffer is filled with 0xff bytes: the same inputs, the
    same output bits."""
    clean, failure = _child(str(tmp_path / "clean.jsonl"), "0")
    assert failure is None, failure   # (after a child that died nothing more is started)
    poisoned, failure = _child(str(tmp_path / "poisoned.jsonl"), "1")
    assert failure is None, failure
    assert list(clean) == list(poisoned) == ["fade", "ragged", "long-idle"]
    for name in clean:
        c, p = clean[name], poisoned[name]
        print(f"{name}: max|y| clean {c['max_abs']!r}, poisoned {p['max_abs']!r}")
        assert c["in"] == p["in"], f"{name}: the two runs drew different inputs"
        assert c["out"] == p["out"], f"{name}: other output bits on poisoned buffers"
        assert c["finite"] and p["finite"] and c["max_abs"] > 0 and p["max_abs"] > 0


# ---- 14: errors --------------------------------------------------------------------------
def test_errors(amd):
    I, O, B, L = 2, 2, 64, 700
    h, x = make(76, I, O, L, 4 * B)
    with pytest.raises(amd.DeviceError, match=r"block size 1024 outside 32\.\.512 \(use the MatrixCrossfadeConvolver\)"):
        amd.MatrixLookaheadCrossfadeConvolver.init(h, 1024, L)
    for wrong in (amd.MatrixConvolver.init(h, B, L), amd.MatrixCrossfadeConvolver.init(h, B, L)):
        with pytest.raises(TypeError):
            amd.MatrixLookaheadCrossfadeConvolver.new(wrong, L, B, 100)
    conv = amd.MatrixLookaheadCrossfadeConvolver.init(h, B, L)
    assert conv.max_buffer_size == B and conv.path() == 2 and not conv.is_crossfading()
    assert amd.MatrixLookaheadCrossfadeConvolver.period() == Q
    with pytest.raises(amd.NotImplementedInReference):
        conv.reset()
    with pytest.raises(amd.ConvolutionPanic):
        conv.process(x[:, :B - 1], B - 1)       # input shorter than max_buffer_size
    with pytest.raises(amd.ConvolutionPanic):
        conv.process(x[:, :B + 1], B + 1)       # output_len above max_buffer_size
    with pytest.raises(amd.ConvolutionPanic):
        conv.update(np.zeros((O, I, L + 1), np.float32))
    assert conv.process(x[:, :B], 10).shape == (O, 10)
