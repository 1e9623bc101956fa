#!/usr/bin/env python3
"""MatrixLookaheadCrossfadeConvolver: the fused path against its composition
path, against the dense MatrixCrossfadeConvolver of the same build and, for the
idle state, against one MatrixLookaheadConvolver.

Sides, alternated in one process, each through process_device_steps:
  fused        a MatrixLookaheadCrossfadeConvolver (paths 1 / 2 of fftconv.h)
  composition  the same after set_fused(False): A and B as two lookahead
               matrices and the mix kernel (path 0)
  dense_xf     a MatrixCrossfadeConvolver, fused: every live convolver streams
               all of its H on every block
  lookahead    one MatrixLookaheadConvolver -- the yardstick of the idle state
               only (it cannot switch responses smoothly)
States:
  idle         no update: one convolver is heard, the other idles
  switching    update_device every UPDATE_EVERY = 256 blocks, the hold and fade
               last half of that: fades and idle stretches both occur, so do the
               <= Q - 1 full-sum blocks after every swap; the updates' IR
               transforms are inside the timed region (the same on every side)
  fading       one update, then a fade longer than the measurement: both
               convolvers live in every block, both served from windows
Per (geometry, state): device events around >= --seconds of steady state per
window, every side warmed, --reps alternations, median and min..max; fused and
composition outputs of the same blocks compared bitwise before anything is
timed.  The parent process never opens the GPU: every (geometry, state) runs in
a child under its own time limit, and the first failure ends the run.

  bench_matrix_la_xf.py [--geoms M1,M2,BIN] [--states idle,switching,fading] [--out DIR]   time, write DIR/timing.json
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fft-convolution_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GEOMS = {  # name: (inputs, outputs, block, IR samples)
    "M1": (32, 32, 64, 16384),
    "M2": (32, 32, 256, 48000),
    "BIN": (64, 2, 256, 48000),   # binaural rendering of 64 sources: O = 2 < Q, two blocks in eight carry anchors
}
STATES = ("idle", "switching", "fading")
SIDES = ("fused", "composition", "dense_xf", "lookahead")
STEPS_PER_CALL = 64
UPDATE_EVERY = 4 * STEPS_PER_CALL   # blocks between updates in the switching state
CHILD_LIMIT_S = 300


class Side:
    def __init__(self, name, state, I, O, B, L, seed=5):
        import numpy as np
        import torch

        import fftconv_amd as F

        self.torch, self.name, self.state, self.I, self.O, self.B, self.L = torch, name, state, I, O, B, L
        rng = np.random.default_rng(seed)
        mk = lambda: (rng.uniform(-1, 1, (O, I, L)) / np.sqrt(L)).astype(np.float32)
        h = mk()
        K = STEPS_PER_CALL
        dev = torch.device("cuda:0")
        self.x = torch.from_numpy(rng.uniform(-1, 1, (K, I, B)).astype(np.float32)).to(dev)
        self.y = torch.zeros((K, O, B), device=dev)
        self.hs = [torch.from_numpy(mk()).to(dev) for _ in range(2)]
        self.calls = 0
        fade = 10 ** 12 if state == "fading" else UPDATE_EVERY * B // 2 - B
        if name == "lookahead":
            self.conv = F.MatrixLookaheadConvolver.init(h, B, L)
        elif name == "dense_xf":
            self.conv = F.MatrixCrossfadeConvolver.new(F.MatrixConvolver.init(h, B, L), L, B, fade)
        else:
            self.conv = F.MatrixLookaheadCrossfadeConvolver.new(F.MatrixLookaheadConvolver.init(h, B, L), L, B, fade)
            self.conv.set_fused(name == "fused")
        if state == "fading":
            self.conv.update_device(self.hs[0].data_ptr(), L, L, 0)
        torch.cuda.synchronize()

    def call(self):
        """STEPS_PER_CALL blocks on torch's current (the null) stream"""
        K, I, O, B = STEPS_PER_CALL, self.I, self.O, self.B
        if self.state == "switching" and self.calls % (UPDATE_EVERY // K) == 0:
            self.conv.update_device(self.hs[(self.calls // (UPDATE_EVERY // K)) % 2].data_ptr(), self.L, self.L, 0)
        self.calls += 1
        self.conv.process_device_steps(self.x.data_ptr(), B, I * B, self.y.data_ptr(), B, O * B, B, K, 0)

    def window(self, calls):
        t = self.torch
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            self.call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (calls * STEPS_PER_CALL)  # us per block


def one(geom, state, seconds, reps):
    import numpy as np
    import torch

    import fftconv_amd as F

    if F.device_count() < 1:
        raise SystemExit("bench_matrix_la_xf.py needs an MI355X (no CPU fallback)")
    I, O, B, L = GEOMS[geom]
    names = ["fused", "composition", "dense_xf"] + (["lookahead"] if state == "idle" else [])
    sides = [Side(n, state, I, O, B, L) for n in names]
    unit = UPDATE_EVERY // STEPS_PER_CALL if state == "switching" else 1  # whole update periods per window
    paths = set()
    for _ in range(2 * unit):  # the same blocks from the same fresh state: the same bits
        paths.add(sides[0].conv.path())
        for s in sides[:2]:
            s.call()
        torch.cuda.synchronize()
        if not np.array_equal(sides[0].y.cpu().numpy(), sides[1].y.cpu().numpy()):
            raise SystemExit(f"{geom} {state}: the fused and the composition outputs differ")
    want = {"idle": {2}, "fading": {1}, "switching": {1, 2}}[state]
    if paths != want or sides[1].conv.path() != 0:
        raise SystemExit(f"{geom} {state}: paths {paths}, expected {want}")
    for s in sides[2:]:  # (every side has made the same calls when the timing starts)
        for _ in range(2 * unit):
            s.call()
    res = {"geometry": geom, "state": state, "inputs": I, "outputs": O, "block": B, "ir": L,
           "segments": -(-L // B)}
    calls = {}
    for s in sides:  # warm every side, then size the window
        for _ in range(2 * unit):
            s.call()
        calls[s.name] = unit * max(1, math.ceil(seconds * 1e6 / (s.window(2 * unit) * STEPS_PER_CALL * unit)))
    us = {s.name: [] for s in sides}
    for _ in range(reps):
        for s in sides:
            us[s.name].append(s.window(calls[s.name]))
    for k, v in us.items():
        med = statistics.median(v)
        res[k] = {"us_per_block": med, "min": min(v), "max": max(v), "windows": v,
                  "window_s": med * calls[k] * STEPS_PER_CALL / 1e6}
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geoms", default="M1,M2,BIN")
    ap.add_argument("--states", default=",".join(STATES))
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_la_xf"))
    ap.add_argument("--one", help="GEOM:STATE, in this process (what the parent starts)")
    a = ap.parse_args()
    if a.one:
        return one(*a.one.split(":"), a.seconds, a.reps)
    os.makedirs(a.out, exist_ok=True)
    out = []
    for g in a.geoms.split(","):
        for st in a.states.split(","):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", f"{g}:{st}", "--seconds",
                                str(a.seconds), "--reps", str(a.reps)], capture_output=True, text=True,
                               timeout=CHILD_LIMIT_S)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"{g} {st}: exit status {p.returncode}; nothing further is started")
            r = json.loads(line[0][7:])
            out.append(r)
            print(json.dumps({"geometry": g, "state": st} |
                             {s: [round(r[s][k], 2) for k in ("us_per_block", "min", "max")] for s in SIDES if s in r}),
                  flush=True)
            json.dump(out, open(os.path.join(a.out, "timing.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
