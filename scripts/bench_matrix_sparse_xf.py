#!/usr/bin/env python3
"""SparseMatrixCrossfadeConvolver against what could run a sparse
routing with response switching before it, and against the floors of its paths.

Sides, alternated in one process, each through process_device_steps:
  fused        the SparseMatrixCrossfadeConvolver (paths 1 / 2 of fftconv.h)
  composition  the same after set_fused(False) (path 0)
  dense_xf     the dense MatrixCrossfadeConvolver with all-zero responses for the
               pairs that are not listed: the only way to run this before
  two_sparse   two plain SparseMatrixConvolver handles fed the same blocks: the
               composition's convolution work without its mix, a floor for path 0
               (switching: one of them gets update_device per period)
  plain        one SparseMatrixConvolver: the yardstick of the idle state only
Geometries (bench_matrix_sparse.py's):
  SP1  64x64, B 64, IR 16384, output o reads inputs (o + 8 j) mod 64: 512 pairs
  SP2  32x32 fully listed: the price of the indirection against the dense crossfade
States (bench_matrix_xf.py's): idle, switching (update_device every 256 blocks,
hold and fade half of that), fading (both convolvers live in every block).
Per (geometry, state) one child process under its own time limit: device
events around >= --seconds of steady state per window, every side warmed,
--reps alternations, median and min..max; fused and composition outputs of the
same blocks compared bitwise, fused against dense_xf within common.REL_TOL.
The parent never opens the GPU; the first failure ends the run.
`--updates`: at SP1, switching, update_input of one source (the 8 pairs that
read it, the source moving by one per update) against the whole update_device,
in stream time: device events around the update call alone.

  bench_matrix_sparse_xf.py [--geoms SP1,SP2] [--states idle,switching,fading] [--out DIR]
  bench_matrix_sparse_xf.py --updates [--out DIR]
  bench_matrix_sparse_xf.py --profile SP1:fading:fused [--blocks N]    one side only, for a separate
      rocprofv3 --kernel-trace --stats -d DIR/kt_SP1_fading_fused -o kt --output-format csv -- python3 ...
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fft-convolution_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_matrix_sparse import GEOMS, pattern  # noqa: E402

STATES = ("idle", "switching", "fading")
SIDES = ("fused", "composition", "dense_xf", "two_sparse", "plain")
STEPS_PER_CALL = 64
UPDATE_EVERY = 4 * STEPS_PER_CALL   # blocks between updates in the switching state
CHILD_LIMIT_S = 400


class Side:
    def __init__(self, name, state, geom, seed=5, update="whole"):
        import numpy as np
        import torch

        import fftconv_amd as F

        I, O, B, L, per = GEOMS[geom]
        self.torch, self.name, self.state, self.I, self.O, self.B, self.L = torch, name, state, I, O, B, L
        self.update_kind = update
        rng = np.random.default_rng(seed)
        self.pairs = pattern(I, O, per)
        N = len(self.pairs)
        mk = lambda: (rng.uniform(-1, 1, (N, L)) / np.sqrt(L)).astype(np.float32)
        h = mk()
        K = STEPS_PER_CALL
        dev = torch.device("cuda:0")
        self.x = torch.from_numpy(rng.uniform(-1, 1, (K, I, B)).astype(np.float32)).to(dev)
        self.y = torch.zeros((K, O, B), device=dev)
        hs = [mk() for _ in range(2)]
        fade = 10 ** 12 if state == "fading" else UPDATE_EVERY * B // 2 - B
        self.calls = self.updates = 0
        self.upd_events = []
        self.twin = None

        def dense(r):
            d = np.zeros((O, I, L), np.float32)
            for n, (o, i) in enumerate(self.pairs):
                d[o, i] = r[n]
            return d

        if name == "dense_xf":
            self.conv = F.MatrixCrossfadeConvolver.new(F.MatrixConvolver.init(dense(h), B, L), L, B, fade)
            hs = [dense(r) for r in hs]
        else:
            plain = F.SparseMatrixConvolver.init(self.pairs, h, I, O, B, L)
            if name in ("plain", "two_sparse"):
                self.conv = plain
                if name == "two_sparse":
                    self.twin = plain.clone()
                    self.y2 = torch.zeros((K, O, B), device=dev)
            else:
                self.conv = F.SparseMatrixCrossfadeConvolver.new(plain, L, B, fade)
                self.conv.set_fused(name == "fused")
        self.hs = [torch.from_numpy(r).to(dev) for r in hs]
        if update == "input":  # the rows of every input's listed pairs, in list order, gathered ahead of the timing
            self.by_input = [[n for n, p in enumerate(self.pairs) if p[1] == i] for i in range(I)]
            self.rows = [[t[idx].contiguous() for idx in self.by_input] for t in self.hs]
        if state == "fading" and name not in ("plain", "two_sparse"):
            self.conv.update_device(self.hs[0].data_ptr(), L, L, 0)
        torch.cuda.synchronize()

    def update(self):
        k, hs = self.updates, self.hs[self.updates % 2]
        self.updates += 1
        if self.name == "two_sparse":  # the handle that is not heard
            return (self.twin if k % 2 == 0 else self.conv).update_device(hs.data_ptr(), self.L, self.L, 0)
        if self.update_kind == "input":
            i = k % self.I
            return self.conv.update_pairs_device([self.pairs[n] for n in self.by_input[i]],
                                                 self.rows[k % 2][i].data_ptr(), self.L, self.L, 0)
        self.conv.update_device(hs.data_ptr(), self.L, self.L, 0)

    def call(self, timed=False):
        """STEPS_PER_CALL blocks on torch's current (the null) stream"""
        K, I, O, B = STEPS_PER_CALL, self.I, self.O, self.B
        if self.state == "switching" and self.name != "plain" and self.calls % (UPDATE_EVERY // K) == 0:
            if timed:
                e0, e1 = (self.torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record()
                self.update()
                e1.record()
                self.upd_events.append((e0, e1))
            else:
                self.update()
        self.calls += 1
        self.conv.process_device_steps(self.x.data_ptr(), B, I * B, self.y.data_ptr(), B, O * B, B, K, 0)
        if self.twin is not None:
            self.twin.process_device_steps(self.x.data_ptr(), B, I * B, self.y2.data_ptr(), B, O * B, B, K, 0)

    def window(self, calls, timed=False):
        t = self.torch
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        self.upd_events = []
        e0.record()
        for _ in range(calls):
            self.call(timed)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (calls * STEPS_PER_CALL)  # us per block


def need_gpu():
    import fftconv_amd as F

    if F.device_count() < 1:
        raise SystemExit("bench_matrix_sparse_xf.py needs an MI355X (no CPU fallback)")


def one(geom, state, seconds, reps):
    import numpy as np
    import torch

    from common import REL_TOL

    need_gpu()
    I, O, B, L, per = GEOMS[geom]
    names = [n for n in SIDES if n != "plain" or state == "idle"]
    sides = [Side(n, state, geom) for n in names]
    unit = UPDATE_EVERY // STEPS_PER_CALL if state == "switching" else 1  # whole update periods per window
    paths = set()
    agree = 0.0
    for _ in range(2 * unit):  # the same blocks from the same fresh state
        paths.add(sides[0].conv.path())
        for s in sides[:3]:
            s.call()
        torch.cuda.synchronize()
        yf, yc, yd = (s.y.cpu().numpy() for s in sides[:3])
        if not np.array_equal(yf, yc):
            raise SystemExit(f"{geom} {state}: the fused and the composition outputs differ")
        agree = max(agree, float(np.abs(yf.astype(np.float64) - yd).max() / np.abs(yd).max()))
    want = {"idle": {2}, "fading": {1}, "switching": {1, 2}}[state]
    if paths != want or sides[1].conv.path() != 0:
        raise SystemExit(f"{geom} {state}: paths {paths}, expected {want}")
    if not agree <= REL_TOL:
        raise SystemExit(f"{geom} {state}: fused and dense_xf differ by {agree:.3e} of max|ref|")
    res = {"geometry": geom, "state": state, "inputs": I, "outputs": O, "block": B, "ir": L,
           "pairs": len(sides[0].pairs), "agree_rel_dense": agree}
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


def updates(geom, seconds, reps):
    """update_input of one source against the whole update, stream time per update"""
    import numpy as np
    import torch

    need_gpu()
    unit = UPDATE_EVERY // STEPS_PER_CALL
    res = {"geometry": geom, "state": "switching"}
    sides = [Side("fused", "switching", geom, update=k) for k in ("whole", "input")]
    for s in sides:
        for _ in range(2 * unit):
            s.call()
        n = unit * max(1, math.ceil(seconds * 1e6 / (s.window(2 * unit) * STEPS_PER_CALL * unit)))
        us, upd = [], []
        for _ in range(reps):
            us.append(s.window(n, timed=True))
            upd.append(statistics.median(a.elapsed_time(b) * 1e3 for a, b in s.upd_events))
        res[s.update_kind] = {"us_per_block": statistics.median(us), "min": min(us), "max": max(us),
                              "update_us": statistics.median(upd), "update_min": min(upd), "update_max": max(upd),
                              "last_patch": s.conv.last_patch()}
    print("RESULT " + json.dumps(res), flush=True)


def profile(geom, state, side, blocks):
    import torch

    need_gpu()
    s = Side(side, state, geom)
    for _ in range(max(1, blocks // STEPS_PER_CALL)):
        s.call()
    torch.cuda.synchronize()


def child(args, what):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True,
                       timeout=CHILD_LIMIT_S)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"{what}: exit status {p.returncode}; nothing further is started")
    return json.loads(line[0][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geoms", default="SP1,SP2")
    ap.add_argument("--states", default=",".join(STATES))
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_sparse_xf"))
    ap.add_argument("--one", help="GEOM:STATE, in this process (what the parent starts)")
    ap.add_argument("--updates", action="store_true", help="update_input against the whole update at SP1")
    ap.add_argument("--updates-child", help="GEOM, in this process")
    ap.add_argument("--profile", help="GEOM:STATE:SIDE, --blocks blocks of that side only")
    ap.add_argument("--blocks", type=int, default=1024)
    a = ap.parse_args()
    if a.one:
        return one(*a.one.split(":"), a.seconds, a.reps)
    if a.updates_child:
        return updates(a.updates_child, a.seconds, a.reps)
    if a.profile:
        return profile(*a.profile.split(":"), a.blocks)
    os.makedirs(a.out, exist_ok=True)
    common = ["--seconds", str(a.seconds), "--reps", str(a.reps)]
    if a.updates:
        r = child(["--updates-child", "SP1"] + common, "SP1 updates")
        print(json.dumps(r), flush=True)
        json.dump(r, open(os.path.join(a.out, "updates.json"), "w"), indent=1)
        return
    out = []
    for g in a.geoms.split(","):
        for st in a.states.split(","):
            r = child(["--one", f"{g}:{st}"] + common, f"{g} {st}")
            out.append(r)
            print(json.dumps({"geometry": g, "state": st, "agree_rel_dense": r["agree_rel_dense"]} |
                             {s: [round(r[s][k], 2) for k in ("us_per_block", "min", "max")] for s in SIDES if s in r}),
                  flush=True)
            json.dump(out, open(os.path.join(a.out, "timing.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
