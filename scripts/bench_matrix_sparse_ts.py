#!/usr/bin/env python3
"""SparseMatrixTwoStageConvolver: the fused path against its composition path,
against the other sparse handles of the same pattern, block and response
length, and against the dense MatrixTwoStageConvolver that runs the pattern
today (all-zero responses for the pairs that are not listed).

Sides, alternated in one process, each through process_device_steps:
  sparse       one SparseMatrixConvolver, block B, IR L
  lookahead    one SparseMatrixLookaheadConvolver, block B, IR L
  dense_ts     one MatrixTwoStageConvolver, inputs x outputs, zeros elsewhere
  composition  a SparseMatrixTwoStageConvolver after set_fused(False) (path 0)
  fused        a SparseMatrixTwoStageConvolver (path 1 at every call: all are aligned)
Geometries (the patterns of bench_matrix_sparse.py):
  SP1  64x64, head 64, IR 16384, 8 inputs per output
  SP2  32x32 fully listed: dense_ts is the dense two-stage M1 of
       bench_matrix_ts.py -- the price of the indirection
Per geometry: device events around >= --seconds of steady state per window, a
window a whole number of tail periods, every side warmed, --reps alternations,
median and min..max of us per head block; then, for the two-stage sides, the
calls of --periods periods timed one by one (an event between consecutive
calls; event overhead included, so these are upper bounds) for the worst single
call, the one that ends a period and carries the tail's block-T convolution.
Fused and composition outputs of the same blocks are compared bitwise first.
The parent process never opens the GPU: every geometry runs in a child under
its own time limit, and the first failure ends the run.

  bench_matrix_sparse_ts.py [--geoms SP1,SP2] [--out DIR]     time, write DIR/timing.json
  bench_matrix_sparse_ts.py --profile SP1:fused [--blocks N]  one side only, for a separate
      rocprofv3 --kernel-trace --stats -d DIR/kt_SP1_fused -o kt --output-format csv -- python3 ...
  bench_matrix_sparse_ts.py --report DIR                      timing.json -> DIR/report.md"""
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

SIDES = ("sparse", "lookahead", "dense_ts", "composition", "fused")
TWO_STAGE = ("dense_ts", "composition", "fused")
CHILD_LIMIT_S = 300


class Side:
    def __init__(self, name, geom, seed=5):
        import numpy as np
        import torch

        import fftconv_amd as F

        I, O, B, L, per = GEOMS[geom]
        self.torch, self.name, self.I, self.O, self.B, self.L = torch, name, I, O, B, L
        rng = np.random.default_rng(seed)
        pairs = pattern(I, O, per)
        h = (rng.uniform(-1, 1, (len(pairs), L)) / np.sqrt(L)).astype(np.float32)
        self.T = F.compute_tail_block_size(B, L)
        self.period = self.T // B
        self.K = K = 4 * self.period  # blocks per process_device_steps call: whole periods
        dev = torch.device("cuda:0")
        self.x = torch.from_numpy(rng.uniform(-1, 1, (K, I, B)).astype(np.float32)).to(dev)
        self.y = torch.zeros((K, O, B), device=dev)
        if name == "sparse":
            self.conv = F.SparseMatrixConvolver.init(pairs, h, I, O, B, L)
        elif name == "lookahead":
            self.conv = F.SparseMatrixLookaheadConvolver.init(pairs, h, I, O, B, L)
        elif name == "dense_ts":
            hd = np.zeros((O, I, L), np.float32)
            for n, (o, i) in enumerate(pairs):
                hd[o, i] = h[n]
            self.conv = F.MatrixTwoStageConvolver.init(hd, B, L)
        else:
            self.conv = F.SparseMatrixTwoStageConvolver.init(pairs, h, I, O, B, L)
            assert self.conv.tail_block_size == self.T
            self.conv.set_fused(name == "fused")
        torch.cuda.synchronize()

    def call(self):
        """K blocks on torch's current (the null) stream"""
        K, I, O, B = self.K, self.I, self.O, self.B
        self.conv.process_device_steps(self.x.data_ptr(), B, I * B, self.y.data_ptr(), B, O * B, B, K, 0)

    def window(self, calls):
        t = self.torch
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            self.call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (calls * self.K)  # us per block

    def per_call(self, periods):
        """us of each call of a period, by position: the median over `periods`
        periods (an event between consecutive one-block calls)"""
        t, I, O, B = self.torch, self.I, self.O, self.B
        n = periods * self.period
        ev = [t.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        ev[0].record()
        for k in range(n):
            j = k % self.K
            self.conv.process_device(self.x.data_ptr() + 4 * j * I * B, B, self.y.data_ptr() + 4 * j * O * B, B, B, 0)
            ev[k + 1].record()
        ev[n].synchronize()
        us = [ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(n)]
        return [statistics.median(us[j::self.period]) for j in range(self.period)]


def one(geom, seconds, reps, periods):
    import numpy as np
    import torch

    import fftconv_amd as F

    if F.device_count() < 1:
        raise SystemExit("bench_matrix_sparse_ts.py needs an MI355X (no CPU fallback)")
    I, O, B, L, per = GEOMS[geom]
    sides = [Side(n, geom) for n in SIDES]
    by = {s.name: s for s in sides}
    comp, fused = by["composition"], by["fused"]
    for _ in range(2):  # the same blocks from the same fresh state: the same bits
        if fused.conv.path(B) != 1 or comp.conv.path(B) != 0:
            raise SystemExit(f"{geom}: paths {fused.conv.path(B)} / {comp.conv.path(B)}, expected 1 / 0")
        for s in (comp, fused):
            s.call()
        torch.cuda.synchronize()
        if not np.array_equal(comp.y.cpu().numpy(), fused.y.cpu().numpy()):
            raise SystemExit(f"{geom}: the fused and the composition outputs differ")
    res = {"geometry": geom, "inputs": I, "outputs": O, "pairs": O * per, "block": B, "ir": L, "tail_block": fused.T,
           "period": fused.period}
    calls = {}
    for s in sides:  # warm every side, then size the window
        for _ in range(2):
            s.call()
        calls[s.name] = max(1, math.ceil(seconds * 1e6 / (s.window(2) * s.K)))
    us = {s.name: [] for s in sides}
    for _ in range(reps):
        for s in sides:
            us[s.name].append(s.window(calls[s.name]))
    for s in sides:
        v = us[s.name]
        med = statistics.median(v)
        res[s.name] = {"us_per_block": med, "min": min(v), "max": max(v), "windows": v,
                       "window_s": med * calls[s.name] * s.K / 1e6}
        if s.name in TWO_STAGE:
            pos = s.per_call(periods)
            res[s.name] |= {"per_call_us_by_position": pos, "worst_call_us": max(pos),
                            "worst_position": pos.index(max(pos))}
    print("RESULT " + json.dumps(res), flush=True)


def profile(geom, side, blocks):
    """one side only, for a separate
    rocprofv3 --kernel-trace --stats -d DIR/kt_GEOM_SIDE -o kt --output-format csv -- python3 ... --profile"""
    import torch

    s = Side(side, geom)
    for _ in range(max(1, blocks // s.K)):
        s.call()
    torch.cuda.synchronize()


def report(out):
    """timing.json -> report.md: the tables DESIGN §4r quotes"""
    rows = json.load(open(os.path.join(out, "timing.json")))
    md = ["| geometry | side | us per head block (median, min..max) | worst call us |", "|---|---|---|---|"]
    for r in rows:
        for s in SIDES:
            v = r[s]
            worst = f"{v['worst_call_us']:.1f} (call {v['worst_position'] + 1} of {r['period']})" \
                if "worst_call_us" in v else "-"
            md.append(f"| {r['geometry']} | {s} | {v['us_per_block']:.2f} ({v['min']:.2f}..{v['max']:.2f}) | {worst} |")
    md += ["", "| geometry | fused against | ratio of medians | spreads overlap |", "|---|---|---|---|"]
    for r in rows:
        f = r["fused"]
        for s in SIDES[:-1]:
            v = r[s]
            overlap = not (f["max"] < v["min"] or v["max"] < f["min"])
            md.append(f"| {r['geometry']} | {s} | {v['us_per_block'] / f['us_per_block']:.2f}x | "
                      f"{'yes' if overlap else 'no'} |")
    open(os.path.join(out, "report.md"), "w").write("\n".join(md) + "\n")
    print("\n".join(md))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geoms", default="SP1,SP2")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--periods", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_sparse_ts"))
    ap.add_argument("--one", help="GEOM, in this process (what the parent starts)")
    ap.add_argument("--profile", help="GEOM:SIDE, --blocks blocks of that side only")
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--report", help="DIR: timing.json -> report.md")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.seconds, a.reps, a.periods)
    if a.profile:
        return profile(*a.profile.split(":"), a.blocks)
    if a.report:
        return report(a.report)
    os.makedirs(a.out, exist_ok=True)
    out = []
    for g in a.geoms.split(","):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", g, "--seconds", str(a.seconds),
                            "--reps", str(a.reps), "--periods", str(a.periods)], capture_output=True, text=True,
                           timeout=CHILD_LIMIT_S)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"{g}: exit status {p.returncode}; nothing further is started")
        r = json.loads(line[0][7:])
        out.append(r)
        print(json.dumps({"geometry": g, "T": r["tail_block"]} |
                         {s: [round(r[s][k], 2) for k in ("us_per_block", "min", "max")] +
                             ([round(r[s]["worst_call_us"], 2)] if s in TWO_STAGE else []) for s in SIDES}),
              flush=True)
        json.dump(out, open(os.path.join(a.out, "timing.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
