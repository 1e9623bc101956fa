#!/usr/bin/env python3
"""MatrixLookaheadConvolver against the dense MatrixConvolver.

Sides, alternated in one process, each through process_device_steps:
  lookahead  one MatrixLookaheadConvolver handle (far-row windows)
  dense      one MatrixConvolver handle, the bar
  full       (--with-full) the lookahead handle with set_windows(0): the cost
             of the blocks after an update, before the windows are back
Per geometry: device events around >= --seconds of steady state per window,
every shape warmed, --reps alternations, median and spread; the sides' outputs
of the same blocks compared at the timed size (common.REL_TOL).

  bench_matrix_la.py [--geoms M1,M2,M3] [--out DIR]        time, write DIR/timing.json
  bench_matrix_la.py --profile M2:lookahead [--blocks N]   one side only, for a separate
      rocprofv3 --kernel-trace --stats -d DIR/kt_M2_lookahead -o kt --output-format csv -- python3 ...
  bench_matrix_la.py --report DIR                          timing.json + kt_*/ -> DIR/report.json, report.md

Byte model of launch A per block (row = 8 B bytes, Q = period, S = segments):
  near  H: O I (min(Q, S) - 1) rows      X: I (min(Q, S) - 1) rows
  far   H: O I (S - Q) / Q rows          X: (O / Q) I (S - 1) rows (each anchoring output's walk
                                             reads the rows of S - Q steps plus Q - 1 to prime)
  partial sums: near O Pn rows written and read; far O Pf rows written (Q rows
  per anchor, one anchor per Q blocks) and read
against the dense matrix's (O I + I) (S - 1) rows and its O P partial rows."""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fft-convolution_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_BYTES_PER_S = 8e12
COMPOSITION_M2_US = 17.6  # replicate-and-sum on the lookahead step at M2
GEOMS = {  # name: (inputs, outputs, block, IR samples) -- DESIGN 4i
    "M1": (32, 32, 64, 16384),
    "M2": (32, 32, 256, 48000),
    "M3": (2, 2, 128, 96000),
}
STEPS_PER_CALL = 64


def parts_of(rows):
    return max(1, min(64, (rows + 63) // 64))


def model_bytes(I, O, B, L, Q):
    S = -(-L // B)
    row = 8 * B
    nq = min(Q, S)
    far = max(S - Q, 0)
    Pn, Pf = parts_of(I * (nq - 1)), parts_of(I * far) if far else 0
    m = {"S": S, "Q": Q, "Pn": Pn, "Pf": Pf,
         "near_H": O * I * (nq - 1) * row, "near_X": I * (nq - 1) * row,
         "far_H": O * I * far * row / Q, "far_X": O * I * (far + Q - 1) * row / Q if far else 0,
         "partials": 2 * O * (Pn + Pf) * row,
         "dense": (O * I + I) * (S - 1) * row + 2 * O * parts_of(I * (S - 1)) * row}
    m["launch_a"] = m["near_H"] + m["near_X"] + m["far_H"] + m["far_X"] + m["partials"]
    return m


class Side:
    def __init__(self, name, I, O, B, L, seed=5, variant=-1):
        import numpy as np
        import torch

        import fftconv_amd as F

        self.torch, self.name, self.I, self.O, self.B = torch, name, I, O, B
        self.F, self.variant = F, variant  # (the kernel variant of this side's launches; -1 = automatic)
        rng = np.random.default_rng(seed)
        h = (rng.uniform(-1, 1, (O, I, L)) / np.sqrt(L)).astype(np.float32)
        K = STEPS_PER_CALL
        dev = torch.device("cuda:0")
        self.x = torch.from_numpy(rng.uniform(-1, 1, (K, I, B)).astype(np.float32)).to(dev)
        self.y = torch.empty((K, O, B), device=dev)
        if name == "dense":
            self.conv = F.MatrixConvolver.init(h, B, L)
        else:
            self.conv = F.MatrixLookaheadConvolver.init(h, B, L)
            self.conv.set_windows(name == "lookahead")
        torch.cuda.synchronize()

    def call(self):
        """STEPS_PER_CALL blocks on torch's current (the null) stream"""
        K, I, O, B = STEPS_PER_CALL, self.I, self.O, self.B
        self.F.set_kernel_variant(self.variant)
        self.conv.process_device_steps(self.x.data_ptr(), B, I * B, self.y.data_ptr(), B, O * B, B, K, 0)
        self.F.set_kernel_variant(-1)

    def window(self, calls):
        t = self.torch
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            self.call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (calls * STEPS_PER_CALL)  # us per block


def time_geometry(name, seconds, reps, with_full, la_variant=-1):
    import numpy as np
    import torch

    import fftconv_amd as F
    from common import REL_TOL

    I, O, B, L = GEOMS[name]
    names = ["lookahead", "dense"] + (["full"] if with_full else [])
    sides = [Side(n, I, O, B, L, variant=-1 if n == "dense" else la_variant) for n in names]
    # same blocks from the same fresh state: the outputs agree (lookahead and full bitwise)
    for s in sides:
        s.call()
    torch.cuda.synchronize()
    ys = {s.name: s.y.cpu().numpy().astype(np.float64) for s in sides}
    agree = float(np.abs(ys["lookahead"] - ys["dense"]).max() / np.abs(ys["dense"]).max())
    if not agree <= REL_TOL:
        raise SystemExit(f"{name}: lookahead and dense differ by {agree:.3e} of max|ref|")
    if with_full and not np.array_equal(ys["lookahead"], ys["full"]):
        raise SystemExit(f"{name}: windows and full sums differ")
    Q = F.MatrixLookaheadConvolver.period()
    res = {"geometry": name, "inputs": I, "outputs": O, "block": B, "ir": L, "period": Q, "agree_rel": agree,
           "lookahead_variant": la_variant,
           "model": model_bytes(I, O, B, L, Q)}
    calls = {}
    for s in sides:  # warm every shape, then size the window
        for _ in range(3):
            s.call()
        calls[s.name] = max(2, math.ceil(seconds * 1e6 / (s.window(4) * STEPS_PER_CALL)))
    us = {s.name: [] for s in sides}
    for _ in range(reps):
        for s in sides:
            us[s.name].append(s.window(calls[s.name]))
    for k, v in us.items():
        med = statistics.median(v)
        res[k] = {"us_per_block": med, "min": min(v), "max": max(v), "windows": v,
                  "window_s": med * calls[k] * STEPS_PER_CALL / 1e6, "out_MS_per_s": O * B / med}
    la, de = res["lookahead"], res["dense"]
    res["dense_over_lookahead"] = de["us_per_block"] / la["us_per_block"]
    # faster by more than the alternations' spread: the slowest lookahead window beats the fastest dense one
    res["faster_beyond_spread"] = la["max"] < de["min"]
    if name == "M2":
        res["over_composition_17_6us"] = la["us_per_block"] / COMPOSITION_M2_US
    return res


def profile(spec, blocks):
    import torch

    name, side = spec.split(":")
    I, O, B, L = GEOMS[name]
    s = Side(side, I, O, B, L)
    for _ in range(max(1, blocks // STEPS_PER_CALL)):
        s.call()
    torch.cuda.synchronize()


def kernel_stats(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    return [{"name": r["Name"], "calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3,
             "total_ms": float(r["TotalDurationNs"]) / 1e6} for r in rows]


def report(d):
    timing = json.load(open(os.path.join(d, "timing.json")))
    lines = ["| geometry | side | us/block (min..max) | output MS/s | launch A us | launch A model MB | share of 8 TB/s |",
             "|---|---|---|---|---|---|---|"]
    for g in timing:
        for side in ("lookahead", "dense", "full"):
            if side not in g:
                continue
            ks = kernel_stats(os.path.join(d, f"kt_{g['geometry']}_{side}"))
            ks.sort(key=lambda r: -r["total_ms"])
            t = g[side]
            t["kernels"] = ks[:6]
            a_us, mb, share = "not measured", "-", "-"
            a = [r for r in ks if "_a_kernel" in r["name"]]
            if a:
                m = g["model"]
                nbytes = m["launch_a"] if side == "lookahead" else m["dense"]
                if side != "full":
                    frac = nbytes / (a[0]["avg_us"] * 1e-6) / HBM_BYTES_PER_S
                    t["launch_a_us"], t["launch_a_model_bytes"], t["launch_a_share_of_8TBs"] = a[0]["avg_us"], nbytes, frac
                    mb, share = f"{nbytes / 1e6:.1f}", f"{100 * frac:.1f} %"
                a_us = f"{a[0]['avg_us']:.1f}"
            lines.append(f"| {g['geometry']} {g['inputs']}x{g['outputs']} B={g['block']} IR={g['ir']} | {side} | "
                         f"{t['us_per_block']:.1f} ({t['min']:.1f}..{t['max']:.1f}) | {t['out_MS_per_s']:.1f} | "
                         f"{a_us} | {mb} | {share} |")
        extra = f", {g['over_composition_17_6us']:.2f} x the composition's 17.6 us" if "over_composition_17_6us" in g else ""
        lines.append(f"| {g['geometry']} | dense / lookahead | {g['dense_over_lookahead']:.2f} x"
                     f"{' (beyond the spread)' if g['faster_beyond_spread'] else ''}{extra}; outputs agree to "
                     f"{g['agree_rel']:.2e} of max | | | | |")
    json.dump(timing, open(os.path.join(d, "report.json"), "w"), indent=1)
    open(os.path.join(d, "report.md"), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geoms", default="M1,M2,M3")
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--with-full", action="store_true")
    ap.add_argument("--la-variant", type=int, default=-1,
                    help="kernel variant of the lookahead side's launches (2 = nontemporal H loads, 0 = plain)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_la"))
    ap.add_argument("--profile")
    ap.add_argument("--blocks", type=int, default=512)
    ap.add_argument("--report")
    a = ap.parse_args()
    if a.report:
        return report(a.report)
    import fftconv_amd as F

    if F.device_count() < 1:
        raise SystemExit("bench_matrix_la.py needs an MI355X (no CPU fallback)")
    if a.profile:
        return profile(a.profile, a.blocks)
    os.makedirs(a.out, exist_ok=True)
    out = []
    for name in a.geoms.split(","):
        r = time_geometry(name, a.seconds, a.reps, a.with_full, a.la_variant)
        out.append(r)
        print(json.dumps({k: r[k] for k in ("geometry", "period", "agree_rel", "dense_over_lookahead",
                                            "faster_beyond_spread")} |
                         {s: {k: round(r[s][k], 2) for k in ("us_per_block", "min", "max", "out_MS_per_s", "window_s")}
                          for s in ("lookahead", "dense", "full") if s in r}), flush=True)
        json.dump(out, open(os.path.join(a.out, "timing.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
