#!/usr/bin/env python3
"""SparseMatrixConvolver against the dense MatrixConvolver that runs the same
pattern today: all-zero responses for the pairs that are not listed.

Sides, alternated in one process, each through process_device_steps:
  sparse  one SparseMatrixConvolver handle holding the listed pairs
  dense   one MatrixConvolver handle, inputs x outputs, zeros elsewhere
Geometries:
  SP1  64x64, B 64, IR 16384, 8 inputs per output: output o reads inputs
       (o + 8 j) mod 64 -- one pair in eight
  SP2  32x32 fully listed against the dense M1 matrix of bench_matrix.py: the
       price of the indirection
Method as bench_matrix.py: device events around >= --seconds of steady state
per window, every shape warmed, --reps alternations, median and min..max; the
two sides' outputs of the same blocks compared as a fraction of max|ref|.

  bench_matrix_sparse.py [--geoms SP1,SP2] [--out DIR]    time, write DIR/timing.json
  bench_matrix_sparse.py --profile SP1:sparse [--blocks N]  one side only, for a separate
      rocprofv3 --kernel-trace --stats -d DIR/kt_SP1_sparse -o kt --output-format csv -- python3 ...
  bench_matrix_sparse.py --report DIR                     timing.json + kt_*/ -> DIR/report.json, report.md

Byte model of the MAC (launch A): H once, each read X row once per output that
reads it, `part` written and read; over that kernel's time from the trace, as
a fraction of 8 TB/s."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fft-convolution_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_matrix import HBM_BYTES_PER_S, STEPS_PER_CALL, kernel_stats, mac_parts  # noqa: E402

GEOMS = {  # name: (inputs, outputs, block, IR samples, inputs per output)
    "SP1": (64, 64, 64, 16384, 8),
    "SP2": (32, 32, 64, 16384, 32),
}


def pattern(I, O, per):
    """output o reads inputs (o + (I / per) j) mod I, j < per; strictly ascending"""
    step = I // per
    return [(o, i) for o in range(O) for i in sorted((o + step * j) % I for j in range(per))]


def mac_model_bytes(pairs, O, B, L, dense_inputs=None):
    """sparse: over the listed pairs; dense_inputs = I: the zero-filled dense matrix"""
    S = -(-L // B)
    row = 8 * B
    if dense_inputs is not None:
        N, parts = O * dense_inputs, O * mac_parts(dense_inputs, S)
        x_rows = N * (S - 1)  # (every output reads every input's rows: counted as on the sparse side)
    else:
        k = [0] * O
        for o, _ in pairs:
            k[o] += 1
        N, parts = len(pairs), sum(mac_parts(v, S) for v in k)
        x_rows = N * (S - 1)
    return {"H": N * (S - 1) * row, "X": x_rows * row, "part": 2 * parts * row, "S": S, "parts": parts, "pairs": N}


class Side:
    def __init__(self, name, geom, seed=5):
        import numpy as np
        import torch

        import fftconv_amd as F

        I, O, B, L, per = GEOMS[geom]
        self.torch, self.name, self.I, self.O, self.B = torch, name, I, O, B
        rng = np.random.default_rng(seed)
        pairs = pattern(I, O, per)
        h = (rng.uniform(-1, 1, (len(pairs), L)) / np.sqrt(L)).astype(np.float32)
        K = STEPS_PER_CALL
        dev = torch.device("cuda:0")
        self.x = torch.from_numpy(rng.uniform(-1, 1, (K, I, B)).astype(np.float32)).to(dev)
        self.y = torch.empty((K, O, B), device=dev)
        if name == "sparse":
            self.conv = F.SparseMatrixConvolver.init(pairs, h, I, O, B, L)
        else:
            hd = np.zeros((O, I, L), np.float32)
            for n, (o, i) in enumerate(pairs):
                hd[o, i] = h[n]
            self.conv = F.MatrixConvolver.init(hd, B, L)
        torch.cuda.synchronize()

    def call(self):
        """STEPS_PER_CALL blocks on torch's current (the null) stream"""
        K, I, O, B = STEPS_PER_CALL, self.I, self.O, self.B
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


def time_geometry(name, seconds, reps):
    import numpy as np
    import torch

    from common import REL_TOL

    I, O, B, L, per = GEOMS[name]
    sides = [Side("sparse", name), Side("dense", name)]
    for s in sides:  # same blocks from the same fresh state: the outputs agree
        s.call()
    torch.cuda.synchronize()
    ys, yd = sides[0].y.cpu().numpy().astype(np.float64), sides[1].y.cpu().numpy().astype(np.float64)
    agree = float(np.abs(ys - yd).max() / np.abs(yd).max())
    if not agree <= REL_TOL:
        raise SystemExit(f"{name}: sparse and dense differ by {agree:.3e} of max|ref|")
    pairs = pattern(I, O, per)
    res = {"geometry": name, "inputs": I, "outputs": O, "block": B, "ir": L, "pairs": len(pairs), "agree_rel": agree,
           "model": {"sparse": mac_model_bytes(pairs, O, B, L), "dense": mac_model_bytes(pairs, O, B, L, I)}}
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
    return res


def profile(spec, blocks):
    import torch

    name, side = spec.split(":")
    s = Side(side, name)
    for _ in range(max(1, blocks // STEPS_PER_CALL)):
        s.call()
    torch.cuda.synchronize()


def report(d):
    timing = json.load(open(os.path.join(d, "timing.json")))
    lines = ["| geometry | side | us/block (min..max) | output MS/s | MAC kernel us | MAC model GB | share of 8 TB/s |",
             "|---|---|---|---|---|---|---|"]
    for g in timing:
        for side, kern in (("sparse", "matrix_sp_a_kernel"), ("dense", "matrix_a_kernel")):
            ks = kernel_stats(os.path.join(d, f"kt_{g['geometry']}_{side}"))
            ks.sort(key=lambda r: -r["total_ms"])
            t = g[side]
            t["kernels"] = ks[:6]
            mac_us, gb, share = "not measured", "-", "-"
            a = [r for r in ks if kern in r["name"]]
            if a:
                m = g["model"][side]
                nbytes = m["H"] + m["X"] + m["part"]
                frac = nbytes / (a[0]["avg_us"] * 1e-6) / HBM_BYTES_PER_S
                t["mac_us"], t["mac_model_bytes"], t["mac_share_of_8TBs"] = a[0]["avg_us"], nbytes, frac
                mac_us, gb, share = f"{a[0]['avg_us']:.1f}", f"{nbytes / 1e9:.4f}", f"{100 * frac:.1f} %"
            lines.append(f"| {g['geometry']} {g['inputs']}x{g['outputs']} B={g['block']} IR={g['ir']} "
                         f"pairs={g['pairs']} | {side} | {t['us_per_block']:.1f} ({t['min']:.1f}..{t['max']:.1f}) | "
                         f"{t['out_MS_per_s']:.1f} | {mac_us} | {gb} | {share} |")
        lines.append(f"| {g['geometry']} | outputs agree | {g['agree_rel']:.2e} of max (tolerance 1e-5) | | | | |")
    json.dump(timing, open(os.path.join(d, "report.json"), "w"), indent=1)
    open(os.path.join(d, "report.md"), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geoms", default="SP1,SP2")
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_sparse"))
    ap.add_argument("--profile")
    ap.add_argument("--blocks", type=int, default=512)
    ap.add_argument("--report")
    a = ap.parse_args()
    if a.report:
        return report(a.report)
    import fftconv_amd as F

    if F.device_count() < 1:
        raise SystemExit("bench_matrix_sparse.py needs an MI355X (no CPU fallback)")
    if a.profile:
        return profile(a.profile, a.blocks)
    os.makedirs(a.out, exist_ok=True)
    out = []
    for name in a.geoms.split(","):
        r = time_geometry(name, a.seconds, a.reps)
        out.append(r)
        print(json.dumps({k: r[k] for k in ("geometry", "pairs", "agree_rel")} |
                         {s: {k: round(r[s][k], 2) for k in ("us_per_block", "min", "max", "out_MS_per_s", "window_s")}
                          for s in ("sparse", "dense")}), flush=True)
        json.dump(out, open(os.path.join(a.out, "timing.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
