#!/usr/bin/env python3
"""SparseMatrixLookaheadConvolver against the SparseMatrixConvolver of the same
build, in one process.

Sides, alternated, each through process_device_steps:
  lookahead  one SparseMatrixLookaheadConvolver handle (far-row windows)
  sparse     one SparseMatrixConvolver handle with the same pattern, the bar
  full       the lookahead handle with set_windows(0): the cost of the <= Q - 1
             blocks after an update, before the windows are back
  dense_la   (SP2 only) a dense MatrixLookaheadConvolver: SP2 lists every pair,
             so the difference is the price of the indirection
Geometries:
  SP1   64x64, B 64, IR 16384, 8 inputs per output (bench_matrix_sparse.py's)
  SP1L  the same pattern at B 256, IR 48000
  SP2   32x32 fully listed, B 64, IR 16384
Method as bench_matrix.py: device events around >= --seconds of
steady state per window, every shape warmed, --reps alternations, median and
min..max.  Before anything is timed the lookahead side's outputs must equal the
full side's bit for bit and the sparse side's within common.REL_TOL.

  bench_matrix_sparse_la.py [--geoms SP1,SP1L,SP2] [--out DIR]   time, write DIR/timing.json
  bench_matrix_sparse_la.py --profile SP1:lookahead [--blocks N] one side only, for a separate
      rocprofv3 --kernel-trace --stats -d DIR/kt_SP1_lookahead -o kt --output-format csv -- python3 ...
  bench_matrix_sparse_la.py --report DIR                         timing.json + kt_*/ -> DIR/report.json, report.md

Byte model of launch A per block (row = 8 B bytes, Q = period, S = segments, N
pairs): H rows per pair  lookahead (min(Q, S) - 1) + (S - Q) / Q, sparse S - 1;
the X rows as many again on the sparse side, on the lookahead side the near
rows plus (S - 1) / Q per pair (an anchor's walk reads S - Q rows plus Q - 1 to
prime); partial sums written and read once per part."""
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
from bench_matrix_sparse import pattern  # noqa: E402

GEOMS = {  # name: (inputs, outputs, block, IR samples, inputs per output)
    "SP1": (64, 64, 64, 16384, 8),
    "SP1L": (64, 64, 256, 48000, 8),
    "SP2": (32, 32, 64, 16384, 32),
}
KERNEL_A = {"lookahead": "matrix_sp_la_a_kernel", "full": "matrix_sp_la_a_kernel", "sparse": "matrix_sp_a_kernel",
            "dense_la": "matrix_la_a_kernel"}
KERNEL_B = {"lookahead": "matrix_sp_la_b_kernel", "full": "matrix_sp_la_b_kernel", "sparse": "matrix_sp_b_kernel",
            "dense_la": "matrix_la_b_kernel"}


def parts_of(rows):
    return max(1, min(64, (rows + 63) // 64))


def model_bytes(pairs, O, B, L, Q):
    S = -(-L // B)
    row = 8 * B
    k = [0] * O
    for o, _ in pairs:
        k[o] += 1
    N, nq, far = len(pairs), min(Q, S), max(S - Q, 0)
    pn = sum(parts_of(v * (nq - 1)) for v in k)
    pf = sum(parts_of(v * far) for v in k if v) if far else 0
    m = {"S": S, "Q": Q, "pairs": N, "near_parts": pn, "far_parts": pf,
         "h_rows_per_pair": {"lookahead": (nq - 1) + far / Q, "sparse": S - 1},
         "lookahead": N * ((nq - 1) + far / Q) * row + N * ((nq - 1) + ((far + Q - 1) / Q if far else 0)) * row
         + 2 * (pn + pf) * row,
         "sparse": 2 * N * (S - 1) * row + 2 * sum(mac_parts(v, S) for v in k) * row}
    return m


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
        elif name == "dense_la":
            if per != I:
                raise SystemExit(f"{geom}: the dense lookahead side needs a fully listed pattern")
            self.conv = F.MatrixLookaheadConvolver.init(h.reshape(O, I, L), B, L)
        else:
            self.conv = F.SparseMatrixLookaheadConvolver.init(pairs, h, I, O, B, L)
            self.conv.set_windows(name == "lookahead")
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

    import fftconv_amd as F
    from common import REL_TOL

    I, O, B, L, per = GEOMS[name]
    names = ["lookahead", "sparse", "full"] + (["dense_la"] if per == I else [])
    sides = [Side(n, name) for n in names]
    # the same blocks from the same fresh state, twice (the second call is served
    # from windows): lookahead == full bitwise, == sparse within tolerance
    agree = 0.0
    for _ in range(2):
        for s in sides:
            s.call()
        torch.cuda.synchronize()
        ys = {s.name: s.y.cpu().numpy() for s in sides}
        if not np.array_equal(ys["lookahead"], ys["full"]):
            raise SystemExit(f"{name}: windows and full sums differ")
        if "dense_la" in ys and not np.array_equal(ys["lookahead"], ys["dense_la"]):
            raise SystemExit(f"{name}: the fully listed pattern differs from the dense lookahead matrix")
        ref = ys["sparse"].astype(np.float64)
        agree = max(agree, float(np.abs(ys["lookahead"] - ref).max() / np.abs(ref).max()))
    if not agree <= REL_TOL:
        raise SystemExit(f"{name}: lookahead and sparse differ by {agree:.3e} of max|ref|")
    if sides[0].conv.anchors() == 0:
        raise SystemExit(f"{name}: nothing anchors")
    Q = F.SparseMatrixLookaheadConvolver.period()
    pairs = pattern(I, O, per)
    res = {"geometry": name, "inputs": I, "outputs": O, "block": B, "ir": L, "pairs": len(pairs), "period": Q,
           "agree_rel": agree, "model": model_bytes(pairs, O, B, L, Q)}
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
    la, sp = res["lookahead"], res["sparse"]
    res["sparse_over_lookahead"] = sp["us_per_block"] / la["us_per_block"]
    # faster by more than the alternations' spread: the slowest lookahead window beats the fastest sparse one
    res["faster_beyond_spread"] = la["max"] < sp["min"]
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
    lines = ["| geometry | side | us/block (min..max) | output MS/s | launch A us | launch B us | launch A model MB | "
             "share of 8 TB/s |", "|---|---|---|---|---|---|---|---|"]
    for g in timing:
        for side in ("lookahead", "sparse", "full", "dense_la"):
            if side not in g:
                continue
            ks = kernel_stats(os.path.join(d, f"kt_{g['geometry']}_{side}"))
            ks.sort(key=lambda r: -r["total_ms"])
            t = g[side]
            t["kernels"] = ks[:6]
            a = [r for r in ks if KERNEL_A[side] in r["name"]]
            b = [r for r in ks if KERNEL_B[side] in r["name"]]
            a_us = b_us = "not measured"
            mb = share = "-"
            if a:
                t["launch_a_us"] = a[0]["avg_us"]
                a_us = f"{a[0]['avg_us']:.1f}"
                if side in g["model"]:
                    nbytes = g["model"][side]
                    frac = nbytes / (a[0]["avg_us"] * 1e-6) / HBM_BYTES_PER_S
                    t["launch_a_model_bytes"], t["launch_a_share_of_8TBs"] = nbytes, frac
                    mb, share = f"{nbytes / 1e6:.1f}", f"{100 * frac:.1f} %"
            if b:
                t["launch_b_us"] = b[0]["avg_us"]
                b_us = f"{b[0]['avg_us']:.1f}"
            lines.append(f"| {g['geometry']} {g['inputs']}x{g['outputs']} B={g['block']} IR={g['ir']} "
                         f"pairs={g['pairs']} | {side} | {t['us_per_block']:.1f} ({t['min']:.1f}..{t['max']:.1f}) | "
                         f"{t['out_MS_per_s']:.1f} | {a_us} | {b_us} | {mb} | {share} |")
        h = g["model"]["h_rows_per_pair"]
        lines.append(f"| {g['geometry']} | sparse / lookahead | {g['sparse_over_lookahead']:.2f} x"
                     f"{' (beyond the spread)' if g['faster_beyond_spread'] else ' (inside the spread)'}; H rows per "
                     f"pair and block {h['sparse']} -> {h['lookahead']:.0f}; outputs agree to {g['agree_rel']:.2e} of "
                     f"max | | | | | |")
    json.dump(timing, open(os.path.join(d, "report.json"), "w"), indent=1)
    open(os.path.join(d, "report.md"), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geoms", default="SP1,SP1L,SP2")
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_sparse_la"))
    ap.add_argument("--profile")
    ap.add_argument("--blocks", type=int, default=512)
    ap.add_argument("--report")
    a = ap.parse_args()
    if a.report:
        return report(a.report)
    import fftconv_amd as F

    if F.device_count() < 1:
        raise SystemExit("bench_matrix_sparse_la.py needs an MI355X (no CPU fallback)")
    if a.profile:
        return profile(a.profile, a.blocks)
    os.makedirs(a.out, exist_ok=True)
    out = []
    for name in a.geoms.split(","):
        r = time_geometry(name, a.seconds, a.reps)
        out.append(r)
        print(json.dumps({k: r[k] for k in ("geometry", "pairs", "agree_rel", "sparse_over_lookahead",
                                            "faster_beyond_spread")} |
                         {s: {k: round(r[s][k], 2) for k in ("us_per_block", "min", "max", "out_MS_per_s", "window_s")}
                          for s in ("lookahead", "sparse", "full", "dense_la") if s in r}), flush=True)
        json.dump(out, open(os.path.join(a.out, "timing.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
