#!/usr/bin/env python3
"""MatrixConvolver against the composition a user can build without it.

Sides, alternated in one process, each through process_device_steps:
  matrix       one MatrixConvolver handle (inputs I, outputs O)
  composition  a uniform FFTConvolver batch of I*O channels, the input
               replicated to [O][I][n] on the device, the outputs summed over
               i with torch -- replication and sum inside the timed region
Per geometry: device events around >= --seconds of steady state per window,
every shape warmed, --reps alternations, median and spread; the two sides'
outputs of the same blocks compared at the timed size (common.REL_TOL).

  bench_matrix.py [--geoms M1,M2,M3] [--out DIR]         time, write DIR/timing.json
  bench_matrix.py --profile M1:matrix [--blocks N]       one side only, for a separate
      rocprofv3 --kernel-trace --stats -d DIR/kt_M1_matrix -o kt --output-format csv -- python3 ...
  bench_matrix.py --report DIR                           timing.json + kt_*/ -> DIR/report.json, report.md

Byte model of the matrix MAC (launch A): H once, X once, `part` written and
read; over that kernel's time from the trace, as a fraction of 8 TB/s."""
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
GEOMS = {  # name: (inputs, outputs, block, IR samples)
    "M1": (32, 32, 64, 16384),
    "M2": (32, 32, 256, 48000),
    "M3": (2, 2, 128, 96000),
}
STEPS_PER_CALL = 64


def mac_parts(I, act):
    """matrix_mac_parts (matrix.hip)"""
    return max(1, min(64, (I * max(act - 1, 0) + 63) // 64))


def mac_model_bytes(I, O, B, L):
    S = -(-L // B)
    P = mac_parts(I, S)
    row = 8 * B
    return {"H": O * I * (S - 1) * row, "X": I * (S - 1) * row, "part": 2 * O * P * row, "S": S, "P": P}


class Side:
    def __init__(self, name, I, O, B, L, seed=5):
        import numpy as np
        import torch

        import fftconv_amd as F

        self.torch, self.name, self.I, self.O, self.B = torch, name, I, O, B
        rng = np.random.default_rng(seed)
        h = (rng.uniform(-1, 1, (O, I, L)) / np.sqrt(L)).astype(np.float32)
        K = STEPS_PER_CALL
        dev = torch.device("cuda:0")
        self.x = torch.from_numpy(rng.uniform(-1, 1, (K, I, B)).astype(np.float32)).to(dev)
        self.y = torch.empty((K, O, B), device=dev)
        if name == "matrix":
            self.conv = F.MatrixConvolver.init(h, B, L)
        else:
            self.conv = F.FFTConvolver.init(h.reshape(O * I, L), B, L, channels=O * I)
            self.yc = torch.empty((K, O * I, B), device=dev)
        torch.cuda.synchronize()

    def call(self):
        """STEPS_PER_CALL blocks on torch's current (the null) stream"""
        K, I, O, B = STEPS_PER_CALL, self.I, self.O, self.B
        if self.name == "matrix":
            self.conv.process_device_steps(self.x.data_ptr(), B, I * B, self.y.data_ptr(), B, O * B, B, K, 0)
        else:
            xr = self.x[:, None].expand(K, O, I, B).contiguous()
            self.conv.process_device_steps(xr.data_ptr(), B, O * I * B, self.yc.data_ptr(), B, O * I * B, B, K, 0)
            self.torch.sum(self.yc.view(K, O, I, B), dim=2, out=self.y)

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

    I, O, B, L = GEOMS[name]
    sides = [Side("matrix", I, O, B, L), Side("composition", I, O, B, L)]
    # same blocks from the same fresh state: the outputs agree
    for s in sides:
        s.call()
    torch.cuda.synchronize()
    ym, yc = sides[0].y.cpu().numpy().astype(np.float64), sides[1].y.cpu().numpy().astype(np.float64)
    agree = float(np.abs(ym - yc).max() / np.abs(yc).max())
    if not agree <= REL_TOL:
        raise SystemExit(f"{name}: matrix and composition differ by {agree:.3e} of max|ref|")
    res = {"geometry": name, "inputs": I, "outputs": O, "block": B, "ir": L, "agree_rel": agree,
           "model": mac_model_bytes(I, O, B, L)}
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
    lines = ["| geometry | side | us/block (min..max) | output MS/s | MAC kernel us | MAC model GB | share of 8 TB/s |",
             "|---|---|---|---|---|---|---|"]
    for g in timing:
        for side in ("matrix", "composition"):
            ks = kernel_stats(os.path.join(d, f"kt_{g['geometry']}_{side}"))
            ks.sort(key=lambda r: -r["total_ms"])
            g[side]["kernels"] = ks[:6]
            t = g[side]
            mac_us, gb, share = "not measured", "-", "-"
            if side == "matrix":
                a = [r for r in ks if "matrix_a_kernel" in r["name"]]
                if a:
                    m = g["model"]
                    nbytes = m["H"] + m["X"] + m["part"]
                    frac = nbytes / (a[0]["avg_us"] * 1e-6) / HBM_BYTES_PER_S
                    if frac > 1.0:
                        raise SystemExit(f"{g['geometry']}: model implies {frac:.2f} x 8 TB/s")
                    t["mac_us"], t["mac_model_bytes"], t["mac_share_of_8TBs"] = a[0]["avg_us"], nbytes, frac
                    mac_us, gb, share = f"{a[0]['avg_us']:.1f}", f"{nbytes / 1e9:.4f}", f"{100 * frac:.1f} %"
            elif ks:
                # the composition's MAC runs inside its step kernels: the largest one's time per launch
                t["mac_us"] = ks[0]["avg_us"]
                t["mac_kernel"] = ks[0]["name"][:80]
                mac_us = f"{ks[0]['avg_us']:.1f} ({ks[0]['name'].split('<')[0].split('::')[-1][:28]})"
            lines.append(f"| {g['geometry']} {g['inputs']}x{g['outputs']} B={g['block']} IR={g['ir']} | {side} | "
                         f"{t['us_per_block']:.1f} ({t['min']:.1f}..{t['max']:.1f}) | {t['out_MS_per_s']:.1f} | "
                         f"{mac_us} | {gb} | {share} |")
        lines.append(f"| {g['geometry']} | outputs agree | {g['agree_rel']:.2e} of max (tolerance 1e-5) | | | | |")
    json.dump(timing, open(os.path.join(d, "report.json"), "w"), indent=1)
    open(os.path.join(d, "report.md"), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geoms", default="M1,M2,M3")
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix"))
    ap.add_argument("--profile")
    ap.add_argument("--blocks", type=int, default=512)
    ap.add_argument("--report")
    a = ap.parse_args()
    if a.report:
        return report(a.report)
    import fftconv_amd as F

    if F.device_count() < 1:
        raise SystemExit("bench_matrix.py needs an MI355X (no CPU fallback)")
    if a.profile:
        return profile(a.profile, a.blocks)
    os.makedirs(a.out, exist_ok=True)
    out = []
    for name in a.geoms.split(","):
        r = time_geometry(name, a.seconds, a.reps)
        out.append(r)
        print(json.dumps({k: r[k] for k in ("geometry", "agree_rel")} |
                         {s: {k: round(r[s][k], 2) for k in ("us_per_block", "min", "max", "out_MS_per_s", "window_s")}
                          for s in ("matrix", "composition")}), flush=True)
        json.dump(out, open(os.path.join(a.out, "timing.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
