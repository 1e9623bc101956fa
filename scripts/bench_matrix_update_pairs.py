#!/usr/bin/env python3
"""MatrixCrossfadeConvolver.update_pairs against the whole update.

State "switching": one update every UPDATE_EVERY = 256 blocks, the hold and
fade last half of that, everything through process_device_steps.  Sides:
  whole    update_device of all O*I responses (the parent commit's code path)
  input    update_input of one source: the O pairs that read input i, i moving
           by one per update (update_pairs_device, rows in device memory)
  pairs8   update_pairs_device of 8 scattered pairs
Each side runs in a child process of its own under a time limit (the parent
never opens the GPU; the first failure ends the run).  A child alternates
--reps times between an idle window (a second handle that is never updated)
and a switching window, device events around >= --seconds each, and reports
per state the median and min..max of us per block, and for the updates the
stream time of one update: device events around the update call alone, inside
the switching windows.  Before timing, the side's outputs are compared bitwise
with a twin that gets update_device(R') for the same blocks.

  bench_matrix_update_pairs.py [--geoms BIN,M1] [--sides whole,input,pairs8] [--out DIR]
      time, write DIR/timing.json
  bench_matrix_update_pairs.py --kernel-stats [--geoms ..] [--out DIR]
      per geometry one separate  rocprofv3 --kernel-trace --stats  run of the
      `input` side (--profile GEOM:SIDE below); adds the patch kernel's calls,
      time and modelled bytes to DIR/kernel_stats.json
  bench_matrix_update_pairs.py --profile BIN:input [--blocks N]     one side only, for rocprofv3

Byte model of one update (spectra rows of S*B float2 per pair): the whole update
uploads O*I*L floats and writes O*I rows; a partial swap reads the listed
pairs' samples, writes their rows, and reads and writes one row per copied pair."""
import argparse
import csv
import glob
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
    "BIN": (64, 2, 256, 48000),   # binaural rendering of 64 sources
    "M1": (32, 32, 64, 16384),
}
SIDES = ("whole", "input", "pairs8")
STEPS_PER_CALL = 64
UPDATE_EVERY = 4 * STEPS_PER_CALL
CHILD_LIMIT_S = 240


def side_pairs(side, I, O, k):
    """the pairs of update k"""
    if side == "input":
        i = k % I
        return [(o, i) for o in range(O)]
    n = I * O
    idx = sorted({(k * 7 + j * (n // 8) + j) % n for j in range(8)})
    return [(p // I, p % I) for p in idx]


def model_bytes(I, O, B, L, listed, copied):
    S = -(-L // B)
    row = 8 * S * B
    return {"whole": 4 * O * I * L + O * I * (4 * L + row), "partial": listed * (4 * L + row) + copied * 2 * row,
            "row": row, "S": S}


class Side:
    def __init__(self, name, I, O, B, L, switching=True, seed=5):
        import numpy as np
        import torch

        import fftconv_amd as F

        self.torch, self.np, self.name, self.I, self.O, self.B, self.L = torch, np, name, I, O, B, L
        self.switching = switching
        rng = np.random.default_rng(seed)
        mk = lambda: (rng.uniform(-1, 1, (O, I, L)) / np.sqrt(L)).astype(np.float32)
        h = mk()
        K = STEPS_PER_CALL
        dev = torch.device("cuda:0")
        self.x = torch.from_numpy(rng.uniform(-1, 1, (K, I, B)).astype(np.float32)).to(dev)
        self.y = torch.zeros((K, O, B), device=dev)
        self.hs = [torch.from_numpy(mk()).to(dev) for _ in range(2)]
        self.calls = self.updates = 0
        self.upd_events = []
        self.conv = F.MatrixCrossfadeConvolver.new(F.MatrixConvolver.init(h, B, L), L, B, UPDATE_EVERY * B // 2 - B)
        torch.cuda.synchronize()

    def update(self):
        k, hs = self.updates, self.hs[self.updates % 2]
        self.updates += 1
        if self.name == "whole":
            return self.conv.update_device(hs.data_ptr(), self.L, self.L, 0)
        pairs = side_pairs(self.name, self.I, self.O, k)
        # rows n of the flat [O*I][L] tensor, in list order
        self.conv.update_pairs_device(pairs, hs.view(-1, self.L).data_ptr(), self.L, self.L, 0)

    def call(self, timed=False):
        """STEPS_PER_CALL blocks on torch's current (the null) stream"""
        K, I, O, B = STEPS_PER_CALL, self.I, self.O, self.B
        if self.switching and self.calls % (UPDATE_EVERY // K) == 0:
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

    def window(self, calls):
        t = self.torch
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        self.upd_events = []
        e0.record()
        for _ in range(calls):
            self.call(timed=True)
        e1.record()
        e1.synchronize()
        upd = [a.elapsed_time(b) * 1e3 for a, b in self.upd_events]  # us of stream time per update
        return e0.elapsed_time(e1) * 1e3 / (calls * STEPS_PER_CALL), upd


class Twin(Side):
    """the same blocks with update_device(R'): the listed rows of the side's update replaced in the heard set"""

    def __init__(self, name, I, O, B, L):
        super().__init__(name, I, O, B, L)
        self.side = name
        self.name = "whole"
        self.base = None

    def update(self):
        k, hs = self.updates, self.hs[self.updates % 2]
        self.updates += 1
        if self.base is None:
            raise SystemExit("Twin needs its base set")
        if self.side != "whole":
            flat, src = self.base.view(-1, self.L), hs.view(-1, self.L)
            for n, (o, i) in enumerate(side_pairs(self.side, self.I, self.O, k)):
                flat[o * self.I + i] = src[n]
        else:
            self.base.copy_(hs)
        self.torch.cuda.synchronize()
        self.conv.update_device(self.base.data_ptr(), self.L, self.L, 0)


def one(geom, side, seconds, reps):
    import numpy as np
    import torch

    import fftconv_amd as F

    if F.device_count() < 1:
        raise SystemExit("bench_matrix_update_pairs.py needs an MI355X (no CPU fallback)")
    I, O, B, L = GEOMS[geom]
    unit = UPDATE_EVERY // STEPS_PER_CALL
    # the same blocks from the same fresh state: the same bits as update_device(R')
    a, t = Side(side, I, O, B, L), Twin(side, I, O, B, L)
    rng = np.random.default_rng(5)
    t.base = torch.from_numpy((rng.uniform(-1, 1, (O, I, L)) / np.sqrt(L)).astype(np.float32)).to("cuda:0")  # = h
    for _ in range(3 * unit):
        assert a.conv.path() == t.conv.path()
        a.call()
        t.call()
        torch.cuda.synchronize()
        if not np.array_equal(a.y.cpu().numpy(), t.y.cpu().numpy()):
            raise SystemExit(f"{geom} {side}: outputs differ from update_device(R')")
    patch = a.conv.last_patch()
    del t
    idle = Side(side, I, O, B, L, switching=False)
    res = {"geometry": geom, "side": side, "inputs": I, "outputs": O, "block": B, "ir": L, "last_patch": patch,
           "model": model_bytes(I, O, B, L, patch[0], patch[1])}
    calls = {}
    for s in (idle, a):
        for _ in range(2 * unit):
            s.call()
        calls[s] = unit * max(1, math.ceil(seconds * 1e6 / (s.window(2 * unit)[0] * STEPS_PER_CALL * unit)))
    us = {"idle": [], "switching": []}
    upd = []
    for _ in range(reps):
        us["idle"].append(idle.window(calls[idle])[0])
        w, u = a.window(calls[a])
        us["switching"].append(w)
        upd.append(statistics.median(u))
    for k, v in us.items():
        res[k] = {"us_per_block": statistics.median(v), "min": min(v), "max": max(v), "windows": v}
    res["update_us"] = {"median": statistics.median(upd), "min": min(upd), "max": max(upd), "windows": upd}
    res["update_us_from_blocks"] = (res["switching"]["us_per_block"] - res["idle"]["us_per_block"]) * UPDATE_EVERY
    print("RESULT " + json.dumps(res), flush=True)


def profile(geom, side, blocks):
    import torch

    s = Side(side, *GEOMS[geom])
    for _ in range(max(1, blocks // STEPS_PER_CALL)):
        s.call()
    torch.cuda.synchronize()


def kernel_stats(geoms, out, blocks):
    """a separate rocprofv3 --kernel-trace --stats run per geometry (nothing else traced)"""
    res = []
    for g in geoms:
        d = os.path.join(out, f"kt_{g}_input")
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "kt", "--output-format", "csv", "--",
                            sys.executable, os.path.abspath(__file__), "--profile", f"{g}:input", "--blocks",
                            str(blocks)], capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        files = glob.glob(os.path.join(d, "**", "kt_kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not files:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"{g}: rocprofv3 exit status {p.returncode}; nothing further is started")
        I, O, B, L = GEOMS[g]
        m = model_bytes(I, O, B, L, O, O)  # steady state: O pairs listed, the previous source's O pairs copied
        for row in csv.DictReader(open(files[0])):
            if "matrix_patch_kernel" in row["Name"]:
                avg = float(row["AverageNs"])
                res.append({"geometry": g, "kernel": row["Name"], "calls": int(row["Calls"]), "avg_us": avg / 1e3,
                            "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3,
                            "model_bytes": m["partial"], "copy_bytes": O * 2 * m["row"],
                            "gb_per_s": m["partial"] / avg})
        os.replace(files[0], os.path.join(out, f"kt_{g}_input_kernel_stats.csv"))
        if not res or res[-1]["geometry"] != g:
            raise SystemExit(f"{g}: no matrix_patch_kernel row in the kernel stats")
        print(json.dumps(res[-1]), flush=True)
    json.dump(res, open(os.path.join(out, "kernel_stats.json"), "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geoms", default="BIN,M1")
    ap.add_argument("--sides", default=",".join(SIDES))
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_patch"))
    ap.add_argument("--one", help="GEOM:SIDE, in this process (what the parent starts)")
    ap.add_argument("--profile", help="GEOM:SIDE, --blocks blocks of that side only")
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--blocks", type=int, default=4096)
    a = ap.parse_args()
    if a.one:
        return one(*a.one.split(":"), a.seconds, a.reps)
    if a.profile:
        return profile(*a.profile.split(":"), a.blocks)
    os.makedirs(a.out, exist_ok=True)
    if a.kernel_stats:
        return kernel_stats(a.geoms.split(","), a.out, a.blocks)
    out = []
    for g in a.geoms.split(","):
        for sd in a.sides.split(","):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", f"{g}:{sd}", "--seconds",
                                str(a.seconds), "--reps", str(a.reps)], capture_output=True, text=True,
                               timeout=CHILD_LIMIT_S)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"{g} {sd}: exit status {p.returncode}; nothing further is started")
            r = json.loads(line[0][7:])
            out.append(r)
            print(json.dumps({"geometry": g, "side": sd, "last_patch": r["last_patch"]} |
                             {s: [round(r[s][k], 2) for k in ("us_per_block", "min", "max")]
                              for s in ("idle", "switching")} |
                             {"update_us": [round(r["update_us"][k], 1) for k in ("median", "min", "max")]}),
                  flush=True)
            json.dump(out, open(os.path.join(a.out, "timing.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
