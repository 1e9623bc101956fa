#!/usr/bin/env python3
"""MatrixTwoStageConvolver: the fused path against its composition path and
against the plain MatrixConvolver of the same block and response length (what
a user of the matrix has without it).

Sides, alternated in one process, each through process_device_steps:
  plain        one MatrixConvolver, block B, IR L
  composition  a MatrixTwoStageConvolver after set_fused(False) (path 0)
  fused        a MatrixTwoStageConvolver (path 1 at every call: all are aligned)
Per geometry: device events around >= --seconds of steady state per window, a
window a whole number of tail periods, every side warmed, --reps alternations,
median and min..max of us per head block; then the calls of --periods periods
timed one by one (an event between consecutive calls; event overhead included,
so these are upper bounds) for the worst single call, the one that ends a
period and carries the tail's block-T convolution.  Fused and composition
outputs of the same blocks are compared bitwise first.  The parent process
never opens the GPU: every geometry runs in a child under its own time limit,
and the first failure ends the run.

  bench_matrix_ts.py [--geoms M1,BIN] [--out DIR]        time, write DIR/timing.json
  bench_matrix_ts.py --profile BIN:fused [--blocks N]    one side only, for a separate
      rocprofv3 --kernel-trace --stats -d DIR/kt_BIN_fused -o kt --output-format csv -- python3 ...

Byte model per head block: H of head and tail0 once, the tail's H once per
period; X once per matrix that streams it (head and tail0 share one stream on
the fused path); `part` written and read per matrix."""
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

GEOMS = {  # name: (inputs, outputs, head block, IR samples)
    "M1": (32, 32, 64, 16384),
    "BIN": (64, 2, 256, 48000),   # binaural rendering of 64 sources
}
SIDES = ("plain", "composition", "fused")
CHILD_LIMIT_S = 300


def parts(I, S):
    return max(1, min(64, (I * max(S - 1, 0) + 63) // 64))  # matrix_mac_parts


def matrix_bytes(I, O, B, n):
    """one block of a plain matrix of block B over n response samples"""
    S = -(-n // B)
    P = parts(I, S)
    row = 8 * B
    return {"H": O * I * S * row, "X": I * max(S - 1, 0) * row, "part": 2 * O * P * row, "S": S, "P": P}


def model_bytes(I, O, B, L, T):
    plain = matrix_bytes(I, O, B, L)
    head = matrix_bytes(I, O, B, min(L, T))
    tail0 = matrix_bytes(I, O, B, min(L - T, T)) if L > T else None
    tail = matrix_bytes(I, O, T, L - 2 * T) if L > 2 * T else None
    period = T // B
    total = lambda m: m["H"] + m["X"] + m["part"] if m else 0
    comp = total(head) + total(tail0) + total(tail) / period
    return {"plain": plain, "head": head, "tail0": tail0, "tail": tail, "period": period,
            "plain_per_block": total(plain), "composition_per_block": comp,
            "fused_per_block": comp - (tail0["X"] if tail0 else 0)}


class Side:
    def __init__(self, name, I, O, B, L, seed=5):
        import numpy as np
        import torch

        import fftconv_amd as F

        self.torch, self.name, self.I, self.O, self.B, self.L = torch, name, I, O, B, L
        rng = np.random.default_rng(seed)
        h = (rng.uniform(-1, 1, (O, I, L)) / np.sqrt(L)).astype(np.float32)
        self.T = F.compute_tail_block_size(B, L)
        self.period = self.T // B
        self.K = K = 4 * self.period  # blocks per process_device_steps call: whole periods
        dev = torch.device("cuda:0")
        self.x = torch.from_numpy(rng.uniform(-1, 1, (K, I, B)).astype(np.float32)).to(dev)
        self.y = torch.zeros((K, O, B), device=dev)
        if name == "plain":
            self.conv = F.MatrixConvolver.init(h, B, L)
        else:
            self.conv = F.MatrixTwoStageConvolver.init(h, B, L)
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
        raise SystemExit("bench_matrix_ts.py needs an MI355X (no CPU fallback)")
    I, O, B, L = GEOMS[geom]
    sides = [Side(n, I, O, B, L) for n in SIDES]
    comp, fused = sides[1], sides[2]
    for _ in range(2):  # the same blocks from the same fresh state: the same bits
        if fused.conv.path(B) != 1 or comp.conv.path(B) != 0:
            raise SystemExit(f"{geom}: paths {fused.conv.path(B)} / {comp.conv.path(B)}, expected 1 / 0")
        for s in (comp, fused):
            s.call()
        torch.cuda.synchronize()
        if not np.array_equal(comp.y.cpu().numpy(), fused.y.cpu().numpy()):
            raise SystemExit(f"{geom}: the fused and the composition outputs differ")
    res = {"geometry": geom, "inputs": I, "outputs": O, "block": B, "ir": L, "tail_block": fused.T,
           "model": model_bytes(I, O, B, L, fused.T)}
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
        pos = s.per_call(periods)
        res[s.name] = {"us_per_block": med, "min": min(v), "max": max(v), "windows": v,
                       "window_s": med * calls[s.name] * s.K / 1e6,
                       "per_call_us_by_position": pos, "worst_call_us": max(pos), "worst_position": pos.index(max(pos))}
    print("RESULT " + json.dumps(res), flush=True)


def profile(geom, side, blocks):
    """one side only, for a separate
    rocprofv3 --kernel-trace --stats -d DIR/kt_GEOM_SIDE -o kt --output-format csv -- python3 ... --profile"""
    import torch

    s = Side(side, *GEOMS[geom])
    for _ in range(max(1, blocks // s.K)):
        s.call()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geoms", default="M1,BIN")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--periods", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_ts"))
    ap.add_argument("--one", help="GEOM, in this process (what the parent starts)")
    ap.add_argument("--profile", help="GEOM:SIDE, --blocks blocks of that side only")
    ap.add_argument("--blocks", type=int, default=1024)
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.seconds, a.reps, a.periods)
    if a.profile:
        return profile(*a.profile.split(":"), a.blocks)
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
                         {s: [round(r[s][k], 2) for k in ("us_per_block", "min", "max", "worst_call_us")] for s in SIDES} |
                         {"model_MB": [round(r["model"][k] / 1e6, 2) for k in
                                       ("plain_per_block", "composition_per_block", "fused_per_block")]}), flush=True)
        json.dump(out, open(os.path.join(a.out, "timing.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
