#!/usr/bin/env python3
"""Call length and grid size of the per-call batch (csrc/la_batch.hpp) against
per-block launches, in one process: us per step of process_device_steps calls
of K steps at C channels (block 256, IR 48000), HIP events on the launch
stream, median of --reps groups of --calls calls.  The per-block handle is
made under VARIANT_NORUN (one launch per block).  FFTCONV_AMD_LIB selects the
library build, so two builds are compared by running this once each.

usage: ab_batch_calls.py [--channels 64,256,1024] [--lengths 8,12,16,24,32,64]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "fft-convolution_amd"))
import fftconv_amd as F  # noqa: E402

VARIANT_NORUN = 2048


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--channels", default="1024")
    p.add_argument("--lengths", default="8,12,16,24,32,64")
    p.add_argument("--block", type=int, default=256)
    p.add_argument("--ir", type=int, default=48000)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--calls", type=int, default=10)
    a = p.parse_args()
    B, L = a.block, a.ir
    out = {}
    for C in [int(v) for v in a.channels.split(",")]:
        rng = np.random.default_rng(C)
        hs = (rng.uniform(-1, 1, (C, L)) / np.sqrt(L)).astype(np.float32)
        x = torch.from_numpy(rng.uniform(-1, 1, (64, C, B)).astype(np.float32)).to("cuda:0")
        y = torch.empty_like(x)
        F.set_kernel_variant(VARIANT_NORUN)
        try:
            per_block = F.FFTConvolver.init(hs, B, L, channels=C)
        finally:
            F.set_kernel_variant(-1)
        batch = F.FFTConvolver.init(hs, B, L, channels=C)
        stream = torch.cuda.Stream("cuda:0")
        torch.cuda.set_stream(stream)
        sh = stream.cuda_stream

        def us_per_step(conv, K, norun):
            F.set_kernel_variant(VARIANT_NORUN if norun else -1)
            try:
                ts = []
                for rep in range(a.reps + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(a.calls):
                        conv.process_device_steps(x.data_ptr(), B, C * B, y.data_ptr(), B, C * B, B, K, sh)
                    e1.record(stream)
                    torch.cuda.synchronize()
                    if rep:  # (the first group warms up)
                        ts.append(e0.elapsed_time(e1) * 1e3 / (a.calls * K))
                return statistics.median(ts), min(ts), max(ts)
            finally:
                F.set_kernel_variant(-1)

        for K in [int(v) for v in a.lengths.split(",")]:
            pb = us_per_step(per_block, K, True)
            # (a call shorter than LA_BATCH_MIN takes the batch while the windows are
            # dropped: the 16-step call before it drops them)
            batch.process_device_steps(x.data_ptr(), B, C * B, y.data_ptr(), B, C * B, B, 16, sh)
            bt = us_per_step(batch, K, False)
            print(f"C={C:5d} k={K:3d}  per-block {pb[0]:7.3f} us/step ({pb[1]:.3f}-{pb[2]:.3f})   "
                  f"batch {bt[0]:7.3f} us/step ({bt[1]:.3f}-{bt[2]:.3f})", flush=True)
            out[f"{C}/{K}"] = [round(pb[0], 3), round(bt[0], 3)]
        del per_block, batch
    print(json.dumps(out))


if __name__ == "__main__":
    main()
