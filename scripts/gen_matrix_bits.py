#!/usr/bin/env python3
"""Writes tests/golden/matrix_bits.json, the fixture of
tests/test_gpu_matrix_bits.py: per case of tests/matrix_bits.py the SHA-256 of
the output bytes, the SHA-256 of the input bytes and max|y|, computed on the
MI355X by the library as it is built in the tree.  Run it at the commit whose
bits are to be kept, BEFORE a kernel file is touched:

    python scripts/gen_matrix_bits.py [--out tests/golden/matrix_bits.json]

Every case runs twice on fresh handles; a case whose two runs differ is an
error and no fixture is written.  Cases added later are recorded the same way
from a build of that commit's library (FFTCONV_AMD_LIB selects it): the whole
fixture is rewritten, and the cases it already held must come out unchanged."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("fft-convolution_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "matrix_bits.json"))
    args = ap.parse_args()
    import fftconv_amd as amd
    from matrix_bits import CASES, run_case

    if amd.device_count() < 1:
        sys.exit("gen_matrix_bits: no HIP device")
    out = {}
    for name in CASES:
        t0 = time.perf_counter()
        a, b = run_case(amd, name), run_case(amd, name)
        if a != b:
            sys.exit(f"gen_matrix_bits: case {name} is not reproducible: {a} != {b}")
        out[name] = a
        print(f"{name}: {time.perf_counter() - t0:.2f} s for two runs, max|y| {a['max_abs']:.6g}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(out)} cases to {args.out}")


if __name__ == "__main__":
    main()
