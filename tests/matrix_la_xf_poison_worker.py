"""The child of tests/test_gpu_matrix_la_xf.py::test_poisoned_buffers: the
"fade", "ragged" and "long-idle" scenarios of the MatrixLookaheadCrossfadeConvolver
(tests/matrix_la_xf_ref.py), one JSON line per scenario.

    matrix_la_xf_poison_worker.py OUT.jsonl

The parent runs it twice, with FFTCONV_POISON_ALLOC=0 and =1 (csrc/host.cpp
poison_alloc), and compares the lines, as tests/test_gpu_poison.py does with
tests/poison_worker.py: a window row, partial sum or delay-line row read before
it was written gives other output bits in the poisoned run.  A line is {"name",
"in": SHA-256 of the responses and the input, "out": SHA-256 of every call's
output, is_crossfading flag and path, "finite", "max_abs"}.  Nothing here reads
or sets an environment variable."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "fft-convolution_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from matrix_la_xf_ref import SCENARIOS  # noqa: E402
from matrix_ref import make  # noqa: E402
from matrix_xf_ref import run_script  # noqa: E402

NAMES = ("fade", "ragged", "long-idle")


def sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(repr((a.shape, str(a.dtype))).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def run(amd, name):
    seed, (I, O, B, L), mbs, fade, build, mrl = SCENARIOS[name]
    script = build(lambda k, n=L: make(seed + k, I, O, n, 1)[0])
    ncalls = sum(1 for kind, _ in script if kind == "call")
    h, x = make(seed, I, O, L, ncalls * mbs)
    conv = amd.MatrixLookaheadCrossfadeConvolver.new(amd.MatrixLookaheadConvolver.init(h, B, L),
                                                     L if mrl is None else mrl, mbs, fade)
    paths = []
    ys, flags = run_script(conv, x, script, mbs, panic=amd.ConvolutionPanic,
                           before_call=lambda k: paths.append(conv.path()))
    y = np.concatenate(ys, axis=1)
    ins = [h, x] + [arg for kind, arg in script if kind != "call"]
    return {"name": name, "in": sha(ins), "out": sha(ys + [np.array(flags), np.array(paths)]),
            "finite": bool(np.isfinite(y).all()), "max_abs": float(np.abs(y).max())}


def main():
    import fftconv_amd as amd

    with open(sys.argv[1], "a") as f:
        for name in NAMES:
            f.write(json.dumps(run(amd, name)) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
