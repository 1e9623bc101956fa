"""Every family bit-identical on 0xff-poisoned buffers.

FFTCONV_POISON_ALLOC=1 (csrc/host.cpp poison_alloc) fills every new device
buffer, shared table, stream-ordered scratch and pinned host stage with 0xff
bytes -- NaN as a float, -1 as an index.  A path that reads memory it never
wrote then computes other bits than on the zero pages a quiet machine hands
out, which is what a long-lived host process that recycles memory would see.
The switch is read once per process, so the scenarios (tests/poison_worker.py)
run in two child processes, one after the other: clean, then poisoned.  Per
scenario the two runs must have drawn the same inputs and produced the same
output hash (outputs, padding and every state tuple read); a finite output
alone would prove nothing, since a partly poisoned spectrum is zero-filled by
the C2R error path.  The matrix_bits cases must also reproduce
tests/golden/matrix_bits.json while poisoned.  The check is deterministic: it
says nothing about stream races, LDS or registers.

Measured on two MI355X machines: the clean child took 47 s on one (the poisoned
one 40 s; about a second per handle created there) and 2.7 s on the other (2.8 s
poisoned).  CHILD_TIMEOUT is about 5 times the slower clean run.

The unmarked test keeps the scenario table honest on any machine: every member
host.cpp allocates must be listed in BUFFERS with the scenarios that use it."""
import json
import os
import re
import subprocess
import sys
import time

import pytest

import poison_worker
from matrix_bits import CASES

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORKER = os.path.join(HERE, "poison_worker.py")
MARKER = "fftconv: FFTCONV_POISON_ALLOC on"
CHILD_TIMEOUT = 240  # seconds; see the module docstring

with open(os.path.join(HERE, "golden", "matrix_bits.json")) as _f:
    GOLDEN = json.load(_f)


def _cases(prefix):
    return tuple(n for n in CASES if n.startswith(prefix))


_UNIFORM = ("uniform-short", "uniform-la-C5-B128-S40", "uniform-windows", "uniform-long-block")
_LA = ("uniform-la-C5-B128-S40", "uniform-la-C11-B128-S70", "uniform-batch-K32", "uniform-batch-K19",
       "uniform-batch-buffered", "uniform-batch-shared", "uniform-batch-nan", "uniform-batch-short-channel",
       "uniform-batch-C11-S70-K69", "crossfade-la")
_TWOSTAGE = ("twostage-32-5000-ragged", "twostage-64-12000", "twostage-64-12000-t0fused", "twostage-64-12000-t0block",
             "twostage-steps", "twostage-clone-reset", "twostage-long-tail", "crossfade-twostage")
_XF = ("crossfade-B64-L700", "crossfade-B128-L1000-x300", "crossfade-la", "crossfade-la-nofmix", "crossfade-la-nopair",
       "crossfade-long-block", "crossfade-clone")
_MXF = _cases("xf-") + _cases("spxf-") + ("xf-ops", "spxf-ops")
_MATRIX = _cases("dense-") + _cases("sparse-") + ("dense-ops", "sparse-ops")
_MLA = _cases("la-") + ("la-ops",)
_SPLA = _cases("spla-") + ("spla-ops",)
_MTS = _cases("ts-") + _cases("spts-") + ("ts-ops", "spts-ops")
_UPDATES = ("uniform-short", "uniform-update-device", "uniform-update-capped-stage", "uniform-update-irblock")
_FFT = ("fft-256", "fft-32768", "fft-1000", "fft-20000", "fft-inverse-status")

# member of csrc/host.cpp that is allocated with .alloc( -> the scenarios that run the code reading it;
# then the five allocations that are not a DevPtr or a PinnedStage, by name
BUFFERS = {
    # Scratch (host-pointer entry points of every class)
    "in": _UNIFORM + _MATRIX, "out": _UNIFORM + _MATRIX,
    # PairLists (update_pairs)
    "d": ("dense-ops", "sparse-ops", "spla-ops", "xf-ops", "spxf-ops", "xf-B64-update-pairs"),
    # UniformCore / MatrixCore geometry
    "H": _UNIFORM + _MATRIX, "X": _UNIFORM + _MATRIX, "pre": _UNIFORM + _LA + _MATRIX, "tw": _UNIFORM + _MATRIX,
    "overlap": _UNIFORM, "inbuf": _UNIFORM, "state": _UNIFORM + _LA,
    "staging": _UPDATES + ("dense-update", "sparse-update", "la-B64-update", "spla-B64-update"),
    "hstage": _UPDATES + _XF + _MXF + ("dense-update", "sparse-update"),
    "gwin": ("uniform-windows", "twostage-long-tail"),
    "laW": _LA, "lav": _LA, "la_res": _LA,
    "lg_prog": ("uniform-long-block", "crossfade-long-block", "twostage-long-tail"),
    "lg_v": ("uniform-long-block", "crossfade-long-block", "twostage-long-tail"),
    # diagnostics, allocated only under FFTCONV_LA_PROBE / FFTCONV_LA_TRACE / FFTCONV_PROC_TRACE /
    # FFTCONV_T0_TRACE, which the worker cannot set and no output depends on
    "la_probe": (), "trace": (), "t0_trace": (),
    # clone()'s buffer copies and the host Fft's status words
    "dst": ("uniform-short", "dense-ops", "twostage-clone-reset", "crossfade-clone", "fft-inverse-status"),
    # two-stage: the run's signal words and the deferred tail0
    "tsig": _TWOSTAGE,
    "t0_xs": _TWOSTAGE, "t0_ys": _TWOSTAGE, "t0_err": _TWOSTAGE, "t0_ov": _TWOSTAGE, "t0_cv": _TWOSTAGE,
    "t0_miss": _TWOSTAGE,
    # crossfade (uniform and matrix)
    "stored": _XF + _MXF, "buf_a": _XF + _MXF, "buf_b": _XF + _MXF, "mix_tab": _XF + _MXF,
    # matrix families
    "part": _MATRIX + _MXF + _MTS, "ovl": _MATRIX + _MLA + _SPLA, "ib": _MATRIX + _MLA + _SPLA,
    "lists": ("dense-ops", "sparse-ops", "spla-ops", "xf-ops", "spxf-ops", "xf-B64-update-pairs"),
    "far": _MLA + _SPLA, "npart": _SPLA, "nplan": _SPLA, "fplan": _SPLA, "d_coff": _SPLA, "nwg": _SPLA, "fwg": _SPLA,
    "d_rowptr": _cases("sparse-") + _cases("spxf-") + _cases("spts-") + _SPLA + ("sparse-ops", "spxf-ops", "spts-ops"),
    "d_col": _cases("sparse-") + _cases("spxf-") + _cases("spts-") + _SPLA + ("sparse-ops", "spxf-ops", "spts-ops"),
    "plan": _cases("sparse-") + _cases("spxf-") + _cases("spts-") + ("sparse-ops", "spxf-ops", "spts-ops"),
    "wg": _cases("sparse-") + _cases("spxf-") + _cases("spts-") + ("sparse-ops", "spxf-ops", "spts-ops"),
    "tin": _MTS,
    # the host form of the public Fft
    "din": _FFT, "dout": _FFT,
    # not DevPtr: hipMalloc'd tables and hipMallocAsync'd scratch
    "fft_twiddles": ("fft-256", "fft-32768", "fft-1000"),
    "lg_tables": ("fft-32768", "fft-20000", "uniform-long-block"),
    "bluestein_tables": ("fft-1000", "fft-20000"),
    "bluestein scratch": ("fft-20000",),
    "four-step scratch": ("fft-32768",),
}
NOT_DEVPTR = ("fft_twiddles", "lg_tables", "bluestein_tables", "bluestein scratch", "four-step scratch")


def test_every_allocation_has_a_scenario():
    with open(os.path.join(ROOT, "fft-convolution_amd", "csrc", "host.cpp")) as f:
        src = f.read()
    members = set(re.findall(r"(\w+)\.alloc\(", src))
    assert len(members) > 40  # (the pattern still finds them)
    missing = sorted(members - set(BUFFERS))
    assert not missing, f"host.cpp allocates {missing}: list them in BUFFERS with a scenario that reads them"
    assert set(BUFFERS) - members == set(NOT_DEVPTR)
    assert src.count("hipMalloc((void **)") == 4 and src.count("hipMallocAsync(") == 2  # DevPtr + NOT_DEVPTR
    for member, names in BUFFERS.items():
        for name in names:
            assert name in poison_worker.SCENARIOS, (member, name)
    assert not set(CASES) - set(poison_worker.SCENARIOS)
    assert poison_worker.FEEDS_NAN <= set(poison_worker.SCENARIOS)


def _read(path):
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        return {r["name"]: r for r in map(json.loads, f)}


def _child(out, poison):
    """(records, stderr, failure or None) of one worker run"""
    env = dict(os.environ, FFTCONV_POISON_ALLOC=poison)
    t0 = time.time()
    p = subprocess.Popen([sys.executable, WORKER, out], env=env, stderr=subprocess.PIPE, text=True)
    try:
        _, err = p.communicate(timeout=CHILD_TIMEOUT)
        failure = None if p.returncode == 0 else f"exit status {p.returncode}"
    except subprocess.TimeoutExpired:
        p.kill()
        _, err = p.communicate()
        failure = f"no end after {CHILD_TIMEOUT} s"
    recs = _read(out)
    print(f"poison worker FFTCONV_POISON_ALLOC={poison}: {time.time() - t0:.1f} s, {len(recs)} scenarios")
    if failure:
        last = list(recs)[-1] if recs else "none"
        failure = (f"the worker with FFTCONV_POISON_ALLOC={poison} ended with {failure}; the last scenario it finished "
                   f"is {last!r}\n{err[-2000:]}")
    return recs, err, failure


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("poison")
    clean, clean_err, failure = _child(str(d / "clean.jsonl"), "0")
    poisoned, poisoned_err = {}, ""
    if failure is None:  # (after a child that died nothing more is started)
        poisoned, poisoned_err, failure = _child(str(d / "poisoned.jsonl"), "1")
    return {"clean": clean, "poisoned": poisoned, "clean_err": clean_err, "poisoned_err": poisoned_err,
            "failure": failure}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(poison_worker.SCENARIOS))
def test_poisoned_run_gives_the_same_bits(runs, name):
    assert runs["failure"] is None, runs["failure"]
    assert name in runs["clean"] and name in runs["poisoned"]
    clean, poisoned = runs["clean"][name], runs["poisoned"][name]
    print(f"{name}: max|y| clean {clean['max_abs']!r}, poisoned {poisoned['max_abs']!r}")
    assert clean["in"] == poisoned["in"], f"{name}: the two runs drew different inputs"
    assert clean["out"] == poisoned["out"], \
        f"{name}: other output bits on poisoned buffers (a read of memory the path never wrote); max|y| " \
        f"{clean['max_abs']!r} clean, {poisoned['max_abs']!r} poisoned"
    if name not in poison_worker.FEEDS_NAN:
        assert clean["finite"] and poisoned["finite"]
    assert clean["max_abs"] > 0 and poisoned["max_abs"] > 0
    if name in CASES:
        assert poisoned["in"] == GOLDEN[name]["in"]
        assert poisoned["out"] == GOLDEN[name]["out"], f"{name}: the poisoned run left the recorded bits"


@pytest.mark.gpu
def test_the_poisoned_child_ran_poisoned(runs):
    assert runs["failure"] is None, runs["failure"]
    assert runs["poisoned_err"].count(MARKER) == 1
    assert MARKER not in runs["clean_err"]
