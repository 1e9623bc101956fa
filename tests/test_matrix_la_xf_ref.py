"""The window rules of the MatrixLookaheadCrossfadeConvolver,
checked on the CPU.  matrix_la_xf_ref.PairModel replays what the host does with
every scenario script of tests/test_gpu_matrix_la_xf.py -- the crossfader, the
pending response, the block walk, the two clocks with the swap and idle rules --
and asserts while it runs, by enumeration over every block and output, that a
window row a block reads was written by that output's latest anchor, at or
after the convolver's tv, and not across a swap or an idle spell.  Here: every
scenario runs through it on the fused and on the composition path, each one
reaches the states it exists for, and the same rules hold on the real
LookaheadClock (tests/host/la_xf_clock_check.cpp, built with the sanitizers)."""
import os
import shutil
import subprocess

import pytest

from matrix_la_ref import Q
from matrix_la_xf_ref import MODELLED, SCENARIOS, lengths_script, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def by_block(m):
    """t -> {convolver: record}"""
    out = {}
    for r in m.blocks:
        out.setdefault(r["t"], {})[r["c"]] = r
    return out


def kinds(rec):
    return {r for r in rec["roles"]} if rec["live"] and rec["far"] else set()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composition"])
@pytest.mark.parametrize("name", MODELLED)
def test_every_window_read_is_valid(name, fused):
    m = model(name, fused)   # (asserts inside)
    ncalls = sum(1 for kind, _ in lengths_script(name) if kind == "call")
    assert len(m.paths) == ncalls
    assert set(m.paths) <= ({0, 1, 2} if fused else {0})
    served = sum(1 for r in m.blocks for x in r["roles"] if r["live"] and r["far"] and x is None)
    assert served > 0, "no block of the scenario is served from a window"


@pytest.mark.parametrize("name", ["fade", "ragged", "long-idle"])
def test_main_scripts_reach_their_states(name):
    m = model(name)
    assert set(m.paths) == {1, 2}
    both_anchor = full_beside_windows = idle = 0
    for t, recs in by_block(m).items():
        if len(recs) < 2:
            continue
        a, b = recs[0], recs[1]
        if a["live"] and b["live"]:
            ka, kb = kinds(a), kinds(b)
            both_anchor += "anchor" in ka and "anchor" in kb
            for x, y in ((ka, kb), (kb, ka)):
                # x's convolver sums in full while every output of the other is served or anchors
                full_beside_windows += "full" in x and "full" not in y and None in y
        else:
            idle += 1
            lone = a if not a["live"] else b
            assert lone["tv"] == t + 1 and lone["roles"] == [None] * len(lone["roles"])
    assert both_anchor > 0 and full_beside_windows > 0 and idle > 0, (both_anchor, full_beside_windows, idle)


def test_fade_is_longer_than_two_periods():
    """Both convolvers are live for more than 2 Q blocks, so the swapped-in one
    runs full sums, then anchors, then is served while the old one still is."""
    m = model("fade")
    first = m.paths.index(1)
    n = m.paths[first:].index(2)
    assert n > 2 * Q
    blocks = by_block(m)
    new = [blocks[t][1] for t in range(first, first + n)]
    assert kinds(new[0]) == {"full", "anchor"}                       # t = tv: only the anchoring outputs do not sum in full
    assert all("full" in kinds(r) for r in new[:Q - 1])
    assert all("full" not in kinds(r) for r in new[Q - 1:])           # steady from tv + Q - 1 on
    assert all(None in kinds(blocks[t][0]) for t in range(first, first + n))


def test_long_idle_invalidates_the_old_windows():
    m = model("long-idle")
    S = -(-SCENARIOS["long-idle"][1][3] // SCENARIOS["long-idle"][1][2])
    second = len(m.paths) - 1 - m.paths[::-1].index(1)  # last call of the second fade
    while m.paths[second - 1] == 1:
        second -= 1
    blocks = by_block(m)
    idle_run = 0
    t = second - 1
    while not blocks[t][0]["live"]:
        idle_run += 1
        t -= 1
    assert idle_run > S + 2
    back = blocks[second][0]
    assert back["live"] and back["tv"] == second
    assert None not in kinds(back), "convolver A read a window from before its idle spell"


def test_out_of_step_and_empty_take_the_composition():
    for name in ("out-of-step", "empty"):
        m = model(name)
        assert m.paths[:4] == [2] * 4 and set(m.paths[4:]) == {0}, (name, m.paths)
    m = model("pending")
    assert m.paths[:8] == [2] * 5 + [1] * 3 and set(m.paths[8:]) == {0}, m.paths


def test_few_segments_have_no_far_rows():
    for segs in (1, 2, 8):
        assert not any(r["far"] for r in model(f"S{segs}").blocks)
    assert all(r["far"] for r in model("S9").blocks)


def test_clock_rules_on_the_real_clock(tmp_path):
    """tests/host/la_xf_clock_check.cpp over csrc/block_walk.hpp, with
    AddressSanitizer and UBSan, as a stand-alone program."""
    cxx = shutil.which("clang++") or shutil.which("g++")
    if cxx is None and os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        cxx = "/opt/rocm/lib/llvm/bin/clang++"
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "la_xf_clock_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "fft-convolution_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "la_xf_clock_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert "la_xf_clock_check: ok" in p.stdout
