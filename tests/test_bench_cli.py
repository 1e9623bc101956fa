"""bench.py's launch contract on the CPU: `--gpus N` without a launcher must
run N rank processes (or fail) -- never report N GPUs from one process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from common import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                          text=True, timeout=120)


def test_gpus2_without_launcher_spawns_two_ranks():
    r = _run(["--gpus", "2", "--spawn-probe"])
    assert r.returncode == 0, r.stderr
    ranks = sorted((json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")), key=lambda d: d["rank"])
    assert [(d["rank"], d["local_rank"], d["world"]) for d in ranks] == [(0, 0, 2), (1, 1, 2)]


def test_launcher_world_size_wins():
    r = _run(["--gpus", "8", "--spawn-probe"], {"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1"})
    assert r.returncode == 0, r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines == [{"rank": 0, "local_rank": 0, "world": 1}]  # one process runs, one rank is reported
    assert "running 1 rank" in r.stderr


def test_full_and_dump_outputs_are_options():
    r = _run(["--gpus", "1", "--full", "--dump-outputs", "unused", "--spawn-probe"])
    assert r.returncode == 0, r.stderr
    assert [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")] == [{"rank": 0, "local_rank": 0, "world": 1}]


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(amd, oracle_mod, tmp_path):
    """A plain run (no --full) times exactly --steps steps, runs no baseline or
    profiler pass, and --dump-outputs writes the last timed step's output block:
    block warmup + steps - 1 of every channel's stream (the ring's dry blocks in
    turn), against the oracle.  S = 67: the lookahead step with all three
    anchor levels."""
    from fftconv_amd import shard

    C, B, L, ring, warmup, steps = 6, 256, 17000, 4, 5, 7
    out = tmp_path / "dump"
    r = _run(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--channels", str(C), "--block", str(B),
              "--ir", str(L), "--ring", str(ring), "--dump-outputs", str(out)])
    assert r.returncode == 0, r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["steps"] == steps and line["warmup"] == warmup and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0 and line["unit"] == "MSamples/s" and line["higher_is_better"] is True
    # value = samples per second of the timed steps (ms_per_step is rounded to 1e-5 ms)
    assert abs(line["value"] - C * B / line["ms_per_step"] / 1e3) <= 1e-2 * line["value"]
    assert line["cpu_baseline"] is None and line["roofline"]["traffic"] is None
    assert line["roofline"]["rocprof_calls"] == 0
    assert sorted(p.name for p in out.iterdir()) == ["y.npy"]
    y = np.load(out / "y.npy")
    assert y.dtype == np.float32 and y.shape == (C, B)
    hs = shard.synth_irs(range(C), L)
    dry = shard.synth_dry(range(C), ring, B)
    for c in range(C):
        ref = oracle_mod.FFTConvolver.init(hs[c], B, L)
        for i in range(warmup + steps):
            exp = ref.process(dry[i % ring, c])
        assert_close(y[c], exp, what=f"channel {c}")


def test_failing_rank_fails_the_job():
    # rank processes that cannot start (a bogus backend on a CPU box) must surface a non-zero status
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--channels", "1", "--ir", "64", "--backend", "nonexistent",
              "--no-cpu-baseline", "--pmc", "off"])
    assert r.returncode != 0
    assert not any(l.startswith("{") for l in r.stdout.splitlines())
