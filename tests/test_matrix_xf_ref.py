"""The yardstick of tests/test_gpu_matrix_xf.py, checked on the CPU: the summed
crossfade oracle (matrix_xf_ref.SummedCrossfadeOracle).  It validates the
reference, not the MatrixCrossfadeConvolver:
  - before any update it is the summed FFTConvolver oracle;
  - once a fade has completed (active_seg_count unchanged) it agrees with f64
    direct convolution with the new responses;
  - the device's order of operations -- an f32 mix of the per-output sums -- is
    modelled with the oracle's own Crossfader and sits 6.7e-8 (full blocks) and
    7.7e-8 (ragged) from the f64 sum of the per-instance mixes, far below REL_TOL."""
import numpy as np
import pytest

from common import REL_TOL, max_rel_err
from matrix_ref import SummedOracle, direct, make
from matrix_xf_ref import SummedCrossfadeOracle, calls, run_script

SHAPES = [
    # name, I, O, B, L, max_buffer_size, crossfade_samples, calls before the update, calls after it
    ("blocks", 3, 2, 64, 1000, 64, 96, 20, 12),
    ("ragged", 3, 2, 64, 1000, 100, 250, 9, 9),
]


def _new(oracle_mod, h, B, L, mbs, fade):
    return SummedCrossfadeOracle(oracle_mod, h, B, L, max_response_length=L, max_buffer_size=mbs,
                                 crossfade_samples=fade)


@pytest.mark.parametrize("name,I,O,B,L,mbs,fade,n0,n1", SHAPES)
def test_equals_summed_oracle_before_any_update(oracle_mod, name, I, O, B, L, mbs, fade, n0, n1):
    h, x = make(21, I, O, L, n0 * mbs)
    ys, flags = run_script(_new(oracle_mod, h, B, L, mbs, fade), x, calls(n0, mbs), mbs)
    plain = SummedOracle(oracle_mod, h, B, L).run(x, [mbs] * n0)
    assert not any(flags)
    e = max_rel_err(np.concatenate(ys, axis=1), plain)
    print(f"{name}: summed crossfade oracle vs summed oracle {e:.3e}")
    assert e <= 1e-12


def test_agrees_with_direct_after_the_fade(oracle_mod):
    """20 blocks with h, update(h2) of the same length, 12 blocks: the fade
    (64 hold + 96 samples) ends in the third block; the swapped-in convolver
    lost its overlap at update(), which only the block after the update
    misses -- from one block after the fade the output is x * h2."""
    I, O, B, L, fade = 3, 2, 64, 1000, 96
    h, x = make(22, I, O, L, 32 * B)
    h2, _ = make(23, I, O, L, 1)
    ref = _new(oracle_mod, h, B, L, B, fade)
    ys, flags = run_script(ref, x, calls(20, B) + [("update", h2)] + calls(12, B), B)
    assert flags == [False] * 20 + [True] * 2 + [False] * 10
    y = np.concatenate(ys, axis=1)
    first = 24 * B  # one block after the call in which the fade completed
    d = direct(oracle_mod, x, h2)
    e = max_rel_err(y[:, first:], d[:, first:])
    print(f"after the fade vs f64 direct with the new responses {e:.3e}")
    assert e <= 1e-6
    assert max_rel_err(y[:, :20 * B], direct(oracle_mod, x, h)[:, :20 * B]) <= 1e-6


class MixOfSums:
    """What the device computes, from oracle parts: A and B as summed
    FFTConvolver oracles, their per-output sums rounded to f32 and mixed by
    the reference's Crossfader (one per output, in lockstep).  Only what the
    shapes here need: updates arrive while no fade is under way."""

    def __init__(self, oracle, h, B, L, mbs, fade):
        self.conv = [SummedOracle(oracle, h, B, L), SummedOracle(oracle, h, B, L)]
        self.xf = [oracle.Crossfader.new(fade, min(mbs, L)) for _ in range(np.asarray(h).shape[0])]
        self.target, self.mbs = 0, mbs

    def update(self, h):
        assert not self.xf[0].state[0]
        self.target ^= 1
        self.conv[self.target].update(h)
        for f in self.xf:
            f.fade_into(self.target)

    def is_crossfading(self):
        return self.xf[0].state[0]

    def process(self, x, out_len):
        sa = self.conv[0].process(x[:, :self.mbs]).astype(np.float32)
        sb = self.conv[1].process(x[:, :self.mbs]).astype(np.float32)
        return np.array([[f.mix(float(sa[o, j]), float(sb[o, j])) for j in range(out_len)]
                         for o, f in enumerate(self.xf)], np.float32)


@pytest.mark.parametrize("name,I,O,B,L,mbs,fade,n0,n1", SHAPES)
def test_mix_of_sums_is_within_tolerance(oracle_mod, name, I, O, B, L, mbs, fade, n0, n1):
    """The f32 mix of per-output sums against the f64 sum of per-instance
    mixes, through a fade to B and a fade back to A."""
    h, x = make(24, I, O, L, (n0 + 2 * n1) * mbs)
    h2, _ = make(25, I, O, L, 1)
    h3, _ = make(26, I, O, L, 1)
    script = calls(n0, mbs) + [("update", h2)] + calls(n1, mbs) + [("update", h3)] + calls(n1, mbs)
    ys, flags = run_script(_new(oracle_mod, h, B, L, mbs, fade), x, script, mbs)
    ym, fm = run_script(MixOfSums(oracle_mod, h, B, L, mbs, fade), x, script, mbs)
    assert flags == fm and any(flags) and not flags[-1]
    ref, got = np.concatenate(ys, axis=1), np.concatenate(ym, axis=1)
    worst = max(max_rel_err(got[o], ref[o]) for o in range(O))
    print(f"{name}: f32 mix of sums vs f64 sum of mixes {worst:.3e}")
    assert worst <= REL_TOL
