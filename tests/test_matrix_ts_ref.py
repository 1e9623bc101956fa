"""The yardstick of tests/test_gpu_matrix_ts.py, checked on the CPU: the summed
two-stage oracle (matrix_ts_ref.SummedTwoStageOracle) and the geometry table
the GPU tests rely on.  It validates the reference, not the
MatrixTwoStageConvolver:
  - the summed oracle agrees with f64 direct convolution over a run longer
    than 2T + L, so all three stages have contributed;
  - T, the three stages' seg counts and the period of every GPU test shape are
    the listed values, in the reference's own f32 arithmetic."""
import numpy as np
import pytest

from common import REL_TOL, max_rel_err
from matrix_ref import direct, make
from matrix_ts_ref import RAGGED, SHAPES, SummedTwoStageOracle, stage_seg_counts


@pytest.mark.parametrize("lengths", ["aligned", "ragged"])
def test_summed_oracle_agrees_with_direct(oracle_mod, lengths):
    I, O, head, L, T, _, _ = SHAPES["three-stage"]
    calls = [head] * 72 if lengths == "aligned" else RAGGED + [64] * 30
    n = sum(calls)
    assert n > 2 * T + L
    h, x = make(51, I, O, L, n)
    ref = SummedTwoStageOracle(oracle_mod, h, head, L)
    assert ref.tail_block_size == T
    y = ref.run(x, calls)
    d = direct(oracle_mod, x, h)
    worst = max(max_rel_err(y[o], d[o]) for o in range(O))
    print(f"{lengths}: summed two-stage oracle vs f64 direct {worst:.3e}")
    assert worst <= REL_TOL
    # reset, then the same run: the same samples
    ref.reset()
    assert np.array_equal(ref.run(x, calls), y)


@pytest.mark.parametrize("name", list(SHAPES))
def test_shape_table(oracle_mod, name):
    I, O, head, L, T, segs, calls = SHAPES[name]
    t, s = stage_seg_counts(oracle_mod, head, L)
    assert (t, s) == (T, segs)
    assert T % head == 0 and T <= 8192
    h, _ = make(52, 1, 1, L, 1)
    assert oracle_mod.TwoStageFFTConvolver.init(h[0, 0], head, L).tail_block_size == T
    if name == "three-stage":
        assert T // head == 8 and calls == 5 * 8
    if name == "split":
        assert calls > 3 * (T // head) and 3 * (segs[0] - 1) == 93
    if name in ("head+tail0", "period-one"):
        assert T == head


def test_geometry_limits(oracle_mod):
    """the header's examples: head 512 / L 262,144 is past the matrix tail's
    limit, head 64 and head 256 are inside it; head 48 does not divide its T"""
    assert oracle_mod.compute_tail_block_size(512, 262144) == 16384
    assert oracle_mod.compute_tail_block_size(64, 262144) == 4096
    assert oracle_mod.compute_tail_block_size(256, 262144) == 8192
    assert oracle_mod.compute_tail_block_size(48, 3000) == 512
