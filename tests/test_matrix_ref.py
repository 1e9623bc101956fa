"""The yardstick of tests/test_gpu_matrix.py, checked on the CPU: the summed
oracle reference (matrix_ref.SummedOracle) agrees with f64 direct convolution
within 1e-6 of max|ref| on the full-block, ragged and split-row shapes.  It
validates the reference, not the MatrixConvolver."""
import pytest

from common import max_rel_err
from matrix_ref import RAGGED_64, RAGGED_256, SummedOracle, direct, make


@pytest.mark.parametrize("name,I,O,B,L,lengths", [
    ("full", 3, 2, 64, 1000, [64] * 40),
    ("ragged64", 3, 2, 64, 1000, RAGGED_64),
    ("ragged256", 2, 2, 256, 1500, RAGGED_256),
    ("split", 4, 2, 32, 4096, [32] * 140),
    ("one-part", 1, 2, 64, 200, [64] * 10),
])
def test_summed_oracle_matches_direct(oracle_mod, name, I, O, B, L, lengths):
    h, x = make(1, I, O, L, sum(lengths))
    ref = SummedOracle(oracle_mod, h, B, L)
    y = ref.run(x, lengths)
    d = direct(oracle_mod, x, h)
    e = max_rel_err(y, d)
    print(f"{name}: summed oracle vs f64 direct {e:.3e}")
    assert e <= 1e-6, (name, e)
