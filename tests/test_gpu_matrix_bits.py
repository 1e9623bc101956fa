"""The matrix families' output bits against a recorded run.  The other matrix
tests compare the families with each other (bitwise) and with an f64 reference
(common.REL_TOL); a change that moved the order of summation in every family
alike would pass them all.  tests/golden/matrix_bits.json (written by
scripts/gen_matrix_bits.py on the MI355X before the matrix kernels were put on
shared row walks, far walks and finish pieces) holds, per case of
tests/matrix_bits.py, the SHA-256 of the inputs and of the output: each case is
recomputed and must give the same hashes.  A differing input hash means the
random stream moved (numpy), not the kernels."""
import json
import os

import pytest

from matrix_bits import CASES, run_case

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matrix_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_fixture_lists_every_case():
    assert sorted(GOLDEN) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_bits(amd, name):
    got, want = run_case(amd, name), GOLDEN[name]
    print(f"{name}: max|y| {got['max_abs']!r} (recorded {want['max_abs']!r})")
    assert got["in"] == want["in"], f"{name}: the inputs differ from the recorded run's (the random stream, not the kernels)"
    assert got["out"] == want["out"], f"{name}: output bits differ from the recorded run (max|y| {got['max_abs']!r}, " \
                                      f"recorded {want['max_abs']!r})"
