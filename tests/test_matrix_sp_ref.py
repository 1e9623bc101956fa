"""The yardstick of tests/test_gpu_matrix_sparse.py, checked on the CPU: the
sparse summed oracle (matrix_sp_ref.SparseSummedOracle) equals
matrix_ref.SummedOracle exactly on a full pattern and agrees with f64 direct
convolution over the listed pairs within 1e-6 of max|ref| (the bound
tests/test_matrix_ref.py holds the dense reference to) on the patterns of the
GPU tests.  It validates the reference, not the SparseMatrixConvolver.  The
rest checks, through the unchanged CPU model of the dense kernels' control flow
(matrix_paths, with inputs := k_o), that every output of every bitwise shape
still reaches the loops it is there for."""
import numpy as np
import pytest

import matrix_ref
from common import max_rel_err
from matrix_paths import geo, parts, walk
from matrix_ref import RAGGED_64, RAGGED_256, SummedOracle
from matrix_sp_ref import (BITWISE, PATTERN_1, PATTERN_256, PROPERTIES, SparseSummedOracle, check_pairs, direct,
                           from_rows, make, rows_of, sp_blocks, sp_len)


def test_full_pattern_equals_the_dense_summed_oracle(oracle_mod):
    """Every pair listed: the same instances summed in the same order, so the
    f64 sums are equal, not merely close; states too, across an update."""
    I, O, B, L = 3, 2, 64, 1000
    h, x = matrix_ref.make(5, I, O, L, sum(RAGGED_64))
    h2, _ = matrix_ref.make(6, I, O, 700, 1)
    pairs = from_rows([list(range(I))] * O)
    dense = SummedOracle(oracle_mod, h, B, L)
    sparse = SparseSummedOracle(oracle_mod, pairs, h.reshape(O * I, L), I, O, B, L)
    pos = 0
    for k, n in enumerate(RAGGED_64):
        if k == 12:
            dense.update(h2)
            sparse.update(h2.reshape(O * I, 700))
        blk = x[:, pos:pos + n]
        assert np.array_equal(dense.process(blk), sparse.process(blk)), k
        assert dense.state() == sparse.state()
        pos += n


@pytest.mark.parametrize("name,pairs,I,O,B,L,lengths", [
    ("full", PATTERN_1, 5, 4, 64, 1000, [64] * 40),
    ("ragged64", PATTERN_1, 5, 4, 64, 1000, RAGGED_64),
    ("ragged256", PATTERN_256, 3, 2, 256, 1500, RAGGED_256),
] + [(s.name, from_rows(s.cols), s.I, len(s.cols), s.B, sp_len(s), [s.B] * sp_blocks(s)) for s in BITWISE])
def test_sparse_oracle_matches_direct(oracle_mod, name, pairs, I, O, B, L, lengths):
    h, x = make(1, pairs, I, L, sum(lengths))
    ref = SparseSummedOracle(oracle_mod, pairs, h, I, O, B, L)
    y = ref.run(x, lengths)
    d = direct(oracle_mod, x, pairs, h, O)
    e = max_rel_err(y, d)
    print(f"{name}: sparse summed oracle vs f64 direct {e:.3e}")
    assert e <= 1e-6, (name, e)
    for o, row in enumerate(rows_of(pairs, O)):
        if not row:
            assert not y[o].any() and not d[o].any(), f"{name}: output {o} has no pair"


def test_patterns_are_valid():
    for pairs, I, O in [(PATTERN_1, 5, 4), (PATTERN_256, 3, 2)] + [(from_rows(s.cols), s.I, len(s.cols))
                                                                  for s in BITWISE]:
        check_pairs(pairs, I, O)
    rows = rows_of(PATTERN_1, 4)
    assert [len(r) for r in rows] == [5, 1, 0, 2]
    assert {i for _, i in PATTERN_256} == {0, 2}  # (input 1 is unused)
    s = BITWISE[0]
    assert s.cols[2][0] == 0 and s.cols[2][-1] == s.I - 1 and len(s.cols[2]) == 11


@pytest.mark.parametrize("s", BITWISE, ids=lambda s: s.name)
def test_outputs_reach_their_paths(s):
    """Each output of a bitwise shape runs, by the model of matrix_row_walk with
    inputs := k_o, the loops it is listed for; the walk visits every row of the
    output's list exactly once."""
    assert len(s.why) == len(s.cols)
    g = geo(s.B)
    for o, (cols, why) in enumerate(zip(s.cols, s.why)):
        k = len(cols)
        w = walk(s.B, k, s.S)
        print(f"{s.name} output {o}: k {k} {g} {w}")
        assert w.exact and w.P == parts(k, s.S)
        for name in why:
            assert PROPERTIES[name](g, w, k), f"{s.name} output {o} (k = {k}) no longer reaches {name!r}: {g} {w}"


def test_skewed_grid_is_compact():
    """The skewed shape's MAC grid: sum of P_o, far below outputs * max P."""
    s = BITWISE[0]
    P = [parts(len(c), s.S) for c in s.cols]
    assert P == [64, 3, 24] and sum(P) < len(P) * max(P)


def test_update_sequence_changes_parts():
    """The update test's lengths on PATTERN_1 (B 64): 1000 -> 700 -> 1000 ->
    130 -> 0 samples move P_0 2 -> 1 -> 2 -> 1 -> 1; an output without pairs
    keeps one (all-zero) part."""
    ks = [len(r) for r in rows_of(PATTERN_1, 4)]
    acts = [-(-n // 64) for n in (1000, 700, 1000, 130, 0)]
    assert [[parts(k, a) for k in ks] for a in acts] == [[2, 1, 1, 1], [1, 1, 1, 1], [2, 1, 1, 1], [1, 1, 1, 1],
                                                         [1, 1, 1, 1]]
