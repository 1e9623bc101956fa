"""The yardstick of tests/test_gpu_matrix.py, checked on the CPU: the summed
oracle reference (matrix_ref.SummedOracle) agrees with f64 direct convolution
within 1e-6 of max|ref| on the full-block, ragged and split-row shapes and on
the path shapes of matrix_paths.SHAPES.  It validates the reference, not the
MatrixConvolver.  The rest checks the CPU model of the kernels' control flow
(matrix_paths): every path shape still reaches the loops it is there for."""
import numpy as np
import pytest

from common import max_rel_err
from matrix_paths import (CAPPED, PROPERTIES, SHAPES, capped_lengths, geo, parts, shape_blocks, shape_id, shape_len,
                          walk)
from matrix_ref import RAGGED_64, RAGGED_256, BlockModel, SummedOracle, direct, make


@pytest.mark.parametrize("name,I,O,B,L,lengths", [
    ("full", 3, 2, 64, 1000, [64] * 40),
    ("ragged64", 3, 2, 64, 1000, RAGGED_64),
    ("ragged256", 2, 2, 256, 1500, RAGGED_256),
    ("split", 4, 2, 32, 4096, [32] * 140),
    ("one-part", 1, 2, 64, 200, [64] * 10),
] + [(shape_id(s), s.I, s.O, s.B, shape_len(s), [s.B] * shape_blocks(s)) for s in SHAPES]
  + [("ragged-" + shape_id(s), s.I, s.O, s.B, shape_len(s), list(capped_lengths(s))) for s in CAPPED])
def test_summed_oracle_matches_direct(oracle_mod, name, I, O, B, L, lengths):
    h, x = make(1, I, O, L, sum(lengths))
    ref = SummedOracle(oracle_mod, h, B, L)
    y = ref.run(x, lengths)
    d = direct(oracle_mod, x, h)
    e = max_rel_err(y, d)
    print(f"{name}: summed oracle vs f64 direct {e:.3e}")
    assert e <= 1e-6, (name, e)


@pytest.mark.parametrize("s", SHAPES, ids=shape_id)
def test_shape_reaches_its_paths(s):
    """Each shape of the GPU path tests runs the kernel paths it is listed
    for, by the model of matrix_row_walk / matrix_b_kernel; the walk visits every
    row exactly once."""
    g, w = geo(s.B), walk(s.B, s.I, s.S)
    print(f"{shape_id(s)}: {g} {w}")
    assert w.exact, f"shape {shape_id(s)}: the row walk is not a partition of the rows"
    for k in s.why:
        assert PROPERTIES[k](s, g, w), f"shape {shape_id(s)} no longer reaches path {k!r}: {g} {w}"


def test_model_reproduces_the_old_shapes():
    """The shapes tests/test_gpu_matrix.py had before the path shapes: only
    B = 2048 and 8192 ever entered the unrolled loop (1 and 6 iterations)."""
    table = {(64, 3, 16): (45, 1, 0, 45), (64, 3, 32): (93, 2, 0, 93), (256, 2, 6): (10, 1, 0, 10),
             (32, 2, 4): (6, 1, 0, 6), (128, 2, 4): (6, 1, 0, 6), (512, 2, 4): (6, 1, 0, 6),
             (2048, 2, 4): (6, 1, 1, 2), (8192, 2, 4): (6, 1, 6, 0), (32, 4, 128): (508, 8, 0, 508)}
    for (B, I, S), want in table.items():
        w = walk(B, I, S)
        assert (w.R, w.P, w.unrolled, w.tail) == want, (B, I, S, w)


def test_walk_partitions_the_rows():
    """matrix_row_walk's (part, group) walk visits every row once for every block
    size, 1..13 inputs and 0..70 active segments (P = 1..15), and above the
    P cap."""
    for log2b in range(5, 14):
        for I in range(1, 14):
            for act in list(range(0, 12)) + [33, 70]:
                w = walk(1 << log2b, I, act)
                assert w.exact and w.unrolled * geo(1 << log2b).U + w.tail == w.R, (1 << log2b, I, act, w)
    for B in (32, 64, 1024):
        assert walk(B, 67, 70).exact and walk(B, 67, 70).rpp > 64


def test_update_sequence_changes_parts():
    """The steps of test_update_changes_parts (B 32, I 4, S 128): P goes 8 ->
    3 -> 8 -> 1 (-> 1 with no active segment)"""
    assert [parts(4, a) for a in (128, 40, 128, 1, 0)] == [8, 3, 8, 1, 1]
    w = walk(32, 4, 40)
    assert (w.R, w.P, w.rpp, w.exact) == (156, 3, 52, True)


def test_block_model_matches_direct(oracle_mod):
    """matrix_ref.BlockModel (the vectorised f64 reference of
    test_many_pairs) against f64 direct convolution, and against the summed
    oracle across an update."""
    I, O, B, L = 2, 3, 64, 100
    h, x = make(2, I, O, L, 6 * B)
    h2, _ = make(3, I, O, L, 1)
    m = BlockModel(h, B, L)
    y = np.concatenate([m.process_block(x[:, k * B:(k + 1) * B]) for k in range(4)], axis=1)
    e = max_rel_err(y, direct(oracle_mod, x[:, :4 * B], h))
    print(f"block model vs f64 direct {e:.3e}")
    assert e <= 1e-12
    ref = SummedOracle(oracle_mod, h, B, L)
    ref.run(x[:, :4 * B], [B] * 4)
    m.update(h2)
    ref.update(h2)
    y = np.concatenate([m.process_block(x[:, k * B:(k + 1) * B]) for k in (4, 5)], axis=1)
    e = max_rel_err(y, ref.run(x[:, 4 * B:], [B] * 2))
    print(f"block model vs summed oracle after update {e:.3e}")
    assert e <= 1e-6
