"""The yardstick of tests/test_gpu_matrix_sparse_xf.py, checked on the CPU: the
sparse summed crossfade oracle (matrix_sp_xf_ref.SparseSummedCrossfadeOracle)
and the walk properties the GPU scenarios' shapes are there for.  It validates
the reference and the shapes, not the SparseMatrixCrossfadeConvolver:
  - with a fully listed pattern it is matrix_xf_ref.SummedCrossfadeOracle, exactly;
  - an output without pairs is all zeros through a fade;
  - every scenario shape reaches the loops it is named for (matrix_paths.walk
    with inputs := k_o).  If an edit breaks one, change the shape, not the
    property."""
import numpy as np
import pytest

from matrix_paths import geo, walk
from matrix_ref import make as make_dense
from matrix_sp_ref import PATTERN_1, PATTERN_256, from_rows, make, rows_of
from matrix_sp_xf_ref import SparseSummedCrossfadeOracle
from matrix_xf_ref import SummedCrossfadeOracle, calls, run_script


def test_fully_listed_equals_the_dense_oracle(oracle_mod):
    I, O, B, L, mbs, fade = 3, 2, 64, 500, 100, 250
    h, x = make_dense(71, I, O, L, 20 * mbs)
    h2, _ = make_dense(72, I, O, L, 1)
    alt = lambda n: [("call", 100 if k % 2 == 0 else 37) for k in range(n)]
    pairs = from_rows([list(range(I))] * O)
    kw = dict(max_response_length=L, max_buffer_size=mbs, crossfade_samples=fade)
    dense = SummedCrossfadeOracle(oracle_mod, h, B, L, **kw)
    sparse = SparseSummedCrossfadeOracle(oracle_mod, pairs, h.reshape(O * I, L), I, O, B, L, **kw)
    yd, fd = run_script(dense, x, alt(6) + [("update", h2)] + alt(14), mbs)
    ys, fs = run_script(sparse, x, alt(6) + [("update", h2.reshape(O * I, L))] + alt(14), mbs)
    assert fd == fs and any(fd) and not fd[-1]
    for a, b in zip(yd, ys):
        assert np.array_equal(a, b)
    # the init form
    dense = SummedCrossfadeOracle(oracle_mod, h, B, L)
    sparse = SparseSummedCrossfadeOracle(oracle_mod, pairs, h.reshape(O * I, L), I, O, B, L)
    yd, fd = run_script(dense, x, calls(3, B) + [("update", h2)] + calls(12, B), B)
    ys, fs = run_script(sparse, x, calls(3, B) + [("update", h2.reshape(O * I, L))] + calls(12, B), B)
    assert fd == fs and any(fd) and not fd[-1]
    for a, b in zip(yd, ys):
        assert np.array_equal(a, b)


def test_output_without_pairs_is_zero_through_a_fade(oracle_mod):
    I, O, B, L = 5, 4, 64, 300
    h, x = make(73, PATTERN_1, I, L, 12 * B)
    h2, _ = make(74, PATTERN_1, I, L, 1)
    ref = SparseSummedCrossfadeOracle(oracle_mod, PATTERN_1, h, I, O, B, L, max_response_length=L, max_buffer_size=B,
                                      crossfade_samples=100)
    ys, flags = run_script(ref, x, calls(3, B) + [("update", h2)] + calls(9, B), B)
    assert any(flags) and not flags[-1]
    y = np.concatenate(ys, axis=1)
    assert not y[2].any()
    assert all(np.abs(y[o]).max() > 0 for o in (0, 1, 3))


def k_of(pattern, outputs):
    return [len(r) for r in rows_of(pattern, outputs)]


def test_main_shape_walks():
    """PATTERN_1 at B 128, L 2045 (S 16): output 0 has 2 parts and groups that
    run both loops with a pair change inside an unrolled batch, output 1 is
    tail-only, output 2 has no pairs, output 3 is unrolled in some groups."""
    B, S = 128, 16
    assert -(-2045 // B) == S and geo(B).G > 1
    k = k_of(PATTERN_1, 4)
    assert k == [5, 1, 0, 2]
    w0, w1, w2, w3 = (walk(B, ko, S) for ko in k)
    assert w0.P == 2 and w0.groups_both > 0 and w0.cross_in_unrolled and w0.exact
    assert w1.R > 0 and w1.unrolled == 0 and w1.tail == w1.R and w1.exact
    assert w2.R == 0 and w2.P == 1 and w2.unrolled == 0 and w2.tail == 0
    assert w3.P == 1 and w3.unrolled > 0 and w3.tail > 0 and w3.exact
    # the plan after the update to 300 samples (test 8's plan rebuild): other part counts
    assert [walk(B, ko, 3).P for ko in k] == [1, 1, 1, 1] and walk(B, 5, 3).R == 10


def test_split_shape_parts():
    """PATTERN_1 at B 32, L 4096 (S 128): parts 10, 2, 1, 4."""
    assert [walk(32, ko, 128).P for ko in k_of(PATTERN_1, 4)] == [10, 2, 1, 4]


@pytest.mark.parametrize("B", [32, 128, 512, 2048, 4096, 8192])
def test_block_size_shapes(B):
    """PATTERN_256 at L = 3 B + 5 (S 4): B 2048, 4096 and 8192 run the unrolled
    loop at two, four and eight slots per thread."""
    k = k_of(PATTERN_256, 2)
    assert k == [2, 1]
    w = [walk(B, ko, 4) for ko in k]
    assert all(v.exact and v.R == 3 * ko for v, ko in zip(w, k))
    g = geo(B)
    if B >= 2048:
        assert (g.G, g.SPT) == (1, {2048: 2, 4096: 4, 8192: 8}[B]) and w[0].unrolled > 0
    if B == 512:
        # one slot per thread, no row groups: unrolled only with more rows (S 8)
        assert (g.G, g.SPT, g.U) == (1, 1, 8) and w[0].unrolled == 0
        w8 = walk(512, 2, 8)
        assert -(-(8 * 512 - 3) // 512) == 8 and w8.unrolled > 0 and w8.exact
