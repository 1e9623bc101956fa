"""The bookkeeping the SparseMatrixLookaheadConvolver adds to the lookahead
matrix, checked on the CPU through matrix_sp_la_ref (a model, not the product):
the class-ordered far plan lists every (output, part) once, the steady far grid
is exactly the anchoring class, the grid sizes are the sums the host computes,
the W = Q and W = 1 far walks over a pair list agree, near and far rows together
are every listed row once, every GPU shape has the properties it is there for,
and a float32 replay that really serves blocks from windows agrees with the
sparse summed oracle."""
import numpy as np
import pytest

import matrix_la_ref as la
import matrix_sp_ref
from common import REL_TOL, max_rel_err
from matrix_la_ref import Q
from matrix_paths import geo
from matrix_sp_la_ref import (MAIN, PROPERTIES, SHAPES, SpLaModel, anchors, counts, far_grid, far_parts, far_plan,
                              far_walk, host_counts, near_parts, near_plan, shape_len, shape_pairs)
from matrix_sp_ref import SparseSummedOracle

PATTERNS = [(s.name, [len(c) for c in s.cols], s.S) for s in SHAPES] + [
    ("one-output", [5], 40), ("nineteen", [(7 * o) % 5 for o in range(19)], 23), ("no-far", [3, 0, 2], 8),
    ("one-segment", [2, 1], 1), ("wide", [64, 0, 1, 130], 188)]


@pytest.mark.parametrize("name,ks,act", PATTERNS, ids=[p[0] for p in PATTERNS])
@pytest.mark.parametrize("q", [4, 8])
def test_class_ordered_plan_lists_every_part_once(name, ks, act, q):
    desc, coff, fplan = far_plan(ks, act, q)
    want = [(o, p) for o, k in enumerate(ks) for p in range(far_parts(k, act, q))]
    assert sorted((o, p) for o, p, _ in desc) == want
    # keys (o % q, o, p) ascending; a descriptor's far row is its (o, p) in output order
    assert [(o % q, o, p) for o, p, _ in desc] == sorted((o % q, o, p) for o, p, _ in desc)
    assert sorted(r for _, _, r in desc) == list(range(len(want))) and fplan[-1] == len(want)
    assert all(r == fplan[o] + p for o, p, r in desc)
    assert len(coff) == q + 1 and coff[0] == 0 and coff[q] == len(desc)
    for c in range(q):
        assert {o % q for o, _, _ in desc[coff[c]:coff[c + 1]]} <= {c}
    # the near grid: every (o, p) once, in output order, at least one part per output
    wg, nplan = near_plan(ks, act, q)
    assert wg == [(o, p) for o, k in enumerate(ks) for p in range(near_parts(k, act, q))]
    assert all(nplan[o + 1] > nplan[o] for o in range(len(ks)))
    # the sums the host computes from its copy of rowptr
    assert host_counts(ks, act, q) == (len(wg), len(desc), coff)


@pytest.mark.parametrize("name,ks,act", PATTERNS, ids=[p[0] for p in PATTERNS])
@pytest.mark.parametrize("t0", [0, 5, 13])
def test_far_grid_holds_the_outputs_with_work(name, ks, act, t0):
    """3 Q blocks after an invalidation at block t0: every output with far rows
    and a role has all its far parts in the grid exactly once; in the steady
    state the grid is exactly the anchoring class, and all of it anchors."""
    tv = t0
    for t in range(t0, t0 + 3 * Q):
        grid = far_grid(t, tv, ks, act)
        assert len(set(grid)) == len(grid)
        listed = {(o, p) for o, p, _ in grid}
        for o, k in enumerate(ks):
            if la.role(t, tv, o) is not None:
                assert all((o, p) in listed for p in range(far_parts(k, act)))
        if la.steady(t, tv):
            assert listed == {(o, p) for o in range(t % Q, len(ks), Q) for p in range(far_parts(ks[o], act))}
            assert all(la.role(t, tv, o) == "anchor" for o, _ in listed)
            _, coff, _ = far_plan(ks, act)
            assert len(grid) == coff[t % Q + 1] - coff[t % Q]
        else:
            assert len(grid) == host_counts(ks, act)[1]
    # anchors(): the outputs of the class that have pairs
    for t in range(2 * Q):
        n = anchors(t, ks, act, 0)
        assert n == (sum(1 for o in range(t % Q, len(ks), Q) if ks[o] > 0) if act > Q else 0)
        assert anchors(t, ks, act, 0, windows=False) == 0 and anchors(t, ks, act, act) == 0


@pytest.mark.parametrize("B,cols_o,act", [(64, [0, 4, 1], 40), (64, [0, 1, 2, 3, 4, 5], 40), (32, list(range(12)), 12),
                                          (256, [2, 0], 20), (512, [0, 1, 2], 12), (128, [3], 9)])
def test_window_and_full_walk_agree_over_a_pair_list(B, cols_o, act):
    """Accumulator j of the W = Q walk at block a lists the (pair, input, s, ring
    index) sequence of the W = 1 walk of block a + j, for every part and group."""
    k = len(cols_o)
    for cur in sorted({0, 1, act // 2, act - 1}):
        for p in range(far_parts(k, act)):
            for g in range(geo(B).G):
                win = far_walk(B, cols_o, act, cur, p, g, Q)
                c = cur
                for j in range(Q):
                    assert win[j] == far_walk(B, cols_o, act, c, p, g, 1)[0], (cur, p, g, j)
                    assert all(i == cols_o[e] for e, i, _, _ in win[j])
                    c = la.next_cur(c, act)


@pytest.mark.parametrize("s", SHAPES, ids=[s.name for s in SHAPES])
def test_near_and_far_visit_every_listed_row_once(s):
    pairs = shape_pairs(s)
    rows = matrix_sp_ref.rows_of(pairs, len(s.cols))
    G = geo(s.B).G
    seen = {}
    for o, row in enumerate(rows):
        k = len(row)
        for p in range(near_parts(k, s.S)):
            for g in range(G):
                for e, sg in la.near_rows(s.B, k, s.S, p, g):
                    assert 1 <= sg < min(Q, s.S)
                    seen[(row[e][0], sg)] = seen.get((row[e][0], sg), 0) + 1
        for p in range(far_parts(k, s.S)):
            for g in range(G):
                for e, sg in la.far_rows(s.B, k, s.S, p, g):
                    assert Q <= sg < s.S
                    seen[(row[e][0], sg)] = seen.get((row[e][0], sg), 0) + 1
    assert seen == {(n, sg): 1 for n in range(len(pairs)) for sg in range(1, s.S)}


@pytest.mark.parametrize("s", SHAPES, ids=[s.name for s in SHAPES])
def test_gpu_shapes_run_what_they_are_there_for(s):
    matrix_sp_ref.check_pairs(shape_pairs(s), s.I, len(s.cols))
    assert counts(shape_pairs(s), len(s.cols)) == [len(c) for c in s.cols]
    for name in s.why:
        assert PROPERTIES[name](s), (s.name, name)


def test_replay_against_the_sparse_summed_oracle(oracle_mod):
    """The float32 replay on outputs 1..4 of the main shape (1, 0, 2 and 3 pairs),
    30 blocks with an update after block 13: blocks really come from windows,
    and the result stays within REL_TOL of the sparse summed oracle; the replay
    without windows too."""
    s = MAIN
    cols = s.cols[1:5]
    pairs = matrix_sp_ref.from_rows(cols)
    O, B, L = len(cols), s.B, shape_len(s)
    h, x = matrix_sp_ref.make(43, pairs, s.I, L, 30 * B)
    h2, _ = matrix_sp_ref.make(44, pairs, s.I, L - 70, 1)
    ref = SparseSummedOracle(oracle_mod, pairs, h, s.I, O, B, L)
    win = SpLaModel(pairs, h, s.I, O, B, L)
    full = SpLaModel(pairs, h, s.I, O, B, L, windows=False)
    for k in range(30):
        if k == 13:
            for m in (ref, win, full):
                m.update(h2)
        blk = x[:, k * B:(k + 1) * B]
        r = ref.process(blk)
        assert not r[1].any()
        for m, what in ((win, "windows"), (full, "full sums")):
            y = m.process_block(blk)
            assert not y[1].any()
            e = max_rel_err(y, r)
            assert e <= REL_TOL, f"{what}, block {k}: {e:.3e}"
    assert win.tally("anchored") > 0 and win.tally("from_window") > 4 * win.tally("anchored") and win.tally("full") > 0
    assert full.tally("anchored") == full.tally("from_window") == 0
