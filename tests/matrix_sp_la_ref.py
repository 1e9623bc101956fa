"""CPU model of the SparseMatrixLookaheadConvolver (fft-convolution_amd/csrc/
matrix_sp_la.hip): matrix_la_ref's schedule and walks used unchanged
with inputs := k_o (output o's pair count), plus what is new here -- the part
counts per output, the far plan ordered by anchor class, the grids launch A
runs, and a float32 replay (one matrix_la_ref.LaModel per output, started at the
output's anchor phase).  Also the GPU tests' shapes with the property each is
there for; tests/test_matrix_sp_la_ref.py checks them on the CPU."""
from collections import namedtuple

import numpy as np

import matrix_la_ref as la
from matrix_la_ref import Q
from matrix_paths import geo
from matrix_sp_ref import from_rows, rows_of


def counts(pairs, outputs):
    """k_o: pairs per output"""
    return [len(r) for r in rows_of(pairs, outputs)]


def near_parts(k, act, q=Q):
    """Pn_o (1 for an output without pairs: one all-zero part)"""
    return la.near_parts(k, act, q)


def far_parts(k, act, q=Q):
    """Pf_o (0 without far rows or without pairs)"""
    return la.far_parts(k, act, q) if k > 0 else 0


def near_plan(ks, act, q=Q):
    """launch A's compact near grid: (o, p) in output order, and the prefix sums"""
    wg, plan = [], [0]
    for o, k in enumerate(ks):
        wg += [(o, p) for p in range(near_parts(k, act, q))]
        plan.append(len(wg))
    return wg, plan


def far_plan(ks, act, q=Q):
    """the far descriptors ordered by (o % q, o, p) as (o, p, far row), the q + 1
    class offsets, and the far rows' prefix sums in output order"""
    fplan = [0]
    for k in ks:
        fplan.append(fplan[-1] + far_parts(k, act, q))
    desc, coff = [], []
    for c in range(q):
        coff.append(len(desc))
        for o in range(c, len(ks), q):
            desc += [(o, p, fplan[o] + p) for p in range(far_parts(ks[o], act, q))]
    coff.append(len(desc))
    return desc, coff, fplan


def host_counts(ks, act, q=Q):
    """what the host computes from its copy of rowptr to size the grids: the
    near total, the far total and the class offsets (no descriptor list)"""
    cls = [0] * q
    for o, k in enumerate(ks):
        cls[o % q] += far_parts(k, act, q)
    coff = [sum(cls[:c]) for c in range(q + 1)]
    return sum(near_parts(k, act, q) for k in ks), coff[q], coff


def far_grid(t, tv, ks, act, q=Q):
    """the far descriptors launch A of block t holds, in grid order: the
    anchoring class's range in the steady state, else all"""
    desc, coff, _ = far_plan(ks, act, q)
    if la.steady(t, tv, q):
        return desc[coff[t % q]:coff[t % q + 1]]
    return desc


def anchors(t, ks, act, cur, windows=True, q=Q):
    """outputs with at least one pair that anchor when block t starts"""
    if not windows or act <= q or cur >= act:
        return 0
    return sum(1 for o in range(t % q, len(ks), q) if ks[o] > 0)


def far_walk(B, cols_o, act, cur, p, g, W, q=Q):
    """matrix_la_ref.far_walk over a pair list: per accumulator the (entry e,
    input, s, ring index) it multiplies, in order"""
    return [[(e, cols_o[e], s, xi) for e, s, xi in lst] for lst in la.far_walk(B, len(cols_o), act, cur, p, g, W, q)]


class SpLaModel:
    """float32 replay on full blocks: output o is a matrix_la_ref.LaModel with
    k_o inputs and one output, fed x[col e], whose block count starts at (-o) %
    q so that it anchors on the handle's blocks t = o (mod q)."""

    def __init__(self, pairs, h, inputs, outputs, B, max_len, q=Q, windows=True):
        h = np.asarray(h, np.float32)
        self.rows = rows_of(pairs, outputs)
        self.B, self.O = B, outputs
        self.out = []
        for o, row in enumerate(self.rows):
            if not row:
                self.out.append(None)
                continue
            m = la.LaModel(h[[n for n, _ in row]][None], B, max_len, q, windows)
            m.t = m.tv = (-o) % q
            self.out.append(m)

    def update(self, h):
        h = np.asarray(h, np.float32)
        for row, m in zip(self.rows, self.out):
            if m is not None:
                m.update(h[[n for n, _ in row]][None])

    def process_block(self, x):
        x = np.asarray(x, np.float32)
        y = np.zeros((self.O, self.B), np.float32)
        for o, (row, m) in enumerate(zip(self.rows, self.out)):
            if m is not None:
                y[o] = m.process_block(x[[i for _, i in row]])[0]
        return y

    def tally(self, name):
        return sum(getattr(m, name) for m in self.out if m is not None)


# ---- the GPU tests' shapes --------------------------------------------------
# `cols` = the inputs of every output; `why` = predicates of PROPERTIES that the
# shape must satisfy (a predicate takes the shape).
SpLaShape = namedtuple("SpLaShape", "name I B S cols why")


def shape_pairs(s):
    return from_rows(s.cols)


def shape_len(s):
    return s.S * s.B


MAIN = SpLaShape(
    "main", 7, 64, 40,
    [[0, 1, 2, 3, 4, 5], [3], [], [0, 4], [1, 2, 3], [0, 1, 2, 4], [4], [0, 1, 2, 3, 4], [1, 3, 4], [2, 4]],
    ("main_counts", "shared_classes", "unread_input", "single_reader", "far_group_spans_pairs"))
NEAR_SPLIT = SpLaShape("near-split", 12, 32, 12, [list(range(12)), [5]], ("near_split",))
SHAPE_32 = SpLaShape("B32", 3, 32, 12, [[0, 1, 2], [], [1]], ("sixteen_groups", "has_far", "thin_output"))
SHAPE_256 = SpLaShape("B256", 3, 256, 20, [[0, 2], [1], []], ("two_groups", "has_far", "thin_output"))
SHAPE_512 = SpLaShape("B512", 3, 512, 12, [[2], [0, 1, 2], []], ("one_group", "has_far", "thin_output"))
SHAPES = [MAIN, NEAR_SPLIT, SHAPE_32, SHAPE_256, SHAPE_512]


def _ks(s):
    return [len(c) for c in s.cols]


def _readers(s, i):
    return [o for o, c in enumerate(s.cols) if i in c]


def _far_group_spans_pairs(s):
    """some 3-pair output has a far row group (contiguous rows) that holds rows
    of two pairs with different inputs"""
    for c in s.cols:
        if len(c) != 3:
            continue
        for p in range(far_parts(3, s.S)):
            for g in range(geo(s.B).G):
                ins = {c[e] for e, _ in la.far_rows(s.B, 3, s.S, p, g)}
                if len(ins) > 1:
                    return True
    return False


PROPERTIES = {
    # outputs 0..5: pair counts 6, 1, 0, 2, 3, 4 with far parts 3, 1, 0, 1, 2, 2
    "main_counts": lambda s: _ks(s)[:6] == [6, 1, 0, 2, 3, 4]
    and [far_parts(k, s.S) for k in _ks(s)[:6]] == [3, 1, 0, 1, 2, 2],
    # output 8 shares class 0 with output 0 and has two far parts; output 9 shares class 1 and has two pairs
    "shared_classes": lambda s: len(s.cols) == 10 and far_parts(_ks(s)[8], s.S) == 2 and _ks(s)[9] == 2,
    "unread_input": lambda s: _readers(s, s.I - 1) == [],
    "single_reader": lambda s: any(len(_readers(s, i)) == 1 for i in range(s.I)),
    "far_group_spans_pairs": _far_group_spans_pairs,
    # output 0 lists every input: 84 near rows in two parts; output 1 one pair
    "near_split": lambda s: _ks(s) == [12, 1] and 12 * (min(Q, s.S) - 1) == 84 and near_parts(12, s.S) == 2
    and far_parts(12, s.S) == 1 and far_parts(1, s.S) == 1,
    "sixteen_groups": lambda s: geo(s.B).G == 16,
    "two_groups": lambda s: geo(s.B).G == 2,
    "one_group": lambda s: geo(s.B).G == 1 and s.B == 512,
    "has_far": lambda s: s.S > Q and max(far_parts(k, s.S) for k in _ks(s)) >= 1,
    "thin_output": lambda s: 0 in _ks(s) and 1 in _ks(s),
}
