"""Reference for the SparseMatrixTwoStageConvolver tests: one oracle
TwoStageFFTConvolver instance per listed (output, input) pair, all created and
reset together and fed the same calls; instance n processes input i_n, output
o is the f64 sum of the instances listed for it (zero when none is).  The
cross of matrix_sp_ref.SparseSummedOracle and matrix_ts_ref.SummedTwoStageOracle.
Also the shape table of tests/test_gpu_matrix_sparse_ts.py, with the per-output
part counts and walk properties each shape is there for (checked on the CPU by
tests/test_matrix_sp_ts_ref.py through matrix_paths.walk / parts, which are used
unchanged with inputs := k_o)."""
from collections import namedtuple

import numpy as np

from matrix_sp_ref import PATTERN_1, check_pairs, from_rows, rows_of


class SparseSummedTwoStageOracle:
    def __init__(self, oracle, pairs, h, inputs, outputs, block, max_len):
        self.pairs = check_pairs(pairs, inputs, outputs)
        self.I, self.O = inputs, outputs
        h = np.asarray(h, np.float32)
        assert h.shape[0] == len(self.pairs)
        self.inst = [oracle.TwoStageFFTConvolver.init(h[n], block, max_len) for n in range(len(self.pairs))]
        self.rows = rows_of(self.pairs, outputs)

    @property
    def tail_block_size(self):
        return self.inst[0].tail_block_size

    def process(self, x) -> np.ndarray:
        """x[I][n] -> f64 [O][n]"""
        x = np.asarray(x, np.float32)
        assert x.shape[0] == self.I
        y = np.zeros((self.O, x.shape[1]), np.float64)
        for o, row in enumerate(self.rows):
            for n, i in row:
                y[o] += self.inst[n].process(x[i]).astype(np.float64)
        return y

    def run(self, x, lengths) -> np.ndarray:
        """consecutive calls of the given lengths over x[I][sum(lengths)]"""
        out, pos = [], 0
        for n in lengths:
            out.append(self.process(x[:, pos:pos + n]))
            pos += n
        return np.concatenate(out, axis=1)

    def reset(self):
        for c in self.inst:
            c.reset()


# `cols` = the inputs of every output; (head, L) is a pair matrix_ts_ref.SHAPES
# pins, so T and segs (S head, S tail0, S tail; None = the stage is absent) are
# the reference's; calls = aligned calls; parts = per stage (head, tail0, tail)
# the outputs' P_o = parts(k_o, S_stage), None for an absent stage; why = per
# output the predicates of PROPERTIES its head-stage walk (head, k_o, S head)
# must satisfy.
SpTsShape = namedtuple("SpTsShape", "I O cols head L T segs calls parts why")
_TWO = [[0, 1], [1]]
SHAPES = {
    # PATTERN_1: all stages, 5 periods, an empty output (2); inputs 1 and 3 are read by output 0 only
    # (inputs that no pair reads: the one-output handles of test_output_sharding_bitwise)
    "three-stage": SpTsShape(5, 4, [[0, 1, 2, 3, 4], [2], [], [0, 4]], 64, 3000, 512, (8, 8, 4), 40,
                             ((1, 1, 1, 1), (1, 1, 1, 1), (1, 1, 1, 1)),
                             [("one_part", "tail_only"), ("one_part", "tail_only"), ("no_rows",),
                              ("one_part", "tail_only")]),
    # head / tail0 P_o = 2 / 1 / 1 (124 and 31 rows): the compact grid is not O * P
    "split": SpTsShape(4, 3, [[0, 1, 2, 3], [2], []], 32, 12000, 1024, (32, 32, 10), 100,
                       ((2, 1, 1), (2, 1, 1), (1, 1, 1)),
                       [("two_parts", "rows124"), ("one_part", "rows31"), ("no_rows",)]),
    # P_o = 4 / 1 / 2; the tail stage (block 512) has P = 2 and runs the unrolled and the tail pass of the pair walk
    "wide": SpTsShape(30, 3, [list(range(30)), [7], [0, 3, 6, 9, 12, 15, 18, 21, 24, 27, 29]], 64, 3000, 512,
                      (8, 8, 4), 40, ((4, 1, 2), (4, 1, 2), (2, 1, 1)),
                      [("four_parts", "tail_only"), ("one_part", "tail_only"), ("two_parts", "tail_only")]),
    # (beyond the issue's table) 63 rows in one part at G = 8: the fused walk's U-rows-in-flight loop below B 512,
    # which no shape above reaches in the head (B1024 does at G = 1)
    "unrolled64": SpTsShape(9, 2, [list(range(9)), [4]], 64, 3000, 512, (8, 8, 4), 24, ((1, 1), (1, 1), (1, 1)),
                            [("one_part", "unrolled", "tail", "cross_unrolled"), ("one_part", "tail_only")]),
    "head-only": SpTsShape(2, 2, _TWO, 64, 50, 64, (1, None, None), 6, ((1, 1), None, None),
                           [("no_rows",), ("no_rows",)]),                      # no tail stages, always composition
    "head+tail0": SpTsShape(2, 2, _TWO, 64, 100, 64, (1, 1, None), 6, ((1, 1), (1, 1), None),
                            [("no_rows",), ("no_rows",)]),                     # zero MAC rows, a period of one call
    "period-one": SpTsShape(2, 2, _TWO, 64, 150, 64, (1, 1, 1), 8, ((1, 1), (1, 1), (1, 1)),
                            [("no_rows",), ("no_rows",)]),                     # both swaps every call
    # the 512-thread geometry in the tail (block 8192), T at the limit
    "B1024": SpTsShape(3, 2, [[0, 1, 2], [1]], 1024, 40000, 8192, (8, 8, 3), 18, ((1, 1), (1, 1), (1, 1)),
                       [("spt2", "one_part", "unrolled", "tail", "both"),
                        ("spt2", "one_part", "unrolled", "tail", "both")]),
    "B8192": SpTsShape(2, 2, _TWO, 8192, 20000, 8192, (1, 1, 1), 4, ((1, 1), (1, 1), (1, 1)),
                       [("spt8", "no_rows"), ("spt8", "no_rows")]),            # the 128 KiB finish
}
assert SHAPES["three-stage"].cols == [[i for o, i in PATTERN_1 if o == k] for k in range(4)]

# predicates over (geo(head), walk(head, k_o, S head), k_o)
PROPERTIES = {
    "unrolled": lambda g, w, k: w.unrolled > 0,
    "tail": lambda g, w, k: w.tail > 0,
    "cross_unrolled": lambda g, w, k: w.cross_in_unrolled,
    "tail_only": lambda g, w, k: w.tail == w.R > 0 and w.unrolled == 0,
    "both": lambda g, w, k: w.groups_both > 0,
    "one_part": lambda g, w, k: w.P == 1 and w.R > 0,
    "two_parts": lambda g, w, k: w.P == 2,
    "four_parts": lambda g, w, k: w.P == 4,
    "rows124": lambda g, w, k: w.R == 124,
    "rows31": lambda g, w, k: w.R == 31,
    "spt2": lambda g, w, k: (g.G, g.SPT, g.U, g.UB) == (1, 2, 4, 8),
    "spt8": lambda g, w, k: (g.G, g.SPT, g.U, g.UB) == (1, 8, 1, 4),
    "no_rows": lambda g, w, k: w.R == 0 and w.P == 1 and w.unrolled == 0 and w.tail == 0,
}


def pairs_of(s):
    return from_rows(s.cols)
