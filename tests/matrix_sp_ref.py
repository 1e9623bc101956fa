"""Reference for the SparseMatrixConvolver tests: one oracle FFTConvolver
instance per listed (output, input) pair, all created / updated / reset
together; instance n processes input i_n, output o is the f64 sum of the
instances listed for it (zero when none is).  Also the patterns and the bitwise
shapes of tests/test_gpu_matrix_sparse.py, with the property each output's pair
count is there for (checked on the CPU by tests/test_matrix_sp_ref.py through
matrix_paths.walk / parts, which are used unchanged with inputs := k_o)."""
from collections import namedtuple

import numpy as np

from common import ir, white


def check_pairs(pairs, inputs, outputs):
    """the ABI's precondition: in range, strictly ascending in (o, i)"""
    pairs = [tuple(int(v) for v in p) for p in pairs]
    assert pairs, "at least one pair"
    assert all(0 <= o < outputs and 0 <= i < inputs for o, i in pairs), pairs
    assert all(a < b for a, b in zip(pairs, pairs[1:])), pairs
    return pairs


def rows_of(pairs, outputs):
    """per output: [(pair index n, input i_n), ...] in list order"""
    rows = [[] for _ in range(outputs)]
    for n, (o, i) in enumerate(pairs):
        rows[o].append((n, i))
    return rows


def from_rows(cols):
    """pair list of a pattern given as one list of inputs per output"""
    return [(o, i) for o, cs in enumerate(cols) for i in cs]


class SparseSummedOracle:
    def __init__(self, oracle, pairs, h, inputs, outputs, block, max_len):
        self.pairs = check_pairs(pairs, inputs, outputs)
        self.I, self.O = inputs, outputs
        h = np.asarray(h, np.float32)
        assert h.shape[0] == len(self.pairs)
        self.inst = [oracle.FFTConvolver.init(h[n], block, max_len) for n in range(len(self.pairs))]
        self.rows = rows_of(self.pairs, outputs)

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

    def update(self, h):
        h = np.asarray(h, np.float32)
        assert h.shape[0] == len(self.pairs)
        for n, c in enumerate(self.inst):
            c.update(h[n])

    def reset(self):
        for c in self.inst:
            c.reset()

    def state(self):
        c = self.inst[0]
        return (c.current, c.active_seg_count, c.fill)


def direct(oracle, x, pairs, h, outputs) -> np.ndarray:
    """f64 direct convolution restricted to the listed pairs, truncated to len(x)"""
    y = np.zeros((outputs, np.asarray(x).shape[1]), np.float64)
    for n, (o, i) in enumerate(pairs):
        y[o] += oracle.direct_convolution(x[i], h[n])
    return y


def make(seed, pairs, inputs, length, samples):
    """(h[N][length], x[I][samples]) from common.ir / common.white"""
    rng = np.random.default_rng(seed)
    h = np.stack([ir(rng, length) for _ in pairs])
    x = np.stack([white(rng, samples) for _ in range(inputs)])
    return h, x


# test 1's pattern (I 5, O 4): a full output, a single pair, an output without
# pairs, two pairs; input 1 and 3 are read by output 0 only
PATTERN_1 = from_rows([[0, 1, 2, 3, 4], [2], [], [0, 4]])
# the 2-output pattern of the ragged B 256 case (I 3): input 1 is unused
PATTERN_256 = from_rows([[0, 2], [2]])

# The bitwise shapes (property 1): `cols` = the inputs of every output, `why` =
# per output the predicates of PROPERTIES that its (B, k_o, S) must satisfy.
# L = S * B - 3, S + 3 full blocks, as matrix_paths' shapes.
SpShape = namedtuple("SpShape", "name B I S cols why")
BITWISE = [
    # the skewed compact grid: 64 + 3 + 24 MAC workgroups, not 3 * 64
    SpShape("skewed", 64, 30, 138, [list(range(30)), [7], [0, 3, 6, 9, 12, 15, 18, 21, 24, 27, 29]],
            [("capped", "unrolled", "tail", "both"), ("three_parts", "tail_only"), ("many_parts", "unrolled", "tail")]),
    SpShape("groups", 128, 11, 7, [list(range(11)), [4, 9]],
            [("two_parts", "unrolled", "tail", "both"), ("one_part", "tail_only")]),
    SpShape("spt2", 1024, 5, 14, [list(range(5)), [1, 4]],
            [("spt2", "two_parts", "unrolled", "tail", "both"), ("spt2", "one_part", "unrolled", "tail", "both")]),
    SpShape("no-rows", 64, 1, 1, [[0]], [("no_rows",)]),
    SpShape("single-row", 64, 1, 2, [[0]], [("single_row",)]),
]

# predicates over (geo(B), walk(B, k_o, act), k_o)
PROPERTIES = {
    "capped": lambda g, w, k: w.R > 4096 and w.P == 64 and w.rpp > 64,
    "unrolled": lambda g, w, k: w.unrolled > 0,
    "tail": lambda g, w, k: w.tail > 0,
    "tail_only": lambda g, w, k: w.tail == w.R > 0 and w.unrolled == 0,
    "both": lambda g, w, k: w.groups_both > 0,
    "one_part": lambda g, w, k: w.P == 1 and w.R > 0,
    "two_parts": lambda g, w, k: w.P == 2,
    "three_parts": lambda g, w, k: w.P == 3,
    "many_parts": lambda g, w, k: 3 < w.P < 64,
    "spt2": lambda g, w, k: (g.G, g.SPT, g.U, g.UB) == (1, 2, 4, 8),
    "no_rows": lambda g, w, k: w.R == 0 and w.P == 1 and w.unrolled == 0 and w.tail == 0,
    "single_row": lambda g, w, k: w.R == 1 and w.P == 1 and w.tail == 1,
}


def sp_len(s):
    """response length: the last segment is ragged"""
    return s.S * s.B - 3


def sp_blocks(s):
    """full blocks per run: the delay line wraps, every row contributes"""
    return s.S + 3
