"""Reference for the MatrixTwoStageConvolver tests: outputs x inputs oracle
TwoStageFFTConvolver instances (o, i), all created and reset together and fed
the same calls; instance (o, i) processes input i, output o is the f64 sum
over i."""
import numpy as np


class SummedTwoStageOracle:
    def __init__(self, oracle, h, block, max_len):
        h = np.asarray(h, np.float32)
        self.O, self.I = h.shape[:2]
        self.inst = [[oracle.TwoStageFFTConvolver.init(h[o, i], block, max_len) for i in range(self.I)]
                     for o in range(self.O)]

    @property
    def tail_block_size(self):
        return self.inst[0][0].tail_block_size

    def process(self, x) -> np.ndarray:
        """x[I][n] -> f64 [O][n]"""
        x = np.asarray(x, np.float32)
        y = np.zeros((self.O, x.shape[1]), np.float64)
        for o in range(self.O):
            for i in range(self.I):
                y[o] += self.inst[o][i].process(x[i]).astype(np.float64)
        return y

    def run(self, x, lengths) -> np.ndarray:
        """consecutive calls of the given lengths over x[I][sum(lengths)]"""
        out, pos = [], 0
        for n in lengths:
            out.append(self.process(x[:, pos:pos + n]))
            pos += n
        return np.concatenate(out, axis=1)

    def reset(self):
        for row in self.inst:
            for c in row:
                c.reset()


# name: (I, O, head, L, T, (S head, S tail0, S tail) -- None = the stage is absent, aligned calls)
SHAPES = {
    "three-stage": (3, 2, 64, 3000, 512, (8, 8, 4), 40),       # 5 periods; the tail's part arrives after 2T
    "split": (3, 2, 32, 12000, 1024, (32, 32, 10), 100),       # P = 2 in head and tail0 (93 rows), 1 in the tail
    "head-only": (2, 2, 64, 50, 64, (1, None, None), 6),       # no tail stages
    "head+tail0": (2, 2, 64, 100, 64, (1, 1, None), 6),        # zero MAC rows, a period of one call
    "period-one": (2, 2, 64, 150, 64, (1, 1, 1), 8),           # T == B: both swaps on every call
    "B1024": (2, 2, 1024, 40000, 8192, (8, 8, 3), 18),         # the 512-thread geometry, T at the limit
    "B8192": (2, 1, 8192, 20000, 8192, (1, 1, 1), 4),          # the 128 KiB finish
}

RAGGED = [64, 1, 7, 64, 56, 64, 64, 30, 34, 64] * 6


def stage_seg_counts(oracle, head, max_len):
    """(T, (S head, S tail0, S tail)) from the reference's own arithmetic: T by
    its compute_tail_block_size, each stage's seg_count by an oracle
    FFTConvolver of that stage's slice length and block (src/fft_convolver.rs
    :352-384)."""
    T = oracle.compute_tail_block_size(head, max_len)

    def segs(n, block):
        return oracle.FFTConvolver.init(np.zeros(n, np.float32), block, n).seg_count

    s_head = segs(min(max_len, T), head)
    s_tail0 = segs(min(max_len - T, T), head) if max_len > T else None
    s_tail = segs(max_len - 2 * T, T) if max_len > 2 * T else None
    return T, (s_head, s_tail0, s_tail)
