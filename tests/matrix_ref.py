"""Reference for the MatrixConvolver tests: inputs x outputs oracle
FFTConvolver instances (o, i), all created / updated / reset together; instance
(o, i) processes input i, output o is the f64 sum over i."""
import numpy as np

from common import ir, white


class SummedOracle:
    def __init__(self, oracle, h, block, max_len):
        h = np.asarray(h, np.float32)
        self.O, self.I = h.shape[:2]
        self.inst = [[oracle.FFTConvolver.init(h[o, i], block, max_len) for i in range(self.I)]
                     for o in range(self.O)]

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

    def update(self, h):
        h = np.asarray(h, np.float32)
        for o in range(self.O):
            for i in range(self.I):
                self.inst[o][i].update(h[o, i])

    def reset(self):
        for row in self.inst:
            for c in row:
                c.reset()

    def state(self):
        c = self.inst[0][0]
        return (c.current, c.active_seg_count, c.fill)


def direct(oracle, x, h) -> np.ndarray:
    """f64 direct convolution y[o] = sum_i x[i] * h[o][i], truncated to len(x)"""
    O, I = np.asarray(h).shape[:2]
    y = np.zeros((O, np.asarray(x).shape[1]), np.float64)
    for o in range(O):
        for i in range(I):
            y[o] += oracle.direct_convolution(x[i], h[o][i])
    return y


class BlockModel:
    """f64 model of the reference's uniformly partitioned convolution for all
    [O][I] pairs at once (numpy.fft over the batch), full blocks only and a
    constant active segment count: for matrices with too many pairs for
    SummedOracle.  update() keeps the delay line and clears the overlap, as
    FFTConvolver::update does."""

    def __init__(self, h, block, max_len):
        self.B = block
        self.S = -(-max_len // block)
        self.update(h)
        self.X = [np.zeros((self.I, block + 1), np.complex128) for _ in range(self.S)]

    def update(self, h):
        h = np.asarray(h, np.float64)
        self.O, self.I, n = h.shape
        assert -(-n // self.B) == self.S
        hp = np.zeros((self.O, self.I, self.S * self.B))
        hp[:, :, :n] = h
        self.H = np.fft.rfft(hp.reshape(self.O, self.I, self.S, self.B), 2 * self.B, axis=3)
        self.ovl = np.zeros((self.O, self.B))

    def process_block(self, x) -> np.ndarray:
        """x[I][B] -> f64 [O][B]"""
        self.X = [np.fft.rfft(np.asarray(x, np.float64), 2 * self.B, axis=1)] + self.X[:-1]
        spec = sum(np.einsum("oif,if->of", self.H[:, :, s], self.X[s]) for s in range(self.S))
        y = np.fft.irfft(spec, 2 * self.B, axis=1)
        out = y[:, :self.B] + self.ovl
        self.ovl = y[:, self.B:]
        return out


def make(seed, inputs, outputs, length, samples):
    """(h[O][I][length], x[I][samples]) from common.ir / common.white"""
    rng = np.random.default_rng(seed)
    h = np.stack([np.stack([ir(rng, length) for _ in range(inputs)]) for _ in range(outputs)])
    x = np.stack([white(rng, samples) for _ in range(inputs)])
    return h, x


RAGGED_64 = [1, 7, 64, 100, 3, 200, 64, 65, 128, 31, 33] * 3
RAGGED_256 = [100, 156, 256, 300, 212, 512, 1]
