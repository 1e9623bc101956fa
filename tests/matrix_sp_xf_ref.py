"""Reference for the SparseMatrixCrossfadeConvolver tests: one oracle
CrossfadeConvolver<FFTConvolver> instance per listed (output, input) pair, all
created and updated together; instance n processes input i_n with the same
calls, output o is the f64 sum of the instances listed for it (zero when none
is).  The crossfaders run in lockstep, so is_crossfading and response_pending
are those of instance 0.  Scripts are matrix_xf_ref.run_script's, patterns
matrix_sp_ref's."""
import numpy as np

from matrix_sp_ref import check_pairs, rows_of


class SparseSummedCrossfadeOracle:
    def __init__(self, oracle, pairs, h, inputs, outputs, block, max_len, *, max_response_length=None,
                 max_buffer_size=None, crossfade_samples=None):
        """With the three keyword arguments: CrossfadeConvolver::new over
        FFTConvolver::init(h[n], block, max_len); without them: the init form,
        CrossfadeConvolver::init(h[n], block, max_len)."""
        self.pairs = check_pairs(pairs, inputs, outputs)
        self.I, self.O = inputs, outputs
        h = np.asarray(h, np.float32)
        assert h.shape[0] == len(self.pairs)
        if crossfade_samples is None:
            make = lambda r: oracle.CrossfadeConvolver.init(r, block, max_len)
        else:
            make = lambda r: oracle.CrossfadeConvolver.new(oracle.FFTConvolver.init(r, block, max_len),
                                                           max_response_length, max_buffer_size, crossfade_samples)
        self.inst = [make(h[n]) for n in range(len(self.pairs))]
        self.rows = rows_of(self.pairs, outputs)

    def process(self, x, out_len=None) -> np.ndarray:
        """x[I][n] -> f64 [O][out_len or n]"""
        x = np.asarray(x, np.float32)
        assert x.shape[0] == self.I
        y = np.zeros((self.O, x.shape[1] if out_len is None else out_len), np.float64)
        for o, row in enumerate(self.rows):
            for n, i in row:
                y[o] += self.inst[n].process(x[i], out_len).astype(np.float64)
        return y

    def update(self, h):
        """h[N][len]: row n is the response of pair n"""
        h = np.asarray(h, np.float32)
        assert h.shape[0] == len(self.pairs)
        for n, c in enumerate(self.inst):
            c.update(h[n])

    def is_crossfading(self) -> bool:
        return self.inst[0].is_crossfading()

    @property
    def response_pending(self) -> bool:
        return self.inst[0].response_pending
