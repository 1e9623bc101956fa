"""Reference for the MatrixCrossfadeConvolver tests: outputs x inputs oracle
CrossfadeConvolver<FFTConvolver> instances (o, i), all created and updated
together; instance (o, i) processes input i with the same calls, output o is
the f64 sum over i.  The crossfaders run in lockstep, so is_crossfading and
response_pending are those of instance (0, 0)."""
import numpy as np


class SummedCrossfadeOracle:
    def __init__(self, oracle, h, block, max_len, *, max_response_length=None, max_buffer_size=None,
                 crossfade_samples=None):
        """With the three keyword arguments: CrossfadeConvolver::new over
        FFTConvolver::init(h[o, i], block, max_len); without them: the init
        form, CrossfadeConvolver::init(h[o, i], block, max_len)."""
        h = np.asarray(h, np.float32)
        self.O, self.I = h.shape[:2]
        if crossfade_samples is None:
            make = lambda r: oracle.CrossfadeConvolver.init(r, block, max_len)
        else:
            make = lambda r: oracle.CrossfadeConvolver.new(oracle.FFTConvolver.init(r, block, max_len),
                                                           max_response_length, max_buffer_size, crossfade_samples)
        self.inst = [[make(h[o, i]) for i in range(self.I)] for o in range(self.O)]

    def process_each(self, x, out_len=None) -> np.ndarray:
        """x[I][n] -> f32 [O][I][out_len or n], the instances' own outputs"""
        x = np.asarray(x, np.float32)
        return np.stack([np.stack([self.inst[o][i].process(x[i], out_len) for i in range(self.I)])
                         for o in range(self.O)])

    def process(self, x, out_len=None) -> np.ndarray:
        """x[I][n] -> f64 [O][out_len or n]"""
        return self.process_each(x, out_len).astype(np.float64).sum(axis=1)

    def update(self, h):
        h = np.asarray(h, np.float32)
        for o in range(self.O):
            for i in range(self.I):
                self.inst[o][i].update(h[o, i])

    def is_crossfading(self) -> bool:
        return self.inst[0][0].is_crossfading()

    @property
    def response_pending(self) -> bool:
        return self.inst[0][0].response_pending


def run_script(ref, x, script, max_buffer_size, panic=None, before_call=None):
    """Drive `ref` (a SummedCrossfadeOracle or a MatrixCrossfadeConvolver)
    through a script of ("update", h), ("update_panics", h) and ("call",
    out_len) steps; each call consumes max_buffer_size samples of x.  An
    "update_panics" step must raise `panic`.  before_call(k), if given, runs
    before call k.  Returns (outputs of every call, is_crossfading after every
    call)."""
    ys, flags, pos = [], [], 0
    for kind, arg in script:
        if kind == "update":
            ref.update(arg)
        elif kind == "update_panics":
            try:
                ref.update(arg)
            except panic:
                continue
            raise AssertionError("update() of a response longer than the stored one did not panic")
        else:
            if before_call is not None:
                before_call(len(ys))
            ys.append(np.asarray(ref.process(x[:, pos:pos + max_buffer_size], arg)))
            flags.append(bool(ref.is_crossfading()))
            pos += max_buffer_size
    return ys, flags


def calls(n, out_len):
    return [("call", out_len)] * n
