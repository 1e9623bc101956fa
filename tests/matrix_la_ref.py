"""CPU model of the MatrixLookaheadConvolver (fft-convolution_amd/csrc/
matrix_la.hip): the anchor schedule (role / steady mirror
kernels.hpp's matrix_la_role / matrix_la_steady), the near walk, the far walk
for a window of W in {1, Q} blocks, and a float32 replay that really serves
blocks from windows computed up to Q - 1 blocks earlier.  The constants are
duplicated on purpose, as in matrix_paths: tests/test_matrix_la_ref.py asserts
the properties the scheme rests on, tests/test_gpu_matrix_la.py asserts that
the library's period and part counts equal the model's."""
import numpy as np

from matrix_paths import geo

Q = 8  # kMatrixLaQ

# the GPU tests' shapes (I, O, B, L): main, largest block with an oracle sum, smallest block
MAIN = (3, 10, 64, 2560)
SHAPE_256 = (2, 3, 256, 256 * 20)
SHAPE_32 = (2, 3, 32, 32 * 12)


def parts_of(rows):
    """matrix_la_parts: about 64 rows per part, at most 64 parts"""
    return min(max((rows + 63) // 64, 1), 64)


def near_parts(I, act, q=Q):
    return parts_of(I * max(min(q, act) - 1, 0))


def far_parts(I, act, q=Q):
    return parts_of(I * (act - q)) if act > q else 0


def role(t, tv, o, q=Q):
    """what output o does with its far rows in launch A of block t: 'anchor',
    'full' or None (served by the window of its latest anchor)"""
    ph = (t - o) % q
    if t - ph < tv:
        return "full"
    return "anchor" if ph == 0 else None


def steady(t, tv, q=Q):
    return t - (q - 1) >= tv


def far_outputs(t, tv, O, q=Q):
    """the outputs launch A holds far workgroups for, in grid order"""
    return list(range(t % q, O, q)) if steady(t, tv, q) else list(range(O))


def next_cur(cur, act):
    return cur - 1 if cur > 0 else act - 1


def near_rows(B, I, act, p, g, q=Q):
    """(i, s) of near part p, row group g, in the order they are added"""
    G = geo(B).G
    nm1 = max(min(q, act) - 1, 0)
    R = I * nm1
    P = near_parts(I, act, q)
    rpp = -(-R // P)
    r1 = min((p + 1) * rpp, R)
    return [(r // nm1, 1 + r % nm1) for r in range(p * rpp + g, r1, G)]


def far_rows(B, I, act, p, g, q=Q):
    """(i, s) of far part p, row group g: a contiguous ascending sub-range"""
    G = geo(B).G
    nf = act - q
    R = I * nf
    P = far_parts(I, act, q)
    rpp = -(-R // P)
    rpg = -(-rpp // G)
    r1 = min((p + 1) * rpp, R)
    q0 = p * rpp + g * rpg
    return [(r // nf, q + r % nf) for r in range(q0, min(q0 + rpg, r1))]


def far_walk(B, I, act, cur, p, g, W, q=Q):
    """the far walk of (part p, group g) with W accumulators, replayed step by
    step as the kernel runs it: per input a ring of W FDL rows that slides by one
    per step.  Returns per accumulator j the list of (i, s, ring index) it
    multiplies, in order; accumulator j is the sum of the block j blocks ahead."""
    cm = cur % act
    xr = lambda e: (cm + e) % act
    out = [[] for _ in range(W)]
    rows = far_rows(B, I, act, p, g, q)
    k = 0
    while k < len(rows):
        i, s0 = rows[k]
        n = 1
        while k + n < len(rows) and rows[k + n][0] == i:
            n += 1
        ring = {e: xr(e) for e in range(s0 - (W - 1), s0)}  # primed with the W - 1 rows before
        for s in range(s0, s0 + n):
            assert (i, s) == rows[k + s - s0]
            ring[s] = xr(s)
            ring.pop(s - W, None)
            assert len(ring) == W
            for j in range(W):
                out[j].append((i, s, ring[s - j]))
        k += n
    return out


class LaModel:
    """float32 replay of the schedule on full blocks: spectra as numpy rfft bins
    (complex64), the sums in the model's part / group / row order, an output's
    block served from the window ring whenever role() says so."""

    def __init__(self, h, B, max_len, q=Q, windows=True):
        h = np.asarray(h, np.float32)
        self.O, self.I, n = h.shape
        self.B, self.q, self.windows = B, q, windows
        self.S = -(-max_len // B)
        self.X = np.zeros((self.I, self.S, B + 1), np.complex64)
        self.ovl = np.zeros((self.O, B), np.float32)
        self.far = {}  # (o, p, t % q) -> partial sum
        self.cur = self.t = self.tv = 0
        self.anchored = self.from_window = self.full = 0
        self._set_h(h)

    def _set_h(self, h):
        n = h.shape[2]
        self.act = -(-n // self.B)
        hp = np.zeros((self.O, self.I, self.S * self.B), np.float32)
        hp[:, :, :n] = h
        self.H = np.fft.rfft(hp.reshape(self.O, self.I, self.S, self.B), 2 * self.B, axis=3).astype(np.complex64)

    def update(self, h):
        self._set_h(np.asarray(h, np.float32))
        self.ovl[:] = 0
        self.tv = self.t

    def _far(self, o, W):
        B, I, act, q = self.B, self.I, self.act, self.q
        for p in range(far_parts(I, act, q)):
            acc = [np.zeros(B + 1, np.complex64) for _ in range(W)]
            for g in range(geo(B).G):
                grp = [np.zeros(B + 1, np.complex64) for _ in range(W)]
                for j, lst in enumerate(far_walk(B, I, act, self.cur, p, g, W, q)):
                    for i, s, xi in lst:
                        grp[j] = grp[j] + self.H[o, i, s] * self.X[i, xi]
                acc = [grp[j] if g == 0 else acc[j] + grp[j] for j in range(W)]
            for j in range(W):
                self.far[(o, p, (self.t + j) % q)] = acc[j]

    def process_block(self, x):
        B, I, act, q = self.B, self.I, self.act, self.q
        if not self.windows or self.cur >= act:
            self.tv = self.t + 1
        self.X[:, self.cur] = np.fft.rfft(np.asarray(x, np.float32), 2 * B, axis=1).astype(np.complex64)
        cm = self.cur % act
        y = np.zeros((self.O, B), np.float32)
        for o in range(self.O):
            near = None
            for p in range(near_parts(I, act, q)):
                part = None
                for g in range(geo(B).G):
                    grp = np.zeros(B + 1, np.complex64)
                    for i, s in near_rows(B, I, act, p, g, q):
                        grp = grp + self.H[o, i, s] * self.X[i, (cm + s) % act]
                    part = grp if part is None else part + grp
                near = part if near is None else near + part
            pre = near
            if act > q:
                r = role(self.t, self.tv, o, q)
                if r == "anchor":
                    self._far(o, q)
                    self.anchored += 1
                elif r == "full":
                    self._far(o, 1)
                    self.full += 1
                else:
                    self.from_window += 1
                far = None
                for p in range(far_parts(I, act, q)):
                    v = self.far[(o, p, self.t % q)]
                    far = v if far is None else far + v
                pre = near + far
            for i in range(I):
                pre = pre + self.X[i, self.cur] * self.H[o, i, 0]
            full = np.fft.irfft(pre.astype(np.complex128), 2 * B).astype(np.float32)
            y[o] = full[:B] + self.ovl[o]
            self.ovl[o] = full[B:]
        self.cur = next_cur(self.cur, act)
        self.t += 1
        return y
