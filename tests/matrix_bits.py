"""The cases of tests/test_gpu_matrix_bits.py and scripts/gen_matrix_bits.py:
every matrix family (dense, sparse, lookahead, crossfade, two-stage) at the
smallest shapes of the CPU-proved tables (matrix_paths.SHAPES, matrix_sp_ref,
matrix_la_ref, matrix_sp_la_ref, matrix_ts_ref, matrix_sp_ts_ref) that reach
every loop of the kernels.  A case draws its inputs from a seeded
numpy.random.default_rng, runs them through one handle and returns every input
array and the output; the fixture tests/golden/matrix_bits.json holds the
SHA-256 of both, so a change of the summation order that is consistent across
the families (which the cross-family bitwise tests cannot see) shows as another
output hash, and another random stream as another input hash."""
import hashlib

import numpy as np

from matrix_la_ref import MAIN as LA_MAIN, Q, SHAPE_32 as LA_32, SHAPE_256 as LA_256
from matrix_paths import CAPPED, RAGGED_64, SHAPES, capped_lengths, shape_blocks, shape_id, shape_len
from matrix_sp_la_ref import (MAIN as SPLA_MAIN, SHAPE_32 as SPLA_32, SHAPE_256 as SPLA_256, SHAPE_512 as SPLA_512,
                              shape_len as spla_len, shape_pairs as spla_pairs)
from matrix_sp_ref import BITWISE, PATTERN_1, PATTERN_256, from_rows
from matrix_sp_ts_ref import SHAPES as SPTS_SHAPES, pairs_of
from matrix_ts_ref import SHAPES as TS_SHAPES

LA_512 = (2, 3, 512, 512 * 12)  # (test_gpu_matrix_la.test_block_sizes)
# the skewed pattern (64 + 3 + 24 parts at S 138) with an output without pairs;
# at B 512 and 1024 it runs at S 7 (3 + 1 + 2 + 1 parts: a 30-pair list through the
# listed walk and four / eight chunks of row-0 terms) beside PATTERN_1 at S 14
SKEWED = from_rows(next(s for s in BITWISE if s.name == "skewed").cols + [[]])


class Draw:
    """seeded inputs; every array drawn is kept for the input hash"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.arrays = []

    def h(self, shape):
        a = (self.rng.uniform(-1, 1, shape) / np.sqrt(max(shape[-1], 1))).astype(np.float32)
        self.arrays.append(a)
        return a

    def x(self, inputs, n):
        a = self.rng.uniform(-1, 1, (inputs, n)).astype(np.float32)
        self.arrays.append(a)
        return a


def ragged(B):
    """calls that start and end anywhere in a block of B"""
    return [1, 7, B, B + 36, 3, 3 * B + 8, B, B + 1, 2 * B, B // 2 - 1, B // 2 + 1] * 2


def run(conv, x, lengths):
    out, pos = [], 0
    for n in lengths:
        out.append(conv.process(x[:, pos:pos + n]))
        pos += n
    assert pos == x.shape[1]
    return np.concatenate(out, axis=1)


# ---- dense and sparse -------------------------------------------------------
def dense_paths(s, variant=-1):
    def case(amd, d):
        L, n = shape_len(s), shape_blocks(s) * s.B
        h, x = d.h((s.O, s.I, L)), d.x(s.I, n)
        amd.set_kernel_variant(variant)
        try:
            return amd.MatrixConvolver.init(h, s.B, L).process(x)
        finally:
            amd.set_kernel_variant(-1)
    return case


def dense_ragged(amd, d):
    s = next(c for c in CAPPED if c.B == 64)
    lengths = capped_lengths(s)
    assert lengths[1:] == tuple(RAGGED_64)
    h, x = d.h((s.O, s.I, shape_len(s))), d.x(s.I, sum(lengths))
    return run(amd.MatrixConvolver.init(h, s.B, shape_len(s)), x, lengths)


def _with_update(conv, d, hshape, B, I, first, short, then):
    """`first` calls, an update to a response of `short` samples, `then` calls"""
    x = d.x(I, sum(first) + sum(then))
    h2 = d.h(hshape[:-1] + (short,))
    y0 = run(conv, x[:, :sum(first)], first)
    conv.update(h2)
    cur, act, _ = conv.state()
    assert cur >= act == -(-short // B), (cur, act)   # active < S, current >= active
    return np.concatenate([y0, run(conv, x[:, sum(first):], then)], axis=1)


def dense_update(amd, d):
    I, O, B, L = 3, 2, 64, 1000
    conv = amd.MatrixConvolver.init(d.h((O, I, L)), B, L)
    return _with_update(conv, d, (O, I, L), B, I, [B] * 5, 130, [B, 10, 54, B, 2 * B, B])


def sparse_case(pairs, I, O, B, S, lengths=None):
    def case(amd, d):
        L = S * B - 3
        ls = [B * (S + 3)] if lengths is None else lengths
        h, x = d.h((len(pairs), L)), d.x(I, sum(ls))
        return run(amd.SparseMatrixConvolver.init(pairs, h, I, O, B, L), x, ls)
    return case


def sparse_update(amd, d):
    I, O, B, L = 5, 4, 64, 1000
    conv = amd.SparseMatrixConvolver.init(PATTERN_1, d.h((len(PATTERN_1), L)), I, O, B, L)
    return _with_update(conv, d, (len(PATTERN_1), L), B, I, [B] * 5, 130, [B, 10, 54, B, 2 * B, B])


# ---- lookahead: >= 3 * Q blocks, so anchors and window-served blocks occur --
def _la_lengths(B, S, how):
    blocks = max(3 * Q, S + 3)
    return ragged(B) + [B] * Q if how == "ragged" else [B] * blocks + [B - 24, 24]


def _la_run(conv, d, hshape, I, B, S, how, windows):
    conv.set_windows(windows)
    if how == "update":  # a shorter response at a block boundary, mid-window for every output: the W = 1 far role
        first, then = [B] * 12, [B] * (2 * Q) + [20, B - 20]
        x, h2 = d.x(I, sum(first) + sum(then)), d.h(hshape[:-1] + (hshape[-1] - 100,))
        y0 = run(conv, x[:, :sum(first)], first)
        conv.update(h2)
        return np.concatenate([y0, run(conv, x[:, sum(first):], then)], axis=1)
    lengths = _la_lengths(B, S, how)
    return run(conv, d.x(I, sum(lengths)), lengths)


def la_case(shape, how, windows=True):
    def case(amd, d):
        I, O, B, L = shape
        conv = amd.MatrixLookaheadConvolver.init(d.h((O, I, L)), B, L)
        return _la_run(conv, d, (O, I, L), I, B, L // B, how, windows)
    return case


def spla_case(s, how, windows=True):
    def case(amd, d):
        pairs, L = spla_pairs(s), spla_len(s)
        conv = amd.SparseMatrixLookaheadConvolver.init(pairs, d.h((len(pairs), L)), s.I, len(s.cols), s.B, L)
        return _la_run(conv, d, (len(pairs), L), s.I, s.B, s.S, how, windows)
    return case


# ---- crossfade: live 1 (idle), 3 (a fade), 2 (reached), and back ------------
def _xf_run(conv, d, hshape, I, mbs, outs, fused, pairs=None):
    """calls of out_len outs[k % len(outs)]: 6, an update, 8 (hold, fade,
    reached), an update back, 6; then, with `pairs`, an update_pairs and 6"""
    if not fused:
        conv.set_fused(False)
    x = d.x(I, (26 if pairs else 20) * mbs)
    ys, k = [], 0

    def calls(n):
        nonlocal k
        for _ in range(n):
            ys.append(conv.process(x[:, k * mbs:(k + 1) * mbs], outs[k % len(outs)]))
            k += 1

    calls(6)
    assert not conv.is_crossfading()
    conv.update(d.h(hshape))
    calls(1)
    assert conv.is_crossfading()
    calls(7)
    assert not conv.is_crossfading()
    conv.update(d.h(hshape))
    calls(6)
    if pairs:
        assert not conv.is_crossfading()
        conv.update_pairs(pairs, d.h((len(pairs), hshape[-1])))
        calls(6)
    return np.concatenate(ys, axis=1)


def xf_case(I, O, B, L, mbs, fade, outs, fused=True, pairs=None):
    def case(amd, d):
        conv = amd.MatrixCrossfadeConvolver.new(amd.MatrixConvolver.init(d.h((O, I, L)), B, L), L, mbs, fade)
        return _xf_run(conv, d, (O, I, L), I, mbs, outs, fused, pairs)
    return case


def spxf_case(pattern, I, O, B, L, mbs, fade, outs, fused=True):
    def case(amd, d):
        base = amd.SparseMatrixConvolver.init(pattern, d.h((len(pattern), L)), I, O, B, L)
        conv = amd.SparseMatrixCrossfadeConvolver.new(base, L, mbs, fade)
        return _xf_run(conv, d, (len(pattern), L), I, mbs, outs, fused)
    return case


# ---- two-stage: at least two tail periods -----------------------------------
def ts_case(name, fused=True):
    def case(amd, d):
        I, O, head, L, T, _, calls = TS_SHAPES[name]
        assert calls * head >= 2 * T
        conv = amd.MatrixTwoStageConvolver.init(d.h((O, I, L)), head, L)
        if not fused:
            conv.set_fused(False)
        return run(conv, d.x(I, calls * head), [head] * calls)
    return case


def spts_case(name, fused=True):
    def case(amd, d):
        s = SPTS_SHAPES[name]
        assert s.calls * s.head >= 2 * s.T
        pairs = pairs_of(s)
        conv = amd.SparseMatrixTwoStageConvolver.init(pairs, d.h((len(pairs), s.L)), s.I, s.O, s.head, s.L)
        if not fused:
            conv.set_fused(False)
        return run(conv, d.x(s.I, s.calls * s.head), [s.head] * s.calls)
    return case


def _cases():
    c = {}
    by_id = {shape_id(s): s for s in SHAPES}
    for sid in ("B32-I60-O2-S138", "B128-I11-O2-S7", "B512-I11-O2-S7", "B1024-I5-O2-S14", "B2048-I5-O2-S14",
                "B4096-I3-O1-S23", "B64-I20-O2-S2", "B64-I1-O1-S1"):
        c[f"dense-{sid}"] = dense_paths(by_id[sid])
    c["dense-ragged-B64-capped"] = dense_ragged
    c["dense-update"] = dense_update
    c["dense-plain-loads-B128"] = dense_paths(by_id["B128-I11-O2-S7"], 0)
    c["dense-nontemporal-B128"] = dense_paths(by_id["B128-I11-O2-S7"], 2)

    c["sparse-B64-skewed"] = sparse_case(SKEWED, 30, 4, 64, 138)
    c["sparse-B64-skewed-ragged"] = sparse_case(SKEWED, 30, 4, 64, 138, [138 * 64] + ragged(64))
    for B in (512, 1024):
        c[f"sparse-B{B}"] = sparse_case(PATTERN_1, 5, 4, B, 14)
        c[f"sparse-B{B}-ragged"] = sparse_case(PATTERN_1, 5, 4, B, 14, ragged(B))
        # the skewed pattern at a short response: 30 / 1 / 11 / 0 pairs, 3 + 1 + 2 + 1 parts at S 7
        c[f"sparse-B{B}-skewed"] = sparse_case(SKEWED, 30, 4, B, 7)
        c[f"sparse-B{B}-skewed-ragged"] = sparse_case(SKEWED, 30, 4, B, 7, ragged(B))
    c["sparse-update"] = sparse_update

    for name, shape in (("B64", LA_MAIN), ("B32", LA_32), ("B256", LA_256), ("B512", LA_512)):
        c[f"la-{name}"] = la_case(shape, "full")
        c[f"la-{name}-windows-off"] = la_case(shape, "full", False)
    c["la-B64-ragged"] = la_case(LA_MAIN, "ragged")
    c["la-B64-update"] = la_case(LA_MAIN, "update")
    for name, s in (("B64", SPLA_MAIN), ("B32", SPLA_32), ("B256", SPLA_256), ("B512", SPLA_512)):
        c[f"spla-{name}"] = spla_case(s, "full")
        c[f"spla-{name}-windows-off"] = spla_case(s, "full", False)
    c["spla-B64-ragged"] = spla_case(SPLA_MAIN, "ragged")
    c["spla-B64-update"] = spla_case(SPLA_MAIN, "update")

    c["xf-B64"] = xf_case(3, 2, 64, 1000, 64, 96, [64])
    c["xf-B64-composition"] = xf_case(3, 2, 64, 1000, 64, 96, [64], fused=False)
    c["xf-B64-ragged"] = xf_case(3, 2, 64, 1000, 100, 150, [100, 37])
    c["xf-B64-update-pairs"] = xf_case(3, 2, 64, 1000, 64, 96, [64], pairs=[(0, 1), (1, 2)])
    c["xf-B1024"] = xf_case(2, 2, 1024, 3 * 1024 + 5, 1024, 1024 + 7, [1024])
    c["spxf-B128"] = spxf_case(PATTERN_1, 5, 4, 128, 2045, 128, 192, [128])
    c["spxf-B128-composition"] = spxf_case(PATTERN_1, 5, 4, 128, 2045, 128, 192, [128], fused=False)
    c["spxf-B128-ragged"] = spxf_case(PATTERN_1, 5, 4, 128, 2045, 200, 300, [200, 75])
    c["spxf-B1024"] = spxf_case(PATTERN_256, 3, 2, 1024, 3 * 1024 + 5, 1024, 1024 + 7, [1024])

    for name in ("three-stage", "split", "B1024"):
        c[f"ts-{name}"] = ts_case(name)
    c["ts-three-stage-composition"] = ts_case("three-stage", fused=False)
    for name in ("three-stage", "wide", "B1024"):
        c[f"spts-{name}"] = spts_case(name)
    c["spts-three-stage-composition"] = spts_case("three-stage", fused=False)
    return c


CASES = _cases()


def sha(arrays):
    m = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a, dtype=np.float32)
        m.update(np.array(a.shape, np.int64).tobytes())
        m.update(a.tobytes())
    return m.hexdigest()


def run_case(amd, name):
    """{"in": SHA-256 of the inputs, "out": SHA-256 of the output, "max_abs": max|y|}"""
    d = Draw(int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little"))
    y = CASES[name](amd, d)
    assert y.dtype == np.float32 and np.isfinite(y).all() and np.abs(y).max() > 0, name
    return {"in": sha(d.arrays), "out": sha([y]), "max_abs": float(np.abs(y).max())}
