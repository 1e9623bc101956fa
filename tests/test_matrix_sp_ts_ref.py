"""The yardstick of tests/test_gpu_matrix_sparse_ts.py, checked on the CPU: the
sparse summed two-stage oracle (matrix_sp_ts_ref.SparseSummedTwoStageOracle)
and the shape table the GPU tests rely on.  It validates the reference, not the
SparseMatrixTwoStageConvolver:
  - the oracle agrees with f64 direct convolution restricted to the pairs over
    a run longer than 2T + L, so all three stages have contributed, and an
    output without pairs is exactly zero;
  - T and the three stages' seg counts of every shape are the listed values, in
    the reference's own arithmetic (matrix_ts_ref.stage_seg_counts);
  - the per-output part counts of every stage and the walk properties claimed in
    the table hold (matrix_paths.walk / parts with inputs := k_o).
And the host side of the handle that needs no device: the Python mirror's own
pair-list check, the loud failure without a device, the exported symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

import matrix_paths
import matrix_ts_ref
from common import REL_TOL, max_rel_err
from matrix_sp_ref import direct, make
from matrix_sp_ts_ref import PROPERTIES, SHAPES, SparseSummedTwoStageOracle, pairs_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(SHAPES)[:2])
def test_oracle_agrees_with_direct(oracle_mod, name):
    s = SHAPES[name]
    pairs = pairs_of(s)
    calls = [s.head] * (-(-(2 * s.T + s.L) // s.head) + 2)
    n = sum(calls)
    assert n > 2 * s.T + s.L
    h, x = make(71, pairs, s.I, s.L, n)
    ref = SparseSummedTwoStageOracle(oracle_mod, pairs, h, s.I, s.O, s.head, s.L)
    assert ref.tail_block_size == s.T
    y = ref.run(x, calls)
    d = direct(oracle_mod, x, pairs, h, s.O)
    for o, cs in enumerate(s.cols):
        if not cs:
            assert not y[o].any() and not d[o].any()
            continue
        err = max_rel_err(y[o], d[o])
        print(f"{name} output {o}: sparse summed two-stage oracle vs f64 direct {err:.3e}")
        assert err <= REL_TOL
    ref.reset()
    assert np.array_equal(ref.run(x, calls), y)


@pytest.mark.parametrize("name", list(SHAPES))
def test_shape_table(oracle_mod, name):
    s = SHAPES[name]
    assert (s.head, s.L) in {(v[2], v[3]) for v in matrix_ts_ref.SHAPES.values()}  # a pair the dense table pins
    assert matrix_ts_ref.stage_seg_counts(oracle_mod, s.head, s.L) == (s.T, s.segs)
    assert s.T % s.head == 0 and s.T <= 8192
    assert len(s.cols) == s.O and all(0 <= i < s.I for cs in s.cols for i in cs)
    assert all(a < b for a, b in zip(pairs_of(s), pairs_of(s)[1:]))
    if s.segs[2] is not None:  # the run passes 2T: the tail's contribution is in it
        assert s.calls * s.head > 2 * s.T


@pytest.mark.parametrize("name", list(SHAPES))
def test_parts_and_walks(name):
    s = SHAPES[name]
    blocks = (s.head, s.head, s.T)
    for stage in range(3):
        if s.segs[stage] is None:
            assert s.parts[stage] is None
            continue
        got = tuple(matrix_paths.parts(len(cs), s.segs[stage]) for cs in s.cols)
        assert got == s.parts[stage], (name, stage, got)
        for cs in s.cols:  # every stage's walk visits each row of the output's pairs exactly once
            assert matrix_paths.walk(blocks[stage], len(cs), s.segs[stage]).exact
    g = matrix_paths.geo(s.head)
    for o, cs in enumerate(s.cols):
        w = matrix_paths.walk(s.head, len(cs), s.segs[0])
        for p in s.why[o]:
            assert PROPERTIES[p](g, w, len(cs)), f"{name} output {o} no longer has property {p}: {g} {w}"
    if name == "split":  # the compact grid: 4 MAC workgroups in head and tail0, not O * max P = 6
        assert sum(s.parts[0]) == 4 < s.O * max(s.parts[0])
    if name == "wide":   # the tail stage's full output: two parts, the unrolled and the tail pass
        w = matrix_paths.walk(s.T, 30, s.segs[2])
        assert w.P == 2 and w.unrolled > 0 and w.tail > 0
        assert sum(s.parts[0]) == 7


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fftconv.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fftconv_matrix_sparse_twostage_[a-z0-9_]+)\s*\(", text)))


def test_handle_without_a_device():
    """The mirror rejects a descending pair list itself, before the library is
    called; the library exports every fftconv_matrix_sparse_twostage_* symbol
    the header declares; and where no device is visible init fails loudly
    (there is no CPU fallback)."""
    import fftconv_amd

    syms = declared_symbols()
    for op in ("init", "update", "reset", "process", "process_device", "process_device_steps", "clone", "destroy",
               "synchronize", "inputs", "outputs", "pairs", "tail_block_size", "set_fused", "path"):
        assert f"fftconv_matrix_sparse_twostage_{op}" in syms, op
    lib = ctypes.CDLL(fftconv_amd.LIB_PATH)
    assert not [s for s in syms if not hasattr(lib, s)]
    assert all(s in fftconv_amd.SIGNATURES for s in syms)
    assert "SparseMatrixTwoStageConvolver" in fftconv_amd.__all__

    h = np.ones((2, 8), np.float32)
    for bad in ([(1, 0), (0, 0)], [(0, 1), (0, 0)], [(0, 0), (0, 0)]):
        with pytest.raises(ValueError, match="strictly ascending"):
            fftconv_amd.SparseMatrixTwoStageConvolver.init(bad, h, 2, 2, 64, 8, device=1 << 20)
    with pytest.raises(ValueError):
        fftconv_amd.SparseMatrixTwoStageConvolver.init([(0, 0)], h, 2, 2, 64, 8)  # two responses, one pair
    if fftconv_amd.device_count() == 0:
        with pytest.raises(fftconv_amd.DeviceError):
            fftconv_amd.SparseMatrixTwoStageConvolver.init([(0, 0), (1, 1)], h, 2, 2, 64, 8)
    else:
        conv = fftconv_amd.SparseMatrixTwoStageConvolver.init([(0, 0), (1, 1)], h, 2, 2, 64, 8)
        assert (conv.inputs, conv.outputs, conv.pairs, conv.tail_block_size) == (2, 2, 2, 64)
