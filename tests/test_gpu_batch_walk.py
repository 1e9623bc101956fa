"""The per-call batch's walk kernel (csrc/la_batch.hpp, la_batch_walk_kernel):
one workgroup per (channel, 64-slot bin slice, window slice), its four waves on
the row groups of a level, then on the level-1 and the near chain.  The slices
are 16 steps long where the grid has 512 workgroups or more and the last slice
is more than half full (lab_wide), else 8: the cases run both, and both sides
of each edge of that rule.

Every case compares process_device_steps bit for bit with the same blocks as
per-block process_device calls on a twin handle, then `channel_state` per
channel and six further per-block steps on both handles; two channels per case
are checked against the oracle with the project's tolerance.  The shapes sit
on the kernel's edges: partial spans and window slices, chains of one row and
empty row groups, ring wrap inside a chain, every bin-slice count, the
flagship's ring length."""
import functools

import numpy as np
import pytest

from common import assert_close, ir, white

pytestmark = pytest.mark.gpu

AFTER = 6  # per-block steps on both handles after the compared calls


@functools.lru_cache(maxsize=None)
def _responses(C, B, S):
    rng = np.random.default_rng(7000 + 100 * C + B + S)
    return np.stack([ir(rng, S * B) for _ in range(C)])


def _blocks(seed, K, C, B):
    rng = np.random.default_rng(seed)
    return white(rng, K * C * B).reshape(K, C, B)


def _steps(conv, xd, K):
    import torch

    C, B = conv.channels, xd.shape[-1]
    yd = torch.empty((K, C, B), dtype=torch.float32, device=xd.device)
    conv.process_device_steps(xd.data_ptr(), B, C * B, yd.data_ptr(), B, C * B, B, K)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def _calls(conv, xd, K):
    import torch

    C, B = conv.channels, xd.shape[-1]
    yd = torch.empty((K, C, B), dtype=torch.float32, device=xd.device)
    for k in range(K):
        conv.process_device(xd[k].data_ptr(), B, yd[k].data_ptr(), B, B)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def _same(got, ref, what):
    assert np.array_equal(got, ref, equal_nan=True), f"{what}: {int(np.sum(got != ref))} samples differ"


def _run(amd, oracle_mod, C, B, S, plan, seed, what, act=None):
    """`plan` -- a list of ("steps" | "calls", k) -- on one handle, the same
    blocks one call each on its twin, then AFTER per-block steps on both.
    act: update every handle to a response of `act` segments first (a handle
    is on the lookahead path from S = 40 up; the level count follows S)."""
    import torch

    hs = _responses(C, B, S)
    batch = amd.FFTConvolver.init(hs, B, S * B, channels=C)
    calls = amd.FFTConvolver.init(hs, B, S * B, channels=C)
    assert batch.lookahead_parts() > 0
    cut = None if act is None else np.ascontiguousarray(hs[:, :act * B])
    if cut is not None:
        batch.update(cut)
        calls.update(cut)
    total = sum(k for _, k in plan)
    x = _blocks(seed, total + AFTER, C, B)
    xd = torch.from_numpy(x).to("cuda:0")
    got, at = [], 0
    for how, k in plan:
        got.append((_steps if how == "steps" else _calls)(batch, xd[at:at + k], k))
        at += k
    got = np.concatenate(got)
    _same(got, _calls(calls, xd[:total], total), f"{what} outputs")
    for c in range(C):
        assert batch.channel_state(c) == calls.channel_state(c), (what, c)
    more_b = _calls(batch, xd[total:], AFTER)
    more_c = _calls(calls, xd[total:], AFTER)
    _same(more_b, more_c, f"{what} later per-block steps")
    for c in range(C):
        assert batch.channel_state(c) == calls.channel_state(c), (what, c, "later")
    y = np.concatenate([got, more_b])
    for c in (0, C - 1):
        ref = oracle_mod.FFTConvolver.init(hs[c], B, S * B)
        if cut is not None:
            ref.update(cut[c])
        for k in range(total + AFTER):
            assert_close(y[k, c], ref.process(x[k, c]), what=f"{what} channel {c} block {k}")
        assert batch.channel_state(c) == (ref.current, ref.active_seg_count, ref.fill), (what, c)


@pytest.mark.parametrize("K", [1, 17, 31, 33, 40, 63, 64, 65])
def test_span_and_slice_edges(amd, oracle_mod, K):
    """One live step, one step into the second window slice, partial and full
    second slices, one step into the third, partial later slices, a full
    chunk, and a second chunk of one step.  (A call of
    fewer than 16 steps takes the batch only while the windows are dropped, so
    K = 1 follows a 16-step batch call.)"""
    plan = [("steps", 16), ("steps", 1)] if K == 1 else [("steps", K)]
    _run(amd, oracle_mod, 5, 256, 70, plan, 100 + K, f"K={K}")


@pytest.mark.parametrize("S,alloc", [(6, 40), (7, 40), (17, 40), (18, 40), (18, 70), (65, 65), (66, 66), (67, 67),
                                     (69, 69)])
def test_level_edges(amd, oracle_mod, S, alloc):
    """One level-1 row (S = 6), two, a full level 1 without level 2 (17), one
    level-2 row and three empty groups (18; under a three-level handle too:
    every level-3 group empty), a full level 2 without level 3 (65), then one
    to four level-3 rows (66, 67, 69: empty groups).  Rings shorter than 40
    rows come from an update of a 40-row handle."""
    _run(amd, oracle_mod, 3, 128, alloc, [("steps", 32)], 200 + S, f"S={S}/{alloc}", act=S if S != alloc else None)


@pytest.mark.parametrize("before", [40 - 3, 40 - 1])
def test_ring_wrap_inside_chains(amd, oracle_mod, before):
    """The ring position near its end at the chunk's start: the chains' X rows
    wrap inside a walk."""
    _run(amd, oracle_mod, 9, 256, 40, [("calls", before), ("steps", 32)], 300 + before, f"before={before}")


def test_chunk_longer_than_ring(amd, oracle_mod):
    """64 steps on a ring of 20 rows: most X rows are the call's own blocks."""
    _run(amd, oracle_mod, 9, 128, 40, [("steps", 64)], 320, "K=64 S=20", act=20)


@pytest.mark.parametrize("B", [128, 256, 512])
def test_every_bin_slice_count(amd, oracle_mod, B):
    """1, 2 and 4 bin slices per channel, three window slices each."""
    _run(amd, oracle_mod, 3, B, 70, [("steps", 33)], 400 + B, f"B={B}")


def test_flagship_ring_length(amd, oracle_mod):
    """The benchmark's 188-row ring and call length, after 5 per-block steps."""
    _run(amd, oracle_mod, 2, 256, 188, [("calls", 5), ("steps", 32)], 500, "S=188")


# ---- the 16-step slices: grids of 512 workgroups (ceil8(C) x bin slices x ceil(K / 16))


@pytest.mark.parametrize("C,K", [(64, 64), (64, 63), (64, 57), (64, 56), (56, 64)])
def test_wide_rule_edges(amd, oracle_mod, C, K):
    """B = 256 (two bin slices).  16-step slices: a full chunk, a partial last
    slice, a last slice of 9 steps; 8-step slices: a last 16-step slice of 8
    (K = 56), and a grid of 448 (C = 56)."""
    _run(amd, oracle_mod, C, 256, 70, [("steps", K)], 600 + C + K, f"C={C} K={K}")


@pytest.mark.parametrize("S,alloc", [(6, 40), (7, 40), (17, 40), (18, 40), (18, 70), (65, 65), (66, 66), (67, 67),
                                     (69, 69)])
def test_wide_level_edges(amd, oracle_mod, S, alloc):
    """test_level_edges' rings under the 16-step slices (128 channels, B = 128, K = 64)."""
    _run(amd, oracle_mod, 128, 128, alloc, [("steps", 64)], 700 + S, f"wide S={S}/{alloc}", act=S if S != alloc else None)


def test_wide_ring_wrap(amd, oracle_mod):
    """The ring position three rows before its end at the chunk's start, 16-step slices."""
    _run(amd, oracle_mod, 64, 256, 40, [("calls", 37), ("steps", 64)], 800, "wide before=37")


@pytest.mark.parametrize("C,B", [(128, 128), (32, 512)])
def test_wide_bin_slice_counts(amd, oracle_mod, C, B):
    """1 and 4 bin slices per channel under the 16-step slices (2: test_wide_rule_edges)."""
    _run(amd, oracle_mod, C, B, 70, [("steps", 64)], 900 + B, f"wide B={B}")
