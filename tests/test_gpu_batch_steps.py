"""process_device_steps on a lookahead batch: the per-call batch of steps
(csrc/la_batch.hpp: spectra, walk, finish and fix-up launches per chunk of up
to 64 steps) against one process_device call per block.

The batch sums every step in the per-block full pass's order, so outputs are
compared bit for bit; `channel_state` and six further per-block steps on both
handles show that the ring commit, the overlap and the state words are what a
per-block run leaves.  Two channels of each case are also checked against the
oracle with the project's tolerance."""
import functools

import numpy as np
import pytest

from common import assert_close, ir, white

pytestmark = pytest.mark.gpu

VARIANT_NORUN = 2048
AFTER = 6  # per-block steps on both handles after the compared calls


@functools.lru_cache(maxsize=None)
def _responses(C, B, S):
    rng = np.random.default_rng(9000 + 100 * C + B + S)
    return np.stack([ir(rng, S * B) for _ in range(C)])


def _blocks(seed, K, C, B):
    rng = np.random.default_rng(seed)
    return white(rng, K * C * B).reshape(K, C, B)


def _steps(conv, xd, K, shared=False):
    """K steps in one process_device_steps call; xd is [K][C][B], or [K][B]
    for the shared dry block (input stride 0)."""
    import torch

    C, B = conv.channels, xd.shape[-1]
    yd = torch.empty((K, C, B), dtype=torch.float32, device=xd.device)
    conv.process_device_steps(xd.data_ptr(), 0 if shared else B, B if shared else C * B, yd.data_ptr(), B, C * B, B, K)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def _calls(conv, xd, K, shared=False):
    """The same K steps as K process_device calls."""
    import torch

    C, B = conv.channels, xd.shape[-1]
    yd = torch.empty((K, C, B), dtype=torch.float32, device=xd.device)
    for k in range(K):
        conv.process_device(xd[k].data_ptr(), 0 if shared else B, yd[k].data_ptr(), B, B)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def _same(got, ref, what):
    assert np.array_equal(got, ref, equal_nan=True), f"{what}: {int(np.sum(got != ref))} samples differ"


def _check_pair(batch, calls, x, plan, oracles=None, shared=False, what=""):
    """Run `plan` -- a list of ("steps" | "calls", k) -- on `batch`, and the
    same blocks one call each on `calls`; then AFTER per-block steps on both.
    Bit-identical outputs and equal channel states throughout; oracles = {c:
    oracle handle in the same state} are fed the same blocks."""
    import torch

    C = batch.channels
    xd = torch.from_numpy(x).to("cuda:0")
    total = sum(k for _, k in plan)
    assert x.shape[0] >= total + AFTER
    got, at = [], 0
    for how, k in plan:
        got.append((_steps if how == "steps" else _calls)(batch, xd[at:at + k], k, shared))
        at += k
    got = np.concatenate(got)
    ref = _calls(calls, xd[:total], total, shared)
    _same(got, ref, f"{what} outputs")
    for c in range(C):
        assert batch.channel_state(c) == calls.channel_state(c), (what, c)
    more_b = _calls(batch, xd[total:total + AFTER], AFTER, shared)
    more_c = _calls(calls, xd[total:total + AFTER], AFTER, shared)
    _same(more_b, more_c, f"{what} later per-block steps")
    for c in range(C):
        assert batch.channel_state(c) == calls.channel_state(c), (what, c, "later")
    y = np.concatenate([got, more_b])
    for c, ref_c in (oracles or {}).items():
        for k in range(total + AFTER):
            r = ref_c.process(x[k] if shared else x[k, c])
            assert np.array_equal(np.isnan(y[k, c]), np.isnan(r)), (what, c, k)
            m = ~np.isnan(r)
            assert_close(y[k, c][m], r[m], what=f"{what} channel {c} block {k}")
        assert batch.channel_state(c) == (ref_c.current, ref_c.active_seg_count, ref_c.fill), (what, c)
    return y


def _pair(amd, C, B, S):
    hs = _responses(C, B, S)
    L = S * B
    batch = amd.FFTConvolver.init(hs, B, L, channels=C)
    calls = amd.FFTConvolver.init(hs, B, L, channels=C)
    assert batch.lookahead_parts() > 0
    return hs, batch, calls


def _oracles(oracle_mod, hs, B, chans):
    return {c: oracle_mod.FFTConvolver.init(hs[c], B, hs.shape[1]) for c in chans}


# two levels / three levels at B = 128, one case each at B = 256 and 512;
# neither 2 nor 8 divides the channel counts
SHAPES = [(5, 128, 40), (11, 128, 70), (5, 256, 66), (11, 512, 66)]


@pytest.mark.parametrize("C,B,S", SHAPES)
@pytest.mark.parametrize("K", [16, 19, 32, 64 + 5])
def test_batch_equals_per_block_calls(amd, oracle_mod, C, B, S, K):
    """A full window slice, a partial one, the benchmark's call length, and a
    chunk boundary with a remainder."""
    hs, batch, calls = _pair(amd, C, B, S)
    x = _blocks(K + C + B, K + AFTER, C, B)
    _check_pair(batch, calls, x, [("steps", K)], _oracles(oracle_mod, hs, B, (0, C - 1)), what=f"K={K}")


@pytest.mark.parametrize("at", [0, 13, 31])
def test_batch_nan_block(amd, oracle_mod, at):
    """A NaN sample at the chunk's first step, in its middle and at its last
    step: that channel's block is zero-filled and kept in the input buffer,
    and its later steps run off the path (the fix-up launch), as per block."""
    C, B, S, K = 5, 128, 40, 32
    hs, batch, calls = _pair(amd, C, B, S)
    x = _blocks(77 + at, K + AFTER, C, B)
    x[at, 2, 17] = np.nan
    _check_pair(batch, calls, x, [("steps", K)], _oracles(oracle_mod, hs, B, (2, 3)), what=f"nan at {at}")


def test_batch_buffered_input(amd, oracle_mod):
    """A B/3 call first: every channel holds buffered samples at the call's
    start and runs the whole call in the fix-up launch."""
    C, B, S, K = 5, 128, 40, 32
    hs, batch, calls = _pair(amd, C, B, S)
    rng = np.random.default_rng(41)
    part = white(rng, C * (B // 3)).reshape(C, B // 3)
    refs = _oracles(oracle_mod, hs, B, (1, 4))
    _same(batch.process(part), calls.process(part), "partial call")
    for c, r in refs.items():
        r.process(part[c])
    x = _blocks(42, K + AFTER, C, B)
    _check_pair(batch, calls, x, [("steps", K)], refs, what="buffered")


def test_batch_short_channel(amd, oracle_mod):
    """update_channel cuts one channel to 3 segments: off the lookahead path
    while its neighbours take the batch."""
    C, B, S, K = 5, 128, 40, 32
    hs, batch, calls = _pair(amd, C, B, S)
    short = hs[3, :3 * B].copy()
    refs = _oracles(oracle_mod, hs, B, (2, 3))
    for h in (batch, calls):
        h.update_channel(3, short)
    refs[3].update(short)
    x = _blocks(43, K + AFTER, C, B)
    _check_pair(batch, calls, x, [("steps", K)], refs, what="short channel")


def test_batch_update_shrinks_ring(amd, oracle_mod):
    """A batch update to L - 30 B at S = 40 leaves 10 active segments: the
    chunk is longer than the ring, so its later blocks overwrite its earlier
    ones in the commit."""
    C, B, S, K = 5, 128, 40, 32
    hs, batch, calls = _pair(amd, C, B, S)
    x0 = _blocks(44, 7, C, B)  # (some history in the ring first, per block)
    import torch

    xd0 = torch.from_numpy(x0).to("cuda:0")
    _same(_calls(batch, xd0, 7), _calls(calls, xd0, 7), "history")
    cut = np.ascontiguousarray(hs[:, :S * B - 30 * B])
    refs = _oracles(oracle_mod, hs, B, (0, 4))
    for c, r in refs.items():
        for k in range(7):
            r.process(x0[k, c])
        r.update(cut[c])
    for h in (batch, calls):
        h.update(cut)
    x = _blocks(45, K + AFTER, C, B)
    _check_pair(batch, calls, x, [("steps", K)], refs, what="shrunk ring")


def test_batch_shared_dry_block(amd, oracle_mod):
    """Input stride 0: every channel reads the same block."""
    C, B, S, K = 5, 128, 40, 19
    hs, batch, calls = _pair(amd, C, B, S)
    x = _blocks(46, K + AFTER, 1, B).reshape(K + AFTER, B)
    _check_pair(batch, calls, x, [("steps", K)], _oracles(oracle_mod, hs, B, (0, 3)), shared=True, what="shared")


def test_batch_consecutive_and_mixed_calls(amd, oracle_mod):
    """Two batch calls in a row (the second enters with the windows dropped,
    so a short one takes the batch too), then batch -> single call -> batch."""
    C, B, S = 11, 128, 70
    hs, batch, calls = _pair(amd, C, B, S)
    x = _blocks(47, 32 + 5 + AFTER, C, B)
    _check_pair(batch, calls, x, [("steps", 32), ("steps", 5)], _oracles(oracle_mod, hs, B, (0, 10)), what="twice")
    hs, batch, calls = _pair(amd, C, B, S)
    x = _blocks(48, 19 + 1 + 16 + AFTER, C, B)
    _check_pair(batch, calls, x, [("steps", 19), ("calls", 1), ("steps", 16)], _oracles(oracle_mod, hs, B, (1, 9)),
                what="batch, single, batch")


def test_batch_norun_variant_same_bits(amd):
    """VARIANT_NORUN keeps process_device_steps on one launch per block: the
    same bits as the batch."""
    C, B, S, K = 5, 256, 66, 32
    hs = _responses(C, B, S)
    x = _blocks(49, K + AFTER, C, B)
    import torch

    xd = torch.from_numpy(x).to("cuda:0")
    outs = []
    for v in (-1, VARIANT_NORUN):
        amd.set_kernel_variant(v)
        try:
            conv = amd.FFTConvolver.init(hs, B, S * B, channels=C)
            y = _steps(conv, xd[:K], K)
            outs.append((np.concatenate([y, _calls(conv, xd[K:], AFTER)]), [conv.channel_state(c) for c in range(C)]))
        finally:
            amd.set_kernel_variant(-1)
    _same(outs[0][0], outs[1][0], "NORUN")
    assert outs[0][1] == outs[1][1]
