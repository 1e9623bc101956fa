"""The child of tests/test_gpu_poison.py: every family once, at the smallest
shapes that reach its code, writing one JSON line per scenario.

    poison_worker.py OUT.jsonl [scenario ...]        (default: every scenario)

The parent runs it twice, with FFTCONV_POISON_ALLOC=0 and =1 (csrc/host.cpp
poison_alloc: every new device buffer, table, scratch and pinned stage filled
with 0xff bytes), and compares the lines: a path that reads memory it never
wrote gives other output bits in the poisoned run.  The switch is read once per
process, which is why this is a child program.

A line is {"name", "in": SHA-256 of every input array drawn, "out": SHA-256 of
every output array and every state tuple read, "finite", "max_abs"}, hashed as
matrix_bits.sha (shape plus bytes), appended and flushed after its scenario, so
the file's last line names the scenario before the one that was running if the
child dies.  Inputs come from a numpy.random.default_rng seeded from the
scenario's name (matrix_bits.Draw).  Nothing here reads or sets an environment
variable."""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "fft-convolution_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import matrix_bits  # noqa: E402
from matrix_la_ref import MAIN as LA_MAIN, Q  # noqa: E402
from matrix_ref import RAGGED_64  # noqa: E402
from matrix_sp_la_ref import MAIN as SPLA_MAIN, shape_len as spla_len, shape_pairs as spla_pairs  # noqa: E402
from matrix_sp_ref import PATTERN_1  # noqa: E402
from matrix_sp_ts_ref import SHAPES as SPTS_SHAPES, pairs_of  # noqa: E402
from matrix_ts_ref import SHAPES as TS_SHAPES  # noqa: E402

# (csrc/variant.hpp)
NOPAIR, NOFMIX, IRBLOCK, T0BLOCK, T0FUSED = 8, 64, 128, 256, 512
AFTER = 6  # per-block calls after a batch of steps (tests/test_gpu_batch_steps.py)


def seed_of(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


class Rec:
    """a scenario's seeded inputs (d) and everything it read back (outs)"""

    def __init__(self, name):
        self.d = matrix_bits.Draw(seed_of(name))
        self.outs = []

    def h(self, *shape):
        return self.d.h(tuple(shape))

    def x(self, rows, n):
        return self.d.x(rows, n)

    def out(self, y):
        y = np.ascontiguousarray(y, dtype=np.float32)
        self.outs.append(y)
        return y

    def state(self, *values):
        """counters and flags, hashed with the outputs"""
        self.outs.append(np.asarray([float(v) for v in values], np.float32).reshape(1, -1))


def run_host(R, conv, x, lengths, out_len=None):
    """consecutive process() calls over x[rows][sum(lengths)]"""
    pos = 0
    for n in lengths:
        R.out(conv.process(x[..., pos:pos + n]) if out_len is None else conv.process(x[..., pos:pos + n], out_len))
        pos += n
    assert pos == x.shape[-1]


def steps_padded(R, conv, x, rows_out, n_in, n, K):
    """process_device_steps on a side stream over padded rows: n_in + 5 floats
    per input row, n + 3 per output row, the output prefilled with -7; the
    padding is hashed with the output"""
    import torch

    rows_in = x.shape[0]
    assert x.shape[1] == K * n_in
    dev = torch.device("cuda:0")
    xs = np.zeros((K, rows_in, n_in + 5), np.float32)
    xs[:, :, :n_in] = x.reshape(rows_in, K, n_in).transpose(1, 0, 2)
    xd = torch.from_numpy(xs).to(dev)
    yd = torch.full((K, rows_out, n + 3), -7.0, device=dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream())
    conv.process_device_steps(xd.data_ptr(), n_in + 5, rows_in * (n_in + 5), yd.data_ptr(), n + 3, rows_out * (n + 3),
                              n, K, s.cuda_stream)
    s.synchronize()
    y = yd.cpu().numpy()
    assert (y[:, :, n:] == -7.0).all() and np.abs(y[:, :, :n]).max() > 0
    R.out(y)


def blocks_device(R, conv, x, B, shared=False):
    """one process_device call per block of x[K][C][B] ([K][B] with input stride 0)"""
    import torch

    xd = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    K, C = x.shape[0], conv.channels
    yd = torch.empty((K, C, B), dtype=torch.float32, device="cuda:0")
    for k in range(K):
        conv.process_device(xd[k].data_ptr(), 0 if shared else B, yd[k].data_ptr(), B, B)
    torch.cuda.synchronize()
    R.out(yd.cpu().numpy())


def steps_device(R, conv, x, B, shared=False):
    """the blocks of x[K][C][B] in one process_device_steps call"""
    import torch

    xd = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    K, C = x.shape[0], conv.channels
    yd = torch.empty((K, C, B), dtype=torch.float32, device="cuda:0")
    conv.process_device_steps(xd.data_ptr(), 0 if shared else B, B if shared else C * B, yd.data_ptr(), B, C * B, B, K)
    torch.cuda.synchronize()
    R.out(yd.cpu().numpy())


def channel_states(R, conv):
    for c in range(conv.channels):
        R.state(*conv.channel_state(c))


# ---- the matrix families: the state operations matrix_bits.CASES omit --------
def _matrix_common(R, conv, I, O, B, first, rest, again, n_steps, K):
    """`first` calls (ending mid-block), a clone continued beside the original
    over `rest`, a reset and `again`, then K padded device steps of n_steps"""
    x = R.x(I, sum(first) + sum(rest))
    run_host(R, conv, x[:, :sum(first)], first)
    R.state(*conv.state())
    twin = conv.clone()
    run_host(R, conv, x[:, sum(first):], rest)
    run_host(R, twin, x[:, sum(first):], rest)
    R.state(*conv.state(), *twin.state())
    conv.reset()
    R.state(*conv.state())
    run_host(R, conv, R.x(I, sum(again)), again)
    conv.reset()
    steps_padded(R, conv, R.x(I, K * n_steps), O, n_steps, n_steps, K)
    R.state(*conv.state())


def dense_ops(F, R):
    import torch

    I, O, B, L = 3, 2, 64, 1000  # (tests/test_gpu_matrix.py test_reset_and_clone, test_process_device_steps)
    conv = F.MatrixConvolver.init(R.h(O, I, L), B, L)
    _matrix_common(R, conv, I, O, B, list(RAGGED_64[:11]), list(RAGGED_64[11:]), [B] * 5 + [17, B - 17], 40, 30)
    conv.update_pairs([(0, 1), (1, 2)], R.h(2, L))  # (test_gpu_matrix_update_pairs.test_plain_matrix)
    run_host(R, conv, R.x(I, 6 * B), [B] * 6)
    # a zero-length response through update_device (test_zero_length_response_device): n zeros per row
    n = 40
    some = torch.ones(8, device="cuda:0")
    conv.update_device(some.data_ptr(), 0, 0)
    R.state(*conv.state())
    xd = torch.ones((I, n + 5), device="cuda:0")
    yd = torch.full((O, n + 3), -7.0, device="cuda:0")
    conv.process_device(xd.data_ptr(), n + 5, yd.data_ptr(), n + 3, n)
    conv.synchronize()
    torch.cuda.synchronize()
    y = R.out(yd.cpu().numpy())
    assert (y[:, :n] == 0.0).all() and (y[:, n:] == -7.0).all()
    R.state(*conv.state())


def sparse_ops(F, R):
    I, O, B, L = 5, 4, 64, 1000  # (tests/test_gpu_matrix_sparse.py test_reset_and_clone, test_process_device_steps)
    P = len(PATTERN_1)
    conv = F.SparseMatrixConvolver.init(PATTERN_1, R.h(P, L), I, O, B, L)
    _matrix_common(R, conv, I, O, B, list(RAGGED_64[:11]), list(RAGGED_64[11:]), [B] * 5 + [17, B - 17], 40, 30)
    conv.update_pairs([PATTERN_1[1], PATTERN_1[-1]], R.h(2, L))
    run_host(R, conv, R.x(I, 6 * B), [B] * 6)
    R.state(*conv.state())


def la_ops(F, R):
    I, O, B, L = LA_MAIN  # (tests/test_gpu_matrix_la.py test_clone_mid_window, test_process_device_steps)
    conv = F.MatrixLookaheadConvolver.init(R.h(O, I, L), B, L)
    # 2 Q + 3 blocks: the clone is taken mid-window, with far rows served from windows
    _matrix_common(R, conv, I, O, B, [B] * (2 * Q + 3), [B] * (2 * Q) + [20, B - 20], [B] * (Q + 3), 40, 30)
    conv.reset()
    steps_padded(R, conv, R.x(I, 30 * B), O, B, B, 30)
    R.state(*conv.state())


def spla_ops(F, R):
    s = SPLA_MAIN  # (tests/test_gpu_matrix_sparse_la.py test_clone_mid_window_and_reset, test_update_pairs_equals_update)
    pairs, L, O = spla_pairs(s), spla_len(s), len(s.cols)
    conv = F.SparseMatrixLookaheadConvolver.init(pairs, R.h(len(pairs), L), s.I, O, s.B, L)
    _matrix_common(R, conv, s.I, O, s.B, [s.B] * (2 * Q + 3), [s.B] * (2 * Q) + [20, s.B - 20], [s.B] * (Q + 3), 40, 30)
    conv.reset()
    steps_padded(R, conv, R.x(s.I, 30 * s.B), O, s.B, s.B, 30)
    conv.update_pairs([pairs[0], pairs[len(pairs) // 2], pairs[-1]], R.h(3, L))  # mid-window after 30 blocks
    run_host(R, conv, R.x(s.I, (2 * Q + 1) * s.B), [s.B] * (2 * Q + 1))
    R.state(*conv.state())


def _xf_ops(R, conv, hshape, I, O, m, pairs):
    """a clone mid-fade continued beside the original, padded device steps
    through the next fade, an update_pairs (reset() is todo!() in the
    reference: NotImplementedInReference)"""
    x = R.x(I, 16 * m)
    run_host(R, conv, x[:, :4 * m], [m] * 4)
    conv.update(R.h(*hshape))
    run_host(R, conv, x[:, 4 * m:6 * m], [m] * 2)
    assert conv.is_crossfading()
    twin = conv.clone()
    assert twin.is_crossfading()
    for c in (conv, twin):
        run_host(R, c, x[:, 6 * m:], [m] * 10)
        R.state(c.is_crossfading(), c.path(), c.diff_pairs())
    assert not conv.is_crossfading()
    conv.update(R.h(*hshape))
    steps_padded(R, conv, R.x(I, 12 * m), O, m, m, 12)
    assert not conv.is_crossfading()
    conv.update_pairs(pairs, R.h(len(pairs), hshape[-1]))
    run_host(R, conv, R.x(I, 8 * m), [m] * 8)
    R.state(conv.is_crossfading(), conv.path(), conv.diff_pairs(), *conv.last_patch())


def xf_ops(F, R):
    I, O, B, L = 3, 2, 64, 1000  # (tests/test_gpu_matrix_xf.py scenario "fade", test_clone_mid_fade)
    conv = F.MatrixCrossfadeConvolver.new(F.MatrixConvolver.init(R.h(O, I, L), B, L), L, 64, 96)
    _xf_ops(R, conv, (O, I, L), I, O, 64, [(0, 1), (1, 2)])


def spxf_ops(F, R):
    I, O, B, L = 5, 4, 128, 2045  # (tests/test_gpu_matrix_sparse_xf.py scenario "fade")
    P = len(PATTERN_1)
    base = F.SparseMatrixConvolver.init(PATTERN_1, R.h(P, L), I, O, B, L)
    conv = F.SparseMatrixCrossfadeConvolver.new(base, L, 128, 192)
    _xf_ops(R, conv, (P, L), I, O, 128, [PATTERN_1[1], PATTERN_1[-1]])


def _ts_ops(R, conv, I, O, head, T):
    """a clone mid-period and mid-block (11 aligned calls and one of 20 samples,
    tests/test_gpu_matrix_ts.py scenario "clone") continued beside the
    original past two periods, a reset, padded device steps over 3 periods"""
    first, rest = [head] * 11 + [20], [head - 20] + [head] * (2 * T // head + 4)
    x = R.x(I, sum(first) + sum(rest))
    run_host(R, conv, x[:, :sum(first)], first)
    twin = conv.clone()
    for c in (conv, twin):
        run_host(R, c, x[:, sum(first):], rest)
    conv.reset()
    run_host(R, conv, R.x(I, 13 * head), [head] * 13)
    conv.reset()
    K = 3 * T // head
    steps_padded(R, conv, R.x(I, K * head), O, head, head, K)
    R.state(conv.tail_block_size, conv.path(head))


def ts_ops(F, R):
    I, O, head, L, T, _, _ = TS_SHAPES["three-stage"]
    conv = F.MatrixTwoStageConvolver.init(R.h(O, I, L), head, L)
    assert conv.tail_block_size == T
    _ts_ops(R, conv, I, O, head, T)


def spts_ops(F, R):
    s = SPTS_SHAPES["three-stage"]
    pairs = pairs_of(s)
    conv = F.SparseMatrixTwoStageConvolver.init(pairs, R.h(len(pairs), s.L), s.I, s.O, s.head, s.L)
    assert conv.tail_block_size == s.T
    _ts_ops(R, conv, s.I, s.O, s.head, s.T)


# ---- uniform ----------------------------------------------------------------
def uniform_short(F, R):
    """no lookahead: the Scratch buffers grow and then serve smaller calls"""
    C, B, L = 3, 64, 1000
    conv = F.FFTConvolver.init(R.h(C, L), B, L, channels=C)
    assert conv.lookahead_parts() == 0
    ragged = [1, 7, 64, 100, 3, 200, 64, 65, 128, 31, 33]
    run_host(R, conv, R.x(C, sum(ragged)), ragged)
    conv.update(R.h(C, 130))
    run_host(R, conv, R.x(C, 3 * B), [B, 10, B - 10, B])
    conv.update_channel(1, R.h(L))
    run_host(R, conv, R.x(C, 2 * B + 9), [B, 9, B])
    conv.update_channel(2, np.zeros(0, np.float32))
    run_host(R, conv, R.x(C, 3 * B), [B] * 3)
    channel_states(R, conv)
    conv.reset()
    run_host(R, conv, R.x(C, 3 * B + 5), [B, 5, 2 * B])
    twin = conv.clone()
    x = R.x(C, 20 * B)
    for c in (conv, twin):
        run_host(R, c, x, [B] * 20)
        channel_states(R, c)


def uniform_la(C, B, S):
    def scenario(F, R):
        conv = F.FFTConvolver.init(R.h(C, S * B), B, S * B, channels=C)
        assert conv.lookahead_parts() > 0
        blocks_device(R, conv, R.x(2 * S * C, B).reshape(2 * S, C, B), B)
        channel_states(R, conv)
        conv.reset()
        blocks_device(R, conv, R.x(S * C, B).reshape(S, C, B), B)
        channel_states(R, conv)
    return scenario


def uniform_batch(C, B, S, K, how=None):
    """process_device_steps on the lookahead step's per-call batch
    (csrc/la_batch.hpp), then AFTER per-block calls: the scenarios of
    tests/test_gpu_batch_steps.py"""
    def scenario(F, R):
        conv = F.FFTConvolver.init(R.h(C, S * B), B, S * B, channels=C)
        assert conv.lookahead_parts() > 0
        if how == "buffered":   # every channel enters with buffered samples: the whole call in the fix-up launch
            R.out(conv.process(R.x(C, B // 3)))
        if how == "short-channel":
            conv.update_channel(3, R.h(3 * B))
        shared = how == "shared"
        x = R.x((K + AFTER) * (1 if shared else C), B)
        x = x.reshape(K + AFTER, B) if shared else x.reshape(K + AFTER, C, B)
        if how == "nan":
            x[13, 2, 17] = np.nan
        steps_device(R, conv, x[:K], B, shared)
        channel_states(R, conv)
        blocks_device(R, conv, x[K:], B, shared)
        channel_states(R, conv)
    return scenario


def uniform_windows(F, R):
    """far-row windows of the generic step at the smallest shape of
    tests/test_gpu_windows.py: past one window period, a partial call, a reset"""
    C, B, S = 11, 1024, 30
    L = S * B - 5
    conv = F.FFTConvolver.init(R.h(C, L), B, L, channels=C)
    assert conv.far_windows() > 0
    lengths = [B] * (S + 12) + [B // 3, B - B // 3] + [B] * 9
    run_host(R, conv, R.x(C, sum(lengths)), lengths)
    channel_states(R, conv)
    conv.reset()
    run_host(R, conv, R.x(C, 12 * B), [B] * 12)
    channel_states(R, conv)


def uniform_long_block(F, R):
    C, B = 2, 16384
    L = 2 * B + 7
    conv = F.FFTConvolver.init(R.h(C, L), B, L, channels=C)
    calls = [5000, 16384, 30000, 11] * 2
    run_host(R, conv, R.x(C, sum(calls)), calls)
    conv.update(R.h(C, 2 * B - 5))
    run_host(R, conv, R.x(C, B + 5000), [B, 5000])
    twin = conv.clone()
    x = R.x(C, 2 * B + 11)
    for c in (conv, twin):
        run_host(R, c, x, [B - 5000, B, 5011])
        channel_states(R, c)


def uniform_update_device(F, R):
    """update_device with stride > len on a side stream"""
    import torch

    C, B, L, n = 3, 64, 1000, 700
    conv = F.FFTConvolver.init(R.h(C, L), B, L, channels=C)
    run_host(R, conv, R.x(C, 5 * B), [B] * 5)
    rows = np.full((C, n + 7), -7.0, np.float32)
    rows[:, :n] = R.h(C, n)
    hd = torch.from_numpy(rows).to("cuda:0")
    s = torch.cuda.Stream("cuda:0")
    s.wait_stream(torch.cuda.current_stream())
    conv.update_device(hd.data_ptr(), n, n + 7, s.cuda_stream)
    s.synchronize()
    run_host(R, conv, R.x(C, 18 * B + 10), [B] * 9 + [10] + [B] * 9)
    channel_states(R, conv)


def uniform_update_capped_stage(F, R):
    """a host update through a pinned stage capped to 3 response rows"""
    C, B = 8, 128
    L = 45 * B
    F.set_host_stage_limit(3 * L * 4)
    try:
        conv = F.FFTConvolver.init(R.h(C, L), B, L, channels=C)
        run_host(R, conv, R.x(C, 4 * B), [B] * 4)
        conv.update(R.h(C, L - 100))
        run_host(R, conv, R.x(C, 50 * B), [B] * 50)
        twin = conv.clone()
        twin.update(R.h(C, L))
        run_host(R, twin, R.x(C, 6 * B), [B] * 6)
        channel_states(R, conv)
    finally:
        F.set_host_stage_limit(0)


def uniform_update_irblock(F, R):
    """the IR transform one segment per workgroup (VARIANT_IRBLOCK) and per wave"""
    C, B, L = 3, 128, 2000
    h, h2, x = R.h(C, L), R.h(C, L - 300), R.x(C, 40 * B)
    for v in (-1, IRBLOCK):
        F.set_kernel_variant(v)
        try:
            conv = F.FFTConvolver.init(h, B, L, channels=C)
            run_host(R, conv, x[:, :20 * B], [B] * 20)
            conv.update(h2)
            run_host(R, conv, x[:, 20 * B:], [B] * 20)
        finally:
            F.set_kernel_variant(-1)
    assert np.array_equal(np.concatenate(R.outs[:40], axis=1), np.concatenate(R.outs[40:], axis=1))


# ---- two-stage --------------------------------------------------------------
def twostage(head, L, calls, variant=-1, periods=2):
    def scenario(F, R):
        F.set_kernel_variant(variant)
        try:
            conv = F.TwoStageFFTConvolver.init(R.h(L), head, L)
            T = conv.tail_block_size
            lengths = list(calls) * (-(-(periods * T + head) // sum(calls)) + 2)
            run_host(R, conv, R.x(1, sum(lengths))[0], lengths)
            R.state(T)
        finally:
            F.set_kernel_variant(-1)
    return scenario


def twostage_steps(F, R):
    """process_device_steps over 3 tail periods (the head's run writes the
    pending spectra, tests/test_gpu_twostage_defer.py); the handle's only
    counter in the ABI, the tail block size, is hashed with the output"""
    head, L, C = 64, 12000, 3
    conv = F.TwoStageFFTConvolver.init(R.h(C, L), head, L, channels=C)
    T = conv.tail_block_size
    K = 3 * T // head + 5
    steps_padded(R, conv, R.x(C, K * head), C, head, head, K)
    R.state(T)
    run_host(R, conv, R.x(C, 4 * head), [head] * 4)


def twostage_clone_reset(F, R):
    head, L = 64, 12000
    conv = F.TwoStageFFTConvolver.init(R.h(L), head, L)
    per = conv.tail_block_size // head
    run_host(R, conv, R.x(1, (per + 9) * head)[0], [head] * (per + 9))  # 9 blocks pending
    twin = conv.clone()
    x = R.x(1, 2 * per * head)[0]
    for c in (conv, twin):
        run_host(R, c, x, [head] * (2 * per))
    run_host(R, conv, R.x(1, 5 * head)[0], [head] * 5)
    conv.reset()
    run_host(R, conv, R.x(1, (2 * per + 3) * head)[0], [head] * (2 * per + 3))


def twostage_long_tail(F, R):
    head, L, T = 512, 200000, 16384
    conv = F.TwoStageFFTConvolver.init(R.h(L), head, L)
    assert conv.tail_block_size == T
    calls = 2 * T // head + 6  # past both tail swaps
    run_host(R, conv, R.x(1, calls * head)[0], [head] * calls)


# ---- crossfade --------------------------------------------------------------
def crossfade(B, L, every, xfade):
    """tests/test_gpu_parity.py test_crossfade_vs_oracle: an update every
    `every` blocks, so some land during a fade and take the pending path"""
    def scenario(F, R):
        h = R.h(L)
        if xfade is None:
            conv = F.CrossfadeConvolver.init(h, B, L)
        else:
            conv = F.CrossfadeConvolver.new(F.FFTConvolver.init(h, B, L), L, B, xfade)
        pending = 0  # updates that arrived during a fade
        for i in range(40):
            if i % every == every - 1:
                pending += conv.is_crossfading()
                conv.update(R.h(int(R.d.rng.integers(1, L + 1))))
            R.out(conv.process(R.x(1, B)[0], B if i % 4 else B // 2))
            R.state(conv.is_crossfading())
        R.state(pending)
        assert pending > 0 or xfade is not None
    return scenario


def crossfade_la(variant):
    """both convolvers on the lookahead step: the fused mix (default), the
    stand-alone mix kernel (NOFMIX), A and B in separate launches (NOPAIR)"""
    def scenario(F, R):
        C, B, S = 3, 256, 66
        L = S * B
        F.set_kernel_variant(variant)
        try:
            base = F.FFTConvolver.init(R.h(C, L), B, L, channels=C)
            assert base.lookahead_parts() > 0
            conv = F.CrossfadeConvolver.new(base, L, B, 3 * B)
            x = R.x(C, 24 * B)
            run_host(R, conv, x[:, :6 * B], [B] * 6)
            conv.update(R.h(C, L))
            run_host(R, conv, x[:, 6 * B:8 * B], [B] * 2)
            assert conv.is_crossfading()
            conv.update(R.h(C, L - 5 * B))  # during the fade: stored
            run_host(R, conv, x[:, 8 * B:], [B] * 16)
            R.state(conv.is_crossfading())
        finally:
            F.set_kernel_variant(-1)
    return scenario


def crossfade_twostage(F, R):
    """tests/test_gpu_crossfade_twostage.py: its smallest shape, and its
    smallest one with a tail (past both tail swaps)"""
    for head, L, C in ((128, 200, 1), (32, 3000, 3)):
        h = R.h(C, L)
        conv = F.CrossfadeConvolver.init(h if C > 1 else h[0], head, L, channels=C, inner=F.TwoStageFFTConvolver)
        T = F.compute_tail_block_size(head, L)
        for i in range(max(2 * T // head + 5, 12)):
            x = R.x(C, head)
            R.out(conv.process(x if C > 1 else x[0], head if i % 5 else head // 2))
        R.state(conv.is_crossfading(), T)


def crossfade_long_block(F, R):
    """the mix table and calls longer than 1024 samples"""
    B = 16384
    L = 3 * B
    conv = F.CrossfadeConvolver.init(R.h(L), B, L)
    x = R.x(1, 10 * B)[0]
    run_host(R, conv, x[:3 * B], [B] * 3)
    conv.update(R.h(L))
    run_host(R, conv, x[3 * B:5 * B], [B] * 2)
    R.state(conv.is_crossfading())
    conv.update(R.h(L - B))
    run_host(R, conv, x[5 * B:], [B] * 5)
    R.state(conv.is_crossfading())


def crossfade_clone(F, R):
    C, B, L = 2, 64, 700
    conv = F.CrossfadeConvolver.init(R.h(C, L), B, L, channels=C)
    x = R.x(C, 18 * B)
    run_host(R, conv, x[:, :4 * B], [B] * 4)
    conv.update(R.h(C, L))
    run_host(R, conv, x[:, 4 * B:6 * B], [B] * 2)
    assert conv.is_crossfading()
    twin = conv.clone()
    for c in (conv, twin):
        run_host(R, c, x[:, 6 * B:], [B] * 12)
        R.state(c.is_crossfading())


# ---- the public Fft ----------------------------------------------------------
def fft(n):
    """forward and inverse, the host form and the device form with row strides
    larger than a row (the padding prefilled with -7 and hashed)"""
    def scenario(F, R):
        import torch

        rows, nbf = 3, 2 * (n // 2 + 1)
        f = F.Fft(n)
        x = R.x(rows, n)
        spec = f.forward(x)
        R.out(spec.view(np.float32))
        back, flags = f.inverse(spec)
        R.out(back)
        R.state(*flags)
        dev = torch.device("cuda:0")
        xs = np.full((rows, n + 8), -7.0, np.float32)
        xs[:, :n] = x
        xd = torch.from_numpy(xs).to(dev)
        sd = torch.full((rows, nbf + 8), -7.0, device=dev)
        bd = torch.full((rows, n + 8), -7.0, device=dev)
        st = torch.full((rows,), 9, dtype=torch.int32, device=dev)
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream())
        f.forward_device(xd.data_ptr(), n + 8, sd.data_ptr(), nbf + 8, rows, s.cuda_stream)
        f.inverse_device(sd.data_ptr(), nbf + 8, bd.data_ptr(), n + 8, rows, st.data_ptr(), s.cuda_stream)
        s.synchronize()
        assert (R.out(sd.cpu().numpy())[:, nbf:] == -7.0).all()
        assert (R.out(bd.cpu().numpy())[:, n:] == -7.0).all()
        R.state(*st.cpu().numpy())
    return scenario


def fft_inverse_status(F, R):
    """an inverse with a non-zero DC imaginary part: the status buffer"""
    for n in (256, 1000):
        f = F.Fft(n)
        spec = f.forward(R.x(3, n)).copy()
        spec[1, 0] += 0.5j
        back, flags = f.inverse(spec)
        assert list(flags) == [False, True, False]
        R.out(back)
        R.state(*flags)


def _scenarios():
    s = {name: None for name in matrix_bits.CASES}  # through matrix_bits.run_case
    s.update({
        "dense-ops": dense_ops, "sparse-ops": sparse_ops, "la-ops": la_ops, "spla-ops": spla_ops,
        "xf-ops": xf_ops, "spxf-ops": spxf_ops, "ts-ops": ts_ops, "spts-ops": spts_ops,
        "uniform-short": uniform_short,
        "uniform-la-C5-B128-S40": uniform_la(5, 128, 40),
        "uniform-la-C11-B128-S70": uniform_la(11, 128, 70),
        "uniform-batch-K32": uniform_batch(5, 128, 40, 32),
        "uniform-batch-K19": uniform_batch(5, 128, 40, 19),
        "uniform-batch-buffered": uniform_batch(5, 128, 40, 32, "buffered"),
        "uniform-batch-shared": uniform_batch(5, 128, 40, 19, "shared"),
        "uniform-batch-nan": uniform_batch(5, 128, 40, 32, "nan"),
        "uniform-batch-short-channel": uniform_batch(5, 128, 40, 32, "short-channel"),
        "uniform-batch-C11-S70-K69": uniform_batch(11, 128, 70, 69),
        "uniform-windows": uniform_windows,
        "uniform-long-block": uniform_long_block,
        "uniform-update-device": uniform_update_device,
        "uniform-update-capped-stage": uniform_update_capped_stage,
        "uniform-update-irblock": uniform_update_irblock,
        "twostage-32-5000-ragged": twostage(32, 5000, [32, 13, 19]),
        "twostage-64-12000": twostage(64, 12000, [64]),
        "twostage-64-12000-t0fused": twostage(64, 12000, [64], T0FUSED),
        "twostage-64-12000-t0block": twostage(64, 12000, [64], T0BLOCK),
        "twostage-steps": twostage_steps,
        "twostage-clone-reset": twostage_clone_reset,
        "twostage-long-tail": twostage_long_tail,
        "crossfade-B64-L700": crossfade(64, 700, 3, None),
        "crossfade-B128-L1000-x300": crossfade(128, 1000, 7, 300),
        "crossfade-la": crossfade_la(-1),
        "crossfade-la-nofmix": crossfade_la(NOFMIX),
        "crossfade-la-nopair": crossfade_la(NOPAIR),
        "crossfade-twostage": crossfade_twostage,
        "crossfade-long-block": crossfade_long_block,
        "crossfade-clone": crossfade_clone,
        "fft-256": fft(256), "fft-32768": fft(1 << 15), "fft-1000": fft(1000), "fft-20000": fft(20000),
        "fft-inverse-status": fft_inverse_status,
    })
    return s


SCENARIOS = _scenarios()
FEEDS_NAN = {"uniform-batch-nan"}  # the scenarios whose input holds a NaN


def run_scenario(F, name):
    if SCENARIOS[name] is None:
        r = matrix_bits.run_case(F, name)
        return {"name": name, "in": r["in"], "out": r["out"], "finite": True, "max_abs": r["max_abs"]}
    R = Rec(name)
    try:
        SCENARIOS[name](F, R)
    finally:
        F.set_kernel_variant(-1)
        F.set_host_stage_limit(0)
    flat = np.concatenate([y.ravel() for y in R.outs])
    return {"name": name, "in": matrix_bits.sha(R.d.arrays), "out": matrix_bits.sha(R.outs),
            "finite": bool(np.isfinite(flat).all()), "max_abs": float(np.nanmax(np.abs(flat)))}


def main():
    out, names = sys.argv[1], sys.argv[2:] or list(SCENARIOS)
    import fftconv_amd as F

    if F.device_count() < 1:
        raise SystemExit("no HIP device visible")
    with open(out, "a") as f:
        for name in names:
            t0 = time.time()
            print(f"{name} ...", end="", file=sys.stderr, flush=True)  # (the one running, should the child die)
            f.write(json.dumps(run_scenario(F, name)) + "\n")
            f.flush()
            os.fsync(f.fileno())
            print(f" {time.time() - t0:.2f} s", file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
