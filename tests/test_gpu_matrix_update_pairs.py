"""update_pairs of the MatrixCrossfadeConvolver and the MatrixConvolver
(include/fftconv.h): update_pairs(pairs, rows) is update(R'), bit for
bit, R' = the base set with the listed pairs replaced.

Every case drives two handles of the same geometry through the same calls: one
gets update_pairs, its twin gets update(R') with R' built here on the host (the
model below keeps the base set: the pending stored response, else the responses
of the convolver the crossfader targets).  Asserted: np.array_equal on every
call's output, equal is_crossfading after every call, equal path() before every
call, and the update_pairs handle against matrix_xf_ref.SummedCrossfadeOracle
fed update(R') within common.REL_TOL."""
import numpy as np
import pytest
import torch

import oracle as oracle_module
from common import assert_close
from matrix_ref import make
from matrix_xf_ref import SummedCrossfadeOracle

pytestmark = pytest.mark.gpu


def pad(a, n):
    a = np.asarray(a, np.float32)
    out = np.zeros(a.shape[:-1] + (n,), np.float32)
    out[..., :a.shape[-1]] = a
    return out


class Pair:
    """The update_pairs handle, its update(R') twin, the oracle and the host
    model of the base set, driven in lockstep."""

    def __init__(self, amd, seed, I, O, B, L, mbs, fade, ncalls, mrl=None, fused=True, with_oracle=True):
        self.amd, self.I, self.O, self.B, self.L, self.mbs = amd, I, O, B, L, mbs
        self.mrl = L if mrl is None else mrl
        self.seed = seed
        self.h, self.x = make(seed, I, O, L, ncalls * mbs)
        new = lambda: amd.MatrixCrossfadeConvolver.new(amd.MatrixConvolver.init(self.h, B, L), self.mrl, mbs, fade)
        self.conv, self.twin = new(), new()
        if not fused:
            self.conv.set_fused(False)
            self.twin.set_fused(False)
        self.ref = SummedCrossfadeOracle(oracle_module, self.h, B, L, max_response_length=self.mrl,
                                         max_buffer_size=mbs, crossfade_samples=fade) if with_oracle else None
        self.cur, self.pending = self.h.copy(), None
        self.pos = 0
        self.got, self.want, self.paths = [], [], []
        assert self.conv.diff_pairs() == 0 and self.conv.last_patch() == (0, 0)

    def rows(self, k, n, length=None):
        """n fresh response rows"""
        length = self.L if length is None else length
        return make(self.seed + 100 + k, n, 1, length, 1)[0][0]

    # -- the model: what update(R) does to the base set ---------------------
    def _whole(self, R, others=True):
        fading = self.twin.is_crossfading()
        if others:
            self.twin.update(R)
            if self.ref is not None:
                self.ref.update(R)
        if fading:
            self.pending = pad(R, self.mrl)
        else:
            self.cur, self.pending = np.asarray(R, np.float32).copy(), None

    def whole(self, R):
        self.conv.update(R)
        self._whole(R)

    def r_prime(self, pairs, rows):
        base = self.pending if self.pending is not None else self.cur
        R = base.copy()
        for (o, i), row in zip(pairs, rows):
            R[o, i] = pad(row, R.shape[2])
        return R

    def partial(self, pairs, rows, how=None):
        """update_pairs on the handle (or how(conv)), update(R') on the twin and the oracle"""
        R = self.r_prime(pairs, rows)
        if how is None:
            self.conv.update_pairs(pairs, rows)
        else:
            how(self.conv)
        self._whole(R)
        return R

    def call(self, out_len=None, n=1):
        for _ in range(n):
            assert self.conv.path() == self.twin.path(), (len(self.got), self.conv.path(), self.twin.path())
            self.paths.append(self.conv.path())
            if self.pending is not None and not self.twin.is_crossfading():
                self.cur, self.pending = self.pending, None  # applied by this process()
            xs = self.x[:, self.pos:self.pos + self.mbs]
            self.pos += self.mbs
            y, yt = self.conv.process(xs, out_len), self.twin.process(xs, out_len)
            assert np.array_equal(y, yt), f"call {len(self.got)}: update_pairs differs from update(R')"
            assert self.conv.is_crossfading() == self.twin.is_crossfading()
            self.got.append(y)
            if self.ref is not None:
                self.want.append(self.ref.process(xs, out_len))
                assert self.conv.is_crossfading() == self.ref.is_crossfading()

    def through_fade(self):
        """calls until the fade under way has ended, and one more"""
        n = 0
        while self.twin.is_crossfading():
            self.call()
            n += 1
            assert n < 64
        self.call()

    def finish(self, what):
        got, want = np.concatenate(self.got, axis=1), np.concatenate(self.want, axis=1)
        assert np.isfinite(got).all()
        for o in range(self.O):
            assert_close(got[o], want[o], what=f"{what} output {o}")


def script_1(p):
    """the script of case 1; returns (last_patch, diff_pairs) after each of its three updates"""
    book = []
    p.call(n=3)
    p.partial([(0, 1), (1, 2)], p.rows(1, 2))
    book.append((p.conv.last_patch(), p.conv.diff_pairs()))
    assert p.conv.is_crossfading()
    p.through_fade()
    p.call(n=2)
    p.partial([(1, 0)], p.rows(2, 1))
    book.append((p.conv.last_patch(), p.conv.diff_pairs()))
    p.through_fade()
    rows = p.rows(3, p.O)
    p.partial([(o, 2) for o in range(p.O)], rows, how=lambda c: c.update_input(2, rows))
    book.append((p.conv.last_patch(), p.conv.diff_pairs()))
    p.call(n=4)
    return book


CASE_1 = [(32, 3 * 32 + 5, True), (2048, 3 * 2048 + 5, True), (64, 37 * 64 + 5, True), (64, 37 * 64 + 5, False),
          (128, 37 * 128 + 5, True)]


@pytest.mark.parametrize("B,L,fused", CASE_1, ids=[f"B{b}{'' if f else '-composition'}" for b, _, f in CASE_1])
def test_block_sizes(amd, B, L, fused):
    """1: the block transform (B 32: 256 threads, B 2048: 512), the wave form
    through LDS (B 64) and with the register stage 0 (B 128); S 38 there: several
    transform workgroups per pair with a ragged last one, an odd row length."""
    p = Pair(amd, 51, 3, 2, B, L, B, B + 7, 24, fused=fused)
    book = script_1(p)
    p.finish(f"B {B}")
    assert set(p.paths) == ({1, 2} if fused else {0}), p.paths
    # 2: the bookkeeping of this script
    assert [b[0] for b in book] == [(2, 0), (1, 2), (2, 1)], book
    assert [b[1] for b in book] == [2, 1, 2], book


def test_bookkeeping_after_a_whole_update(amd):
    """2: a whole update gives (6, 0) and |D| = 6; an update_pairs after it copies 6 minus the listed pairs."""
    p = Pair(amd, 52, 3, 2, 64, 200, 64, 71, 16)
    p.call(n=2)
    p.whole(make(152, 3, 2, 200, 1)[0])
    assert p.conv.last_patch() == (6, 0) and p.conv.diff_pairs() == 6
    p.through_fade()
    p.partial([(0, 0), (1, 1)], p.rows(1, 2))
    assert p.conv.last_patch() == (2, 4) and p.conv.diff_pairs() == 2
    p.through_fade()
    p.partial([(0, 0)], p.rows(2, 1))
    assert p.conv.last_patch() == (1, 1) and p.conv.diff_pairs() == 1
    p.through_fade()
    p.finish("bookkeeping")


def test_split_rows(amd):
    """3: S 128, P >= 2; a partial swap at block 100 and another after the
    unheard convolver has idled for more than S + 2 blocks."""
    p = Pair(amd, 53, 4, 2, 32, 4096, 32, 40, 250)
    assert amd.MatrixConvolver.init(p.h, 32, 4096).mac_parts >= 2
    p.call(n=100)
    p.partial([(0, 3), (1, 0), (1, 1)], p.rows(1, 3))
    p.call(n=136)
    p.partial([(0, 0), (1, 1)], p.rows(2, 2))
    p.call(n=12)
    p.finish("split")
    assert set(p.paths) == {1, 2}, p.paths


def pending_pair(amd, seed, mrl=None):
    # B 64, S 4, a fade of 3 calls after a hold of one
    p = Pair(amd, seed, 3, 2, 64, 200, 64, 150, 24, mrl=mrl)
    p.call(n=2)
    p.partial([(0, 0)], p.rows(0, 1))
    p.call()
    assert p.conv.is_crossfading()
    return p


def after_pending(p, what):
    """the pending response is applied by the first process() after the fade, and path() says so beforehand"""
    n = 0
    while p.twin.is_crossfading():
        p.call()
        n += 1
        assert n < 64
    assert p.conv.path() == p.twin.path() == 1, (p.conv.path(), p.twin.path())  # (the pending swap counted)
    p.call()
    assert p.conv.is_crossfading()
    p.through_fade()
    p.call(n=2)
    p.finish(what)


def test_pending_two_partials_share_a_pair(amd):
    p = pending_pair(amd, 54)
    p.partial([(0, 1), (1, 2)], p.rows(1, 2))
    assert p.conv.last_patch() == (1, 0)  # (nothing applied yet)
    p.call()
    p.partial([(1, 0), (1, 2)], p.rows(2, 2, 150))  # (1, 2) again, shorter: the later rows win
    after_pending(p, "two partials")
    assert p.conv.diff_pairs() == 3 and p.conv.last_patch() == (3, 1)


def test_pending_whole_then_partial(amd):
    p = pending_pair(amd, 55)
    p.whole(make(155, 3, 2, 200, 1)[0])
    p.partial([(0, 2), (1, 0)], p.rows(1, 2))
    after_pending(p, "whole then partial")
    assert p.conv.diff_pairs() == 6 and p.conv.last_patch() == (6, 0)


def test_pending_shared_whole_then_partial(amd):
    """a whole response given once for every pair (stride 0) is expanded before it is patched"""
    p = pending_pair(amd, 56)
    one = p.rows(7, 1)[0]
    R = np.broadcast_to(one, (p.O, p.I, p.L)).copy()
    rc = p.amd.lib().fftconv_matrix_crossfade_update(p.conv._h, one.ctypes.data_as(p.amd._fp), p.L, 0)
    assert rc == 0
    p._whole(R)
    p.partial([(1, 1)], p.rows(1, 1))
    after_pending(p, "shared whole then partial")


def test_pending_partial_then_whole(amd):
    p = pending_pair(amd, 57)
    p.partial([(0, 2), (1, 0)], p.rows(1, 2))
    p.whole(make(157, 3, 2, 200, 1)[0])
    after_pending(p, "partial then whole")
    assert p.conv.diff_pairs() == 6 and p.conv.last_patch() == (6, 0)


def test_partial_after_the_fade_with_a_whole_response_pending(amd):
    """no process() between the end of the fade and the call: update(R') swaps at once, R' from the stored response"""
    p = pending_pair(amd, 58)
    p.whole(make(158, 3, 2, 200, 1)[0])
    n = 0
    while p.twin.is_crossfading():
        p.call()
        n += 1
        assert n < 64
    p.partial([(0, 1)], p.rows(1, 1, 120))
    assert p.conv.is_crossfading() and p.twin.is_crossfading()
    p.through_fade()
    p.call(n=2)
    p.finish("partial on a pending whole")


def test_pending_unsupported_length(amd):
    """4: the stored length gives another active segment count than the base
    convolver's: FFTCONV_E_UNSUPPORTED, and the handle goes on as a twin that
    never received the call."""
    p = pending_pair(amd, 59, mrl=100)  # ceil(100 / 64) = 2, the convolvers have 4 active segments
    with pytest.raises(amd.DeviceError, match=r"status -3"):
        p.conv.update_pairs([(0, 1)], p.rows(1, 1, 100))
    p.through_fade()
    p.call(n=3)
    p.finish("unsupported")


def test_device_variant(amd):
    """5: rows from a torch tensor with stride > len, on a non-default stream, a shorter len that is zero-padded."""
    p = Pair(amd, 60, 3, 2, 64, 37 * 64 + 5, 64, 71, 20)
    p.call(n=3)
    pairs, n, stride = [(0, 2), (1, 0), (1, 1)], 1000, 1536
    rows = p.rows(1, 3, n)
    t = torch.zeros((3, stride), dtype=torch.float32, device="cuda")
    t[:, :n] = torch.from_numpy(rows).cuda()
    t[:, n:] = 7.0  # (never read)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    p.partial(pairs, rows, how=lambda c: c.update_pairs_device(pairs, t.data_ptr(), n, stride, s.cuda_stream))
    assert p.conv.last_patch() == (3, 0)
    p.call()
    # during the fade: the rows go to the stored response
    p.partial(pairs[:2], rows[:2], how=lambda c: c.update_pairs_device(pairs[:2], t.data_ptr(), n, stride, s.cuda_stream))
    p.through_fade()
    p.through_fade()
    p.finish("device rows")
    s.synchronize()


def test_errors_leave_the_handle_unchanged(amd):
    """6: a descending, a repeated and an out-of-range pair and len > len' raise; an empty list is update(R_base)."""
    p = Pair(amd, 61, 3, 2, 64, 200, 64, 71, 20)
    p.call(n=2)
    p.partial([(0, 1)], p.rows(1, 1, 150))
    p.through_fade()
    r = p.rows(2, 2, 150)
    for pairs in ([(1, 0), (0, 2)], [(0, 1), (0, 1)], [(0, 3), (1, 0)], [(2, 0), (1, 0)]):
        with pytest.raises(amd.ConvolutionPanic):
            p.conv.update_pairs(pairs, r)
    # the base set was applied at L = 200 (the handle's creation): the first
    # update_pairs kept that length, so 200 is accepted and 201 cannot exist
    # (max_response_length); after a whole update of 150 samples len' = 150
    p.whole(make(161, 3, 2, 150, 1)[0])
    p.through_fade()
    with pytest.raises(amd.ConvolutionPanic):
        p.conv.update_pairs([(0, 0)], p.rows(3, 1, 151))
    assert not p.conv.is_crossfading() and p.conv.diff_pairs() == 6
    p.call(n=2)
    p.partial([], np.zeros((0, 0), np.float32))
    assert p.conv.is_crossfading() and p.conv.last_patch() == (0, 6) and p.conv.diff_pairs() == 0
    p.through_fade()
    p.finish("errors")


def test_clone_with_a_partial_update_pending(amd):
    """7: a clone taken with a partial update pending and D non-empty continues bit-identically."""
    p = pending_pair(amd, 62)
    p.partial([(0, 1), (1, 2)], p.rows(1, 2))
    assert p.conv.diff_pairs() == 1
    c = p.conv.clone()
    assert c.diff_pairs() == 1 and c.last_patch() == p.conv.last_patch()
    pos = p.pos
    for _ in range(10):
        assert c.path() == p.conv.path()
        p.call()
        y = c.process(p.x[:, pos:pos + p.mbs])
        pos += p.mbs
        assert np.array_equal(y, p.got[-1])
        assert c.is_crossfading() == p.conv.is_crossfading()
        assert c.diff_pairs() == p.conv.diff_pairs() and c.last_patch() == p.conv.last_patch()
    assert p.conv.last_patch() == (2, 1)
    p.finish("clone")


@pytest.mark.parametrize("B,L", [(64, 1000), (4096, 2 * 4096 + 5)])
def test_plain_matrix(amd, B, L):
    """8: MatrixConvolver.update_pairs against update(R'), bitwise."""
    I, O = 3, 2
    h, x = make(63, I, O, L, 8 * B)
    a, b = amd.MatrixConvolver.init(h, B, L), amd.MatrixConvolver.init(h, B, L)
    pairs = [(0, 1), (1, 0), (1, 2)]
    rows = make(163, 3, 1, L - 3, 1)[0][0]
    R = h.copy()
    for (o, i), row in zip(pairs, rows):
        R[o, i] = pad(row, L)
    n = B + 17
    for k in range(3):
        assert np.array_equal(a.process(x[:, k * n:(k + 1) * n]), b.process(x[:, k * n:(k + 1) * n]))
    a.update_pairs(pairs, rows)
    b.update(R)
    assert a.state() == b.state()
    for k in range(3, 6):
        ya, yb = a.process(x[:, k * n:(k + 1) * n]), b.process(x[:, k * n:(k + 1) * n])
        assert np.array_equal(ya, yb), k
        assert np.isfinite(ya).all() and np.abs(ya).max() > 0
    for bad in ([(1, 0), (0, 1)], [(0, 1), (0, 1)], [(0, 3)]):
        with pytest.raises(amd.ConvolutionPanic):
            a.update_pairs(bad, rows[:len(bad)])
    with pytest.raises(amd.ConvolutionPanic):
        a.update_pairs([(0, 0)], np.zeros((1, L + 1), np.float32))
