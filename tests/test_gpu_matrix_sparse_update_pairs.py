"""SparseMatrixConvolver.update_pairs (include/fftconv.h): update(R') at the
length of the last init / update, R' = the responses the handle holds with the
listed pairs replaced, bit for bit in outputs and state, against a twin that
gets the whole R'.  Every listed pair must belong to the pattern."""
import numpy as np
import pytest
import torch

from matrix_sp_ref import PATTERN_1, make

pytestmark = pytest.mark.gpu


def pad(a, n):
    a = np.asarray(a, np.float32)
    out = np.zeros(a.shape[:-1] + (n,), np.float32)
    out[..., :a.shape[-1]] = a
    return out


@pytest.mark.parametrize("B,L", [(128, 2045), (2048, 3 * 2048 + 5)])
def test_update_pairs_equals_update(amd, B, L):
    I, O = 5, 4
    h, x = make(63, PATTERN_1, I, L, 12 * (B + 17))
    a, b = (amd.SparseMatrixConvolver.init(PATTERN_1, h, I, O, B, L) for _ in range(2))
    n = B + 17
    pos = 0

    def both(k):
        nonlocal pos
        for _ in range(k):
            ya, yb = a.process(x[:, pos:pos + n]), b.process(x[:, pos:pos + n])
            pos += n
            assert np.array_equal(ya, yb), pos
            assert np.isfinite(ya).all() and np.abs(ya[[0, 1, 3]]).max() > 0 and not ya[2].any()

    both(3)
    # rows shorter than the held set's length: zero-padded to it
    pairs = [(0, 1), (1, 2), (3, 4)]
    rows = make(163, pairs, 1, L - 3, 1)[0]
    R = h.copy()
    for p, row in zip(pairs, rows):
        R[PATTERN_1.index(p)] = pad(row, L)
    a.update_pairs(pairs, rows)
    b.update(R)
    assert a.state() == b.state()
    both(3)
    # after a whole update to a shorter length the base set has that length (another plan)
    L2 = L // 3
    R = make(164, PATTERN_1, I, L2, 1)[0]
    a.update(R)
    b.update(R)
    both(1)
    with pytest.raises(amd.ConvolutionPanic):
        a.update_pairs([(0, 0)], np.zeros((1, L2 + 1), np.float32))
    # the device variant: stride > len, on a non-default stream
    pairs = [(0, 0), (0, 4), (3, 0)]
    rows = make(165, pairs, 1, L2 - 9, 1)[0]
    stride = L2 + 11
    t = torch.full((3, stride), 7.0, dtype=torch.float32, device="cuda")
    t[:, :L2 - 9] = torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    a.update_pairs_device(pairs, t.data_ptr(), L2 - 9, stride, s.cuda_stream)
    R = R.copy()
    for p, row in zip(pairs, rows):
        R[PATTERN_1.index(p)] = pad(row, L2)
    b.update(R)
    assert a.state() == b.state()
    both(3)
    # an empty list is update(R)
    a.update_pairs([], np.zeros((0, 0), np.float32))
    b.update(R)
    both(2)
    s.synchronize()


def test_pairs_must_belong_to_the_pattern(amd):
    I, O, B, L = 5, 4, 128, 500
    h, x = make(64, PATTERN_1, I, L, 4 * B)
    a, b = (amd.SparseMatrixConvolver.init(PATTERN_1, h, I, O, B, L) for _ in range(2))
    assert np.array_equal(a.process(x[:, :B]), b.process(x[:, :B]))
    rows = make(166, [(0, 0)] * 2, 1, L, 1)[0]
    for bad in ([(1, 0)], [(2, 3)], [(0, 1), (3, 1)]):
        with pytest.raises(amd.ConvolutionPanic, match="is not in the pattern"):
            a.update_pairs(bad, rows[:len(bad)])
    for bad in ([(1, 2), (0, 1)], [(0, 1), (0, 1)], [(0, 5)], [(4, 0)]):
        with pytest.raises(amd.ConvolutionPanic):
            a.update_pairs(bad, rows[:len(bad)])
    assert a.state() == b.state()
    for k in range(1, 4):  # the handle is unchanged: no overlap was zeroed
        assert np.array_equal(a.process(x[:, k * B:(k + 1) * B]), b.process(x[:, k * B:(k + 1) * B]))
