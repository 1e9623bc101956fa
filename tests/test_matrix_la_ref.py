"""The scheme of the MatrixLookaheadConvolver, checked on the CPU through
matrix_la_ref (a model of the schedule and of both walks, not the product):
the index argument that lets an anchor run in launch A with the kernel boundary
as the only ordering, that every (output, block) is served exactly once, that a
window's accumulator and a full sum list the same rows in the same order, that
near and far rows together are every row once, and that a float32 replay which
really serves blocks from windows agrees with the summed oracle."""
import numpy as np
import pytest

import matrix_ref
from common import REL_TOL, max_rel_err
from matrix_la_ref import (MAIN, SHAPE_32, SHAPE_256, LaModel, far_outputs, far_parts, far_rows, far_walk, near_parts,
                           near_rows, next_cur, role, steady)
from matrix_paths import geo
from matrix_ref import SummedOracle


@pytest.mark.parametrize("q", [4, 8])
def test_anchor_reads_no_row_written_before_its_use(q):
    """For every 2 <= active <= 40, current < active: the far sum of block a + j
    (j < q) computed at block a reads ring index (cur - j + s) % active, q <= s <
    active; blocks a .. a + j - 1 write the indices their own `current` names.
    The two sets are disjoint, and block a's own row is not read either."""
    for act in range(2, 41):
        for cur in range(act):
            written, c = [], cur
            for j in range(q):
                # (written = rows of blocks a .. a + j - 1; plus block a's own for the launch itself)
                reads = {(cur - j + s) % act for s in range(q, act)}
                assert not reads & set(written), (act, cur, j)
                assert cur not in reads, (act, cur, j)
                written.append(c)
                c = next_cur(c, act)
            # the rows a window reads are the rows the full sum of that block reads
            c = cur
            for j in range(q):
                assert {(c + s) % act for s in range(q, act)} == {(cur - j + s) % act for s in range(q, act)}
                c = next_cur(c, act)


@pytest.mark.parametrize("q", [4, 8])
@pytest.mark.parametrize("O", [1, 3, 10, 19])
@pytest.mark.parametrize("t0", [0, 5, 13])
def test_every_output_block_is_served_exactly_once(q, O, t0):
    """3 q blocks after an invalidation at block t0: each (output, block) is
    served once, by a full sum or by a window row that an anchor of the same
    output wrote for exactly that block and nobody overwrote since; the grid's
    list of far outputs holds every output with work; at most q - 1 full blocks
    per output."""
    tv = t0
    slot = {}  # (o, t % q) -> block the row was computed for
    fulls = [0] * O
    for t in range(t0, t0 + 3 * q):
        listed = far_outputs(t, tv, O, q)
        for o in range(O):
            r = role(t, tv, o, q)
            if r is not None:
                assert o in listed, (t, o)
            if r == "anchor":
                assert (t - o) % q == 0
                for j in range(q):
                    # (the previous window's rows t .. t + q - 1 - q are consumed: none is still ahead)
                    assert slot.get((o, (t + j) % q), -1) < t
                    slot[(o, (t + j) % q)] = t + j
            elif r == "full":
                slot[(o, t % q)] = t
                fulls[o] += 1
            assert slot[(o, t % q)] == t, (t, o, r)  # launch B's row is this block's
        if steady(t, tv, q):
            assert all(role(t, tv, o, q) == "anchor" for o in listed)
    assert max(fulls) <= q - 1
    # anchors per block are even: ceil or floor of O / q
    for t in range(t0 + q, t0 + 3 * q):
        n = sum(role(t, tv, o, q) == "anchor" for o in range(O))
        assert n in (O // q, -(-O // q))


def test_invalid_while_current_exceeds_active():
    """tv = t + 1 (what the host passes while current >= active or with the
    windows off): every output sums in full, none anchors."""
    for t in range(40):
        assert all(role(t, t + 1, o) == "full" for o in range(12))
        assert not steady(t, t + 1)


@pytest.mark.parametrize("I,B,act", [(3, 64, 40), (2, 256, 20), (2, 32, 12), (2, 512, 12), (5, 128, 9), (32, 256, 188)])
@pytest.mark.parametrize("q", [4, 8])
def test_window_and_full_walk_agree(I, B, act, q):
    """Accumulator j of the W = q walk at block a lists the (row, ring index)
    sequence of the W = 1 walk of block a + j, for every part and group."""
    G = geo(B).G
    for cur in sorted({0, 1, act // 2, act - 1}):
        for p in range(far_parts(I, act, q)):
            for g in range(G):
                win = far_walk(B, I, act, cur, p, g, q, q)
                c = cur
                for j in range(q):
                    assert win[j] == far_walk(B, I, act, c, p, g, 1, q)[0], (cur, p, g, j)
                    c = next_cur(c, act)


@pytest.mark.parametrize("I,B,act", [(3, 64, 40), (2, 256, 20), (2, 32, 12), (2, 512, 12), (2, 64, 5), (1, 64, 1),
                                     (5, 128, 9), (32, 256, 188), (7, 32, 700)])
@pytest.mark.parametrize("q", [4, 8])
def test_near_and_far_visit_every_row_once(I, B, act, q):
    G = geo(B).G
    seen = {}
    for p in range(near_parts(I, act, q)):
        for g in range(G):
            for i, s in near_rows(B, I, act, p, g, q):
                assert 1 <= s < min(q, act)
                seen[(i, s)] = seen.get((i, s), 0) + 1
    for p in range(far_parts(I, act, q)):
        for g in range(G):
            rows = far_rows(B, I, act, p, g, q)
            assert rows == sorted(rows)
            for i, s in rows:
                assert q <= s < act
                seen[(i, s)] = seen.get((i, s), 0) + 1
    assert seen == {(i, s): 1 for i in range(I) for s in range(1, act)}


def test_gpu_shapes_run_what_they_are_there_for():
    I, O, B, L = MAIN
    act = L // B
    assert I * (act - 8) == 96 and far_parts(I, act) == 2 and O > 8
    # (a far part that crosses a pair boundary: its rows name two inputs)
    assert any(len({i for g in range(geo(B).G) for i, _ in far_rows(B, I, act, p, g)}) > 1 for p in range(2))
    I, O, B, L = SHAPE_256
    assert geo(B).G == 2 and far_parts(I, L // B) == 1
    assert geo(512).G == 1
    I, O, B, L = SHAPE_32
    assert geo(B).G == 16 and far_parts(I, L // B) == 1


def test_replay_against_the_summed_oracle(oracle_mod):
    """The float32 replay on the main shape, 30 blocks with an update after
    block 13: blocks really come from windows, and the result stays within
    REL_TOL of the summed oracle; the replay without windows too."""
    I, O, B, L = MAIN
    O = 3
    h, x = matrix_ref.make(41, I, O, L, 30 * B)
    h2, _ = matrix_ref.make(42, I, O, L - 70, 1)
    ref = SummedOracle(oracle_mod, h, B, L)
    win, full = LaModel(h, B, L), LaModel(h, B, L, windows=False)
    for k in range(30):
        if k == 13:
            for m in (ref, win, full):
                m.update(h2)
        blk = x[:, k * B:(k + 1) * B]
        r = ref.process(blk)
        for m, what in ((win, "windows"), (full, "full sums")):
            e = max_rel_err(m.process_block(blk), r)
            assert e <= REL_TOL, f"{what}, block {k}: {e:.3e}"
        assert (win.cur, win.act) == ref.state()[:2]
    assert win.anchored > 0 and win.from_window > 4 * win.anchored and win.full > 0
    assert full.anchored == full.from_window == 0
