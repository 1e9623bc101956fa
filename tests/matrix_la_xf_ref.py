"""Scenarios and host model of the MatrixLookaheadCrossfadeConvolver tests
(DESIGN 4t): the scripts tests/test_gpu_matrix_la_xf.py runs on the device, and
a CPU model of what the host does with them -- the crossfader's state machine,
the pending response, the block walk and the two LookaheadClocks with the swap
and idle rules -- over matrix_la_ref.role / steady.  The model keeps, per
convolver and output, which block anchored every window row; `blocks` is what
tests/test_matrix_la_xf_ref.py enumerates."""
import functools

from matrix_la_ref import MAIN, Q, SHAPE_32, SHAPE_256, role, steady
from matrix_xf_ref import calls

FADE = 24 * 64  # the main scripts' fade: both convolvers live for more than 2 * Q blocks of 64


def alt(n, a=100, b=37):
    return [("call", a if k % 2 == 0 else b) for k in range(n)]


# name -> (seed, (I, O, B, L), max_buffer_size, crossfade_samples, script builder, max_response_length or None)
# mk(k) / mk(k, n): response set k of n samples (default L)
def _scenarios():
    I, O, B, L = MAIN
    sc = {
        # hold, fade and reached across one-block calls, then back towards A
        "fade": (61, MAIN, 64, FADE, lambda mk: calls(20, 64) + [("update", mk(1))] + calls(40, 64) +
                 [("update", mk(2))] + calls(30, 64), None),
        # swaps land mid-block, output_len 100 and 37, the state advances by 100
        "ragged": (62, MAIN, 100, FADE, lambda mk: alt(9) + [("update", mk(1))] + alt(30) + [("update", mk(2))] +
                   alt(30), None),
        # two updates during one fade, one too long for the stored response (1500): the swap applied after
        # the fade ends the in-step state
        "pending": (63, MAIN, 64, 96, lambda mk: calls(5, 64) + [("update", mk(1))] + calls(1, 64) +
                    [("update", mk(2, 1200)), ("update_panics", mk(3, 1600)), ("update", mk(4, 1500))] +
                    calls(12, 64), 1500),
        # the first target is the only live convolver for 50 > S + 2 = 42 blocks before the second swap
        "long-idle": (64, MAIN, 64, 5 * 64, lambda mk: calls(10, 64) + [("update", mk(1))] + calls(57, 64) +
                      [("update", mk(2))] + calls(16, 64), None),
        # an update to another ceil(len / B), and an empty response: composition from then on
        "out-of-step": (65, MAIN, 64, 96, lambda mk: calls(4, 64) + [("update", mk(1, 1000))] + calls(6, 64) +
                        [("update", mk(2, 1000))] + calls(6, 64) + [("update", mk(3))] + calls(6, 64), None),
        "empty": (66, MAIN, 64, 96, lambda mk: calls(4, 64) + [("update", mk(1, 0))] + calls(6, 64) +
                  [("update", mk(2))] + calls(6, 64) + [("update", mk(3))] + calls(6, 64), None),
    }
    # block sizes: a swap after 11 blocks, a fade of 9 B + 7 samples, calls of B - 24 and 24 at the end
    for name, (i, o, b, l) in (("B32", SHAPE_32), ("B128", (2, 3, 128, 128 * 12)), ("B256", SHAPE_256),
                               ("B512", (2, 3, 512, 512 * 12))):
        sc[name] = (67, (i, o, b, l), b, 9 * b + 7, lambda mk, b=b: calls(11, b) + [("update", mk(1))] + calls(14, b) +
                    [("call", b - 24), ("call", 24)], None)
    # few segments: 1, 2, 8 (no far rows) and 9 (one far row per input)
    for segs in (1, 2, 8, 9):
        sc[f"S{segs}"] = (68, (3, 10, 64, segs * 64), 64, 3 * 64 + 11, lambda mk: calls(10, 64) + [("update", mk(1))] +
                          calls(12, 64) + [("call", 30)], None)
    return sc


SCENARIOS = _scenarios()
MODELLED = ("fade", "ragged", "pending", "long-idle", "B32", "B128", "B256", "B512", "S9")


class Crossfader:
    """The crossfader's state machine (src/crossfade_convolver.rs:192-279) without the gains."""

    def __init__(self, fading, hold):
        self.fading, self.hold, self.counter, self.approaching, self.target = fading, hold, 0, False, 0

    def fade_into(self, t):
        if self.target == t:
            return
        if not self.approaching:
            self.counter, self.approaching, self.target = -self.hold, True, t
        elif self.counter >= 0:
            self.counter, self.target = self.fading - self.counter, t
        else:
            self.approaching, self.target = False, t

    def advance(self, n):
        for _ in range(n):
            if not self.approaching:
                return
            self.counter += 1
            if self.counter == self.fading:
                self.approaching = False


class Clock:
    """block_walk.hpp's LookaheadClock"""

    def __init__(self):
        self.t = self.tv = 0
        self.windows = True

    def invalidate(self, fill):
        self.tv = self.t + 1 if fill else self.t

    def begin_chunk(self, fill, cur, act):
        if fill == 0 and (not self.windows or cur >= act):
            self.tv = self.t + 1

    def idle_chunk(self, fill):
        if fill == 0:
            self.tv = self.t + 1


class Conv:
    def __init__(self, S):
        self.cur, self.act, self.fill, self.clk = 0, S, 0, Clock()
        self.rows = {}    # (output, window row) -> (block that wrote it, 'anchor' or 'full', epoch)
        self.epoch = 0    # bumped by every swap into this convolver and by every block it idles through


class PairModel:
    """The host side of one handle.  run() returns one record per (block,
    convolver): dict(t, c, live, tv, roles) with roles[o] in 'anchor', 'full',
    None -- and asserts, for every output served from a window, that the row was
    anchored by that output's latest anchor, at or after tv, in the convolver's
    current epoch."""

    def __init__(self, shape, mbs, fade, mrl, fused=True):
        self.I, self.O, self.B, self.L = shape
        self.S = -(-self.L // self.B)
        self.mbs, self.fused = mbs, fused
        self.stored_len = self.L if mrl is None else mrl
        self.xf = Crossfader(fade, min(mbs, self.stored_len))
        self.cv = [Conv(self.S), Conv(self.S)]
        self.pending = None
        self.in_step = True
        self.blocks, self.paths = [], []

    def _swap(self, n):
        to = 1 - self.xf.target
        c = self.cv[to]
        if n > self.L:
            raise ValueError("New impulse response is longer than initialized length")
        c.act = -(-n // self.B)
        c.clk.invalidate(c.fill)
        c.epoch += 1
        self.xf.fade_into(to)

    def update(self, n):
        if not self.xf.approaching:
            self._swap(n)
            self.pending = None
        else:
            if n > self.stored_len:
                raise ValueError("assertion failed: response_len <= self.stored_response.len()")
            self.pending = self.stored_len

    def _agree(self):
        a, b = self.cv
        return (a.cur, a.act, a.fill) == (b.cur, b.act, b.fill) and a.act > 0 and a.clk.t == b.clk.t

    def _chunk(self, c, conv, live, k):
        if live:
            conv.clk.begin_chunk(conv.fill, conv.cur, conv.act)
        else:
            conv.clk.idle_chunk(conv.fill)
            if conv.fill == 0:
                conv.epoch += 1
        if conv.fill == 0:
            t, tv = conv.clk.t, conv.clk.tv
            roles = [None] * self.O
            if live and conv.act > Q:
                for o in range(self.O):
                    r = roles[o] = role(t, tv, o)
                    if r == "anchor":
                        assert conv.cur < conv.act
                        for j in range(Q):
                            conv.rows[o, (t + j) % Q] = (t, "anchor", conv.epoch)
                    elif r == "full":
                        conv.rows[o, t % Q] = (t, "full", conv.epoch)
                    else:
                        at, how, epoch = conv.rows[o, t % Q]
                        assert how == "anchor" and at == t - (t - o) % Q and at >= tv and epoch == conv.epoch, \
                            (c, o, t, tv, at, how, epoch, conv.epoch)
                    if r != "full" and steady(t, tv):
                        assert r == ("anchor" if o % Q == t % Q else None)
            self.blocks.append(dict(t=t, c=c, live=live, tv=tv, roles=roles, far=conv.act > Q))
        conv.fill += k
        if conv.fill == self.B:
            conv.fill = 0
            conv.cur = conv.cur - 1 if conv.cur > 0 else conv.act - 1
            conv.clk.t += 1

    def call(self, out_len):
        if not self.xf.approaching and self.pending is not None:
            self._swap(self.pending)
            self.pending = None
        self.in_step = self.in_step and self._agree()
        path = 0 if not (self.fused and self.in_step) else (1 if self.xf.approaching else 2)
        self.paths.append(path)
        for c, conv in enumerate(self.cv):
            live = path == 0 or self.xf.approaching or c == self.xf.target
            if path == 0 and conv.act == 0:
                continue
            done = 0
            while done < self.mbs:
                k = min(self.mbs - done, self.B - conv.fill)
                self._chunk(c, conv, live, k)
                done += k
        self.xf.advance(out_len)

    def run(self, script):
        """script entries: ('update', response length), ('update_panics', length), ('call', out_len)"""
        for kind, arg in script:
            if kind == "update":
                self.update(arg)
            elif kind == "update_panics":
                try:
                    self.update(arg)
                except ValueError:
                    continue
                raise AssertionError("update did not fail")
            else:
                self.call(arg)
        return self.blocks


@functools.lru_cache(maxsize=None)
def lengths_script(name):
    """the scenario's script with every response replaced by its length"""
    seed, shape, mbs, fade, build, mrl = SCENARIOS[name]
    L = shape[3]
    return tuple(build(lambda k, n=L: n))


def model(name, fused=True):
    seed, shape, mbs, fade, build, mrl = SCENARIOS[name]
    m = PairModel(shape, mbs, fade, mrl, fused)
    m.run(lengths_script(name))
    return m
