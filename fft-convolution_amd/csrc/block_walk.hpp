// block_walk.hpp -- the host-side walk of FFTConvolver::process
// (src/fft_convolver.rs:222-294) that every matrix handle shares, and the block
// clock of the lookahead matrices.  No device code and no HIP:
// host.cpp uses it, and tests/host/matrix_walk_check.cpp drives it stand-alone
// under the sanitizers.
#pragma once
#include <stddef.h>

namespace fftconv {

// The reference's {current, active_seg_count, input_buffer_fill}: one triple
// for all instances of a matrix, advanced when a chunk is enqueued.
struct BlockWalk {
    size_t cur = 0, act = 0, fill = 0;

    // the samples of the next launch: never past the block in progress (:224-227)
    size_t chunk(size_t left, size_t B) const { return left < B - fill ? left : B - fill; }
    // the launch of k = chunk() samples is enqueued; true: it completed a block (:277-291)
    bool advance(size_t k, size_t B) {
        fill += k;
        if (fill != B) return false;
        fill = 0;
        cur = cur > 0 ? cur - 1 : act - 1;
        return true;
    }
};

// the lookahead period Q (kernels.hpp's kMatrixLaQ; host.cpp asserts they agree)
constexpr long long kLookaheadPeriod = 8;

// The block count that schedules the far-row anchors:
//   t   blocks started since init (the block the next fill == 0 chunk starts)
//   tv  windows anchored before block tv are invalid: init, reset, update and
//       every block that starts with current >= active (or with the windows
//       switched off) move it past every anchor made so far
struct LookaheadClock {
    long long t = 0, tv = 0;
    bool windows = true;

    // no anchor made so far counts from here on; the block in progress (fill >
    // 0) has made its anchors already, so they are past too
    void invalidate(size_t fill) { tv = fill ? t + 1 : t; }
    // ahead of a chunk's launch: a block that starts here makes no anchor
    void begin_chunk(size_t fill, size_t cur, size_t act) {
        if (fill == 0 && (!windows || cur >= act)) tv = t + 1;
    }
    // ahead of a chunk's launch of a convolver that idles (a crossfaded pair's
    // convolver the crossfader has Reached away from): the block
    // makes no anchor and reads no window, and whatever was anchored before the
    // idle spell never counts again -- t moves on, tv stays ahead of it
    void idle_chunk(size_t fill) {
        if (fill == 0) tv = t + 1;
    }
    void block_done() { ++t; }
    // reset() with `fill` samples buffered: the block in progress is dropped and
    // its number is not used again
    void reset(size_t fill) {
        if (fill) ++t;
        invalidate(0);
    }
    // every window a block reads was anchored at or after tv (matrix_la_steady)
    bool steady() const { return t - (kLookaheadPeriod - 1) >= tv; }
};

}  // namespace fftconv
