// la_xf_clock_check.cpp -- the window rules of a crossfaded pair of lookahead
// matrices on the real LookaheadClock (csrc/block_walk.hpp), driven
// stand-alone, without a GPU: one convolver of the pair goes through live, idle
// and swapped-in spells of every length and phase, in whole blocks and in ragged
// chunks, and every window row a block reads must have been anchored by that
// output's latest anchor, at or after tv, and not across an idle spell or a
// swap.  Built with the sanitizers and run once:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I fft-convolution_amd/csrc tests/host/la_xf_clock_check.cpp -o la_xf_clock_check && ./la_xf_clock_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "block_walk.hpp"

using namespace fftconv;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

namespace {

constexpr size_t B = 64;
constexpr long long Q = kLookaheadPeriod;
constexpr int O = 10;  // two outputs share the anchor classes 0 and 1

// kernels.hpp's matrix_la_role: 1 anchor, 2 full sum, 0 served by a window
int role(long long t, long long tv, int o) {
    const int ph = (int)(((t - o) % Q + Q) % Q);
    if (t - ph < tv) return 2;
    return ph == 0 ? 1 : 0;
}

struct Row {
    long long at = -1;  // the block that wrote the row
    bool anchor = false;
    long epoch = -1;
};

// one convolver of the pair
struct Conv {
    BlockWalk w;
    LookaheadClock clk;
    std::vector<Row> rows = std::vector<Row>((size_t)O * Q);
    long epoch = 0;  // bumped by every swap and by every block idled through
    long served = 0, anchored = 0, full = 0, idled = 0;

    // a chunk of k samples, as MatrixLookaheadCore::xf_chunk_begin and the launch see it
    void chunk(size_t k, bool live) {
        if (live)
            clk.begin_chunk(w.fill, w.cur, w.act);
        else
            clk.idle_chunk(w.fill);
        if (w.fill == 0) {
            const long long t = clk.t, tv = clk.tv;
            if (!live) {
                ++epoch;
                ++idled;
                CHECK(tv == t + 1);  // every output would sum in full: nothing anchored so far counts
                for (int o = 0; o < O; ++o) CHECK(role(t, tv, o) == 2);
            } else {
                for (int o = 0; o < O; ++o) {
                    const int r = role(t, tv, o);
                    if (r == 1) {
                        CHECK(w.cur < w.act);
                        for (long long j = 0; j < Q; ++j) rows[(size_t)o * Q + (size_t)((t + j) % Q)] = {t, true, epoch};
                        ++anchored;
                    } else if (r == 2) {
                        rows[(size_t)o * Q + (size_t)(t % Q)] = {t, false, epoch};
                        ++full;
                    } else {
                        const Row &x = rows[(size_t)o * Q + (size_t)(t % Q)];
                        const long long ph = ((t - o) % Q + Q) % Q;
                        CHECK(x.anchor && x.at == t - ph && x.at >= tv && x.epoch == epoch);
                        ++served;
                    }
                }
            }
        }
        if (w.advance(k, B)) clk.block_done();
    }
    void run(size_t samples, size_t call, bool live) {
        for (size_t done = 0; done < samples;) {
            const size_t n = samples - done < call ? samples - done : call;
            for (size_t d = 0; d < n;) {
                const size_t k = w.chunk(n - d, B);
                chunk(k, live);
                d += k;
            }
            done += n;
        }
    }
    void swap() {  // update(): the plan is the same, the windows are not
        clk.invalidate(w.fill);
        ++epoch;
    }
};

void spells() {
    const size_t S = 40;
    for (size_t call : {(size_t)64, (size_t)100, (size_t)37})
        for (size_t live0 : {(size_t)0, (size_t)3, (size_t)20})
            for (size_t idle = 0; idle <= 2 * (size_t)Q + 1; ++idle)
                for (size_t odd : {(size_t)0, (size_t)17}) {
                    Conv c;
                    c.w.act = S;
                    c.run(live0 * B + odd, call, true);
                    c.run(idle * B, call, false);   // the crossfader has Reached the other convolver
                    const long long t0 = c.clk.t;
                    c.swap();                          // ... and comes back: a swap into this one
                    CHECK(c.clk.tv == (c.w.fill ? t0 + 1 : t0));
                    const long served0 = c.served;
                    c.run(B - c.w.fill, call, true);   // the block of the swap, or the first one after it
                    CHECK(c.served == served0);        // ... reads no window
                    c.run(4 * (size_t)Q * B, call, true);
                    CHECK(c.clk.steady() && c.served > served0);
                    // an idle spell with no swap after it (set_fused(0), a clone): live again, nothing old is read
                    c.run(5 * B, call, false);
                    CHECK(c.clk.tv >= c.clk.t);
                    c.run(2 * (size_t)Q * B, call, true);
                    CHECK(c.anchored > 0 && c.full > 0);
                }
}

// the idle rule itself
void idle_rule() {
    LookaheadClock c;
    c.t = 12;
    c.tv = 3;
    c.idle_chunk(5);  // mid-block: the block in progress made its anchors while live
    CHECK(c.tv == 3);
    c.idle_chunk(0);
    CHECK(c.tv == 13 && !c.steady());
    c.block_done();
    CHECK(c.t == 13 && c.tv == 13);
    c.idle_chunk(0);
    CHECK(c.tv == 14);
    c.invalidate(9);  // a swap mid-block, right after the idle spell
    CHECK(c.tv == 14);
}

}  // namespace

int main() {
    idle_rule();
    spells();
    std::puts("la_xf_clock_check: ok");
    return 0;
}
