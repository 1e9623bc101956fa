// matrix_walk_check.cpp -- the block walk and the lookahead clock that every
// matrix handle's process_device shares (csrc/block_walk.hpp), driven
// stand-alone, without a GPU: ragged calls against the reference's loop
// (src/fft_convolver.rs:222-294) and the {t, tv} rules of DESIGN §4n as
// tests/matrix_la_ref.py states them.  Built with the sanitizers and run once:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I fft-convolution_amd/csrc tests/host/matrix_walk_check.cpp -o matrix_walk_check && ./matrix_walk_check
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

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

constexpr size_t B = 32;
constexpr long long Q = kLookaheadPeriod;

// one process_device call of n samples, as host.cpp walks it; returns the blocks completed
size_t call(BlockWalk &w, size_t n, LookaheadClock *clk = nullptr) {
    size_t sum = 0, blocks = 0;
    for (size_t done = 0; done < n;) {
        if (clk) clk->begin_chunk(w.fill, w.cur, w.act);
        const size_t fill0 = w.fill, cur0 = w.cur;
        const size_t k = w.chunk(n - done, B);
        CHECK(k > 0 && k <= n - done);
        CHECK(fill0 + k <= B);  // no chunk crosses a block boundary
        const bool completed = w.advance(k, B);
        CHECK(completed == (fill0 + k == B));
        if (completed) {
            CHECK(w.fill == 0);
            CHECK(w.cur == (cur0 ? cur0 - 1 : w.act - 1));
            ++blocks;
            if (clk) clk->block_done();
        } else {
            CHECK(w.fill == fill0 + k);
            CHECK(w.cur == cur0);
        }
        sum += k;
        done += k;
    }
    CHECK(sum == n);
    return blocks;
}

// (a) ragged calls
void ragged_calls() {
    const size_t lens[] = {0, 1, B - 1, B, B + 1, 3 * B + 5}, fills[] = {0, 1, B - 1}, acts[] = {1, 2, 5};
    for (size_t act : acts)
        for (size_t fill0 : fills)
            for (size_t n : lens)
                for (size_t cur0 = 0; cur0 < act; ++cur0) {
                    BlockWalk w;
                    w.act = act;
                    w.cur = cur0;
                    w.fill = fill0;
                    const size_t blocks = call(w, n);
                    CHECK(blocks == (fill0 + n) / B);
                    CHECK(w.fill == (fill0 + n) % B);
                    size_t cur = cur0;  // `cur ? cur - 1 : act - 1`, once per completed block
                    for (size_t b = 0; b < blocks; ++b) cur = cur ? cur - 1 : act - 1;
                    CHECK(w.cur == cur);
                    CHECK(w.act == act);
                }
}

bool steady(long long t, long long tv) { return t - (Q - 1) >= tv; }  // tests/matrix_la_ref.py

// blocks walked from an invalidation until a block first starts steady
long long blocks_until_steady(BlockWalk &w, LookaheadClock &c) {
    for (long long blocks = 0; blocks < 4 * Q; ++blocks) {
        c.begin_chunk(w.fill, w.cur, w.act);  // (what the next block's first chunk sees)
        if (steady(c.t, c.tv)) {
            CHECK(c.steady());
            return blocks;
        }
        CHECK(!c.steady());
        CHECK(call(w, B, &c) == 1);
    }
    return -1;
}

// (b) the clock
void clock_rules() {
    LookaheadClock c;
    CHECK(c.t == 0 && c.tv == 0 && c.windows);

    c.t = 5;
    c.invalidate(0);
    CHECK(c.tv == 5);
    c.invalidate(7);  // a block in progress has made its anchors already
    CHECK(c.tv == 6);

    c = LookaheadClock();
    c.t = 3;
    c.reset(0);  // at a block boundary: the number is the next block's
    CHECK(c.t == 3 && c.tv == 3);
    c.reset(9);  // mid-block: t is bumped first, then everything before it is invalid
    CHECK(c.t == 4 && c.tv == 4);

    // a block that begins with cur >= act, or with the windows off, makes no anchor
    c = LookaheadClock();
    c.t = 10;
    c.tv = 2;
    c.begin_chunk(0, 1, 3);
    CHECK(c.tv == 2);
    c.begin_chunk(4, 3, 3);  // (not the start of a block)
    CHECK(c.tv == 2);
    c.begin_chunk(0, 3, 3);
    CHECK(c.tv == 11);
    c.tv = 2;
    c.windows = false;
    c.begin_chunk(0, 0, 3);
    CHECK(c.tv == 11);
    c.block_done();
    CHECK(c.t == 11);

    // steady first holds exactly Q - 1 blocks after the last invalidation
    const size_t act = 3 * (size_t)Q;
    for (size_t fill0 : {(size_t)0, (size_t)5}) {
        BlockWalk w;
        w.act = act;
        c = LookaheadClock();
        CHECK(call(w, 2 * Q * B + fill0, &c) == 2 * (size_t)Q);  // well into the steady state
        CHECK(w.fill == fill0);
        c.invalidate(w.fill);  // an update
        if (fill0) CHECK(call(w, B - fill0, &c) == 1);  // the block in progress ends
        CHECK(c.t == c.tv);
        CHECK(blocks_until_steady(w, c) == Q - 1);

        call(w, fill0, &c);
        c.reset(w.fill);  // a reset
        w.cur = w.fill = 0;
        CHECK(c.t == c.tv);
        CHECK(blocks_until_steady(w, c) == Q - 1);
    }
    // from init, with cur >= act for the first blocks (a short response after a
    // long one): those blocks keep moving tv, so steady comes Q - 1 blocks after the last of them
    {
        BlockWalk w;
        w.act = 2;
        w.cur = 4;  // three blocks start with cur >= act
        c = LookaheadClock();
        CHECK(call(w, 3 * B, &c) == 3);
        CHECK(w.cur == 1 && c.tv == 3 && c.t == 3);
        CHECK(blocks_until_steady(w, c) == Q - 1);
    }
}

}  // namespace

int main() {
    ragged_calls();
    clock_rules();
    std::puts("matrix_walk_check: ok");
    return 0;
}
