// pair_book_check.cpp -- the host-side bookkeeping of update_pairs
// (csrc/pair_book.hpp: list validation, the diff set D, the pending list) driven
// stand-alone, without a GPU, through the scripts of cases 2 and 4 of
// tests/test_gpu_matrix_update_pairs.py.  Built with the sanitizers and run
// once:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I fft-convolution_amd/csrc tests/host/pair_book_check.cpp -o pair_book_check && ./pair_book_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pair_book.hpp"

using namespace fftconv;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

namespace {

constexpr size_t I = 3, O = 2, N = I * O;

struct List {
    std::vector<uint32_t> o, i;
    List(std::initializer_list<std::pair<uint32_t, uint32_t>> p) {
        for (auto &e : p) {
            o.push_back(e.first);
            i.push_back(e.second);
        }
    }
};

// validate into idx (exactly N entries: an overrun is the sanitizer's to find)
size_t valid(const List &l, std::vector<uint32_t> &idx) {
    CHECK(l.o.size() <= N);
    CHECK(check_pairs(l.o.size(), l.o.data(), l.i.data(), I, O, idx.data()) == PAIRS_OK);
    return l.o.size();
}

// what MatrixCrossfadeCore does with the book: a direct partial swap
void swap_partial(PairBook &b, const List &l, std::vector<uint32_t> &idx, std::vector<uint32_t> &cp, size_t tr,
                  size_t copied, size_t nd) {
    const size_t n = valid(l, idx);
    const size_t ncp = b.partial_applied(idx.data(), n, cp.data());
    CHECK(n == tr && ncp == copied && b.nd == nd);
    CHECK(b.last[0] == tr && b.last[1] == copied);
    for (size_t k = 1; k < ncp; ++k) CHECK(cp[k - 1] < cp[k]);
    for (size_t k = 0; k < ncp; ++k)
        for (size_t m = 0; m < n; ++m) CHECK(cp[k] != idx[m]);
}

// the pending partial response is applied
void apply_pending(PairBook &b, std::vector<uint32_t> &idx, std::vector<uint32_t> &cp, size_t tr, size_t copied) {
    CHECK(b.partial);
    const size_t n = b.pending_list(idx.data());
    CHECK(n == b.np && n == tr);
    for (size_t k = 1; k < n; ++k) CHECK(idx[k - 1] < idx[k]);
    const size_t ncp = b.partial_applied(idx.data(), n, cp.data());
    CHECK(ncp == copied && b.nd == tr);
    b.clear_pending();
    CHECK(!b.partial && b.np == 0);
}

}  // namespace

int main() {
    std::vector<uint32_t> idx(N), cp(N);

    // list validation
    {
        List ok{{0, 1}, {1, 2}}, desc{{1, 0}, {0, 2}}, rep{{0, 1}, {0, 1}}, in_range{{0, 3}, {1, 0}}, out_range{{2, 0}};
        List all{{0, 0}, {0, 1}, {0, 2}, {1, 0}, {1, 1}, {1, 2}};
        CHECK(valid(ok, idx) == 2 && idx[0] == 1 && idx[1] == 5);
        CHECK(check_pairs(2, desc.o.data(), desc.i.data(), I, O, idx.data()) == PAIRS_ORDER);
        CHECK(check_pairs(2, rep.o.data(), rep.i.data(), I, O, idx.data()) == PAIRS_ORDER);
        CHECK(check_pairs(2, in_range.o.data(), in_range.i.data(), I, O, idx.data()) == PAIRS_RANGE);
        CHECK(check_pairs(1, out_range.o.data(), out_range.i.data(), I, O, idx.data()) == PAIRS_RANGE);
        CHECK(valid(all, idx) == N && idx[N - 1] == N - 1);
        CHECK(check_pairs(0, nullptr, nullptr, I, O, idx.data()) == PAIRS_OK);
    }

    // case 2: the script of case 1, then a whole update
    {
        PairBook b;
        b.init(N);
        CHECK(b.nd == 0 && b.np == 0 && !b.partial && b.last[0] == 0 && b.last[1] == 0);
        swap_partial(b, List{{0, 1}, {1, 2}}, idx, cp, 2, 0, 2);
        swap_partial(b, List{{1, 0}}, idx, cp, 1, 2, 1);
        swap_partial(b, List{{0, 2}, {1, 2}}, idx, cp, 2, 1, 2);  // update_input(2)
        b.whole_applied();
        CHECK(b.nd == N && b.last[0] == N && b.last[1] == 0);
        swap_partial(b, List{{0, 0}, {1, 1}}, idx, cp, 2, 4, 2);
        swap_partial(b, List{{0, 0}}, idx, cp, 1, 1, 1);
        swap_partial(b, List{}, idx, cp, 0, 1, 0);  // the empty list: update(R_base)
        PairBook c;
        c.init(N);
        c.copy_from(b);
        CHECK(c.nd == b.nd && c.last[0] == b.last[0] && c.last[1] == b.last[1] && c.d == b.d);
    }

    // case 4: pending partial updates
    {
        PairBook b;
        b.init(N);
        swap_partial(b, List{{0, 0}}, idx, cp, 1, 0, 1);  // the fade starts
        // two partial updates during the fade that share (1, 2)
        size_t n = valid(List{{0, 1}, {1, 2}}, idx);
        b.merge_pending(idx.data(), n);
        CHECK(b.partial && b.np == 2 && b.nd == 1);
        n = valid(List{{1, 0}, {1, 2}}, idx);
        b.merge_pending(idx.data(), n);
        CHECK(b.np == 3);
        PairBook c;  // a clone with the partial update pending
        c.init(N);
        c.copy_from(b);
        apply_pending(b, idx, cp, 3, 1);
        apply_pending(c, idx, cp, 3, 1);
        CHECK(b.d == c.d && b.last[0] == 3 && b.last[1] == 1);

        // whole then partial: the stored rows are patched, the response stays whole
        b.clear_pending();  // (the whole update stored)
        CHECK(!b.partial);
        b.whole_applied();  // applied by the first process() after the fade
        CHECK(b.nd == N && b.last[0] == N);

        // partial then whole: the whole response replaces the partial one
        n = valid(List{{0, 2}, {1, 0}}, idx);
        b.merge_pending(idx.data(), n);
        CHECK(b.partial && b.np == 2);
        b.clear_pending();
        CHECK(!b.partial && b.np == 0);
        CHECK(b.pending_list(idx.data()) == 0);
        b.whole_applied();

        // an empty partial update pending: update(R_base) once the fade has ended
        b.merge_pending(idx.data(), 0);
        CHECK(b.partial && b.np == 0);
        apply_pending(b, idx, cp, 0, N);
        CHECK(b.nd == 0);
    }
    std::puts("pair_book_check: ok");
    return 0;
}
