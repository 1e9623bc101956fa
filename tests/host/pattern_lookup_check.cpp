// pattern_lookup_check.cpp -- the sparse matrices' update_pairs on the host
// (csrc/pair_book.hpp: check_pairs_in_pattern and a PairBook of N listed pairs)
// driven stand-alone, without a GPU, through the bookkeeping script of
// tests/test_gpu_matrix_sparse_xf.py (test_update_pairs_idle_swaps_and_bookkeeping)
// and the error lists of its test_errors_leave_the_handle_unchanged.  Built with
// the sanitizers and run once:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I fft-convolution_amd/csrc tests/host/pattern_lookup_check.cpp -o pattern_lookup_check && ./pattern_lookup_check
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

// PATTERN_1 of tests/matrix_sp_ref.py (I 5, O 4): five pairs, one pair, none, two pairs
constexpr size_t I = 5, O = 4, N = 8;
const std::vector<int> rowptr{0, 5, 6, 6, 8};
const std::vector<int> col{0, 1, 2, 3, 4, 2, 0, 4};

struct List {
    std::vector<uint32_t> o, i;
    List(std::initializer_list<std::pair<uint32_t, uint32_t>> p) {
        for (auto &e : p) {
            o.push_back(e.first);
            i.push_back(e.second);
        }
    }
};

PairListError look(const List &l, std::vector<uint32_t> &idx, size_t *bad = nullptr) {
    CHECK(l.o.size() <= N);  // (the caller's n > N check; idx has exactly N entries)
    return check_pairs_in_pattern(l.o.size(), l.o.data(), l.i.data(), rowptr.data(), col.data(), I, O, idx.data(), bad);
}

// what SparseMatrixCrossfadeCore does with the book: a direct partial swap
void swap_partial(PairBook &b, const List &l, std::vector<uint32_t> &idx, std::vector<uint32_t> &cp, size_t tr,
                  size_t copied, size_t nd) {
    CHECK(look(l, idx) == PAIRS_OK);
    const size_t n = l.o.size();
    for (size_t k = 1; k < n; ++k) CHECK(idx[k - 1] < idx[k]);
    for (size_t k = 0; k < n; ++k) CHECK(idx[k] < N && (uint32_t)col[idx[k]] == l.i[k]);
    const size_t ncp = b.partial_applied(idx.data(), n, cp.data());
    CHECK(n == tr && ncp == copied && b.nd == nd);
    CHECK(b.last[0] == tr && b.last[1] == copied);
    for (size_t k = 1; k < ncp; ++k) CHECK(cp[k - 1] < cp[k]);
    for (size_t k = 0; k < ncp; ++k)
        for (size_t m = 0; m < n; ++m) CHECK(cp[k] != idx[m]);
}

}  // namespace

int main() {
    std::vector<uint32_t> idx(N), cp(N);

    // the lookup: list positions
    {
        List all{{0, 0}, {0, 1}, {0, 2}, {0, 3}, {0, 4}, {1, 2}, {3, 0}, {3, 4}};
        CHECK(look(all, idx) == PAIRS_OK);
        for (size_t n = 0; n < N; ++n) CHECK(idx[n] == n);
        CHECK(look(List{{0, 1}, {1, 2}, {3, 4}}, idx) == PAIRS_OK && idx[0] == 1 && idx[1] == 5 && idx[2] == 7);
        CHECK(look(List{}, idx) == PAIRS_OK);  // the empty list: update(base)
        CHECK(check_pairs_in_pattern(0, nullptr, nullptr, rowptr.data(), col.data(), I, O, idx.data()) == PAIRS_OK);
    }

    // the error lists
    {
        size_t bad = 99;
        CHECK(look(List{{0, 1}, {1, 0}}, idx, &bad) == PAIRS_ABSENT && bad == 1);   // absent
        CHECK(look(List{{1, 1}}, idx, &bad) == PAIRS_ABSENT && bad == 0);
        CHECK(look(List{{1, 3}}, idx) == PAIRS_ABSENT);                              // past the row's last input
        CHECK(look(List{{2, 0}}, idx) == PAIRS_ABSENT);                              // an output without pairs
        CHECK(look(List{{0, 1}, {2, 4}}, idx, &bad) == PAIRS_ABSENT && bad == 1);
        CHECK(look(List{{0, 1}, {0, 1}}, idx) == PAIRS_ORDER);                       // repeated
        CHECK(look(List{{3, 0}, {0, 1}}, idx) == PAIRS_ORDER);                       // descending
        CHECK(look(List{{0, 2}, {0, 1}}, idx) == PAIRS_ORDER);
        CHECK(look(List{{0, 5}}, idx) == PAIRS_RANGE);                               // out of range
        CHECK(look(List{{4, 0}}, idx) == PAIRS_RANGE);
        CHECK(look(List{{0, 0}, {4, 0}}, idx, &bad) == PAIRS_RANGE && bad == 1);
    }

    // the bookkeeping script of the GPU test
    {
        PairBook b;
        b.init(N);
        CHECK(b.nd == 0 && b.np == 0 && !b.partial && b.last[0] == 0 && b.last[1] == 0);
        swap_partial(b, List{{0, 1}, {1, 2}}, idx, cp, 2, 0, 2);
        swap_partial(b, List{{0, 1}, {3, 4}}, idx, cp, 2, 1, 2);  // copies the first list's pairs minus its own
        b.whole_applied();
        CHECK(b.nd == N && b.last[0] == N && b.last[1] == 0);
        swap_partial(b, List{{0, 0}, {3, 0}}, idx, cp, 2, N - 2, 2);
        swap_partial(b, List{{0, 0}, {3, 0}}, idx, cp, 2, 0, 2);                             // update_input(0)
        swap_partial(b, List{{0, 0}, {0, 1}, {0, 2}, {0, 3}, {0, 4}}, idx, cp, 5, 1, 5);     // update_output(0)
        swap_partial(b, List{}, idx, cp, 0, 5, 0);                                           // update(base)

        // two partial updates during a fade that share (3, 4), and a clone
        swap_partial(b, List{{0, 0}}, idx, cp, 1, 0, 1);
        CHECK(look(List{{0, 1}, {3, 4}}, idx) == PAIRS_OK);
        b.merge_pending(idx.data(), 2);
        CHECK(look(List{{1, 2}, {3, 4}}, idx) == PAIRS_OK);
        b.merge_pending(idx.data(), 2);
        CHECK(b.partial && b.np == 3 && b.nd == 1);
        PairBook c;
        c.init(N);
        c.copy_from(b);
        for (PairBook *k : {&b, &c}) {
            const size_t n = k->pending_list(idx.data());
            CHECK(n == 3 && idx[0] == 1 && idx[1] == 5 && idx[2] == 7);
            CHECK(k->partial_applied(idx.data(), n, cp.data()) == 1 && cp[0] == 0 && k->nd == 3);
            k->clear_pending();
            CHECK(!k->partial && k->np == 0);
        }
        CHECK(b.d == c.d);
    }
    std::puts("pattern_lookup_check: ok");
    return 0;
}
