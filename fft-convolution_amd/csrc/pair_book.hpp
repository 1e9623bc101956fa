// pair_book.hpp -- the host-side bookkeeping of update_pairs: the
// pair-list validation, the diff set D of a crossfaded matrix (the pairs whose
// spectra may differ between its convolvers A and B) and the list of a pending
// partial update.  No device code and no HIP: host.cpp uses it, and
// tests/host/pair_book_check.cpp drives it stand-alone under the sanitizers.
// Every buffer is sized by init(); nothing here allocates afterwards.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace fftconv {

enum PairListError { PAIRS_OK = 0, PAIRS_RANGE = 1, PAIRS_ORDER = 2, PAIRS_ABSENT = 3 };

// pairs (pair_out[n], pair_in[n]) must be in range and strictly ascending in
// o * I + i (so: no repeats); idx[n] = o * I + i (room for O * I entries)
inline PairListError check_pairs(size_t n, const uint32_t *pair_out, const uint32_t *pair_in, size_t I, size_t O,
                                 uint32_t *idx) {
    size_t prev = 0;
    for (size_t k = 0; k < n; ++k) {
        if (pair_out[k] >= O || pair_in[k] >= I) return PAIRS_RANGE;
        const size_t p = (size_t)pair_out[k] * I + pair_in[k];
        if (k > 0 && p <= prev) return PAIRS_ORDER;  // (strictly ascending and in range: k < O * I)
        idx[k] = (uint32_t)p;
        prev = p;
    }
    return PAIRS_OK;
}

// check_pairs for a sparse matrix's update_pairs: the pairs must be in range,
// strictly ascending in (o, i) and belong to the CSR pattern (rowptr[O + 1],
// col[N], each row's inputs ascending); idx[n] = the pair's position in the
// pattern's list (room for N entries).  *bad = the first offending entry.
inline PairListError check_pairs_in_pattern(size_t n, const uint32_t *pair_out, const uint32_t *pair_in,
                                            const int *rowptr, const int *col, size_t I, size_t O, uint32_t *idx,
                                            size_t *bad = nullptr) {
    for (size_t k = 0; k < n; ++k) {
        if (bad) *bad = k;
        const uint32_t o = pair_out[k], i = pair_in[k];
        if (o >= O || i >= I) return PAIRS_RANGE;
        if (k > 0 && (o < pair_out[k - 1] || (o == pair_out[k - 1] && i <= pair_in[k - 1]))) return PAIRS_ORDER;
        int lo = rowptr[o], hi = rowptr[o + 1];  // (binary search of output o's row)
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if ((uint32_t)col[mid] < i)
                lo = mid + 1;
            else
                hi = mid;
        }
        if (lo >= rowptr[o + 1] || (uint32_t)col[lo] != i) return PAIRS_ABSENT;
        idx[k] = (uint32_t)lo;  // (ascending and in the pattern: k < N)
    }
    return PAIRS_OK;
}

struct PairBook {
    size_t pairs = 0;
    std::vector<uint8_t> d;    // d[p]: pair p is in D
    std::vector<uint8_t> pnd;  // pnd[p]: pair p is listed by the pending partial update
    size_t nd = 0, np = 0;
    bool partial = false;      // the pending response is a partial one (its rows at the pairs' own positions)
    size_t last[2] = {0, 0};   // pairs transformed / copied by the last applied swap

    void init(size_t n) {
        pairs = n;
        d.assign(n, 0);
        pnd.assign(n, 0);
        nd = np = 0;
        partial = false;
        last[0] = last[1] = 0;
    }
    // a whole update was applied to one convolver: every pair may differ
    void whole_applied() {
        for (size_t p = 0; p < pairs; ++p) d[p] = 1;
        nd = pairs;
        last[0] = pairs;
        last[1] = 0;
    }
    // a partial swap of the ascending list lst into the non-target convolver:
    // cp = D \ lst (ascending, room for `pairs` entries), then D = lst
    size_t partial_applied(const uint32_t *lst, size_t n, uint32_t *cp) {
        for (size_t k = 0; k < n; ++k) d[lst[k]] |= 2;  // (2: listed now)
        size_t ncp = 0;
        for (size_t p = 0; p < pairs; ++p) {
            if (d[p] == 1) cp[ncp++] = (uint32_t)p;
            d[p] = (d[p] & 2) ? 1 : 0;
        }
        nd = n;
        last[0] = n;
        last[1] = ncp;
        return ncp;
    }
    // a partial update joins the pending one (the caller has written its rows)
    void merge_pending(const uint32_t *lst, size_t n) {
        for (size_t k = 0; k < n; ++k)
            if (!pnd[lst[k]]) {
                pnd[lst[k]] = 1;
                ++np;
            }
        partial = true;
    }
    // the pending list, ascending (room for `pairs` entries)
    size_t pending_list(uint32_t *out) const {
        size_t n = 0;
        for (size_t p = 0; p < pairs; ++p)
            if (pnd[p]) out[n++] = (uint32_t)p;
        return n;
    }
    // the pending response was applied, or a whole one replaced it
    void clear_pending() {
        if (np)
            for (size_t p = 0; p < pairs; ++p) pnd[p] = 0;
        np = 0;
        partial = false;
    }
    void copy_from(const PairBook &o) {  // (same `pairs`: a clone's book)
        d = o.d;
        pnd = o.pnd;
        pairs = o.pairs; nd = o.nd; np = o.np; partial = o.partial;
        last[0] = o.last[0];
        last[1] = o.last[1];
    }
};

}  // namespace fftconv
