// matrix_sp.hpp -- what the families over a listed pair set (matrix_sp.hip,
// matrix_sp_xf.hip, matrix_sp_ts.hip, matrix_sp_la.hip) add to matrix.hpp: the
// pair-list row source of the walks and the one-workgroup prefix scan of the
// plan kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "matrix.hpp"
#include "packed.hpp"

namespace fftconv {

// Row source of an output's pair list [n0, n0 + ko), part p of P: index e of a
// walk is pair n0 + e, its input a load of col[n0 + e]; the partial sum goes to
// row `row` (the workgroup's position in its compact grid, or the far row); the
// rows per part are computed here, ceil(rows / P).  Entry e standing for input
// e, the walk is the dense one of a matrix with ko inputs: the same bits.
struct ListedRows {
    static constexpr bool kListed = true;
    const int *cols;  // col + n0
    int n0, ko, p, P;
    size_t row;
    __device__ __forceinline__ int count() const { return ko; }
    __device__ __forceinline__ size_t first_pair() const { return (size_t)n0; }
    __device__ __forceinline__ size_t out_row() const { return row; }
    __device__ __forceinline__ long long rpp(long long R) const { return (R + P - 1) / P; }
    __device__ __forceinline__ int col(int e) const { return cols[e]; }
};
// MAC workgroup m of a compact grid of PT, described by wg[m] = {rowptr[o],
// k_o, p, P_o}: all it needs in ONE load (site: a part past `part`, a pair list
// past `col`)
__device__ __forceinline__ ListedRows listed_rows(const int4 *wg, const int *col, int m, int PT, int N, int site) {
    const int4 d = wg[m];
    const int n0 = d.x, ko = d.y, p = d.z, P = d.w;
    DBG_CHECK(m >= 0 && m < PT && p >= 0 && p < P && n0 >= 0 && ko >= 0 && n0 + ko <= N, site, m, p, PT, n0 + ko);
    return {col + n0, n0, ko, p, P, (size_t)m};
}

// Exclusive prefix sums over value(0 .. n - 1) by one workgroup of kPlanNT
// threads: thread t sums a contiguous run, thread 0 scans the run sums, every
// thread emits its run as emit(j, prefix, value).  `sums` is kPlanNT + 1 ints
// of LDS.  Returns the total.  A plan kernel may scan several times.
constexpr int kPlanNT = 256;
template <class V, class E>
__device__ __forceinline__ int plan_scan(int *sums, int n, V value, E emit) {
    const int tid = threadIdx.x;
    const long long per = ((long long)n + kPlanNT - 1) / kPlanNT;
    const long long b0 = (long long)tid * per;
    const int j0 = (int)(b0 < n ? b0 : n);
    const int j1 = (int)(b0 + per < n ? b0 + per : n);
    int sum = 0;
    for (int j = j0; j < j1; ++j) sum += value(j);
    __syncthreads();  // (the previous scan's reads of `sums` are done)
    sums[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int t = 0; t < kPlanNT; ++t) {
            const int v = sums[t];
            sums[t] = acc;
            acc += v;
        }
        sums[kPlanNT] = acc;
    }
    __syncthreads();  // (and every global write of the scans before this one is visible)
    int acc = sums[tid];
    for (int j = j0; j < j1; ++j) {
        const int v = value(j);
        emit(j, acc, v);
        acc += v;
    }
    return sums[kPlanNT];
}

}  // namespace fftconv
