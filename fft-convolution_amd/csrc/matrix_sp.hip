// matrix_sp.hip -- gfx950 kernels of the SparseMatrixConvolver:
//   y[o] = sum over the listed pairs (o, i) of x[i] * h[(o, i)]
// as N reference FFTConvolver instances in lockstep, one per listed pair, in
// CSR order (strictly ascending (o, i)).  The dense matrix's scheme (matrix.hip)
// with an output's pair list in place of 0..I-1: one delay line per input, the
// spectra summed per output before ONE inverse transform.
//
// HBM layout (packed rows: B float2 per row, slot 0 = (DC, Nyquist)):
//   H      float2 [N][S][B]      IR spectra, pair n = channel n of the IR transform
//   X      float2 [I][S][B]      one FDL per input
//   ovl    float  [O][B]         summed overlap per output
//   ib     float  [I][B]         input buffer per input (zero past the fill)
//   pre    float2 [O][B]         summed pre_multiplied, kept across partial chunks
//   part   float2 [sum P_o][B]   split-row partial sums, output o's at plan[o]
//   rowptr int    [O + 1]        pairs of output o = [rowptr[o], rowptr[o + 1])
//   col    int    [N]            input of pair n
//   plan   int    [O + 1]        prefix sums of P_o for the current active_seg_count
//   wg     int4   [sum P_o]      MAC workgroup m of launch A = {rowptr[o], k_o, p, P_o}
//
// Output o with k_o pairs runs the row walk and the finish's sums (matrix.hpp)
// of a dense matrix with k_o inputs, entry e of its list standing for input e
// (ListedRows, matrix_sp.hpp): the same rows in the same order into the same
// accumulators, so its bits are that dense matrix's.  The kernel boundary is the only ordering, as in matrix.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_lds.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "matrix.hpp"
#include "matrix_sp.hpp"
#include "packed.hpp"

namespace fftconv {
namespace {

// plan[o] = P_0 + ... + P_(o-1), P_o = matrix_parts_rule(k_o, act), by one
// workgroup (plan_scan) -- and, per MAC workgroup m = plan[o] + p of launch A,
// wg[m] = {rowptr[o], k_o, p, P_o}: all a MAC workgroup needs in ONE load (a
// search of the prefix sums costs log2(O) dependent loads before the first row
// is requested, several times the walk of a 128-row part).
__global__ __launch_bounds__(kPlanNT) void matrix_sp_plan_kernel(const int *rowptr, int *plan, int4 *wg, int O,
                                                                 int act) {
    __shared__ int sums[kPlanNT + 1];
    const int pt = plan_scan(
        sums, O, [&](int o) { return matrix_parts_rule(rowptr[o + 1] - rowptr[o], act); },
        [&](int o, int acc, int P) {
            const int n0 = rowptr[o], ko = rowptr[o + 1] - n0;
            plan[o] = acc;
            for (int p = 0; p < P; ++p) wg[acc + p] = make_int4(n0, ko, p, P);
        });
    if (threadIdx.x == 0) plan[O] = pt;
}

// Launch A: blocks [0, I) are the R2C workgroups, blocks I + m, m < PT, the MAC
// workgroups of the compact grid (launched only for a chunk that starts a
// block): workgroup m = (output o, part p) with plan[o] <= m < plan[o + 1], p =
// m - plan[o], read from wg[m], runs the row walk over output o's pair list
// (sites 54, 55, 56).
template <int LOG2B, int NT, bool NTL>
__global__ __launch_bounds__(NT) void matrix_sp_a_kernel(MatrixSpArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x;
    if (b < a.m.I) {
        matrix_r2c<LOG2B, NT>(a.m, b, smem);
    } else {
        matrix_row_walk<LOG2B, NT, NTL, 54>(listed_rows(a.wg, a.col, b - a.m.I, a.PT, a.N, 55), MacStreams{a.m},
                                            a.m.act - 1, smem);
    }
}

// Launch B, workgroup = output o: matrix_b_kernel over output o's P_o parts and
// its pair list -- pre = part[plan[o]] + part[plan[o] + 1] + ... (or the kept
// pre[o]), conv = pre + sum_e X[col e][current] (.) H[pair e][0] in ascending e,
// one C2R with 1/N, overlap-add, overlap saved when the block completes.  An
// output without pairs has one all-zero part and no terms: it writes zeros and
// keeps a zero overlap.
template <int LOG2B, int NT>
__global__ __launch_bounds__(NT) void matrix_sp_b_kernel(MatrixSpArgs a) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int B = Gm::B, F = Gm::F, SPT = Gm::SPT;
    constexpr int UB = SPT == 1 ? 16 : (SPT == 2 ? 8 : 4);  // terms in flight per slot
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *bufA = reinterpret_cast<float2 *>(smem);
    float2 *bufB = bufA + B;
    const int tid = threadIdx.x;
    const int o = blockIdx.x;
    const int fill = a.m.fill, k = a.m.k;
    const bool complete = fill + k == B;
    const int P = a.plan[o + 1] - a.plan[o];
    const int n0 = a.rowptr[o];
    const int ko = a.rowptr[o + 1] - n0;
    const size_t SF = (size_t)a.m.S * F;
    float4 *pre4 = reinterpret_cast<float4 *>(a.m.pre) + (size_t)o * F;
    const float4 *part4 = reinterpret_cast<const float4 *>(a.m.part) + (size_t)a.plan[o] * F;
    const float4 *H4 = reinterpret_cast<const float4 *>(a.m.H) + (size_t)n0 * SF;
    const float4 *X4 = reinterpret_cast<const float4 *>(a.m.X) + (size_t)a.m.cur * F;
    const int *colo = a.col + n0;
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
        const int f = tid + q * NT;
        if (f < F) {
            // (both sums strictly in ascending order; the loads of UB terms are
            // issued before their adds, so the chain waits once per UB terms.
            // The inputs of a chunk of terms are loaded one chunk ahead, the
            // first chunk's ahead of the parts: the wait for `col` never sits
            // between a chunk's adds and its row requests)
            int cn[UB / 2];
#pragma unroll
            for (int u = 0; u < UB / 2; ++u) cn[u] = u < ko ? colo[u] : 0;  // (uniform over the workgroup)
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (fill == 0) {
                for (int p = 0; p < P; p += UB) {
                    float4 t[UB];
#pragma unroll
                    for (int u = 0; u < UB; ++u)
                        if (p + u < P) t[u] = part4[(size_t)(p + u) * F + f];
#pragma unroll
                    for (int u = 0; u < UB; ++u)
                        if (p + u < P) v = p + u == 0 ? t[u] : vadd(v, t[u]);
                }
            } else {
                v = pre4[f];
            }
            if (!complete) pre4[f] = v;
            for (int e = 0; e < ko; e += UB / 2) {
                float4 xs[UB / 2], hs[UB / 2];
                int c[UB / 2];
#pragma unroll
                for (int u = 0; u < UB / 2; ++u) {
                    c[u] = cn[u];
                    cn[u] = e + UB / 2 + u < ko ? colo[e + UB / 2 + u] : 0;
                }
#pragma unroll
                for (int u = 0; u < UB / 2; ++u) {
                    if (e + u < ko) {
                        DBG_CHECK(c[u] >= 0 && c[u] < a.m.I, 57, c[u], e + u, a.m.I, o);  // (site 57: a `col` entry >= I)
                        xs[u] = X4[(size_t)c[u] * SF + f];
                        hs[u] = H4[(size_t)(e + u) * SF + f];
                    }
                }
#pragma unroll
                for (int u = 0; u < UB / 2; ++u)
                    if (e + u < ko) v = slot_mac(v, xs[u], hs[u], f);
            }
            reinterpret_cast<float4 *>(bufA)[f] = v;
        }
    }
    const float *y = finish_c2r<LOG2B, NT>(bufA, bufB, a.m.tw);
    float *outc = a.m.out + (long long)o * a.m.out_stride;
    float *ovc = a.m.ovl + (size_t)o * B;
    overlap_add<LOG2B, NT>(y, ovc, fill, k, [&](int j, float v) { outc[j] = v; });
    if (complete) overlap_save<LOG2B, NT>(y, ovc);
}

template <int LOG2B>
hipError_t launch_matrix_sp_t(const MatrixSpArgs &a, hipStream_t s) {
    constexpr int NT = matrix_nt(LOG2B);
    using Gm = MGeo<LOG2B, NT>;
    auto ka = a.m.nt_h ? matrix_sp_a_kernel<LOG2B, NT, true> : matrix_sp_a_kernel<LOG2B, NT, false>;
    auto kb = matrix_sp_b_kernel<LOG2B, NT>;
    const long long grid = (long long)a.m.I + (a.m.fill == 0 ? (long long)a.PT : 0);
    if (hipError_t e = launch_dyn(ka, dim3((unsigned)grid), dim3(NT), Gm::lds_a, s, a); e != hipSuccess) return e;
    return launch_dyn(kb, dim3(a.m.O), dim3(NT), Gm::lds_b, s, a);
}

}  // namespace

hipError_t launch_matrix_sp_plan(const int *rowptr, int *plan, int4 *wg, int O, int act, hipStream_t s) {
    if (!rowptr || !plan || !wg || O <= 0 || act < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(matrix_sp_plan_kernel, dim3(1), dim3(kPlanNT), 0, s, rowptr, plan, wg, O, act);
    return hipGetLastError();
}

hipError_t launch_matrix_sp_chunk(int log2b, const MatrixSpArgs &a, hipStream_t s) {
    const MatrixArgs &m = a.m;
    if (!matrix_chunk_in_range(log2b, m.I, m.O, m.S, m.cur, m.act, m.fill, m.k) || a.N <= 0 || a.PT < m.O || !a.rowptr ||
        !a.col || !a.plan || !a.wg)
        return hipErrorInvalidValue;
    if ((long long)m.I + (long long)a.PT > (long long)INT32_MAX) return hipErrorInvalidValue;
    return dispatch_log2<5, kMaxLog2Fused>(log2b, hipErrorInvalidValue,
                                           [&](auto L) { return launch_matrix_sp_t<L()>(a, s); });
}

}  // namespace fftconv
