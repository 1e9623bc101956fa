// matrix_sp_ts.hip -- gfx950 kernels of the SparseMatrixTwoStageConvolver
// (DESIGN §4r): the head and tail0 sparse matrices of a two-stage handle, at an
// aligned call (a whole head block on a block boundary of the tail period), in
// the two launches of matrix_ts.hip over the CSR pattern of matrix_sp.hip.
//
//   launch A  [0, I)   one R2C per input, the row written to X_head and X_tail0,
//                      the block copied to tail_input[i][fill..]
//                      (src/fft_convolver.rs:459-461) from the registers that
//                      feed the transform
//             I + m    MAC workgroup m < PT = (output o, part p) from wg[m], for
//                      H_head and H_tail0 in one pass (matrix_sp.hpp): every X
//                      row and `col` entry loaded once, from the head's delay line
//   launch B  (o, 0)   the head's finish of matrix_sp_b_kernel (sum of the
//                      output's parts, + the row-0 terms in ascending e, C2R,
//                      overlap-add) with the sub-chunk sums of :438-454 in its
//                      epilogue:
//                        out[j] = ((y / N + ovl) + tail_precalculated0[pos + j])
//                                 + tail_precalculated[pos + j]
//             (o, 1)   tail0's finish into tail_output0[o][fill..] (:464-472),
//                      with its own overlap
//
// Head and tail0 have the same pattern and active_seg_count, so one plan / wg
// serves both.  Each matrix's arithmetic is the plain sparse matrix's, and the
// two sums are added in twostage order, so an aligned call computes the bits
// that head.process, matrix_ts_accum_kernel and tail0.process compute, and
// output o those of a dense two-stage matrix with k_o inputs.  Nothing in a
// launch reads what that launch writes: tail_output0 and tail_precalculated0
// are different buffers until the host swaps them after the launch, and the
// kernel boundary is the only ordering.  A finish workgroup needs the plain
// one's two LDS buffers, no more.
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

template <int LOG2B, int NT, bool NTL>
__global__ __launch_bounds__(NT) void matrix_sp_ts_a_kernel(MatrixSpTsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x;
    if (b < a.I) {
        matrix_r2c_block<LOG2B, NT>(a, b, smem);
        return;
    }
    // (the row walk over the pair list, two H streams; its DBG_CHECK sites are 77, 78 and 79)
    matrix_row_walk<LOG2B, NT, NTL, 77>(listed_rows(a.wg, a.col, b - a.I, a.PT, a.N, 78),
                                        MacStreamsPair<MatrixSpTsArgs>{a}, a.act - 1, smem);
}

// Launch B, workgroup = (output o, matrix c): matrix_sp_b_kernel's finish of a
// whole block (fill 0, k = B), c = 0 for the head, c = 1 for tail0, side by
// side as matrix_ts_b_kernel (the finish is a latency chain), with its epilogue
// (ts_epilogue).  An output without pairs has one all-zero part and no terms: it
// writes zeros (plus the precalculated sums, which are zero for it too) and
// keeps a zero overlap in both stages.
template <int LOG2B, int NT>
__global__ __launch_bounds__(NT) void matrix_sp_ts_b_kernel(MatrixSpTsArgs a) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int B = Gm::B, F = Gm::F, SPT = Gm::SPT;
    constexpr int UB = SPT == 1 ? 16 : (SPT == 2 ? 8 : 4);  // terms in flight per slot
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *bufA = reinterpret_cast<float2 *>(smem);
    float2 *bufB = bufA + B;
    const int tid = threadIdx.x;
    const int o = blockIdx.x;
    const int c = blockIdx.y;  // (uniform over the workgroup)
    const int P = a.plan[o + 1] - a.plan[o];
    const int n0 = a.rowptr[o];
    const int ko = a.rowptr[o + 1] - n0;
    DBG_CHECK(P >= 1 && a.plan[o + 1] <= a.PT && n0 >= 0 && ko >= 0 && n0 + ko <= a.N, 80, o, P, a.PT,
              n0 + ko);  // (site 80: a part past `part`, a pair list past `col`)
    const size_t SF = (size_t)a.S * F;
    const int *colo = a.col + n0;
    const float4 *part4 = reinterpret_cast<const float4 *>(a.part[c]) + (size_t)a.plan[o] * F;
    const float4 *H4 = reinterpret_cast<const float4 *>(a.H[c]) + (size_t)n0 * SF;
    const float4 *X4 = reinterpret_cast<const float4 *>(a.X[c]) + (size_t)a.cur * F;
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
        const int f = tid + q * NT;
        if (f < F) {
            // (both sums strictly in ascending order, the inputs of a chunk of
            // terms loaded one chunk ahead, as matrix_sp_b_kernel)
            int cn[UB / 2];
#pragma unroll
            for (int u = 0; u < UB / 2; ++u) cn[u] = u < ko ? colo[u] : 0;  // (uniform over the workgroup)
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int p = 0; p < P; p += UB) {
                float4 t[UB];
#pragma unroll
                for (int u = 0; u < UB; ++u)
                    if (p + u < P) t[u] = part4[(size_t)(p + u) * F + f];
#pragma unroll
                for (int u = 0; u < UB; ++u)
                    if (p + u < P) v = p + u == 0 ? t[u] : vadd(v, t[u]);
            }
            for (int e = 0; e < ko; e += UB / 2) {
                float4 xs[UB / 2], hs[UB / 2];
                int ci[UB / 2];
#pragma unroll
                for (int u = 0; u < UB / 2; ++u) {
                    ci[u] = cn[u];
                    cn[u] = e + UB / 2 + u < ko ? colo[e + UB / 2 + u] : 0;
                }
#pragma unroll
                for (int u = 0; u < UB / 2; ++u) {
                    if (e + u < ko) {
                        DBG_CHECK(ci[u] >= 0 && ci[u] < a.I, 81, ci[u], e + u, a.I, o);  // (site 81: a `col` entry >= I)
                        xs[u] = X4[(size_t)ci[u] * SF + f];
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
    const float *y = finish_c2r<LOG2B, NT>(bufA, bufB, a.tw);
    ts_epilogue<LOG2B, NT>(a, o, c, y);
}

template <int LOG2B>
hipError_t launch_matrix_sp_ts_t(const MatrixSpTsArgs &a, hipStream_t s) {
    constexpr int NT = matrix_nt(LOG2B);
    using Gm = MGeo<LOG2B, NT>;
    auto ka = a.nt_h ? matrix_sp_ts_a_kernel<LOG2B, NT, true> : matrix_sp_ts_a_kernel<LOG2B, NT, false>;
    auto kb = matrix_sp_ts_b_kernel<LOG2B, NT>;
    const long long grid = (long long)a.I + (long long)a.PT;
    if (hipError_t e = launch_dyn(ka, dim3((unsigned)grid), dim3(NT), Gm::lds_a_pair, s, a); e != hipSuccess) return e;
    return launch_dyn(kb, dim3(a.O, 2), dim3(NT), Gm::lds_b, s, a);
}

}  // namespace

hipError_t launch_matrix_sp_ts_block(int log2b, const MatrixSpTsArgs &a, hipStream_t s) {
    if (!matrix_chunk_in_range(log2b, a.I, a.O, a.S, a.cur, a.act, 0, 1 << log2b) || a.N <= 0 || a.PT < a.O || !a.rowptr ||
        !a.col || !a.plan || !a.wg || a.T < (1LL << log2b) || !a.tin || !a.tout0 || !a.p0)
        return hipErrorInvalidValue;
    for (int c = 0; c < 2; ++c)
        if (!a.H[c] || !a.X[c] || !a.ovl[c] || !a.part[c]) return hipErrorInvalidValue;
    if ((long long)a.I + (long long)a.PT > (long long)INT32_MAX) return hipErrorInvalidValue;
    return dispatch_log2<5, kMaxLog2Fused>(log2b, hipErrorInvalidValue,
                                           [&](auto L) { return launch_matrix_sp_ts_t<L()>(a, s); });
}

}  // namespace fftconv
