// matrix_sp_xf.hip -- gfx950 kernels of the SparseMatrixCrossfadeConvolver
// (DESIGN §4p): the two sparse matrices A and B of a crossfaded handle, while
// they are in step, in the two launches per chunk of matrix_xf.hip over the CSR
// pattern of matrix_sp.hip.
//
//   launch A  [0, I)   one R2C per input, the row written to X_A and X_B, both
//                      input buffers maintained
//             I + m    (a chunk that starts a block) MAC workgroup m < PT =
//                      (output o, part p) from wg[m]: the listed row walk on
//                      the live convolver's H, or -- both live -- one pass with
//                      every X row and `col` entry loaded once for H_A and H_B
//             last     (first chunk of a call inside a fade) one lane walks
//                      mix_value into the call's device table
//   launch B  o        per live convolver the finish of matrix_sp_b_kernel (sum
//                      of parts or kept pre, + the row-0 terms in ascending e,
//                      C2R, overlap-add, overlap / pre kept), then the mix
//
// A and B have the same active_seg_count, so one plan / wg serves both.  Each
// convolver's arithmetic is the plain sparse matrix's: a fused chunk computes
// the bits the two plain chunks and crossfade_mix_kernel compute, and output o
// those of a dense crossfaded matrix with k_o inputs.  The kernel boundary is
// the only ordering.  A's samples wait in `out` between the two passes of the
// finish (same thread, same address), the fade curve is a device table, so
// every block size 32..8192 runs fused with the plain finish's LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_lds.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "matrix.hpp"
#include "matrix_sp.hpp"
#include "mix.hpp"
#include "packed.hpp"

namespace fftconv {
namespace {

// PAIR = both convolvers live.  Two kernels, not one branch: the one-stream MAC
// of the idle state then keeps the plain sparse MAC's register budget (one
// kernel for both took SP1's idle block from 21.1 to 23.7 us).
template <int LOG2B, int NT, bool NTL, bool PAIR>
__global__ __launch_bounds__(NT) void matrix_sp_xf_a_kernel(MatrixSpXfArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x;
    if (a.walk && b == (int)gridDim.x - 1) {  // launch B and the call's later chunks read the table
        if (threadIdx.x == 0) mix_walk(a.mix, a.walk);
        return;
    }
    if (b < a.I) {
        matrix_r2c_pair<LOG2B, NT>(a, b, smem);
        return;
    }
    // (the row walk over the pair list; its DBG_CHECK sites are 63, 64 and 65)
    const ListedRows rw = listed_rows(a.wg, a.col, b - a.I, a.PT, a.N, 64);
    if constexpr (PAIR)
        matrix_row_walk<LOG2B, NT, NTL, 63>(rw, MacStreamsPair<MatrixSpXfArgs>{a}, a.act - 1, smem);
    else
        matrix_row_walk<LOG2B, NT, NTL, 63>(rw, MacStreamsOf<MatrixSpXfArgs>{a, a.live == 1 ? 0 : 1}, a.act - 1, smem);
}

// Launch B, workgroup = output o: matrix_sp_b_kernel's finish for each live
// convolver in turn (A, then B), and the crossfader's mix of the two samples
// in B's epilogue, as matrix_xf_b_kernel.  Only the first mix.n - off samples
// of the chunk are written.  An output without pairs has one all-zero part and
// no terms: it writes zeros and keeps a zero overlap in both convolvers.
template <int LOG2B, int NT>
__global__ __launch_bounds__(NT) void matrix_sp_xf_b_kernel(MatrixSpXfArgs a) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int B = Gm::B, F = Gm::F, SPT = Gm::SPT;
    constexpr int UB = SPT == 1 ? 16 : (SPT == 2 ? 8 : 4);  // terms in flight per slot
    constexpr float invN = 1.0f / (float)(2 * B);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *bufA = reinterpret_cast<float2 *>(smem);
    float2 *bufB = bufA + B;
    const int tid = threadIdx.x;
    const int o = blockIdx.x;
    const int fill = a.fill, k = a.k;
    const bool complete = fill + k == B;
    const bool both = a.live == 3;
    const int P = a.plan[o + 1] - a.plan[o];
    const int n0 = a.rowptr[o];
    const int ko = a.rowptr[o + 1] - n0;
    DBG_CHECK(P >= 1 && a.plan[o + 1] <= a.PT && n0 >= 0 && ko >= 0 && n0 + ko <= a.N, 66, o, P, a.PT,
              n0 + ko);  // (site 66: a part past `part`, a pair list past `col`)
    const size_t SF = (size_t)a.S * F;
    const int *colo = a.col + n0;
    float *outc = a.out + (long long)o * a.out_stride;
    const int n_out = a.mix.n - a.off;  // samples of this chunk inside output_len
    for (int c = 0; c < 2; ++c) {
        if (!((a.live >> c) & 1)) continue;  // (uniform over the workgroup)
        float4 *pre4 = reinterpret_cast<float4 *>(a.pre[c]) + (size_t)o * F;
        const float4 *part4 = reinterpret_cast<const float4 *>(a.part[c]) + (size_t)a.plan[o] * F;
        const float4 *H4 = reinterpret_cast<const float4 *>(a.H[c]) + (size_t)n0 * SF;
        const float4 *X4 = reinterpret_cast<const float4 *>(a.X[c]) + (size_t)a.cur * F;
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
            const int f = tid + q * NT;
            if (f < F) {
                // (both sums strictly in ascending order, the inputs of a chunk
                // of terms loaded one chunk ahead, as matrix_sp_b_kernel)
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
                    int ci[UB / 2];
#pragma unroll
                    for (int u = 0; u < UB / 2; ++u) {
                        ci[u] = cn[u];
                        cn[u] = e + UB / 2 + u < ko ? colo[e + UB / 2 + u] : 0;
                    }
#pragma unroll
                    for (int u = 0; u < UB / 2; ++u) {
                        if (e + u < ko) {
                            DBG_CHECK(ci[u] >= 0 && ci[u] < a.I, 67, ci[u], e + u, a.I, o);  // (site 67: a `col` entry >= I)
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
        __syncthreads();
        for (int m = tid; m < B; m += NT) bufB[m] = real_pre<LOG2B, NT>(bufA, m, a.tw);
        __syncthreads();
        const float *y = reinterpret_cast<const float *>(lds_cfft<LOG2B, NT, true>(bufB, bufA, a.tw));
        float *ovc = a.ovl[c] + (size_t)o * B;
        for (int j = tid; j < k; j += NT) {
            const float v = y[fill + j] * invN + ovc[fill + j];
            if (j < n_out) {
                if (!both || c == 0)
                    outc[j] = v;  // (both live: A's sample waits here for B's pass, same thread)
                else
                    outc[j] = mix_sample(a.mix, a.off + j, outc[j], v, a.mix.vtab);
            }
        }
        if (complete) {
            __syncthreads();  // (every overlap read above is done)
            for (int j = tid; j < B; j += NT) ovc[j] = y[B + j] * invN;
        }
        __syncthreads();  // (the next convolver reuses both buffers)
    }
}

template <int LOG2B>
hipError_t launch_matrix_sp_xf_t(const MatrixSpXfArgs &a, hipStream_t s) {
    constexpr int NT = matrix_nt(LOG2B);
    using Gm = MGeo<LOG2B, NT>;
    auto ka = a.live == 3
                  ? (a.nt_h ? matrix_sp_xf_a_kernel<LOG2B, NT, true, true> : matrix_sp_xf_a_kernel<LOG2B, NT, false, true>)
                  : (a.nt_h ? matrix_sp_xf_a_kernel<LOG2B, NT, true, false> : matrix_sp_xf_a_kernel<LOG2B, NT, false, false>);
    auto kb = matrix_sp_xf_b_kernel<LOG2B, NT>;
    const long long grid = (long long)a.I + (a.fill == 0 ? (long long)a.PT : 0) + (a.walk ? 1 : 0);
    const size_t lds_a = a.live == 3 ? Gm::lds_a_pair : Gm::lds_a;
    if (hipError_t e = launch_dyn(ka, dim3((unsigned)grid), dim3(NT), lds_a, s, a); e != hipSuccess) return e;
    return launch_dyn(kb, dim3(a.O), dim3(NT), Gm::lds_b, s, a);
}

}  // namespace

hipError_t launch_matrix_sp_xf_chunk(int log2b, const MatrixSpXfArgs &a, hipStream_t s) {
    if (!matrix_chunk_in_range(log2b, a.I, a.O, a.S, a.cur, a.act, a.fill, a.k) || a.N <= 0 || a.PT < a.O || !a.rowptr ||
        !a.col || !a.plan || !a.wg || a.live < 1 || a.live > 3 || a.off < 0 || a.mix.n < 0)
        return hipErrorInvalidValue;
    if (a.mix.approaching && !a.mix.vtab) return hipErrorInvalidValue;
    if ((long long)a.I + (long long)a.PT + 1 > (long long)INT32_MAX) return hipErrorInvalidValue;
    return dispatch_log2<5, kMaxLog2Fused>(log2b, hipErrorInvalidValue,
                                           [&](auto L) { return launch_matrix_sp_xf_t<L()>(a, s); });
}

}  // namespace fftconv
