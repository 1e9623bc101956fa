// matrix.hip -- gfx950 kernels of the MatrixConvolver:
//   y[o] = sum_i x[i] * h[o][i]        (o < outputs O, i < inputs I)
// as I*O reference FFTConvolver instances (o, i) in lockstep, with ONE
// frequency-domain delay line per input shared by every output, and the
// spectra summed per output before ONE inverse transform.
//
// HBM layout (packed rows: B float2 per row, slot 0 = (DC, Nyquist)):
//   H    float2 [O][I][S][B]  IR spectra, pair o*I + i = channel of the IR transform
//   X    float2 [I][S][B]     one FDL per input
//   ovl  float  [O][B]        summed overlap per output
//   ib   float  [I][B]        input buffer per input (zero past the fill)
//   pre  float2 [O][B]        summed pre_multiplied, kept across partial chunks
//   part float2 [O][P][B]     split-row partial sums of one block
//
// A chunk (the reference's `processing`, src/fft_convolver.rs:221-227: a piece
// of a call inside one block) is two launches on one stream; the host keeps
// {current, active, fill} and passes them by value.  The kernel boundary is the
// only ordering between producers and consumers: launch A's MAC workgroups
// read FDL rows of earlier blocks only, never the row its R2C workgroups write.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_lds.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "matrix.hpp"
#include "packed.hpp"

namespace fftconv {
namespace {

// Launch A: blocks [0, I) are the R2C workgroups, blocks I + o * P + p the MAC
// workgroups (launched only for a chunk that starts a block): the row walk over
// the dense rows 1 <= s < active (sites 50, 51).
template <int LOG2B, int NT, bool NTL>
__global__ __launch_bounds__(NT) void matrix_a_kernel(MatrixArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x;
    if (b < a.I) {
        matrix_r2c<LOG2B, NT>(a, b, smem);
    } else {
        matrix_row_walk<LOG2B, NT, NTL, 50>(dense_rows(a, b - a.I, 51), MacStreams{a}, a.act - 1, smem);
    }
}

// Launch B, workgroup = output o: pre = part[o][0] + part[o][1] + ... (or the
// kept pre[o] when the chunk starts mid-block), conv = pre + sum_i
// X[i][current] (.) H[o][i][0] in ascending i (:256-261 summed over i), one
// C2R with 1/N (:264, :44-46), overlap-add (:270-274), overlap saved when the
// block completes (:283-284), pre[o] kept when it does not.
template <int LOG2B, int NT>
__global__ __launch_bounds__(NT) void matrix_b_kernel(MatrixArgs a) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int B = Gm::B, F = Gm::F, SPT = Gm::SPT;
    constexpr int UB = SPT == 1 ? 16 : (SPT == 2 ? 8 : 4);  // terms in flight per slot
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *bufA = reinterpret_cast<float2 *>(smem);
    float2 *bufB = bufA + B;
    const int tid = threadIdx.x;
    const int o = blockIdx.x;
    const int fill = a.fill, k = a.k;
    const bool complete = fill + k == B;
    float4 *pre4 = reinterpret_cast<float4 *>(a.pre) + (size_t)o * F;
    const float4 *part4 = reinterpret_cast<const float4 *>(a.part) + (size_t)o * a.P * F;
    const float4 *H4 = reinterpret_cast<const float4 *>(a.H) + (size_t)o * a.I * a.S * F;
    const float4 *X4 = reinterpret_cast<const float4 *>(a.X) + (size_t)a.cur * F;
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
        const int f = tid + q * NT;
        if (f < F) {
            // (both sums strictly in ascending order; the loads of UB terms are
            // issued before their adds, so the chain waits once per UB terms)
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (fill == 0) {
                for (int p = 0; p < a.P; p += UB) {
                    float4 t[UB];
#pragma unroll
                    for (int u = 0; u < UB; ++u)
                        if (p + u < a.P) t[u] = part4[(size_t)(p + u) * F + f];
#pragma unroll
                    for (int u = 0; u < UB; ++u)
                        if (p + u < a.P) v = p + u == 0 ? t[u] : vadd(v, t[u]);
                }
            } else {
                v = pre4[f];
            }
            if (!complete) pre4[f] = v;
            for (int i = 0; i < a.I; i += UB / 2) {
                float4 xs[UB / 2], hs[UB / 2];
#pragma unroll
                for (int u = 0; u < UB / 2; ++u) {
                    if (i + u < a.I) {
                        xs[u] = X4[(size_t)(i + u) * a.S * F + f];
                        hs[u] = H4[(size_t)(i + u) * a.S * F + f];
                    }
                }
#pragma unroll
                for (int u = 0; u < UB / 2; ++u)
                    if (i + u < a.I) v = slot_mac(v, xs[u], hs[u], f);
            }
            reinterpret_cast<float4 *>(bufA)[f] = v;
        }
    }
    const float *y = finish_c2r<LOG2B, NT>(bufA, bufB, a.tw);
    float *outc = a.out + (long long)o * a.out_stride;
    float *ovc = a.ovl + (size_t)o * B;
    overlap_add<LOG2B, NT>(y, ovc, fill, k, [&](int j, float v) { outc[j] = v; });
    if (complete) overlap_save<LOG2B, NT>(y, ovc);
}

template <int LOG2B>
hipError_t launch_matrix_t(const MatrixArgs &a, hipStream_t s) {
    constexpr int NT = matrix_nt(LOG2B);
    using Gm = MGeo<LOG2B, NT>;
    auto ka = a.nt_h ? matrix_a_kernel<LOG2B, NT, true> : matrix_a_kernel<LOG2B, NT, false>;
    auto kb = matrix_b_kernel<LOG2B, NT>;
    const long long grid = (long long)a.I + (a.fill == 0 ? (long long)a.O * a.P : 0);
    if (hipError_t e = launch_dyn(ka, dim3((unsigned)grid), dim3(NT), Gm::lds_a, s, a); e != hipSuccess) return e;
    return launch_dyn(kb, dim3(a.O), dim3(NT), Gm::lds_b, s, a);
}

}  // namespace

// P: about 64 rows per part, at most 64 parts -- a function of (inputs,
// active_seg_count) only, never of the outputs or the device, so a matrix
// split by outputs over handles computes the same bits
int matrix_mac_parts(int inputs, int log2b, int seg_count, int active) {
    (void)log2b;
    (void)seg_count;
    return matrix_parts_rule(inputs, active);
}

hipError_t launch_matrix_chunk(int log2b, const MatrixArgs &a, hipStream_t s) {
    if (!matrix_chunk_in_range(log2b, a.I, a.O, a.S, a.cur, a.act, a.fill, a.k) || a.P <= 0) return hipErrorInvalidValue;
    if ((long long)a.I + (long long)a.O * a.P > (long long)INT32_MAX) return hipErrorInvalidValue;
    return dispatch_log2<5, kMaxLog2Fused>(log2b, hipErrorInvalidValue,
                                           [&](auto L) { return launch_matrix_t<L()>(a, s); });
}

}  // namespace fftconv
