// matrix_ts.hip -- gfx950 kernels of the MatrixTwoStageConvolver:
// the head and tail0 matrices of a two-stage handle, at an aligned call (a
// whole head block on a block boundary of the tail period), in the plain
// matrix's two launches.
//
//   launch A  [0, I)       one R2C per input, the row written to X_head and
//                          X_tail0, the block copied to tail_input[i][fill..]
//                          (src/fft_convolver.rs:459-461) from the registers
//                          that feed the transform
//             I + o*P + p  the MAC of (output o, part p) for both responses in
//                          one pass over the rows (the row walk over two H
//                          streams): every X row loaded once, from the head's
//                          delay line
//   launch B  (o, 0)       the head's finish (sum of parts, + X[cur] (.) H[0],
//                          C2R, overlap-add) with the sub-chunk sums of
//                          :438-454 in its epilogue:
//                            out[j] = ((y / N + ovl) + tail_precalculated0[pos + j])
//                                     + tail_precalculated[pos + j]
//             (o, 1)       tail0's finish into tail_output0[o][fill..]
//                          (:464-472), with its own overlap
//
// Each matrix's arithmetic is the plain matrix's (matrix.hpp, matrix.hip): the
// same P rule, rows per part, row-group order and ascending adds, and the two
// sums are added in twostage order, so an aligned call computes the bits that
// head.process, the sub-chunk kernel below and tail0.process compute.  Nothing
// in a launch reads what that launch writes: tail_output0 and
// tail_precalculated0 are different buffers until the host swaps them after
// the launch, and the kernel boundary is the only ordering, as in matrix.hip.
// A finish workgroup needs the plain one's two LDS buffers, no more.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_lds.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "matrix.hpp"
#include "packed.hpp"

namespace fftconv {
namespace {

// (DBG_CHECK sites 52, 53: the two-stream walk's)
template <int LOG2B, int NT, bool NTL>
__global__ __launch_bounds__(NT) void matrix_ts_a_kernel(MatrixTsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x;
    if (b < a.I) {
        matrix_r2c_block<LOG2B, NT>(a, b, smem);
        return;
    }
    matrix_row_walk<LOG2B, NT, NTL, 52>(dense_rows(a, b - a.I, 53), MacStreamsPair<MatrixTsArgs>{a}, a.act - 1, smem);
}

// Launch B, workgroup = (output o, matrix c): matrix_b_kernel's finish of a
// whole block (fill 0, k = B), c = 0 for the head, c = 1 for tail0, with the
// two-stage epilogue (ts_epilogue, matrix.hpp).  The two finishes touch disjoint buffers, so they run side by side: the finish is a
// latency chain (I + P dependent loads, two transforms), and one workgroup
// running both in turn took 12.6 us (32 x 32, B 64) / 20.2 us (64 x 2, B 256)
// per block against 8.7 / 13.4 us for the plain finish (profiles/matrix_ts).
template <int LOG2B, int NT>
__global__ __launch_bounds__(NT) void matrix_ts_b_kernel(MatrixTsArgs a) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int B = Gm::B, F = Gm::F, SPT = Gm::SPT;
    constexpr int UB = SPT == 1 ? 16 : (SPT == 2 ? 8 : 4);  // terms in flight per slot
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *bufA = reinterpret_cast<float2 *>(smem);
    float2 *bufB = bufA + B;
    const int tid = threadIdx.x;
    const int o = blockIdx.x;
    const int c = blockIdx.y;  // (uniform over the workgroup)
    const float4 *part4 = reinterpret_cast<const float4 *>(a.part[c]) + (size_t)o * a.P * F;
    const float4 *H4 = reinterpret_cast<const float4 *>(a.H[c]) + (size_t)o * a.I * a.S * F;
    const float4 *X4 = reinterpret_cast<const float4 *>(a.X[c]) + (size_t)a.cur * F;
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
        const int f = tid + q * NT;
        if (f < F) {
            // (both sums strictly in ascending order, as matrix_b_kernel)
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int p = 0; p < a.P; p += UB) {
                float4 t[UB];
#pragma unroll
                for (int u = 0; u < UB; ++u)
                    if (p + u < a.P) t[u] = part4[(size_t)(p + u) * F + f];
#pragma unroll
                for (int u = 0; u < UB; ++u)
                    if (p + u < a.P) v = p + u == 0 ? t[u] : vadd(v, t[u]);
            }
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
    ts_epilogue<LOG2B, NT>(a, o, c, y);
}

// the sub-chunk of the composition path: blocks [0, O) the outputs' sums,
// blocks [O, O + I) the inputs' copies
__global__ void matrix_ts_accum_kernel(MatrixTsAccumArgs a) {
    const int b = blockIdx.x;
    if (b < a.O) {
        if (!a.p0 && !a.p1) return;
        float *o = a.out + (long long)b * a.out_stride + a.sb;
        const float *p0 = a.p0 ? a.p0 + (long long)b * a.T + a.pos : nullptr;
        const float *p1 = a.p1 ? a.p1 + (long long)b * a.T + a.pos : nullptr;
        for (int j = threadIdx.x; j < a.cnt; j += blockDim.x) {
            float v = o[j];
            if (p0) v += p0[j];
            if (p1) v += p1[j];
            o[j] = v;
        }
    } else {
        const int i = b - a.O;
        const float *x = a.in + (long long)i * a.in_stride + a.sb;
        float *ti = a.tail_input + (long long)i * a.T + a.fill;
        for (int j = threadIdx.x; j < a.cnt; j += blockDim.x) ti[j] = x[j];
    }
}

template <int LOG2B>
hipError_t launch_matrix_ts_t(const MatrixTsArgs &a, hipStream_t s) {
    constexpr int NT = matrix_nt(LOG2B);
    using Gm = MGeo<LOG2B, NT>;
    auto ka = a.nt_h ? matrix_ts_a_kernel<LOG2B, NT, true> : matrix_ts_a_kernel<LOG2B, NT, false>;
    auto kb = matrix_ts_b_kernel<LOG2B, NT>;
    const long long grid = (long long)a.I + (long long)a.O * a.P;
    if (hipError_t e = launch_dyn(ka, dim3((unsigned)grid), dim3(NT), Gm::lds_a_pair, s, a); e != hipSuccess) return e;
    return launch_dyn(kb, dim3(a.O, 2), dim3(NT), Gm::lds_b, s, a);
}

}  // namespace

hipError_t launch_matrix_ts_block(int log2b, const MatrixTsArgs &a, hipStream_t s) {
    if (!matrix_chunk_in_range(log2b, a.I, a.O, a.S, a.cur, a.act, 0, 1 << log2b) || a.P <= 0 || a.T < (1LL << log2b) ||
        !a.tin || !a.tout0 || !a.p0)
        return hipErrorInvalidValue;
    if ((long long)a.I + (long long)a.O * a.P > (long long)INT32_MAX) return hipErrorInvalidValue;
    return dispatch_log2<5, kMaxLog2Fused>(log2b, hipErrorInvalidValue,
                                           [&](auto L) { return launch_matrix_ts_t<L()>(a, s); });
}

hipError_t launch_matrix_ts_accum(const MatrixTsAccumArgs &a, hipStream_t s) {
    if (a.I <= 0 || a.O <= 0 || a.cnt <= 0) return hipSuccess;
    if (a.pos < 0 || a.fill < 0 || a.sb < 0 || (long long)a.pos + a.cnt > a.T || (long long)a.fill + a.cnt > a.T ||
        (long long)a.I + a.O > (long long)INT32_MAX)
        return hipErrorInvalidValue;
    return launch_dyn(matrix_ts_accum_kernel, dim3((unsigned)(a.I + a.O)), dim3(a.cnt >= 256 ? 256 : 64), 0, s, a);
}

}  // namespace fftconv
