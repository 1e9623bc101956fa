// matrix_xf.hip -- gfx950 kernels of the MatrixCrossfadeConvolver:
// the two matrices A and B of a crossfaded handle, while they are in step, in
// the plain matrix's two launches per chunk.
//
//   launch A  [0, I)       one R2C per input, the row written to X_A and X_B,
//                          both input buffers maintained
//             last         (first chunk of a call inside a fade) one lane walks
//                          mix_value into the call's device table
//             I + o*P + p  the MAC of (output o, part p), for a chunk that
//                          starts a block: the row walk on the live convolver's
//                          H, or -- both live -- one pass over the rows with
//                          every X row loaded once for H_A and H_B
//   launch B  o            per live convolver the finish of matrix_b_kernel
//                          (sum of parts or kept pre, + X[cur] (.) H[0], C2R,
//                          overlap-add, overlap / pre kept), then the mix
//
// Each convolver's arithmetic is the plain matrix's (matrix.hpp, matrix.hip):
// the same P rule, rows per part, row-group order and ascending adds, so a
// fused chunk computes the bits the two plain chunks and crossfade_mix_kernel
// compute.  The kernel boundary is the only ordering, as in matrix.hip.
//
// The finish needs no LDS beyond the plain one's two buffers: A's samples wait
// in `out` (thread j writes out[j] in A's pass and reads it back in B's pass --
// the same thread, the same address) and the mix_value walk is a device table
// filled once per call by launch A of the call's first chunk, so every block
// size 32..8192 runs fused.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_lds.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "matrix.hpp"
#include "mix.hpp"
#include "packed.hpp"

namespace fftconv {
namespace {

// convolver c of the pair as the plain matrix's arguments
__device__ __forceinline__ MatrixArgs xf_view(const MatrixXfArgs &a, int c) {
    MatrixArgs m;
    m.H = a.H[c]; m.X = a.X[c]; m.ovl = a.ovl[c]; m.ib = a.ib[c]; m.pre = a.pre[c]; m.part = a.part[c];
    m.tw = a.tw; m.in = a.in; m.in_stride = a.in_stride; m.out = a.out; m.out_stride = a.out_stride;
    m.I = a.I; m.O = a.O; m.S = a.S; m.P = a.P; m.rpp = a.rpp;
    m.cur = a.cur; m.act = a.act; m.fill = a.fill; m.k = a.k; m.nt_h = a.nt_h;
    return m;
}

// the launches' dynamic LDS (launch A's MAC may walk two H streams)
template <int LOG2B, int NT>
struct XGeo {
    using Gm = MGeo<LOG2B, NT>;
    static constexpr size_t lds_a = Gm::lds_a_pair;
    static constexpr size_t lds_b = Gm::fft_bytes;
};

// (DBG_CHECK sites: 50, 51 one convolver live; 52, 53 both)
template <int LOG2B, int NT, bool NTL>
__global__ __launch_bounds__(NT) void matrix_xf_a_kernel(MatrixXfArgs a) {
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
    const int m = b - a.I;
    if (a.live == 3)
        matrix_row_walk<LOG2B, NT, NTL, 52>(dense_rows(a, m, 53), MacStreamsPair<MatrixXfArgs>{a}, a.act - 1, smem);
    else {
        const MatrixArgs v = xf_view(a, a.live == 1 ? 0 : 1);
        matrix_row_walk<LOG2B, NT, NTL, 50>(dense_rows(v, m, 51), MacStreams{v}, v.act - 1, smem);
    }
}

// Launch B, workgroup = output o: matrix_b_kernel's finish for each live
// convolver in turn (A, then B), and the crossfader's mix of the two samples
// (src/crossfade_convolver.rs:75-77) in B's epilogue.  Only the first
// mix.n = output_len samples of the call are written.
template <int LOG2B, int NT>
__global__ __launch_bounds__(NT) void matrix_xf_b_kernel(MatrixXfArgs a) {
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
    float *outc = a.out + (long long)o * a.out_stride;
    const int n_out = a.mix.n - a.off;  // samples of this chunk inside output_len
    for (int c = 0; c < 2; ++c) {
        if (!((a.live >> c) & 1)) continue;  // (uniform over the workgroup)
        float4 *pre4 = reinterpret_cast<float4 *>(a.pre[c]) + (size_t)o * F;
        const float4 *part4 = reinterpret_cast<const float4 *>(a.part[c]) + (size_t)o * a.P * F;
        const float4 *H4 = reinterpret_cast<const float4 *>(a.H[c]) + (size_t)o * a.I * a.S * F;
        const float4 *X4 = reinterpret_cast<const float4 *>(a.X[c]) + (size_t)a.cur * F;
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
            const int f = tid + q * NT;
            if (f < F) {
                // (both sums strictly in ascending order, as matrix_b_kernel)
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
hipError_t launch_matrix_xf_t(const MatrixXfArgs &a, hipStream_t s) {
    constexpr int NT = matrix_nt(LOG2B);
    using Xg = XGeo<LOG2B, NT>;
    auto ka = a.nt_h ? matrix_xf_a_kernel<LOG2B, NT, true> : matrix_xf_a_kernel<LOG2B, NT, false>;
    auto kb = matrix_xf_b_kernel<LOG2B, NT>;
    const long long grid = (long long)a.I + (a.fill == 0 ? (long long)a.O * a.P : 0) + (a.walk ? 1 : 0);
    if (hipError_t e = launch_dyn(ka, dim3((unsigned)grid), dim3(NT), Xg::lds_a, s, a); e != hipSuccess) return e;
    return launch_dyn(kb, dim3(a.O), dim3(NT), Xg::lds_b, s, a);
}

}  // namespace

hipError_t launch_matrix_xf_chunk(int log2b, const MatrixXfArgs &a, hipStream_t s) {
    if (!matrix_chunk_in_range(log2b, a.I, a.O, a.S, a.cur, a.act, a.fill, a.k) || a.P <= 0 || a.live < 1 || a.live > 3 ||
        a.off < 0 || a.mix.n < 0)
        return hipErrorInvalidValue;
    if (a.mix.approaching && !a.mix.vtab) return hipErrorInvalidValue;
    if ((long long)a.I + (long long)a.O * a.P + 1 > (long long)INT32_MAX) return hipErrorInvalidValue;
    return dispatch_log2<5, kMaxLog2Fused>(log2b, hipErrorInvalidValue,
                                           [&](auto L) { return launch_matrix_xf_t<L()>(a, s); });
}

}  // namespace fftconv
