// matrix_la_xf.hip -- gfx950 kernels of the MatrixLookaheadCrossfadeConvolver
// (DESIGN §4t): the two lookahead matrices A and B of a crossfaded handle, while
// they are in step, in the lookahead matrix's two launches per chunk.
//
//   launch A  [0, I)          one R2C per input, the row written to X_A and X_B,
//                             both input buffers maintained
//             I + o*Pn + p    the near walk of (output o, part p), for a chunk
//                             that starts a block: on the live convolver's H, or
//                             -- both live -- one pass with every X row loaded
//                             once for H_A and H_B
//             then per live convolver c (A first) its far workgroups n*Pf + p,
//                             as matrix_la_a_kernel's, from that convolver's own
//                             tv: anchor, full sum or nothing
//             last            (first chunk of a call inside a fade) one lane walks
//                             mix_value into the call's device table
//   launch B  o               per live convolver matrix_la_b_kernel's finish
//                             (near parts, the window row's far parts, near +
//                             far, the row-0 terms, C2R, overlap-add, overlap /
//                             pre kept), then the mix as matrix_xf_b_kernel
//
// Each convolver's arithmetic is the lookahead matrix's (matrix.hpp,
// matrix_la.hip): the same Pn / Pf rules, rows per part, row-group order and
// ascending adds, so a fused chunk computes the bits the two lookahead chunks
// and crossfade_mix_kernel compute.  An idle convolver (the crossfader has
// Reached the other one) gets its delay line and input buffer only: it makes no
// anchor and reads no window, and the host keeps its tv past t.  The kernel
// boundary is the only ordering, as in matrix.hip.
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

constexpr int Q = kMatrixLaQ;

// convolver c of the pair as the plain matrix's arguments (part = the near parts)
__device__ __forceinline__ MatrixArgs la_xf_view(const MatrixLaXfArgs &a, int c) {
    MatrixArgs m;
    m.H = a.H[c]; m.X = a.X[c]; m.ovl = a.ovl[c]; m.ib = a.ib[c]; m.pre = a.pre[c]; m.part = a.part[c];
    m.tw = a.tw; m.in = a.in; m.in_stride = a.in_stride; m.out = a.out; m.out_stride = a.out_stride;
    m.I = a.I; m.O = a.O; m.S = a.S; m.P = a.P; m.rpp = a.rpp;
    m.cur = a.cur; m.act = a.act; m.fill = a.fill; m.k = a.k; m.nt_h = a.nt_h;
    return m;
}

// output o's far rows as a row source: Pf parts of rppf rows, window rows far[o][p]
struct PairFarRows {
    static constexpr bool kListed = false;
    int I, o, p, Pf, rppf;
    __device__ __forceinline__ int count() const { return I; }
    __device__ __forceinline__ size_t first_pair() const { return (size_t)o * I; }
    __device__ __forceinline__ size_t out_row() const { return (size_t)o * Pf + p; }
    __device__ __forceinline__ int rpp(long long) const { return rppf; }
    __device__ __forceinline__ int col(int) const { return 0; }
};

// the launches' dynamic LDS: launch A holds the pair walk's two group
// reductions or one anchor's Q; launch B is matrix_la_b_kernel's
template <int LOG2B, int NT>
struct LxGeo {
    using Gm = MGeo<LOG2B, NT>;
    using Lg = LaGeo<LOG2B, NT>;
    static constexpr size_t lds_a = Gm::lds_a_pair > Lg::lds_a ? Gm::lds_a_pair : Lg::lds_a;
    static constexpr size_t lds_b = Gm::lds_b;
};

// (DBG_CHECK sites: near 82, 83 one convolver live; 84, 85 both; far 86 a far
// workgroup past the launch's, 87 a far row past H / X, 88 a window row past
// `far`, 89 a ring index >= active)
template <int LOG2B, int NT, bool NTL>
__global__ __launch_bounds__(NT) void matrix_la_xf_a_kernel(MatrixLaXfArgs a) {
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
    const int nn = a.O * a.P;
    const int nb = (a.act < Q ? a.act : Q) - 1;
    if (m < nn) {
        if (a.live == 3)
            matrix_row_walk<LOG2B, NT, NTL, 84>(dense_rows(a, m, 85), MacStreamsPair<MatrixLaXfArgs>{a}, nb, smem);
        else {
            const MatrixArgs v = la_xf_view(a, a.live == 1 ? 0 : 1);
            matrix_row_walk<LOG2B, NT, NTL, 82>(dense_rows(v, m, 83), MacStreams{v}, nb, smem);
        }
        return;
    }
    // the far workgroups of A, then those of B
    long long mf = m - nn;
    const long long fa = matrix_la_xf_far_groups(a, 0);
    const int c = mf < fa ? 0 : 1;
    if (c == 1) mf -= fa;
    DBG_CHECK(((a.live >> c) & 1) && mf >= 0 && mf < matrix_la_xf_far_groups(a, c), 86, c, (int)mf, a.live, (int)fa);
    const long long tv = a.tv[c];
    const int n = (int)(mf / a.Pf), p = (int)(mf % a.Pf);
    const int o = matrix_la_steady(a.t, tv) ? (int)(a.t % Q) + n * Q : n;
    DBG_CHECK(o >= 0 && o < a.O && p >= 0 && p < a.Pf, 88, o, p, a.O, a.Pf);
    const int role = matrix_la_role(a.t, tv, o);
    const MatrixArgs v = la_xf_view(a, c);
    const PairFarRows rw{a.I, o, p, a.Pf, a.rppf};
    const FarStreams st{{v}, a.far[c]};
    if (role == 1)
        matrix_far_walk<LOG2B, NT, NTL, Q, 87>(rw, st, a.t, smem);
    else if (role == 2)
        matrix_far_walk<LOG2B, NT, NTL, 1, 87>(rw, st, a.t, smem);
}

// Launch B, workgroup = output o: matrix_la_b_kernel's finish for each live
// convolver in turn (A, then B), and the crossfader's mix of the two samples
// (src/crossfade_convolver.rs:75-77) in B's epilogue.  A's samples wait in `out`
// (thread j writes out[j] in A's pass and reads it back in B's: the same thread,
// the same address).  Only the first mix.n = output_len samples of the call are
// written.
template <int LOG2B, int NT>
__global__ __launch_bounds__(NT) void matrix_la_xf_b_kernel(MatrixLaXfArgs a) {
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
        const float4 *far4 =
            reinterpret_cast<const float4 *>(a.far[c]) + ((size_t)o * a.Pf * Q + (size_t)(a.t % Q)) * F;
        const float4 *H4 = reinterpret_cast<const float4 *>(a.H[c]) + (size_t)o * a.I * a.S * F;
        const float4 *X4 = reinterpret_cast<const float4 *>(a.X[c]) + (size_t)a.cur * F;
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
            const int f = tid + q * NT;
            if (f < F) {
                // (every sum strictly in ascending order, as matrix_la_b_kernel)
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
                    if (a.Pf > 0) {
                        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
                        for (int p = 0; p < a.Pf; p += UB) {
                            float4 t[UB];
#pragma unroll
                            for (int u = 0; u < UB; ++u)
                                if (p + u < a.Pf) t[u] = far4[(size_t)(p + u) * Q * F + f];
#pragma unroll
                            for (int u = 0; u < UB; ++u)
                                if (p + u < a.Pf) w = p + u == 0 ? t[u] : vadd(w, t[u]);
                        }
                        v = vadd(v, w);
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

// the far workgroups of the launch, both convolvers'
inline long long far_groups(const MatrixLaXfArgs &a) {
    return matrix_la_xf_far_groups(a, 0) + matrix_la_xf_far_groups(a, 1);
}

template <int LOG2B>
hipError_t launch_matrix_la_xf_t(const MatrixLaXfArgs &a, hipStream_t s) {
    constexpr int NT = matrix_nt(LOG2B);
    using Lx = LxGeo<LOG2B, NT>;
    auto ka = a.nt_h ? matrix_la_xf_a_kernel<LOG2B, NT, true> : matrix_la_xf_a_kernel<LOG2B, NT, false>;
    auto kb = matrix_la_xf_b_kernel<LOG2B, NT>;
    long long grid = a.I;
    if (a.fill == 0) grid += (long long)a.O * a.P + far_groups(a);
    if (a.walk) ++grid;
    if (hipError_t e = launch_dyn(ka, dim3((unsigned)grid), dim3(NT), Lx::lds_a, s, a); e != hipSuccess) return e;
    return launch_dyn(kb, dim3(a.O), dim3(NT), Lx::lds_b, s, a);
}

}  // namespace

hipError_t launch_matrix_la_xf_chunk(int log2b, const MatrixLaXfArgs &a, hipStream_t s) {
    if (!matrix_chunk_in_range(log2b, a.I, a.O, a.S, a.cur, a.act, a.fill, a.k) || a.P <= 0 || a.live < 1 || a.live > 3 ||
        a.off < 0 || a.mix.n < 0)
        return hipErrorInvalidValue;
    if (a.mix.approaching && !a.mix.vtab) return hipErrorInvalidValue;
    if (a.t < 0 || a.Pf < 0 || a.Pf > 64 || (a.Pf > 0) != (a.act > kMatrixLaQ)) return hipErrorInvalidValue;
    if (a.Pf > 0 && (a.rppf <= 0 || (long long)a.rppf * a.Pf < (long long)a.I * (a.act - kMatrixLaQ)))
        return hipErrorInvalidValue;
    for (int c = 0; c < 2; ++c) {
        if (!((a.live >> c) & 1)) continue;
        if (a.tv[c] < 0 || (a.Pf > 0 && !a.far[c])) return hipErrorInvalidValue;
        // an anchor reads the FDL rows of Q future blocks: only while current < active
        if (a.Pf > 0 && a.tv[c] <= a.t && a.cur >= a.act) return hipErrorInvalidValue;
    }
    if ((long long)a.I + (long long)a.O * a.P + 2ll * a.O * a.Pf + 1 > (long long)INT32_MAX) return hipErrorInvalidValue;
    return dispatch_log2<5, kMatrixLaMaxLog2B>(log2b, hipErrorInvalidValue,
                                               [&](auto L) { return launch_matrix_la_xf_t<L()>(a, s); });
}

}  // namespace fftconv
