// matrix_xf.hip -- gfx950 kernels of the MatrixCrossfadeConvolver:
// the two matrices A and B of a crossfaded handle, while they are in step, in
// the plain matrix's two launches per chunk.
//
//   launch A  [0, I)       one R2C per input, the row written to X_A and X_B,
//                          both input buffers maintained
//             last         (first chunk of a call inside a fade) one lane walks
//                          mix_value into the call's device table
//             I + o*P + p  the MAC of (output o, part p), for a chunk that
//                          starts a block: matrix_mac on the live convolver's H,
//                          or -- both live -- one pass over the rows with every
//                          X row loaded once for H_A and H_B
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

// rows in flight of the two-H MAC (three streams per row instead of two: the
// plain U still compiles without scratch), and the launches' dynamic LDS
template <int LOG2B, int NT>
struct XGeo {
    using Gm = MGeo<LOG2B, NT>;
    static constexpr int U = Gm::U;
    static constexpr size_t lds_a = Gm::fft_bytes > 2 * Gm::red_bytes ? Gm::fft_bytes : 2 * Gm::red_bytes;
    static constexpr size_t lds_b = Gm::fft_bytes;
};

// matrix_r2c for both convolvers: ib_A == ib_B and the row is the same, so one
// transform, every store twice.
template <int LOG2B, int NT>
__device__ __forceinline__ void xf_r2c(const MatrixXfArgs &a, int i, unsigned char *smem) {
    constexpr int B = 1 << LOG2B;
    float2 *bufA = reinterpret_cast<float2 *>(smem);
    float2 *bufB = bufA + B;
    const int tid = threadIdx.x;
    const int fill = a.fill, k = a.k;
    const float *inc = a.in + (long long)i * a.in_stride;
    float *ib0 = a.ib[0] + (size_t)i * B, *ib1 = a.ib[1] + (size_t)i * B;
    auto sample = [&](int j) -> float {
        if (j < fill) return ib0[j];
        if (j < fill + k) return inc[j - fill];
        return 0.f;
    };
    for (int m = tid; m < B; m += NT) {
        float2 z = make_float2(0.f, 0.f);
        if (2 * m < B) {
            z.x = sample(2 * m);
            z.y = sample(2 * m + 1);
        }
        bufA[m] = z;
    }
    __syncthreads();  // (every read of ib[i] is done)
    if (fill + k == B) {
        if (fill > 0)
            for (int j = tid; j < B; j += NT) ib0[j] = ib1[j] = 0.f;
    } else {
        for (int j = tid; j < k; j += NT) ib0[fill + j] = ib1[fill + j] = inc[j];
    }
    const float2 *Z = lds_cfft<LOG2B, NT, false>(bufA, bufB, a.tw);
    const size_t at = ((size_t)i * a.S + a.cur) * B;
    float2 *row0 = a.X[0] + at, *row1 = a.X[1] + at;
    for (int m = tid; m < B; m += NT) row0[m] = row1[m] = real_post<LOG2B, NT>(Z, m, a.tw);
}

// matrix_mac for both convolvers in one pass over the rows: the walk, the
// part bounds and each accumulator's order of additions are matrix_mac's; row
// X[i][..] is loaded once (from X_A) and multiplied with H_A and H_B.
template <int LOG2B, int NT, bool NTL>
__device__ __forceinline__ void xf_mac_pair(const MatrixXfArgs &a, int o, int p, unsigned char *smem) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int F = Gm::F, G = Gm::G, SPT = Gm::SPT, U = XGeo<LOG2B, NT>::U;
    const int tid = threadIdx.x;
    const int f0 = G > 1 ? tid % F : tid;
    const int g = G > 1 ? tid / F : 0;
    const int act = a.act, am1 = act - 1;
    const long long R = (long long)a.I * am1;
    const long long r0 = (long long)p * a.rpp;
    const long long r1 = r0 + a.rpp < R ? r0 + a.rpp : R;
    DBG_CHECK(o >= 0 && o < a.O && p >= 0 && p < a.P, 53, o, p, a.O, a.P);  // (site 53: a part past `part`)
    const int cm = a.cur % act;
    const size_t hbase = (size_t)o * a.I * a.S * F;
    const float4 *HA4 = reinterpret_cast<const float4 *>(a.H[0]) + hbase;
    const float4 *HB4 = reinterpret_cast<const float4 *>(a.H[1]) + hbase;
    const float4 *X4 = reinterpret_cast<const float4 *>(a.X[0]);

    Acc2 accA[SPT], accB[SPT];
#pragma unroll
    for (int s = 0; s < SPT; ++s) {
        accA[s].zero();
        accB[s].zero();
    }
    long long r = r0 + g;
    int i = 0, s = 1;
    if (am1 > 0) {
        i = (int)(r / am1);
        s = 1 + (int)(r % am1);
    }
    auto advance = [&]() {
        r += G;
        s += G;
        while (s > am1) {
            s -= am1;
            ++i;
        }
    };
    auto hoff = [&]() {
        DBG_CHECK(i >= 0 && i < a.I && s >= 1 && s < a.S, 52, i, s, a.I, a.S);  // (site 52: a MAC row past H / X)
        return ((size_t)i * a.S + s) * F + f0;
    };
    auto xrow = [&]() {
        int xi = cm + s;
        if (xi >= act) xi -= act;
        return X4 + ((size_t)i * a.S + xi) * F + f0;
    };
    while (r + (long long)(U - 1) * G < r1) {
        float4 ha[U][SPT], hb[U][SPT], xv[U][SPT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t h = hoff();
            const float4 *xp = xrow();
#pragma unroll
            for (int q = 0; q < SPT; ++q) {
                ha[u][q] = ld4<NTL>(HA4 + h + q * NT);
                hb[u][q] = ld4<NTL>(HB4 + h + q * NT);
                xv[u][q] = ld4<false>(xp + q * NT);
            }
            advance();
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < SPT; ++q) {
                accA[q].mac(ha[u][q], xv[u][q]);
                accB[q].mac(hb[u][q], xv[u][q]);
            }
    }
    while (r < r1) {
        const size_t h = hoff();
        const float4 *xp = xrow();
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
            const float4 x = ld4<false>(xp + q * NT);
            accA[q].mac(ld4<NTL>(HA4 + h + q * NT), x);
            accB[q].mac(ld4<NTL>(HB4 + h + q * NT), x);
        }
        advance();
    }

    const size_t pbase = ((size_t)o * a.P + p) * F;
    float4 *dstA = reinterpret_cast<float4 *>(a.part[0]) + pbase;
    float4 *dstB = reinterpret_cast<float4 *>(a.part[1]) + pbase;
    if constexpr (G > 1) {
        float4 *redA = reinterpret_cast<float4 *>(smem);
        float4 *redB = redA + NT;
        redA[g * F + f0] = accA[0].get(f0);
        redB[g * F + f0] = accB[0].get(f0);
        __syncthreads();
        if (tid < F) {
            float4 v = redA[f0], w = redB[f0];
#pragma unroll
            for (int q = 1; q < G; ++q) {
                v = vadd(v, redA[q * F + f0]);
                w = vadd(w, redB[q * F + f0]);
            }
            dstA[f0] = v;
            dstB[f0] = w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
            dstA[f0 + q * NT] = accA[q].get(f0 + q * NT);
            dstB[f0 + q * NT] = accB[q].get(f0 + q * NT);
        }
    }
}

template <int LOG2B, int NT, bool NTL>
__global__ __launch_bounds__(NT) void matrix_xf_a_kernel(MatrixXfArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x;
    if (a.walk && b == (int)gridDim.x - 1) {  // launch B and the call's later chunks read the table
        if (threadIdx.x == 0) mix_walk(a.mix, a.walk);
        return;
    }
    if (b < a.I) {
        xf_r2c<LOG2B, NT>(a, b, smem);
        return;
    }
    const int m = b - a.I;
    if (a.live == 3)
        xf_mac_pair<LOG2B, NT, NTL>(a, m / a.P, m % a.P, smem);
    else
        matrix_mac<LOG2B, NT, NTL>(xf_view(a, a.live == 1 ? 0 : 1), m / a.P, m % a.P, smem);
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
    if (a.I <= 0 || a.O <= 0 || a.k <= 0 || a.act <= 0 || a.P <= 0 || a.fill < 0 || a.fill + a.k > (1 << log2b) ||
        a.cur < 0 || a.cur >= a.S || a.act > a.S || a.live < 1 || a.live > 3 || a.off < 0 || a.mix.n < 0)
        return hipErrorInvalidValue;
    if (a.mix.approaching && !a.mix.vtab) return hipErrorInvalidValue;
    if ((long long)a.I + (long long)a.O * a.P + 1 > (long long)INT32_MAX) return hipErrorInvalidValue;
    return dispatch_log2<5, kMaxLog2Fused>(log2b, hipErrorInvalidValue,
                                           [&](auto L) { return launch_matrix_xf_t<L()>(a, s); });
}

}  // namespace fftconv
