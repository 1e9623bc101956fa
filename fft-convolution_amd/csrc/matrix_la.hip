// matrix_la.hip -- gfx950 kernels of the MatrixLookaheadConvolver:
// the MatrixConvolver (matrix.hip) with ONE level of far-row windows.  With the
// period Q = kMatrixLaQ an output's rows H[o][i][s] (.) X[i][(current + s) %
// active] are split at Q:
//   near  1 <= s < Q       summed every block (the dense walk over fewer rows)
//   far   Q <= s < active  summed by an ANCHOR once every Q blocks: one walk over
//                          the far rows of output o in launch A of block a
//                          produces the far sums of blocks a .. a + Q - 1
// The far sum of block a + j needs the FDL rows of blocks a + j - s <= a - 1
// only, all of which launch A of block a can read: they are neither the row its
// R2C workgroups write nor rewritten before block a + j runs (DESIGN §4n has
// the index argument).  Output o anchors on blocks t = o (mod Q); the host
// counts blocks and passes {t, tv} by value, every workgroup derives its role
// from them (kernels.hpp: matrix_la_role).  The kernel boundary is the only
// ordering, as in matrix.hip.
//
// HBM layout beyond matrix.hip's:
//   part float2 [O][Pn][B]     near partial sums of one block
//   far  float2 [O][Pf][Q][B]  far partial sums, window row = block % Q
//
// The near walk and the finish kernel are copies of matrix_mac and
// matrix_b_kernel, not templates over them: the dense kernels keep their
// instruction streams (the decision of §4m).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_lds.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "matrix.hpp"
#include "packed.hpp"

namespace fftconv {
namespace {

constexpr int Q = kMatrixLaQ;

template <int LOG2B, int NT>
struct LaGeo {
    using Gm = MGeo<LOG2B, NT>;
    static_assert(Gm::SPT == 1, "one 16-byte slot per thread");
    // the anchor's group reduction: Q accumulators of every thread
    static constexpr size_t red_bytes = Gm::G > 1 ? (size_t)Q * NT * sizeof(float4) : 0;
    static constexpr size_t lds_a = Gm::lds_a > red_bytes ? Gm::lds_a : red_bytes;
};

// Near role of launch A, workgroup = (output o, near part p): matrix_mac over
// the rows 1 <= s < min(Q, active), flattened i-major as r = i * nm1 + s - 1.
template <int LOG2B, int NT, bool NTL>
__device__ __forceinline__ void matrix_la_near(const MatrixArgs &a, int o, int p, unsigned char *smem) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int F = Gm::F, G = Gm::G, SPT = Gm::SPT, U = Gm::U;
    const int tid = threadIdx.x;
    const int f0 = G > 1 ? tid % F : tid;
    const int g = G > 1 ? tid / F : 0;
    const int act = a.act, nm1 = (act < Q ? act : Q) - 1;
    const long long R = (long long)a.I * nm1;
    const long long r0 = (long long)p * a.rpp;
    const long long r1 = r0 + a.rpp < R ? r0 + a.rpp : R;
    DBG_CHECK(o >= 0 && o < a.O && p >= 0 && p < a.P, 59, o, p, a.O, a.P);  // (site 59: a near part past `part`)
    const int cm = a.cur % act;  // (current may exceed active after an update, :248)
    const float4 *H4 = reinterpret_cast<const float4 *>(a.H) + (size_t)o * a.I * a.S * F;
    const float4 *X4 = reinterpret_cast<const float4 *>(a.X);

    Acc2 acc[SPT];
#pragma unroll
    for (int s = 0; s < SPT; ++s) acc[s].zero();
    long long r = r0 + g;
    int i = 0, s = 1;
    if (nm1 > 0) {
        i = (int)(r / nm1);
        s = 1 + (int)(r % nm1);
    }
    auto advance = [&]() {
        r += G;
        s += G;
        while (s > nm1) {
            s -= nm1;
            ++i;
        }
    };
    auto hrow = [&]() {
        DBG_CHECK(i >= 0 && i < a.I && s >= 1 && s < a.S, 58, i, s, a.I, a.S);  // (site 58: a near row past H / X)
        return H4 + ((size_t)i * a.S + s) * F + f0;
    };
    auto xrow = [&]() {
        int xi = cm + s;
        if (xi >= act) xi -= act;
        return X4 + ((size_t)i * a.S + xi) * F + f0;
    };
    while (r + (long long)(U - 1) * G < r1) {
        float4 hv[U][SPT], xv[U][SPT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float4 *hp = hrow(), *xp = xrow();
#pragma unroll
            for (int q = 0; q < SPT; ++q) {
                hv[u][q] = ld4<NTL>(hp + q * NT);
                xv[u][q] = ld4<false>(xp + q * NT);
            }
            advance();
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < SPT; ++q) acc[q].mac(hv[u][q], xv[u][q]);
    }
    while (r < r1) {
        const float4 *hp = hrow(), *xp = xrow();
#pragma unroll
        for (int q = 0; q < SPT; ++q) acc[q].mac(ld4<NTL>(hp + q * NT), ld4<false>(xp + q * NT));
        advance();
    }

    float4 *dst = reinterpret_cast<float4 *>(a.part) + ((size_t)o * a.P + p) * F;
    if constexpr (G > 1) {
        float4 *red = reinterpret_cast<float4 *>(smem);
        red[g * F + f0] = acc[0].get(f0);
        __syncthreads();
        if (tid < F) {
            float4 v = red[f0];
#pragma unroll
            for (int q = 1; q < G; ++q) v = vadd(v, red[q * F + f0]);
            dst[f0] = v;
        }
    } else {
#pragma unroll
        for (int q = 0; q < SPT; ++q) dst[f0 + q * NT] = acc[q].get(f0 + q * NT);
    }
}

// Far role of launch A, workgroup = (output o, far part p), window length W:
// the rows (i, s), Q <= s < active, flattened i-major as r = i * (active - Q) +
// s - Q; part p holds rows [p * rppf, (p + 1) * rppf), group g of the workgroup
// the CONTIGUOUS rows [g * rpg, (g + 1) * rpg) of the part in ascending order,
// the groups are added in ascending g.  Accumulator j < W is the sum of block t
// + j: row (i, s) meets X[i][(current - j + s) % active], the FDL row that block
// t + j finds at (its current + s) % active.  The W rows X[i][current + s - W +
// 1 .. current + s] of a step slide by one row per step, so a step loads one H
// row and one X row for W MACs.  W = 1 is the plain far sum of block t; W = Q
// the anchor.  Accumulator j visits the rows in the order, and through the same
// Acc2::mac, as the W = 1 walk of block t + j: the same bits.
// Partial sums go to window row (t + j) % Q of far[o][p].
template <int LOG2B, int NT, bool NTL, int W>
__device__ __forceinline__ void matrix_la_far(const MatrixLaArgs &la, int o, int p, unsigned char *smem) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int F = Gm::F, G = Gm::G;
    constexpr int UB = 8;  // rows in flight (a multiple of the slide of one row per step)
    const MatrixArgs &a = la.m;
    const int tid = threadIdx.x;
    const int f0 = G > 1 ? tid % F : tid;
    const int g = G > 1 ? tid / F : 0;
    const int act = a.act, nf = act - Q;  // far rows per input, > 0
    const long long R = (long long)a.I * nf;
    const long long r0 = (long long)p * la.rppf;
    const long long r1 = r0 + la.rppf < R ? r0 + la.rppf : R;
    const int rpg = (la.rppf + G - 1) / G;
    const long long q0 = r0 + (long long)g * rpg;
    const long long q1 = q0 + rpg < r1 ? q0 + rpg : r1;
    DBG_CHECK(o >= 0 && o < a.O && p >= 0 && p < la.Pf, 61, o, p, a.O, la.Pf);  // (site 61: a window row past `far`)
    const int cm = a.cur % act;  // (W > 1 runs only while current < active)
    const float4 *H4 = reinterpret_cast<const float4 *>(a.H) + (size_t)o * a.I * a.S * F + f0;
    const float4 *X4 = reinterpret_cast<const float4 *>(a.X) + f0;

    Acc2 acc[W];
#pragma unroll
    for (int j = 0; j < W; ++j) acc[j].zero();
    long long r = q0;
    while (r < q1) {  // one input per turn
        const int i = (int)(r / nf);
        const int s0 = Q + (int)(r % nf);
        const long long left = q1 - r;
        const int len = left < (long long)(act - s0) ? (int)left : act - s0;
        DBG_CHECK(i >= 0 && i < a.I && s0 >= Q && s0 + len <= a.S, 60, i, s0, len, a.S);  // (site 60: a far row past H / X)
        const float4 *Hp = H4 + ((size_t)i * a.S + s0) * F;
        const float4 *Xi = X4 + (size_t)i * a.S * F;
        auto xrow = [&](int e) {  // FDL row of block t - e
            int xi = cm + e;
            if (xi >= act) xi -= act;
            DBG_CHECK(e >= 1 && xi >= 0 && xi < act, 62, e, xi, act, cm);  // (site 62: a ring index >= active)
            return Xi + (size_t)xi * F;
        };
        // v[m] = X row of step n - (W - 1) + m: the W - 1 rows before the
        // batch, then the batch's own
        float4 v[UB + W - 1];
#pragma unroll
        for (int k = 0; k < UB + W - 1; ++k) v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < W - 1; ++k) v[k] = ld4<false>(xrow(s0 - (W - 1) + k));
        for (int n = 0; n < len; n += UB) {
            float4 hv[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                if (n + u < len) {
                    hv[u] = ld4<NTL>(Hp + (size_t)(n + u) * F);
                    v[W - 1 + u] = ld4<false>(xrow(s0 + n + u));
                }
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                if (n + u < len) {
#pragma unroll
                    for (int j = 0; j < W; ++j) acc[j].mac(hv[u], v[W - 1 + u - j]);
                }
            }
#pragma unroll
            for (int k = 0; k < W - 1; ++k) v[k] = v[k + UB];
        }
        r += len;
    }

    const int slot0 = (int)(la.t % Q);
    float4 *dst = reinterpret_cast<float4 *>(la.far) + ((size_t)o * la.Pf + p) * Q * F;
    if constexpr (G > 1) {
        float4 *red = reinterpret_cast<float4 *>(smem);  // [W][G][F]
#pragma unroll
        for (int j = 0; j < W; ++j) red[(j * G + g) * F + f0] = acc[j].get(f0);
        __syncthreads();
        for (int idx = tid; idx < W * F; idx += NT) {
            const int j = idx / F, f = idx % F;
            float4 s = red[(j * G) * F + f];
#pragma unroll
            for (int q = 1; q < G; ++q) s = vadd(s, red[(j * G + q) * F + f]);
            dst[(size_t)((slot0 + j) % Q) * F + f] = s;
        }
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) dst[(size_t)((slot0 + j) % Q) * F + f0] = acc[j].get(f0);
    }
}

// Launch A: blocks [0, I) are the R2C workgroups; for a chunk that starts a
// block, blocks I + o * Pn + p the near workgroups, then the far workgroups
// n * Pf + p: n counts the anchoring outputs t % Q + n * Q while every other
// output has a window (matrix_la_steady), else n = o and an output that needs
// nothing leaves at once.
template <int LOG2B, int NT, bool NTL>
__global__ __launch_bounds__(NT) void matrix_la_a_kernel(MatrixLaArgs la) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MatrixArgs &a = la.m;
    const int b = blockIdx.x;
    if (b < a.I) {
        matrix_r2c<LOG2B, NT>(a, b, smem);
        return;
    }
    const int m = b - a.I;
    const int nn = a.O * a.P;
    if (m < nn) {
        matrix_la_near<LOG2B, NT, NTL>(a, m / a.P, m % a.P, smem);
        return;
    }
    const int mf = m - nn;
    const int n = mf / la.Pf, p = mf % la.Pf;
    const int o = matrix_la_steady(la.t, la.tv) ? (int)(la.t % Q) + n * Q : n;
    const int role = matrix_la_role(la.t, la.tv, o);
    if (role == 1)
        matrix_la_far<LOG2B, NT, NTL, Q>(la, o, p, smem);
    else if (role == 2)
        matrix_la_far<LOG2B, NT, NTL, 1>(la, o, p, smem);
}

// Launch B, workgroup = output o: matrix_b_kernel with pre = near + far, near =
// part[o][0] + part[o][1] + ..., far = the Pf parts of window row t % Q in
// ascending order (no far term when Pf = 0).
template <int LOG2B, int NT>
__global__ __launch_bounds__(NT) void matrix_la_b_kernel(MatrixLaArgs la) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int B = Gm::B, F = Gm::F, SPT = Gm::SPT;
    constexpr int UB = SPT == 1 ? 16 : (SPT == 2 ? 8 : 4);  // terms in flight per slot
    constexpr float invN = 1.0f / (float)(2 * B);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MatrixArgs &a = la.m;
    float2 *bufA = reinterpret_cast<float2 *>(smem);
    float2 *bufB = bufA + B;
    const int tid = threadIdx.x;
    const int o = blockIdx.x;
    const int fill = a.fill, k = a.k;
    const bool complete = fill + k == B;
    float4 *pre4 = reinterpret_cast<float4 *>(a.pre) + (size_t)o * F;
    const float4 *part4 = reinterpret_cast<const float4 *>(a.part) + (size_t)o * a.P * F;
    const float4 *far4 =
        reinterpret_cast<const float4 *>(la.far) + ((size_t)o * la.Pf * Q + (size_t)(la.t % Q)) * F;
    const float4 *H4 = reinterpret_cast<const float4 *>(a.H) + (size_t)o * a.I * a.S * F;
    const float4 *X4 = reinterpret_cast<const float4 *>(a.X) + (size_t)a.cur * F;
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
        const int f = tid + q * NT;
        if (f < F) {
            // (every sum strictly in ascending order; the loads of UB terms are
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
                if (la.Pf > 0) {
                    float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
                    for (int p = 0; p < la.Pf; p += UB) {
                        float4 t[UB];
#pragma unroll
                        for (int u = 0; u < UB; ++u)
                            if (p + u < la.Pf) t[u] = far4[(size_t)(p + u) * Q * F + f];
#pragma unroll
                        for (int u = 0; u < UB; ++u)
                            if (p + u < la.Pf) w = p + u == 0 ? t[u] : vadd(w, t[u]);
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
    float *outc = a.out + (long long)o * a.out_stride;
    float *ovc = a.ovl + (size_t)o * B;
    for (int j = tid; j < k; j += NT) outc[j] = y[fill + j] * invN + ovc[fill + j];
    if (complete) {
        __syncthreads();  // (every overlap read above is done)
        for (int j = tid; j < B; j += NT) ovc[j] = y[B + j] * invN;
    }
}

template <int LOG2B>
hipError_t launch_matrix_la_t(const MatrixLaArgs &la, hipStream_t s) {
    constexpr int NT = matrix_nt(LOG2B);
    using Gm = MGeo<LOG2B, NT>;
    using Lg = LaGeo<LOG2B, NT>;
    const MatrixArgs &a = la.m;
    auto ka = a.nt_h ? matrix_la_a_kernel<LOG2B, NT, true> : matrix_la_a_kernel<LOG2B, NT, false>;
    auto kb = matrix_la_b_kernel<LOG2B, NT>;
    long long grid = a.I;
    if (a.fill == 0) grid += (long long)a.O * a.P + (long long)matrix_la_far_outputs(la.t, la.tv, a.O) * la.Pf;
    if (hipError_t e = launch_dyn(ka, dim3((unsigned)grid), dim3(NT), Lg::lds_a, s, la); e != hipSuccess) return e;
    return launch_dyn(kb, dim3(a.O), dim3(NT), Gm::lds_b, s, la);
}

}  // namespace

hipError_t launch_matrix_la_chunk(int log2b, const MatrixLaArgs &la, hipStream_t s) {
    const MatrixArgs &a = la.m;
    if (a.I <= 0 || a.O <= 0 || a.k <= 0 || a.act <= 0 || a.P <= 0 || a.fill < 0 || a.fill + a.k > (1 << log2b) ||
        a.cur < 0 || a.cur >= a.S || a.act > a.S)
        return hipErrorInvalidValue;
    if (la.t < 0 || la.tv < 0 || la.Pf < 0 || la.Pf > 64 || (la.Pf > 0) != (a.act > kMatrixLaQ))
        return hipErrorInvalidValue;
    if (la.Pf > 0 && (la.rppf <= 0 || (long long)la.rppf * la.Pf < (long long)a.I * (a.act - kMatrixLaQ) || !la.far))
        return hipErrorInvalidValue;
    // an anchor reads the FDL rows of Q future blocks: only while current < active
    if (la.Pf > 0 && la.tv <= la.t && a.cur >= a.act) return hipErrorInvalidValue;
    if ((long long)a.I + (long long)a.O * (a.P + la.Pf) > (long long)INT32_MAX) return hipErrorInvalidValue;
    return dispatch_log2<5, kMatrixLaMaxLog2B>(log2b, hipErrorInvalidValue,
                                               [&](auto L) { return launch_matrix_la_t<L()>(la, s); });
}

}  // namespace fftconv
