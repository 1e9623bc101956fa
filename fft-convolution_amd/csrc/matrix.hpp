// matrix.hpp -- the device roles of the MatrixConvolver's launch A and its
// geometry, shared by matrix.hip, matrix_xf.hip (the crossfaded matrix) and
// matrix_ts.hip (the two-stage matrix): one definition, so every family
// computes the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_lds.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "packed.hpp"

namespace fftconv {

// (tests/matrix_paths.py mirrors these constants, matrix_nt, UB and the P rule
// to prove which loops each test shape runs: change them together)
template <int LOG2B, int NT>
struct MGeo {
    static constexpr int B = 1 << LOG2B;
    static constexpr int F = B / 2;                     // 16-byte slots per row
    static constexpr int G = F >= NT ? 1 : NT / F;      // row groups of a MAC workgroup
    static constexpr int SPT = F >= NT ? F / NT : 1;    // slots per thread
    static constexpr int U = SPT == 1 ? 8 : (SPT == 2 ? 4 : (SPT == 4 ? 2 : 1));  // rows in flight
    static constexpr size_t fft_bytes = 2 * (size_t)B * sizeof(float2);
    static constexpr size_t red_bytes = G > 1 ? (size_t)NT * sizeof(float4) : 0;
    static constexpr size_t lds_a = fft_bytes > red_bytes ? fft_bytes : red_bytes;
    static constexpr size_t lds_b = fft_bytes;
    static constexpr size_t lds_a_pair = fft_bytes > 2 * red_bytes ? fft_bytes : 2 * red_bytes;  // (matrix_mac_pair)
};

// R2C role of launch A, workgroup = input i: append the chunk to ib[i],
// transform the zero-padded buffer into X[i][current] (:229-241), clear ib[i]
// when the block completes (:280).
template <int LOG2B, int NT>
__device__ __forceinline__ void matrix_r2c(const MatrixArgs &a, int i, unsigned char *smem) {
    constexpr int B = 1 << LOG2B;
    float2 *bufA = reinterpret_cast<float2 *>(smem);
    float2 *bufB = bufA + B;
    const int tid = threadIdx.x;
    const int fill = a.fill, k = a.k;
    const float *inc = a.in + (long long)i * a.in_stride;
    float *ibc = a.ib + (size_t)i * B;
    auto sample = [&](int j) -> float {
        if (j < fill) return ibc[j];
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
            for (int j = tid; j < B; j += NT) ibc[j] = 0.f;
    } else {
        for (int j = tid; j < k; j += NT) ibc[fill + j] = inc[j];
    }
    const float2 *Z = lds_cfft<LOG2B, NT, false>(bufA, bufB, a.tw);
    float2 *row = a.X + ((size_t)i * a.S + a.cur) * B;
    for (int m = tid; m < B; m += NT) row[m] = real_post<LOG2B, NT>(Z, m, a.tw);
}

// MAC role of launch A, workgroup = (output o, part p): the rows H[o][i][s] (.)
// X[i][(current + s) % active], s >= 1, all i, flattened i-major as
// r = i * (active - 1) + s - 1; part p sums rows [p * rpp, (p + 1) * rpp) into
// part[o][p].  Group g of the workgroup takes the part's rows g, g + G, ... in
// ascending order, the groups are added in ascending g: a function of (I, B,
// active, P) only.
template <int LOG2B, int NT, bool NTL>
__device__ __forceinline__ void matrix_mac(const MatrixArgs &a, int o, int p, unsigned char *smem) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int F = Gm::F, G = Gm::G, SPT = Gm::SPT, U = Gm::U;
    const int tid = threadIdx.x;
    const int f0 = G > 1 ? tid % F : tid;
    const int g = G > 1 ? tid / F : 0;
    const int act = a.act, am1 = act - 1;
    const long long R = (long long)a.I * am1;
    const long long r0 = (long long)p * a.rpp;
    const long long r1 = r0 + a.rpp < R ? r0 + a.rpp : R;
    DBG_CHECK(o >= 0 && o < a.O && p >= 0 && p < a.P, 51, o, p, a.O, a.P);  // (site 51: a part past `part`)
    const int cm = a.cur % act;  // (current may exceed active after an update, :248)
    const float4 *H4 = reinterpret_cast<const float4 *>(a.H) + (size_t)o * a.I * a.S * F;
    const float4 *X4 = reinterpret_cast<const float4 *>(a.X);

    Acc2 acc[SPT];
#pragma unroll
    for (int s = 0; s < SPT; ++s) acc[s].zero();
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
    auto hrow = [&]() {
        DBG_CHECK(i >= 0 && i < a.I && s >= 1 && s < a.S, 50, i, s, a.I, a.S);  // (site 50: a MAC row past H / X)
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

// matrix_mac for two matrices that share their delay lines row for row (the
// crossfaded matrix's A and B, the two-stage matrix's head and tail0), in one
// pass over the rows: the walk, the part bounds and each accumulator's order of
// additions are matrix_mac's; row X[i][..] is loaded once (from X[0]) and
// multiplied with H[0] and H[1].  Args: MatrixXfArgs or MatrixTsArgs (H[2],
// X[2], part[2] and the scalars of MatrixArgs).  (The plain U rows in flight
// still compile without scratch with three streams per row instead of two.)
template <int LOG2B, int NT, bool NTL, class Args>
__device__ __forceinline__ void matrix_mac_pair(const Args &a, int o, int p, unsigned char *smem) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int F = Gm::F, G = Gm::G, SPT = Gm::SPT, U = Gm::U;
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

constexpr int matrix_nt(int log2b) { return log2b <= 10 ? 256 : 512; }

}  // namespace fftconv
