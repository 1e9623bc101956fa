// matrix_sp.hpp -- the sparse matrix's pair walk over one or two H streams,
// shared by matrix_sp_xf.hip (the crossfaded sparse matrix's A and B) and
// matrix_sp_ts.hip (the sparse two-stage matrix's head and tail0): one
// definition, so both families compute the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "matrix.hpp"
#include "packed.hpp"

namespace fftconv {

// MAC workgroup m = (output o, part p) from wg[m]: matrix_sp_mac's walk -- the
// same row flattening, part bounds, row groups and `col` reload only where the
// walk moves to another pair -- over NH H streams: NH == 1 reads convolver c0's
// H, NH == 2 multiplies each X row (from X[0]; X[1] is equal row for row) with
// H[0] and H[1] into two accumulator sets, each in matrix_mac's order.
// Args: MatrixSpXfArgs or MatrixSpTsArgs (H[2], X[2], part[2], wg, col and the
// scalars I, S, N, PT, cur, act).  SITE: the first of the walk's three
// DBG_CHECK site numbers in the including file (MAC row, part, `col` entry).
template <int LOG2B, int NT, bool NTL, int NH, int SITE, class Args>
__device__ __forceinline__ void matrix_sp_mac_streams(const Args &a, int m, int c0, unsigned char *smem) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int F = Gm::F, G = Gm::G, SPT = Gm::SPT, U = Gm::U;
    const int tid = threadIdx.x;
    const int f0 = G > 1 ? tid % F : tid;
    const int g = G > 1 ? tid / F : 0;
    const int4 d = a.wg[m];
    const int n0 = d.x, ko = d.y, p = d.z, P = d.w;
    DBG_CHECK(m >= 0 && m < a.PT && p >= 0 && p < P && n0 >= 0 && ko >= 0 && n0 + ko <= a.N, SITE + 1, m, p, a.PT,
              n0 + ko);  // (site + 1: a part past `part`, a pair list past `col`)
    const int S = a.S;
    const int act = a.act, am1 = act - 1;
    const long long R = (long long)ko * am1;
    const long long rpp = (R + P - 1) / P;
    const long long r0 = (long long)p * rpp;
    const long long r1 = r0 + rpp < R ? r0 + rpp : R;
    const int cm = a.cur % act;  // (current may exceed active after an update)
    const float4 *H4[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h)
        H4[h] = reinterpret_cast<const float4 *>(a.H[NH == 2 ? h : c0]) + (size_t)n0 * S * F;
    const float4 *X4 = reinterpret_cast<const float4 *>(a.X[NH == 2 ? 0 : c0]);
    const int *colo = a.col + n0;

    Acc2 acc[NH][SPT];
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int s = 0; s < SPT; ++s) acc[h][s].zero();
    long long r = r0 + g;
    int e = 0, s = 1;
    if (am1 > 0) {
        e = (int)(r / am1);
        s = 1 + (int)(r % am1);
    }
    int c = e < ko ? colo[e] : 0;  // (a group past the part's rows reads nothing)
    auto advance = [&]() {
        r += G;
        s += G;
        if (s > am1) {
            do {
                s -= am1;
                ++e;
            } while (s > am1);
            c = e < ko ? colo[e] : 0;
        }
    };
    auto hoff = [&]() {
        DBG_CHECK(e >= 0 && e < ko && s >= 1 && s < S, SITE, e, s, ko, S);  // (site: a MAC row past H / X)
        return ((size_t)e * S + s) * F + f0;
    };
    auto xrow = [&]() {
        DBG_CHECK(c >= 0 && c < a.I, SITE + 2, c, e, a.I, m);  // (site + 2: a `col` entry >= I)
        int xi = cm + s;
        if (xi >= act) xi -= act;
        return X4 + ((size_t)c * S + xi) * F + f0;
    };
    while (r + (long long)(U - 1) * G < r1) {
        float4 hv[NH][U][SPT], xv[U][SPT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t ho = hoff();
            const float4 *xp = xrow();
#pragma unroll
            for (int q = 0; q < SPT; ++q) {
#pragma unroll
                for (int h = 0; h < NH; ++h) hv[h][u][q] = ld4<NTL>(H4[h] + ho + q * NT);
                xv[u][q] = ld4<false>(xp + q * NT);
            }
            advance();
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < SPT; ++q)
#pragma unroll
                for (int h = 0; h < NH; ++h) acc[h][q].mac(hv[h][u][q], xv[u][q]);
    }
    while (r < r1) {
        const size_t ho = hoff();
        const float4 *xp = xrow();
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
            const float4 x = ld4<false>(xp + q * NT);
#pragma unroll
            for (int h = 0; h < NH; ++h) acc[h][q].mac(ld4<NTL>(H4[h] + ho + q * NT), x);
        }
        advance();
    }

    float4 *dst[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) dst[h] = reinterpret_cast<float4 *>(a.part[NH == 2 ? h : c0]) + (size_t)m * F;
    if constexpr (G > 1) {
        float4 *red = reinterpret_cast<float4 *>(smem);
#pragma unroll
        for (int h = 0; h < NH; ++h) red[h * NT + g * F + f0] = acc[h][0].get(f0);
        __syncthreads();
        if (tid < F) {
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                float4 v = red[h * NT + f0];
#pragma unroll
                for (int q = 1; q < G; ++q) v = vadd(v, red[h * NT + q * F + f0]);
                dst[h][f0] = v;
            }
        }
    } else {
#pragma unroll
        for (int q = 0; q < SPT; ++q)
#pragma unroll
            for (int h = 0; h < NH; ++h) dst[h][f0 + q * NT] = acc[h][q].get(f0 + q * NT);
    }
}

}  // namespace fftconv
