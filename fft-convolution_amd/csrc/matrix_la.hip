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
// The near walk is matrix.hpp's row walk over min(Q, active) - 1 rows per input,
// the far walk and the finish's pieces are matrix.hpp's too.
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

// output o's far rows as a row source: Pf parts of rppf rows, window rows
// far[o][p] (site 61: a window row past `far`)
struct DenseFarRows {
    static constexpr bool kListed = false;
    const MatrixLaArgs &la;
    int o, p;
    __device__ __forceinline__ int count() const { return la.m.I; }
    __device__ __forceinline__ size_t first_pair() const { return (size_t)o * la.m.I; }
    __device__ __forceinline__ size_t out_row() const { return (size_t)o * la.Pf + p; }
    __device__ __forceinline__ int rpp(long long) const { return la.rppf; }
    __device__ __forceinline__ int col(int) const { return 0; }
};

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
    if (m < nn) {  // (sites 58, 59: a near row past H / X, a near part past `part`)
        matrix_row_walk<LOG2B, NT, NTL, 58>(dense_rows(a, m, 59), MacStreams{a}, (a.act < Q ? a.act : Q) - 1, smem);
        return;
    }
    const int mf = m - nn;
    const int n = mf / la.Pf, p = mf % la.Pf;
    const int o = matrix_la_steady(la.t, la.tv) ? (int)(la.t % Q) + n * Q : n;
    DBG_CHECK(o >= 0 && o < a.O && p >= 0 && p < la.Pf, 61, o, p, a.O, la.Pf);
    const int role = matrix_la_role(la.t, la.tv, o);
    const DenseFarRows rw{la, o, p};
    const FarStreams st{{a}, la.far};
    if (role == 1)  // (sites 60, 62: a far row past H / X, a ring index >= active)
        matrix_far_walk<LOG2B, NT, NTL, Q, 60>(rw, st, la.t, smem);
    else if (role == 2)
        matrix_far_walk<LOG2B, NT, NTL, 1, 60>(rw, st, la.t, smem);
}

// Launch B, workgroup = output o: matrix_b_kernel with pre = near + far, near =
// part[o][0] + part[o][1] + ..., far = the Pf parts of window row t % Q in
// ascending order (no far term when Pf = 0).
template <int LOG2B, int NT>
__global__ __launch_bounds__(NT) void matrix_la_b_kernel(MatrixLaArgs la) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int B = Gm::B, F = Gm::F, SPT = Gm::SPT;
    constexpr int UB = SPT == 1 ? 16 : (SPT == 2 ? 8 : 4);  // terms in flight per slot
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
    const float *y = finish_c2r<LOG2B, NT>(bufA, bufB, a.tw);
    float *outc = a.out + (long long)o * a.out_stride;
    float *ovc = a.ovl + (size_t)o * B;
    overlap_add<LOG2B, NT>(y, ovc, fill, k, [&](int j, float v) { outc[j] = v; });
    if (complete) overlap_save<LOG2B, NT>(y, ovc);
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
    if (!matrix_chunk_in_range(log2b, a.I, a.O, a.S, a.cur, a.act, a.fill, a.k) || a.P <= 0) return hipErrorInvalidValue;
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
