// matrix_sp.hip -- gfx950 kernels of the SparseMatrixConvolver:
//   y[o] = sum over the listed pairs (o, i) of x[i] * h[(o, i)]
// as N reference FFTConvolver instances in lockstep, one per listed pair, in
// CSR order (strictly ascending (o, i)).  The dense matrix's scheme (matrix.hip)
// with an output's pair list in place of 0..I-1: one delay line per input, the
// spectra summed per output before ONE inverse transform.
//
// HBM layout (packed rows: B float2 per row, slot 0 = (DC, Nyquist)):
//   H      float2 [N][S][B]      IR spectra, pair n = channel n of the IR transform
//   X      float2 [I][S][B]      one FDL per input
//   ovl    float  [O][B]         summed overlap per output
//   ib     float  [I][B]         input buffer per input (zero past the fill)
//   pre    float2 [O][B]         summed pre_multiplied, kept across partial chunks
//   part   float2 [sum P_o][B]   split-row partial sums, output o's at plan[o]
//   rowptr int    [O + 1]        pairs of output o = [rowptr[o], rowptr[o + 1])
//   col    int    [N]            input of pair n
//   plan   int    [O + 1]        prefix sums of P_o for the current active_seg_count
//   wg     int4   [sum P_o]      MAC workgroup m of launch A = {rowptr[o], k_o, p, P_o}
//
// Output o with k_o pairs runs matrix_mac's walk and matrix_b_kernel's sums of a
// dense matrix with k_o inputs, entry e of its list standing for input e: the
// same rows in the same order into the same accumulators, so its bits are that
// dense matrix's.  The kernel boundary is the only ordering, as in matrix.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_lds.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "matrix.hpp"
#include "packed.hpp"

namespace fftconv {
namespace {

// plan[o] = P_0 + ... + P_(o-1), P_o = matrix_parts_rule(k_o, act): one
// workgroup; thread t sums a contiguous run of outputs, thread 0 scans the 256
// run sums, every thread writes its run -- and, per MAC workgroup m = plan[o] +
// p of launch A, wg[m] = {rowptr[o], k_o, p, P_o}: all a MAC workgroup needs in
// ONE load (a search of the prefix sums costs log2(O) dependent loads before
// the first row is requested, several times the walk of a 128-row part).
constexpr int kPlanNT = 256;
__global__ __launch_bounds__(kPlanNT) void matrix_sp_plan_kernel(const int *rowptr, int *plan, int4 *wg, int O,
                                                                 int act) {
    __shared__ int sums[kPlanNT];
    const int tid = threadIdx.x;
    const long long per = ((long long)O + kPlanNT - 1) / kPlanNT;
    const long long b0 = (long long)tid * per;
    const int o0 = (int)(b0 < O ? b0 : O);
    const int o1 = (int)(b0 + per < O ? b0 + per : O);
    int sum = 0;
    for (int o = o0; o < o1; ++o) sum += matrix_parts_rule(rowptr[o + 1] - rowptr[o], act);
    sums[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int t = 0; t < kPlanNT; ++t) {
            const int v = sums[t];
            sums[t] = acc;
            acc += v;
        }
        plan[O] = acc;
    }
    __syncthreads();
    int acc = sums[tid];
    for (int o = o0; o < o1; ++o) {
        const int n0 = rowptr[o], ko = rowptr[o + 1] - n0;
        const int P = matrix_parts_rule(ko, act);
        plan[o] = acc;
        for (int p = 0; p < P; ++p) wg[acc + p] = make_int4(n0, ko, p, P);
        acc += P;
    }
}

// MAC role of launch A, workgroup m of the compact grid = (output o, part p)
// with plan[o] <= m < plan[o + 1], p = m - plan[o], read from wg[m]: matrix_mac
// (matrix.hpp) over output o's pair list.  The rows H[pair e][s] (.)
// X[col e][(current + s) % active], s >= 1, are flattened pair-major as
// r = e * (active - 1) + s - 1; part p sums rows [p * rpp, (p + 1) * rpp),
// rpp = ceil(k_o * (active - 1) / P_o); group g takes the part's rows g, g + G,
// ... in ascending order, the groups are added in ascending g.  Lanes of one
// wave hold different e at B <= 256 (G > 1), so the input of a row is a
// per-lane load of `col`, redone only when the walk moves to another pair.
template <int LOG2B, int NT, bool NTL>
__device__ __forceinline__ void matrix_sp_mac(const MatrixSpArgs &a, int m, unsigned char *smem) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int F = Gm::F, G = Gm::G, SPT = Gm::SPT, U = Gm::U;
    const int tid = threadIdx.x;
    const int f0 = G > 1 ? tid % F : tid;
    const int g = G > 1 ? tid / F : 0;
    const int4 d = a.wg[m];
    const int n0 = d.x, ko = d.y, p = d.z, P = d.w;
    DBG_CHECK(m >= 0 && m < a.PT && p >= 0 && p < P && n0 >= 0 && ko >= 0 && n0 + ko <= a.N, 55, m, p, a.PT,
              n0 + ko);  // (site 55: a part past `part`, a pair list past `col`)
    const int S = a.m.S;
    const int act = a.m.act, am1 = act - 1;
    const long long R = (long long)ko * am1;
    const long long rpp = (R + P - 1) / P;
    const long long r0 = (long long)p * rpp;
    const long long r1 = r0 + rpp < R ? r0 + rpp : R;
    const int cm = a.m.cur % act;  // (current may exceed active after an update, :248)
    const float4 *H4 = reinterpret_cast<const float4 *>(a.m.H) + (size_t)n0 * S * F;
    const float4 *X4 = reinterpret_cast<const float4 *>(a.m.X);
    const int *colo = a.col + n0;

    Acc2 acc[SPT];
#pragma unroll
    for (int s = 0; s < SPT; ++s) acc[s].zero();
    long long r = r0 + g;
    int e = 0, s = 1;
    if (am1 > 0) {
        e = (int)(r / am1);
        s = 1 + (int)(r % am1);
    }
    // (the row's input is reloaded only where the walk moves to another pair:
    // measured against a load per row ahead of each batch, SP1's launch A is
    // 8 % faster this way and SP2's the same)
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
    auto hrow = [&]() {
        DBG_CHECK(e >= 0 && e < ko && s >= 1 && s < S, 54, e, s, ko, S);  // (site 54: a MAC row past H / X)
        return H4 + ((size_t)e * S + s) * F + f0;
    };
    auto xrow = [&]() {
        DBG_CHECK(c >= 0 && c < a.m.I, 56, c, e, a.m.I, m);  // (site 56: a `col` entry >= I)
        int xi = cm + s;
        if (xi >= act) xi -= act;
        return X4 + ((size_t)c * S + xi) * F + f0;
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

    float4 *dst = reinterpret_cast<float4 *>(a.m.part) + (size_t)m * F;
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

// Launch A: blocks [0, I) are the R2C workgroups (matrix_r2c, unchanged),
// blocks I + m, m < PT, the MAC workgroups (launched only for a chunk that
// starts a block).
template <int LOG2B, int NT, bool NTL>
__global__ __launch_bounds__(NT) void matrix_sp_a_kernel(MatrixSpArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x;
    if (b < a.m.I) {
        matrix_r2c<LOG2B, NT>(a.m, b, smem);
    } else {
        matrix_sp_mac<LOG2B, NT, NTL>(a, b - a.m.I, smem);
    }
}

// Launch B, workgroup = output o: matrix_b_kernel over output o's P_o parts and
// its pair list -- pre = part[plan[o]] + part[plan[o] + 1] + ... (or the kept
// pre[o]), conv = pre + sum_e X[col e][current] (.) H[pair e][0] in ascending e,
// one C2R with 1/N, overlap-add, overlap saved when the block completes.  An
// output without pairs has one all-zero part and no terms: it writes zeros and
// keeps a zero overlap.
template <int LOG2B, int NT>
__global__ __launch_bounds__(NT) void matrix_sp_b_kernel(MatrixSpArgs a) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int B = Gm::B, F = Gm::F, SPT = Gm::SPT;
    constexpr int UB = SPT == 1 ? 16 : (SPT == 2 ? 8 : 4);  // terms in flight per slot
    constexpr float invN = 1.0f / (float)(2 * B);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *bufA = reinterpret_cast<float2 *>(smem);
    float2 *bufB = bufA + B;
    const int tid = threadIdx.x;
    const int o = blockIdx.x;
    const int fill = a.m.fill, k = a.m.k;
    const bool complete = fill + k == B;
    const int P = a.plan[o + 1] - a.plan[o];
    const int n0 = a.rowptr[o];
    const int ko = a.rowptr[o + 1] - n0;
    const size_t SF = (size_t)a.m.S * F;
    float4 *pre4 = reinterpret_cast<float4 *>(a.m.pre) + (size_t)o * F;
    const float4 *part4 = reinterpret_cast<const float4 *>(a.m.part) + (size_t)a.plan[o] * F;
    const float4 *H4 = reinterpret_cast<const float4 *>(a.m.H) + (size_t)n0 * SF;
    const float4 *X4 = reinterpret_cast<const float4 *>(a.m.X) + (size_t)a.m.cur * F;
    const int *colo = a.col + n0;
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
        const int f = tid + q * NT;
        if (f < F) {
            // (both sums strictly in ascending order; the loads of UB terms are
            // issued before their adds, so the chain waits once per UB terms.
            // The inputs of a chunk of terms are loaded one chunk ahead, the
            // first chunk's ahead of the parts: the wait for `col` never sits
            // between a chunk's adds and its row requests)
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
                int c[UB / 2];
#pragma unroll
                for (int u = 0; u < UB / 2; ++u) {
                    c[u] = cn[u];
                    cn[u] = e + UB / 2 + u < ko ? colo[e + UB / 2 + u] : 0;
                }
#pragma unroll
                for (int u = 0; u < UB / 2; ++u) {
                    if (e + u < ko) {
                        DBG_CHECK(c[u] >= 0 && c[u] < a.m.I, 57, c[u], e + u, a.m.I, o);  // (site 57: a `col` entry >= I)
                        xs[u] = X4[(size_t)c[u] * SF + f];
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
    for (int m = tid; m < B; m += NT) bufB[m] = real_pre<LOG2B, NT>(bufA, m, a.m.tw);
    __syncthreads();
    const float *y = reinterpret_cast<const float *>(lds_cfft<LOG2B, NT, true>(bufB, bufA, a.m.tw));
    float *outc = a.m.out + (long long)o * a.m.out_stride;
    float *ovc = a.m.ovl + (size_t)o * B;
    for (int j = tid; j < k; j += NT) outc[j] = y[fill + j] * invN + ovc[fill + j];
    if (complete) {
        __syncthreads();  // (every overlap read above is done)
        for (int j = tid; j < B; j += NT) ovc[j] = y[B + j] * invN;
    }
}

template <int LOG2B>
hipError_t launch_matrix_sp_t(const MatrixSpArgs &a, hipStream_t s) {
    constexpr int NT = matrix_nt(LOG2B);
    using Gm = MGeo<LOG2B, NT>;
    auto ka = a.m.nt_h ? matrix_sp_a_kernel<LOG2B, NT, true> : matrix_sp_a_kernel<LOG2B, NT, false>;
    auto kb = matrix_sp_b_kernel<LOG2B, NT>;
    const long long grid = (long long)a.m.I + (a.m.fill == 0 ? (long long)a.PT : 0);
    if (hipError_t e = launch_dyn(ka, dim3((unsigned)grid), dim3(NT), Gm::lds_a, s, a); e != hipSuccess) return e;
    return launch_dyn(kb, dim3(a.m.O), dim3(NT), Gm::lds_b, s, a);
}

}  // namespace

hipError_t launch_matrix_sp_plan(const int *rowptr, int *plan, int4 *wg, int O, int act, hipStream_t s) {
    if (!rowptr || !plan || !wg || O <= 0 || act < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(matrix_sp_plan_kernel, dim3(1), dim3(kPlanNT), 0, s, rowptr, plan, wg, O, act);
    return hipGetLastError();
}

hipError_t launch_matrix_sp_chunk(int log2b, const MatrixSpArgs &a, hipStream_t s) {
    const MatrixArgs &m = a.m;
    if (m.I <= 0 || m.O <= 0 || a.N <= 0 || m.k <= 0 || m.act <= 0 || a.PT < m.O || m.fill < 0 ||
        m.fill + m.k > (1 << log2b) || m.cur < 0 || m.cur >= m.S || m.act > m.S || !a.rowptr || !a.col || !a.plan || !a.wg)
        return hipErrorInvalidValue;
    if ((long long)m.I + (long long)a.PT > (long long)INT32_MAX) return hipErrorInvalidValue;
    return dispatch_log2<5, kMaxLog2Fused>(log2b, hipErrorInvalidValue,
                                           [&](auto L) { return launch_matrix_sp_t<L()>(a, s); });
}

}  // namespace fftconv
