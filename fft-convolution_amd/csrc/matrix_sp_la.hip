// matrix_sp_la.hip -- gfx950 kernels of the SparseMatrixLookaheadConvolver
// (DESIGN §4q): the SparseMatrixConvolver (matrix_sp.hip) with the far-row
// windows of the MatrixLookaheadConvolver (matrix_la.hip).  Output o with k_o
// listed pairs runs matrix_la.hip's near walk, far walk and finish of a dense
// lookahead matrix with k_o inputs, entry e of its pair list standing for input
// e: the same rows in the same order into the same accumulators, so its bits
// are that matrix's single output.  The schedule is §4n's unchanged: output o
// anchors on blocks t = o (mod Q), the host passes {t, tv} by value, the kernel
// boundary is the only ordering.
//
// HBM layout beyond matrix_sp.hip's (H [N][S][B], X [I][S][B], rowptr, col):
//   part  float2 [sum Pn_o][B]     near partial sums of one block, output o's at nplan[o]
//   far   float2 [sum Pf_o][Q][B]  far partial sums, output o's at fplan[o], window row = block % Q
//   nplan int    [O + 1]           prefix sums of Pn_o
//   fplan int    [O + 1]           prefix sums of Pf_o (output order)
//   nwg   int4   [sum Pn_o]        near workgroup m = nplan[o] + p: {rowptr[o], k_o, p, Pn_o}
//   fwg   int4   [2 * sum Pf_o]    far workgroups ordered by (o % Q, o, p), two entries each:
//                                  {rowptr[o], k_o, o, p}, {Pf_o, fplan[o] + p, 0, 0}
//   coff  int    [Q + 1]           first far workgroup of every anchor class
// In the steady state launch A holds the far workgroups of the anchoring class
// only, a contiguous range of fwg.
//
// The near walk, the far walk and the finish's pieces are matrix.hpp's over the
// pair-list row source of matrix_sp.hpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_lds.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "matrix.hpp"
#include "matrix_sp.hpp"
#include "packed.hpp"

namespace fftconv {
namespace {

constexpr int Q = kMatrixLaQ;

// The plan for `act` active segments: near descriptors in output order, the far
// rows' prefix sums in output order, then the far descriptors ordered by anchor
// class -- position j of that order is output o = c + n * Q, the classes c in
// ascending order and n ascending inside a class -- with the class offsets.
__global__ __launch_bounds__(kPlanNT) void matrix_sp_la_plan_kernel(const int *rowptr, int *nplan, int *fplan,
                                                                    int4 *nwg, int4 *fwg, int *coff, int O, int act) {
    __shared__ int sums[kPlanNT + 1];
    auto ko_of = [&](int o) { return rowptr[o + 1] - rowptr[o]; };
    const int pnt = plan_scan(
        sums, O, [&](int o) { return matrix_sp_la_pn(ko_of(o), act); },
        [&](int o, int acc, int P) {
            const int n0 = rowptr[o], ko = rowptr[o + 1] - n0;
            nplan[o] = acc;
            for (int p = 0; p < P; ++p) nwg[acc + p] = make_int4(n0, ko, p, P);
        });
    const int pft = plan_scan(
        sums, O, [&](int o) { return matrix_sp_la_pf(ko_of(o), act); }, [&](int o, int acc, int) { fplan[o] = acc; });
    auto output_at = [&](int j) {  // the j-th output in (o % Q, o) order
        int c = 0;
        for (; c < Q - 1; ++c) {
            const int cnt = c < O ? (O - c + Q - 1) / Q : 0;
            if (j < cnt) break;
            j -= cnt;
        }
        return c + j * Q;
    };
    plan_scan(
        sums, O, [&](int j) { return matrix_sp_la_pf(ko_of(output_at(j)), act); },
        [&](int j, int acc, int P) {
            const int o = output_at(j);
            const int n0 = rowptr[o], ko = rowptr[o + 1] - n0;
            if (o < Q) coff[o] = acc;  // (the first output of class o)
            const int f0 = fplan[o];   // (scan 2 wrote it, two barriers ago)
            for (int p = 0; p < P; ++p) {
                fwg[2 * (size_t)(acc + p)] = make_int4(n0, ko, o, p);
                fwg[2 * (size_t)(acc + p) + 1] = make_int4(P, f0 + p, 0, 0);
            }
        });
    if (threadIdx.x == 0) {
        nplan[O] = pnt;
        fplan[O] = pft;
        for (int c = O < Q ? O : Q; c <= Q; ++c) coff[c] = pft;  // (classes without outputs, and the end)
    }
}

// Launch A: blocks [0, I) are the R2C workgroups; for a chunk that starts a
// block, blocks I + m, m < PnT, the near workgroups -- workgroup m of the compact
// near grid = (output o, part p), read from nwg[m], runs the row walk over the
// rows (e, s), 1 <= s < min(Q, active), of output o's pair list (sites 68, 69,
// 70) -- then a.flen far workgroups, descriptors a.fbase + 0, 1, ...: the
// anchoring class's while every other output has a window (matrix_la_steady),
// else all of them, and an output that needs nothing leaves at once.  A far
// workgroup = (output o, far part p) with its pair list at n0 and its window
// rows at far row `frow` runs the far walk pair by pair (sites 71, 73, 74).
template <int LOG2B, int NT, bool NTL>
__global__ __launch_bounds__(NT) void matrix_sp_la_a_kernel(MatrixSpLaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x;
    if (b < a.m.I) {
        matrix_r2c<LOG2B, NT>(a.m, b, smem);
        return;
    }
    const int m = b - a.m.I;
    if (m < a.PnT) {
        matrix_row_walk<LOG2B, NT, NTL, 68>(listed_rows(a.nwg, a.col, m, a.PnT, a.N, 69), MacStreams{a.m},
                                            (a.m.act < Q ? a.m.act : Q) - 1, smem);
        return;
    }
    const int w = a.fbase + (m - a.PnT);
    const int4 d0 = a.fwg[2 * (size_t)w], d1 = a.fwg[2 * (size_t)w + 1];
    const int n0 = d0.x, ko = d0.y, o = d0.z, p = d0.w, Pf = d1.x, frow = d1.y;
    DBG_CHECK(w >= 0 && w < a.PfT && o >= 0 && o < a.m.O && p >= 0 && p < Pf && frow >= 0 && frow < a.PfT && n0 >= 0 &&
                  ko > 0 && n0 + ko <= a.N,
              72, w, o, frow, n0 + ko);  // (site 72: a window row past `far`, a pair list past `col`)
    const int role = matrix_la_role(a.t, a.tv, o);
    const ListedRows rw{a.col + n0, n0, ko, p, Pf, (size_t)frow};
    const FarStreams st{{a.m}, a.far};
    if (role == 1)
        matrix_far_walk<LOG2B, NT, NTL, Q, 71>(rw, st, a.t, smem);
    else if (role == 2)
        matrix_far_walk<LOG2B, NT, NTL, 1, 71>(rw, st, a.t, smem);
}

// Launch B, workgroup = output o: matrix_la_b_kernel over output o's parts and
// pair list -- pre = near + far, near = part[nplan[o]] + part[nplan[o] + 1] +
// ..., far = the Pf_o parts of window row t % Q in ascending order (no far term
// when Pf_o = 0), or the kept pre[o]; then the row-0 terms X[col e][current] (.)
// H[pair e][0] in ascending e with the chunk-ahead `col` loads, one C2R with
// 1/N, overlap-add.  An output without pairs has one all-zero near part, no far
// part and no terms: it writes zeros and keeps a zero overlap.
template <int LOG2B, int NT>
__global__ __launch_bounds__(NT) void matrix_sp_la_b_kernel(MatrixSpLaArgs a) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int B = Gm::B, F = Gm::F, SPT = Gm::SPT;
    constexpr int UB = SPT == 1 ? 16 : (SPT == 2 ? 8 : 4);  // terms in flight per slot
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *bufA = reinterpret_cast<float2 *>(smem);
    float2 *bufB = bufA + B;
    const int tid = threadIdx.x;
    const int o = blockIdx.x;
    const int fill = a.m.fill, k = a.m.k;
    const bool complete = fill + k == B;
    const int np0 = a.nplan[o], Pn = a.nplan[o + 1] - np0;
    const int fp0 = a.fplan[o], Pf = a.fplan[o + 1] - fp0;
    const int n0 = a.rowptr[o];
    const int ko = a.rowptr[o + 1] - n0;
    DBG_CHECK(Pn >= 1 && np0 + Pn <= a.PnT && Pf >= 0 && fp0 + Pf <= a.PfT && n0 >= 0 && ko >= 0 && n0 + ko <= a.N, 75,
              o, np0 + Pn, fp0 + Pf, n0 + ko);  // (site 75: a part past `part` / `far`, a pair list past `col`)
    const size_t SF = (size_t)a.m.S * F;
    float4 *pre4 = reinterpret_cast<float4 *>(a.m.pre) + (size_t)o * F;
    const float4 *part4 = reinterpret_cast<const float4 *>(a.m.part) + (size_t)np0 * F;
    const float4 *far4 = reinterpret_cast<const float4 *>(a.far) + ((size_t)fp0 * Q + (size_t)(a.t % Q)) * F;
    const float4 *H4 = reinterpret_cast<const float4 *>(a.m.H) + (size_t)n0 * SF;
    const float4 *X4 = reinterpret_cast<const float4 *>(a.m.X) + (size_t)a.m.cur * F;
    const int *colo = a.col + n0;
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
        const int f = tid + q * NT;
        if (f < F) {
            // (every sum strictly in ascending order; the loads of UB terms are
            // issued before their adds, so the chain waits once per UB terms.
            // The inputs of a chunk of terms are loaded one chunk ahead, the
            // first chunk's ahead of the parts)
            int cn[UB / 2];
#pragma unroll
            for (int u = 0; u < UB / 2; ++u) cn[u] = u < ko ? colo[u] : 0;  // (uniform over the workgroup)
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (fill == 0) {
                for (int p = 0; p < Pn; p += UB) {
                    float4 t[UB];
#pragma unroll
                    for (int u = 0; u < UB; ++u)
                        if (p + u < Pn) t[u] = part4[(size_t)(p + u) * F + f];
#pragma unroll
                    for (int u = 0; u < UB; ++u)
                        if (p + u < Pn) v = p + u == 0 ? t[u] : vadd(v, t[u]);
                }
                if (Pf > 0) {
                    float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
                    for (int p = 0; p < Pf; p += UB) {
                        float4 t[UB];
#pragma unroll
                        for (int u = 0; u < UB; ++u)
                            if (p + u < Pf) t[u] = far4[(size_t)(p + u) * Q * F + f];
#pragma unroll
                        for (int u = 0; u < UB; ++u)
                            if (p + u < Pf) w = p + u == 0 ? t[u] : vadd(w, t[u]);
                    }
                    v = vadd(v, w);
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
                        DBG_CHECK(c[u] >= 0 && c[u] < a.m.I, 76, c[u], e + u, a.m.I, o);  // (site 76: a `col` entry >= I)
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
    const float *y = finish_c2r<LOG2B, NT>(bufA, bufB, a.m.tw);
    float *outc = a.m.out + (long long)o * a.m.out_stride;
    float *ovc = a.m.ovl + (size_t)o * B;
    overlap_add<LOG2B, NT>(y, ovc, fill, k, [&](int j, float v) { outc[j] = v; });
    if (complete) overlap_save<LOG2B, NT>(y, ovc);
}

template <int LOG2B>
hipError_t launch_matrix_sp_la_t(const MatrixSpLaArgs &a, hipStream_t s) {
    constexpr int NT = matrix_nt(LOG2B);
    using Gm = MGeo<LOG2B, NT>;
    using Lg = LaGeo<LOG2B, NT>;
    auto ka = a.m.nt_h ? matrix_sp_la_a_kernel<LOG2B, NT, true> : matrix_sp_la_a_kernel<LOG2B, NT, false>;
    auto kb = matrix_sp_la_b_kernel<LOG2B, NT>;
    long long grid = a.m.I;
    if (a.m.fill == 0) grid += (long long)a.PnT + (long long)a.flen;
    if (hipError_t e = launch_dyn(ka, dim3((unsigned)grid), dim3(NT), Lg::lds_a, s, a); e != hipSuccess) return e;
    return launch_dyn(kb, dim3(a.m.O), dim3(NT), Gm::lds_b, s, a);
}

}  // namespace

hipError_t launch_matrix_sp_la_plan(const int *rowptr, int *nplan, int *fplan, int4 *nwg, int4 *fwg, int *coff, int O,
                                    int act, hipStream_t s) {
    if (!rowptr || !nplan || !fplan || !nwg || !coff || O <= 0 || act < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(matrix_sp_la_plan_kernel, dim3(1), dim3(kPlanNT), 0, s, rowptr, nplan, fplan, nwg, fwg, coff, O,
                       act);
    return hipGetLastError();
}

hipError_t launch_matrix_sp_la_chunk(int log2b, const MatrixSpLaArgs &a, hipStream_t s) {
    const MatrixArgs &m = a.m;
    if (!matrix_chunk_in_range(log2b, m.I, m.O, m.S, m.cur, m.act, m.fill, m.k) || a.N <= 0 || a.PnT < m.O || !a.rowptr ||
        !a.col || !a.nplan || !a.fplan || !a.nwg)
        return hipErrorInvalidValue;
    if (a.t < 0 || a.tv < 0 || a.PfT < 0 || (a.PfT > 0) != (m.act > kMatrixLaQ)) return hipErrorInvalidValue;
    if (a.fbase < 0 || a.flen < 0 || (long long)a.fbase + a.flen > (long long)a.PfT) return hipErrorInvalidValue;
    if (a.PfT > 0 && (!a.far || !a.fwg)) return hipErrorInvalidValue;
    // an anchor reads the FDL rows of Q future blocks: only while current < active
    if (a.PfT > 0 && a.tv <= a.t && m.cur >= m.act) return hipErrorInvalidValue;
    // outside the steady state every far workgroup is launched
    if (!matrix_la_steady(a.t, a.tv) && m.fill == 0 && (a.fbase != 0 || a.flen != a.PfT)) return hipErrorInvalidValue;
    if ((long long)m.I + (long long)a.PnT + (long long)a.flen > (long long)INT32_MAX) return hipErrorInvalidValue;
    return dispatch_log2<5, kMatrixLaMaxLog2B>(log2b, hipErrorInvalidValue,
                                               [&](auto L) { return launch_matrix_sp_la_t<L()>(a, s); });
}

}  // namespace fftconv
