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
// The walks and the finish kernel are copies of matrix_la.hip's with the pair
// list in place of 0..I-1, not templates over them: those kernels keep their
// instruction streams (the decision of §4m / §4n).
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
struct SpLaGeo {
    using Gm = MGeo<LOG2B, NT>;
    static_assert(Gm::SPT == 1, "one 16-byte slot per thread");
    // the anchor's group reduction: Q accumulators of every thread (LaGeo::lds_a)
    static constexpr size_t red_bytes = Gm::G > 1 ? (size_t)Q * NT * sizeof(float4) : 0;
    static constexpr size_t lds_a = Gm::lds_a > red_bytes ? Gm::lds_a : red_bytes;
};

// Exclusive prefix sums over value(0 .. n - 1) by one workgroup, as
// matrix_sp_plan_kernel's: thread t sums a contiguous run, thread 0 scans the
// run sums, every thread emits its run.  Returns the total.
constexpr int kPlanNT = 256;
template <class V, class E>
__device__ __forceinline__ int plan_scan(int *sums, int n, V value, E emit) {
    const int tid = threadIdx.x;
    const long long per = ((long long)n + kPlanNT - 1) / kPlanNT;
    const long long b0 = (long long)tid * per;
    const int j0 = (int)(b0 < n ? b0 : n);
    const int j1 = (int)(b0 + per < n ? b0 + per : n);
    int sum = 0;
    for (int j = j0; j < j1; ++j) sum += value(j);
    __syncthreads();  // (the previous scan's reads of `sums` are done)
    sums[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int t = 0; t < kPlanNT; ++t) {
            const int v = sums[t];
            sums[t] = acc;
            acc += v;
        }
        sums[kPlanNT] = acc;
    }
    __syncthreads();  // (and every global write of the scans before this one is visible)
    int acc = sums[tid];
    for (int j = j0; j < j1; ++j) {
        const int v = value(j);
        emit(j, acc, v);
        acc += v;
    }
    return sums[kPlanNT];
}

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

// Near role of launch A, workgroup m of the compact near grid = (output o, part
// p), read from nwg[m]: matrix_la_near over output o's pair list -- the rows
// (e, s), 1 <= s < min(Q, active), flattened pair-major as r = e * nm1 + s - 1.
// The input of a row is a per-lane load of `col`, redone only where the walk
// moves to another pair (matrix_sp_mac).
template <int LOG2B, int NT, bool NTL>
__device__ __forceinline__ void matrix_sp_la_near(const MatrixSpLaArgs &a, int m, unsigned char *smem) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int F = Gm::F, G = Gm::G, SPT = Gm::SPT, U = Gm::U;
    const int tid = threadIdx.x;
    const int f0 = G > 1 ? tid % F : tid;
    const int g = G > 1 ? tid / F : 0;
    const int4 d = a.nwg[m];
    const int n0 = d.x, ko = d.y, p = d.z, P = d.w;
    DBG_CHECK(m >= 0 && m < a.PnT && p >= 0 && p < P && n0 >= 0 && ko >= 0 && n0 + ko <= a.N, 69, m, p, a.PnT,
              n0 + ko);  // (site 69: a near part past `part`, a pair list past `col`)
    const int S = a.m.S;
    const int act = a.m.act, nm1 = (act < Q ? act : Q) - 1;
    const long long R = (long long)ko * nm1;
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
    if (nm1 > 0) {
        e = (int)(r / nm1);
        s = 1 + (int)(r % nm1);
    }
    int c = e < ko ? colo[e] : 0;  // (a group past the part's rows reads nothing)
    auto advance = [&]() {
        r += G;
        s += G;
        if (s > nm1) {
            do {
                s -= nm1;
                ++e;
            } while (s > nm1);
            c = e < ko ? colo[e] : 0;
        }
    };
    auto hrow = [&]() {
        DBG_CHECK(e >= 0 && e < ko && s >= 1 && s < S, 68, e, s, ko, S);  // (site 68: a near row past H / X)
        return H4 + ((size_t)e * S + s) * F + f0;
    };
    auto xrow = [&]() {
        DBG_CHECK(c >= 0 && c < a.m.I, 70, c, e, a.m.I, m);  // (site 70: a `col` entry >= I)
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

// Far role of launch A, one far workgroup = (output o, far part p) with window
// length W, its pair list at n0 and its window rows at far row `frow`:
// matrix_la_far going pair by pair.  The rows (e, s), Q <= s < active, are
// flattened pair-major as r = e * (active - Q) + s - Q; part p holds rows [p *
// rppf, (p + 1) * rppf), rppf = ceil(k_o * (active - Q) / Pf_o); group g the
// CONTIGUOUS rows [g * rpg, (g + 1) * rpg) of the part in ascending order, the
// groups are added in ascending g.  Accumulator j < W is the sum of block t + j
// (matrix_la.hip has the argument); W = 1 is the plain far sum of block t, W =
// Q the anchor, both through the same Acc2::mac in the same order: the same
// bits.  One turn of the outer loop covers the rows of one pair: its input is
// one `col` load, issued a turn ahead.
template <int LOG2B, int NT, bool NTL, int W>
__device__ __forceinline__ void matrix_sp_la_far(const MatrixSpLaArgs &a, int n0, int ko, int p, int Pf, int frow,
                                                 unsigned char *smem) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int F = Gm::F, G = Gm::G;
    constexpr int UB = 8;  // rows in flight (a multiple of the slide of one row per step)
    const int tid = threadIdx.x;
    const int f0 = G > 1 ? tid % F : tid;
    const int g = G > 1 ? tid / F : 0;
    const int S = a.m.S;
    const int act = a.m.act, nf = act - Q;  // far rows per pair, > 0
    const long long R = (long long)ko * nf;
    const long long rppf = (R + Pf - 1) / Pf;
    const long long r0 = (long long)p * rppf;
    const long long r1 = r0 + rppf < R ? r0 + rppf : R;
    const long long rpg = (rppf + G - 1) / G;
    const long long q0 = r0 + (long long)g * rpg;
    const long long q1 = q0 + rpg < r1 ? q0 + rpg : r1;
    const int cm = a.m.cur % act;  // (W > 1 runs only while current < active)
    const float4 *H4 = reinterpret_cast<const float4 *>(a.m.H) + (size_t)n0 * S * F + f0;
    const float4 *X4 = reinterpret_cast<const float4 *>(a.m.X) + f0;
    const int *colo = a.col + n0;

    Acc2 acc[W];
#pragma unroll
    for (int j = 0; j < W; ++j) acc[j].zero();
    long long r = q0;
    int cnext = r < q1 ? colo[(int)(r / nf)] : 0;
    while (r < q1) {  // one pair per turn
        const int e = (int)(r / nf);
        const int s0 = Q + (int)(r % nf);
        const long long left = q1 - r;
        const int len = left < (long long)(act - s0) ? (int)left : act - s0;
        DBG_CHECK(e >= 0 && e < ko && s0 >= Q && s0 + len <= S, 71, e, s0, len, S);  // (site 71: a far row past H / X)
        const int c = cnext;
        if (r + len < q1) cnext = colo[e + 1];  // (the next turn starts pair e + 1 <= k_o - 1)
        DBG_CHECK(c >= 0 && c < a.m.I, 74, c, e, a.m.I, frow);  // (site 74: a `col` entry >= I)
        const float4 *Hp = H4 + ((size_t)e * S + s0) * F;
        const float4 *Xi = X4 + (size_t)c * S * F;
        auto xrow = [&](int k) {  // FDL row of block t - k
            int xi = cm + k;
            if (xi >= act) xi -= act;
            DBG_CHECK(k >= 1 && xi >= 0 && xi < act, 73, k, xi, act, cm);  // (site 73: a ring index >= active)
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

    const int slot0 = (int)(a.t % Q);
    float4 *dst = reinterpret_cast<float4 *>(a.far) + (size_t)frow * Q * F;
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

// Launch A: blocks [0, I) are the R2C workgroups (matrix_r2c, unchanged); for a
// chunk that starts a block, blocks I + m, m < PnT, the near workgroups, then
// a.flen far workgroups, descriptors a.fbase + 0, 1, ...: the anchoring class's
// while every other output has a window (matrix_la_steady), else all of them,
// and an output that needs nothing leaves at once.
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
        matrix_sp_la_near<LOG2B, NT, NTL>(a, m, smem);
        return;
    }
    const int w = a.fbase + (m - a.PnT);
    const int4 d0 = a.fwg[2 * (size_t)w], d1 = a.fwg[2 * (size_t)w + 1];
    const int n0 = d0.x, ko = d0.y, o = d0.z, p = d0.w, Pf = d1.x, frow = d1.y;
    DBG_CHECK(w >= 0 && w < a.PfT && o >= 0 && o < a.m.O && p >= 0 && p < Pf && frow >= 0 && frow < a.PfT && n0 >= 0 &&
                  ko > 0 && n0 + ko <= a.N,
              72, w, o, frow, n0 + ko);  // (site 72: a window row past `far`, a pair list past `col`)
    const int role = matrix_la_role(a.t, a.tv, o);
    if (role == 1)
        matrix_sp_la_far<LOG2B, NT, NTL, Q>(a, n0, ko, p, Pf, frow, smem);
    else if (role == 2)
        matrix_sp_la_far<LOG2B, NT, NTL, 1>(a, n0, ko, p, Pf, frow, smem);
}

// Launch B, workgroup = output o: matrix_la_b_kernel over output o's parts and
// pair list -- pre = near + far, near = part[nplan[o]] + part[nplan[o] + 1] +
// ..., far = the Pf_o parts of window row t % Q in ascending order (no far term
// when Pf_o = 0), or the kept pre[o]; then the row-0 terms X[col e][current] (.)
// H[pair e][0] in ascending e with matrix_sp_b_kernel's chunk-ahead `col`
// loads, one C2R with 1/N, overlap-add.  An output without pairs has one
// all-zero near part, no far part and no terms: it writes zeros and keeps a
// zero overlap.
template <int LOG2B, int NT>
__global__ __launch_bounds__(NT) void matrix_sp_la_b_kernel(MatrixSpLaArgs a) {
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
hipError_t launch_matrix_sp_la_t(const MatrixSpLaArgs &a, hipStream_t s) {
    constexpr int NT = matrix_nt(LOG2B);
    using Gm = MGeo<LOG2B, NT>;
    using Lg = SpLaGeo<LOG2B, NT>;
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
    if (m.I <= 0 || m.O <= 0 || a.N <= 0 || m.k <= 0 || m.act <= 0 || a.PnT < m.O || m.fill < 0 ||
        m.fill + m.k > (1 << log2b) || m.cur < 0 || m.cur >= m.S || m.act > m.S || !a.rowptr || !a.col || !a.nplan ||
        !a.fplan || !a.nwg)
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
