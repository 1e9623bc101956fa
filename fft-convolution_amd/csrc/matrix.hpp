// matrix.hpp -- the device roles every matrix family is composed of (DESIGN
// §4s): the geometry, the R2C role, ONE row walk (the MAC of launch A, plain
// and near), ONE far walk (the lookahead families' windows) and what follows the
// sums in the finish (launch B: C2R, overlap-add, overlap save, the two-stage
// epilogue).  The walks are templates over a ROW SOURCE -- the dense matrix's
// inputs 0..I-1 (DenseRows, below) or an output's pair list (ListedRows,
// matrix_sp.hpp) -- and over the H streams.  One definition, so every family
// sums the same rows in the same order through the same Acc2::mac: the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

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
    static constexpr size_t lds_a_pair = fft_bytes > 2 * red_bytes ? fft_bytes : 2 * red_bytes;  // (two H streams)
};

// launch A of the lookahead families (matrix_la.hip, matrix_sp_la.hip)
template <int LOG2B, int NT>
struct LaGeo {
    using Gm = MGeo<LOG2B, NT>;
    static_assert(Gm::SPT == 1, "one 16-byte slot per thread");
    // the anchor's group reduction: Q accumulators of every thread
    static constexpr size_t red_bytes = Gm::G > 1 ? (size_t)kMatrixLaQ * NT * sizeof(float4) : 0;
    static constexpr size_t lds_a = Gm::lds_a > red_bytes ? Gm::lds_a : red_bytes;
};

constexpr int matrix_nt(int log2b) { return log2b <= 10 ? 256 : 512; }

// what every launch_*_chunk / _block checks of {I, O, k, act, fill, cur, S}
// (a whole block: fill 0, k = B)
inline bool matrix_chunk_in_range(int log2b, int I, int O, int S, int cur, int act, int fill, int k) {
    return I > 0 && O > 0 && k > 0 && act > 0 && fill >= 0 && fill + k <= (1 << log2b) && cur >= 0 && cur < S && act <= S;
}

// R2C role of launch A, one workgroup per input, for ND destinations (the
// convolvers of a pair hold equal input buffers and delay lines): append the
// chunk `inc` to the input buffers ib[d], transform the zero-padded buffer into
// the rows row[d] = X_d[i][current] (:229-241), clear the input buffers when
// the block completes (:280).  tap(j, x) sees every sample of the buffer as it
// is read (the two-stage matrix's copy into tail_input).  A whole block is
// (fill 0, k = B) as constants: the input buffers are then neither read nor
// written.  (Every store goes to the last destination first.)
template <int LOG2B, int NT, int ND, class Tap>
__device__ __forceinline__ void matrix_r2c(const float2 *tw, const float *inc, float *const (&ib)[ND],
                                           float2 *const (&row)[ND], int fill, int k, unsigned char *smem, Tap tap) {
    constexpr int B = 1 << LOG2B;
    float2 *bufA = reinterpret_cast<float2 *>(smem);
    float2 *bufB = bufA + B;
    const int tid = threadIdx.x;
    auto sample = [&](int j) -> float {
        if (j < fill) return ib[0][j];
        if (j < fill + k) return inc[j - fill];
        return 0.f;
    };
    for (int m = tid; m < B; m += NT) {
        float2 z = make_float2(0.f, 0.f);
        if (2 * m < B) {
            z.x = sample(2 * m);
            z.y = sample(2 * m + 1);
            tap(2 * m, z.x);
            tap(2 * m + 1, z.y);
        }
        bufA[m] = z;
    }
    __syncthreads();  // (every read of ib[i] is done)
    if (fill + k == B) {
        if (fill > 0)
            for (int j = tid; j < B; j += NT)
#pragma unroll
                for (int d = ND - 1; d >= 0; --d) ib[d][j] = 0.f;
    } else {
        for (int j = tid; j < k; j += NT) {
            const float x = inc[j];
#pragma unroll
            for (int d = ND - 1; d >= 0; --d) ib[d][fill + j] = x;
        }
    }
    const float2 *Z = lds_cfft<LOG2B, NT, false>(bufA, bufB, tw);
    for (int m = tid; m < B; m += NT) {
        const float2 z = real_post<LOG2B, NT>(Z, m, tw);
#pragma unroll
        for (int d = ND - 1; d >= 0; --d) row[d][m] = z;
    }
}
struct NoTap {
    __device__ __forceinline__ void operator()(int, float) const {}
};
// the plain chunk of one convolver
template <int LOG2B, int NT>
__device__ __forceinline__ void matrix_r2c(const MatrixArgs &a, int i, unsigned char *smem) {
    constexpr int B = 1 << LOG2B;
    const int fill = a.fill, k = a.k;
    const float *inc = a.in + (long long)i * a.in_stride;
    float *const ib[1] = {a.ib + (size_t)i * B};
    float2 *const row[1] = {a.X + ((size_t)i * a.S + a.cur) * B};
    matrix_r2c<LOG2B, NT, 1>(a.tw, inc, ib, row, fill, k, smem, NoTap{});
}
// the chunk of a pair's two convolvers (MatrixXfArgs, MatrixSpXfArgs)
template <int LOG2B, int NT, class Args>
__device__ __forceinline__ void matrix_r2c_pair(const Args &a, int i, unsigned char *smem) {
    constexpr int B = 1 << LOG2B;
    const int fill = a.fill, k = a.k;
    const float *inc = a.in + (long long)i * a.in_stride;
    float *const ib[2] = {a.ib[0] + (size_t)i * B, a.ib[1] + (size_t)i * B};
    const size_t at = ((size_t)i * a.S + a.cur) * B;
    float2 *const row[2] = {a.X[0] + at, a.X[1] + at};
    matrix_r2c<LOG2B, NT, 2>(a.tw, inc, ib, row, fill, k, smem, NoTap{});
}
// a whole block for the head's and tail0's delay lines, copied into tail_input
// (src/fft_convolver.rs:459-461) from the registers that feed the transform
// (MatrixTsArgs, MatrixSpTsArgs)
template <int LOG2B, int NT, class Args>
__device__ __forceinline__ void matrix_r2c_block(const Args &a, int i, unsigned char *smem) {
    constexpr int B = 1 << LOG2B;
    const float *inc = a.in + (long long)i * a.in_stride;
    float *tic = a.tin + (long long)i * a.T;
    float *const ib[2] = {nullptr, nullptr};
    const size_t at = ((size_t)i * a.S + a.cur) * B;
    float2 *const row[2] = {a.X[0] + at, a.X[1] + at};
    matrix_r2c<LOG2B, NT, 2>(a.tw, inc, ib, row, 0, B, smem, [&](int j, float x) { tic[j] = x; });
}

// What a walk reads and writes: NH H streams that share one delay line (the
// crossfaded matrix's A and B, the two-stage matrix's head and tail0: X[1]
// equals X[0] row for row, so every X row is loaded once, from X[0]), one
// destination of partial sums per stream.  Views of the kernel's argument
// block, read where the walk uses them.
struct MacStreams {  // one matrix (MatrixArgs, or the `m` of the sparse and lookahead blocks)
    static constexpr int NH = 1;
    const MatrixArgs &a;
    __device__ __forceinline__ const float2 *H(int) const { return a.H; }
    __device__ __forceinline__ const float2 *X() const { return a.X; }
    __device__ __forceinline__ float2 *out(int) const { return a.part; }
    __device__ __forceinline__ int I() const { return a.I; }
    __device__ __forceinline__ int S() const { return a.S; }
    __device__ __forceinline__ int act() const { return a.act; }
    __device__ __forceinline__ int cur() const { return a.cur; }
};
template <class Args>
struct MacStreamsOf {  // convolver c of a pair's argument block (H[2], X[2], part[2])
    static constexpr int NH = 1;
    const Args &a;
    int c;
    __device__ __forceinline__ const float2 *H(int) const { return a.H[c]; }
    __device__ __forceinline__ const float2 *X() const { return a.X[c]; }
    __device__ __forceinline__ float2 *out(int) const { return a.part[c]; }
    __device__ __forceinline__ int I() const { return a.I; }
    __device__ __forceinline__ int S() const { return a.S; }
    __device__ __forceinline__ int act() const { return a.act; }
    __device__ __forceinline__ int cur() const { return a.cur; }
};
template <class Args>
struct MacStreamsPair {  // both convolvers of a pair
    static constexpr int NH = 2;
    const Args &a;
    __device__ __forceinline__ const float2 *H(int h) const { return a.H[h]; }
    __device__ __forceinline__ const float2 *X() const { return a.X[0]; }
    __device__ __forceinline__ float2 *out(int h) const { return a.part[h]; }
    __device__ __forceinline__ int I() const { return a.I; }
    __device__ __forceinline__ int S() const { return a.S; }
    __device__ __forceinline__ int act() const { return a.act; }
    __device__ __forceinline__ int cur() const { return a.cur; }
};
struct FarStreams : MacStreams {  // one matrix, the partial sums into the far windows
    float2 *far;
    __device__ __forceinline__ float2 *out(int) const { return far; }
};

// Row source of the dense matrix, workgroup (output o, part p) of P: index e
// of the walk is input e, the output's H rows start at pair o * I, its partial
// sum is row o * P + p, the rows per part come from the arguments.
struct DenseRows {
    static constexpr bool kListed = false;
    int I, o, p, P, rows_per_part;
    __device__ __forceinline__ int count() const { return I; }
    __device__ __forceinline__ size_t first_pair() const { return (size_t)o * I; }
    __device__ __forceinline__ size_t out_row() const { return (size_t)o * P + p; }
    __device__ __forceinline__ int rpp(long long) const { return rows_per_part; }
    __device__ __forceinline__ int col(int) const { return 0; }
};
// workgroup m = o * P + p of a dense MAC grid (Args: I, O, P, rpp; site: a part
// past `part`)
template <class Args>
__device__ __forceinline__ DenseRows dense_rows(const Args &a, int m, int site) {
    const int o = m / a.P, p = m % a.P;
    DBG_CHECK(o >= 0 && o < a.O && p >= 0 && p < a.P, site, o, p, a.O, a.P);
    return {a.I, o, p, a.P, a.rpp};
}

// fn(0), fn(1), ... for the N <= 2 H streams of a walk, expanded when the
// template is instantiated and not by the loop unroller: as loops over h the
// two-stream walk takes 4 more VGPRs at B >= 1024 and loses a wave per SIMD with
// nontemporal loads; this form compiles to the hand-written
// two-stream walk's code.
template <int N, class Fn>
__device__ __forceinline__ void each_stream(Fn fn) {
    static_assert(N == 1 || N == 2, "one or two H streams");
    fn(0);
    if constexpr (N == 2) fn(1);
}

// THE ROW WALK: the MAC role of launch A for one part of one output.  With nb
// rows per index (active - 1 for the plain matrices; min(Q, active) - 1 for the
// near rows of the lookahead ones) the rows H[e][s] (.) X[input of e][(current
// + s) % active], 1 <= s <= nb, are flattened index-major as r = e * nb + s - 1;
// part p sums rows [p * rpp, (p + 1) * rpp) into its partial sum.  Group g of
// the workgroup takes the part's rows g, g + G, ... in ascending order, the
// groups are added in ascending g: a function of (row count, B, active, P)
// only.  Every X row is multiplied with the NH H streams into NH accumulator
// sets, each in the one-stream order.  (The plain U rows in flight still compile
// without scratch with three streams per row instead of two.)
//
// The two row sources advance differently, on purpose: the dense walk steps `e`
// in a plain loop; the listed walk reloads the row's input `col[e]` only where
// it moves to another pair (lanes of one wave hold different e at B <= 256, so
// it is a per-lane load: measured against a load per row ahead of each batch,
// SP1's launch A is 8 % faster this way and SP2's the same).
// SITE: the walk's DBG_CHECK sites -- SITE a MAC row past H / X, SITE + 2 a
// `col` entry >= I (SITE + 1 is the row source's own check).
template <int LOG2B, int NT, bool NTL, int SITE, class Rows, class Streams>
__device__ __forceinline__ void matrix_row_walk(const Rows &rw, const Streams &st, int nb, unsigned char *smem) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int F = Gm::F, G = Gm::G, SPT = Gm::SPT, U = Gm::U, NH = Streams::NH;
    const int tid = threadIdx.x;
    const int f0 = G > 1 ? tid % F : tid;
    const int g = G > 1 ? tid / F : 0;
    const int act = st.act(), n = rw.count();
    const long long R = (long long)n * nb;
    const auto rpp = rw.rpp(R);
    const long long r0 = (long long)rw.p * rpp;
    const long long r1 = r0 + rpp < R ? r0 + rpp : R;
    const int cm = st.cur() % act;  // (current may exceed active after an update, :248)
    const int S = st.S();
    const size_t hbase = rw.first_pair() * S * F;
    const float4 *H4[NH];
    each_stream<NH>([&](int h) { H4[h] = reinterpret_cast<const float4 *>(st.H(h)) + hbase; });
    const float4 *X4 = reinterpret_cast<const float4 *>(st.X());

    Acc2 acc[NH][SPT];
#pragma unroll
    for (int s = 0; s < SPT; ++s) each_stream<NH>([&](int h) { acc[h][s].zero(); });
    long long r = r0 + g;
    int e = 0, s = 1;
    if (nb > 0) {
        e = (int)(r / nb);
        s = 1 + (int)(r % nb);
    }
    int c = 0;
    if constexpr (Rows::kListed) c = e < n ? rw.col(e) : 0;  // (a group past the part's rows reads nothing)
    auto advance = [&]() {
        r += G;
        s += G;
        if constexpr (Rows::kListed) {
            if (s > nb) {
                do {
                    s -= nb;
                    ++e;
                } while (s > nb);
                c = e < n ? rw.col(e) : 0;
            }
        } else {
            while (s > nb) {
                s -= nb;
                ++e;
            }
        }
    };
    // The H row of the walk's position.  One stream: its pointer, formed before
    // the X row's.  Two streams: ONE row offset kept for both and added to each
    // base at the load -- two pointers cost 6 VGPRs and, at B <= 256, a wave per
    // SIMD.
    using HRow = typename std::conditional<NH == 1, const float4 *, size_t>::type;
    auto hrow = [&]() -> HRow {
        DBG_CHECK(e >= 0 && e < n && s >= 1 && s < S, SITE, e, s, n, S);
        const size_t off = ((size_t)e * S + s) * F + f0;
        if constexpr (NH == 1) {
            return H4[0] + off;
        } else {
            return off;
        }
    };
    auto hload = [&](HRow hr, int h, int q) {
        if constexpr (NH == 1) {
            return ld4<NTL>(hr + q * NT);
        } else {
            return ld4<NTL>(H4[h] + hr + q * NT);
        }
    };
    auto xrow = [&]() {
        if constexpr (Rows::kListed) DBG_CHECK(c >= 0 && c < st.I(), SITE + 2, c, e, st.I(), (int)rw.out_row());
        int xi = cm + s;
        if (xi >= act) xi -= act;
        return X4 + ((size_t)(Rows::kListed ? c : e) * S + xi) * F + f0;
    };
    while (r + (long long)(U - 1) * G < r1) {
        float4 hv[NH][U][SPT], xv[U][SPT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const HRow hr = hrow();
            const float4 *xp = xrow();
#pragma unroll
            for (int q = 0; q < SPT; ++q) {
                each_stream<NH>([&](int h) { hv[h][u][q] = hload(hr, h, q); });
                xv[u][q] = ld4<false>(xp + q * NT);
            }
            advance();
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < SPT; ++q)
                each_stream<NH>([&](int h) { acc[h][q].mac(hv[h][u][q], xv[u][q]); });
    }
    while (r < r1) {
        const HRow hr = hrow();
        const float4 *xp = xrow();
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
            const float4 x = ld4<false>(xp + q * NT);
            each_stream<NH>([&](int h) { acc[h][q].mac(hload(hr, h, q), x); });
        }
        advance();
    }

    float4 *dst[NH];
    each_stream<NH>([&](int h) { dst[h] = reinterpret_cast<float4 *>(st.out(h)) + rw.out_row() * F; });
    if constexpr (G > 1) {
        float4 *red = reinterpret_cast<float4 *>(smem);  // [NH][G][F]
        each_stream<NH>([&](int h) { red[h * NT + g * F + f0] = acc[h][0].get(f0); });
        __syncthreads();
        if (tid < F) {
            each_stream<NH>([&](int h) {
                float4 v = red[h * NT + f0];
#pragma unroll
                for (int q = 1; q < G; ++q) v = vadd(v, red[h * NT + q * F + f0]);
                dst[h][f0] = v;
            });
        }
    } else {
#pragma unroll
        for (int q = 0; q < SPT; ++q)
            each_stream<NH>([&](int h) { dst[h][f0 + q * NT] = acc[h][q].get(f0 + q * NT); });
    }
}

// THE FAR WALK: the far role of launch A of the lookahead families, one
// workgroup = (output o, far part p), window length W.  The rows (e, s), Q <= s
// < active, are flattened index-major as r = e * (active - Q) + s - Q; part p
// holds rows [p * rppf, (p + 1) * rppf), group g of the workgroup the CONTIGUOUS
// rows [g * rpg, (g + 1) * rpg) of the part in ascending order, the groups are
// added in ascending g.  Accumulator j < W is the sum of block t + j: row (e, s)
// meets X[input of e][(current - j + s) % active], the FDL row that block t + j
// finds at (its current + s) % active.  The W rows X[..][current + s - W + 1 ..
// current + s] of a step slide by one row per step, so a step loads one H row
// and one X row for W MACs.  W = 1 is the plain far sum of block t; W = Q the
// anchor.  Accumulator j visits the rows in the order, and through the same
// Acc2::mac, as the W = 1 walk of block t + j: the same bits.  Partial sums go
// to window row (t + j) % Q of far row rw.out_row().  One turn of the outer loop
// covers the rows of one index; a listed source loads that turn's input one
// turn ahead.
// SITE: SITE a far row past H / X, SITE + 2 a ring index >= active, SITE + 3 a
// `col` entry >= I (SITE + 1 is the caller's check of the window row).
template <int LOG2B, int NT, bool NTL, int W, int SITE, class Rows>
__device__ __forceinline__ void matrix_far_walk(const Rows &rw, const FarStreams &st, long long t, unsigned char *smem) {
    using Gm = MGeo<LOG2B, NT>;
    constexpr int F = Gm::F, G = Gm::G, Q = kMatrixLaQ;
    constexpr int UB = 8;  // rows in flight (a multiple of the slide of one row per step)
    const int tid = threadIdx.x;
    const int f0 = G > 1 ? tid % F : tid;
    const int g = G > 1 ? tid / F : 0;
    const int S = st.S(), act = st.act(), nf = act - Q;  // far rows per index, > 0
    const int n = rw.count();
    const long long R = (long long)n * nf;
    const auto rppf = rw.rpp(R);
    const long long r0 = (long long)rw.p * rppf;
    const long long r1 = r0 + rppf < R ? r0 + rppf : R;
    const auto rpg = (rppf + G - 1) / G;
    const long long q0 = r0 + (long long)g * rpg;
    const long long q1 = q0 + rpg < r1 ? q0 + rpg : r1;
    const int cm = st.cur() % act;  // (W > 1 runs only while current < active)
    const float4 *H4 = reinterpret_cast<const float4 *>(st.H(0)) + rw.first_pair() * S * F + f0;
    const float4 *X4 = reinterpret_cast<const float4 *>(st.X()) + f0;

    Acc2 acc[W];
#pragma unroll
    for (int j = 0; j < W; ++j) acc[j].zero();
    long long r = q0;
    int cnext = 0;
    if constexpr (Rows::kListed) cnext = r < q1 ? rw.col((int)(r / nf)) : 0;
    while (r < q1) {  // one index per turn
        const int e = (int)(r / nf);
        const int s0 = Q + (int)(r % nf);
        const long long left = q1 - r;
        const int len = left < (long long)(act - s0) ? (int)left : act - s0;
        DBG_CHECK(e >= 0 && e < n && s0 >= Q && s0 + len <= S, SITE, e, s0, len, S);
        int c = e;
        if constexpr (Rows::kListed) {
            c = cnext;
            if (r + len < q1) cnext = rw.col(e + 1);  // (the next turn starts pair e + 1 <= k_o - 1)
            DBG_CHECK(c >= 0 && c < st.I(), SITE + 3, c, e, st.I(), (int)rw.out_row());
        }
        const float4 *Hp = H4 + ((size_t)e * S + s0) * F;
        const float4 *Xi = X4 + (size_t)c * S * F;
        auto xrow = [&](int k) {  // FDL row of block t - k
            int xi = cm + k;
            if (xi >= act) xi -= act;
            DBG_CHECK(k >= 1 && xi >= 0 && xi < act, SITE + 2, k, xi, act, cm);
            return Xi + (size_t)xi * F;
        };
        // v[m] = X row of step n - (W - 1) + m: the W - 1 rows before the
        // batch, then the batch's own
        float4 v[UB + W - 1];
#pragma unroll
        for (int k = 0; k < UB + W - 1; ++k) v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < W - 1; ++k) v[k] = ld4<false>(xrow(s0 - (W - 1) + k));
        for (int m = 0; m < len; m += UB) {
            float4 hv[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                if (m + u < len) {
                    hv[u] = ld4<NTL>(Hp + (size_t)(m + u) * F);
                    v[W - 1 + u] = ld4<false>(xrow(s0 + m + u));
                }
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                if (m + u < len) {
#pragma unroll
                    for (int j = 0; j < W; ++j) acc[j].mac(hv[u], v[W - 1 + u - j]);
                }
            }
#pragma unroll
            for (int k = 0; k < W - 1; ++k) v[k] = v[k + UB];
        }
        r += len;
    }

    const int slot0 = (int)(t % Q);
    float4 *dst = reinterpret_cast<float4 *>(st.out(0)) + rw.out_row() * Q * F;
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

// ---- THE FINISH (launch B, one workgroup per output): the shared pieces ------
// conv = pre + the row-0 terms, pre = the parts of launch A summed (or the kept
// pre when the chunk starts mid-block); one C2R with 1/N (:264, :44-46);
// overlap-add (:270-274); the overlap saved when the block completes (:283-284).
// The per-slot sums (parts, window rows, row-0 terms) are each finish kernel's
// own text: written as shared helpers they compile to fewer registers and less
// memory-level parallelism, and the crossfaded matrices measured 6-15 % slower
// per block.  What follows the sums is shared by the six finishes
// with a plain or two-stage sink; the two crossfaded finishes (the mix in their
// sink) keep their whole text -- with these pieces they measured 1 % slower.

// spectrum in bufA -> the 2B samples y (unscaled)
template <int LOG2B, int NT>
__device__ __forceinline__ const float *finish_c2r(float2 *bufA, float2 *bufB, const float2 *tw) {
    constexpr int B = 1 << LOG2B;
    __syncthreads();
    for (int m = threadIdx.x; m < B; m += NT) bufB[m] = real_pre<LOG2B, NT>(bufA, m, tw);
    __syncthreads();
    return reinterpret_cast<const float *>(lds_cfft<LOG2B, NT, true>(bufB, bufA, tw));
}

// sample j of the chunk = y[fill + j] / N + overlap, handed to sink(j, v)
template <int LOG2B, int NT, class Sink>
__device__ __forceinline__ void overlap_add(const float *y, const float *ovc, int fill, int k, Sink sink) {
    constexpr float invN = 1.0f / (float)(2 << LOG2B);
    for (int j = threadIdx.x; j < k; j += NT) sink(j, y[fill + j] * invN + ovc[fill + j]);
}
// the completed block's second half becomes the overlap
template <int LOG2B, int NT>
__device__ __forceinline__ void overlap_save(const float *y, float *ovc) {
    constexpr int B = 1 << LOG2B;
    constexpr float invN = 1.0f / (float)(2 * B);
    __syncthreads();  // (every overlap read before this is done)
    for (int j = threadIdx.x; j < B; j += NT) ovc[j] = y[B + j] * invN;
}

// The epilogue of a two-stage finish, whole block, matrix c of workgroup
// (o, c): the head's samples go out with the sub-chunk sums of :438-454,
//   out[j] = ((y / N + ovl) + tail_precalculated0[pos + j]) + tail_precalculated[pos + j],
// tail0's into tail_output0[o][fill..] (:464-472); each keeps its own overlap.
// (Args: MatrixTsArgs or MatrixSpTsArgs)
template <int LOG2B, int NT, class Args>
__device__ __forceinline__ void ts_epilogue(const Args &a, int o, int c, const float *y) {
    constexpr int B = 1 << LOG2B;
    float *ovc = a.ovl[c] + (size_t)o * B;
    if (c == 0) {
        float *outc = a.out + (long long)o * a.out_stride;
        const float *p0 = a.p0 + (long long)o * a.T;
        const float *p1 = a.p1 ? a.p1 + (long long)o * a.T : nullptr;
        overlap_add<LOG2B, NT>(y, ovc, 0, B, [&](int j, float v) {  // v: the head's sample (:417)
            v += p0[j];                                              // :439-445
            if (p1) v += p1[j];                                      // :448-454
            outc[j] = v;
        });
    } else {
        float *t0c = a.tout0 + (long long)o * a.T;
        overlap_add<LOG2B, NT>(y, ovc, 0, B, [&](int j, float v) { t0c[j] = v; });
    }
    overlap_save<LOG2B, NT>(y, ovc);
}

}  // namespace fftconv
