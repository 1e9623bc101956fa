// la_batch.hpp -- the lookahead step for a call that holds its blocks in
// advance (fftconv_uniform_process_device_steps): k steps of every channel in
// four launches instead of k.
//
// The per-block launch (la.hpp) may know nothing after block s, so it
// recovers the reuse of H and FDL rows over time through windows of partial
// sums in HBM: 36.5 row transfers per cfg2 channel-block.  A k-step call has
// that reuse for free: X_t depends on input block t only, and the state
// carried from step to step is the overlap half-block and the ring position.
// So a chunk of k <= LA_BATCH_MAX steps runs as
//   1. spectra  R2C of every block (wave_r2c_post, as la_step's chain) into a
//               staging row per step -- not the ring: block t0+j overwrites
//               block t0+j-act, which the steps before it still sum;
//   2. walk     per (channel, 64-slot bin slice, window slice of JW = 16 or
//               8 steps) every chain of the canonical order with JW
//               accumulators (la_walk_x):
//               levels 3 and 2 in their NG groups (one wave each), then the
//               level-1 and the near chain on two waves, combined in LDS in
//               the full pass's order (la_step, anyfull) into one `pre` row
//               per step.  X for row i at chunk step j is block t0+j-i:
//               staging row j-i for i <= j, else ring row (cur0 + i - j) %
//               act as the ring stands at the chunk's start.  Each H row and
//               each FDL row is loaded once per window slice; the slices of
//               one (channel, bin slice) sit 8 workgroups apart, on one XCD,
//               whose L2 serves the rows they share (as la_anchor_far);
//   3. finish   per channel, four steps at a time (one wave each): conv =
//               slot_mac(pre_j, X_j, H[0]), the C2R error test, wave_c2r,
//               overlap-add with the overlap handed from step to step in
//               LDS, the output; X_j goes to ring row (cur0 - j) % act in
//               step order; then the overlap and the state word a per-block
//               run would leave (no live window);
//   4. fix-up   channels off the lookahead path at the chunk's start, and
//               channels whose C2R failed at step j (stopped there exactly
//               as la_step stops), run their remaining steps as la_fallback
//               would, one per loop turn (`resume` word per channel; the
//               workgroups of every other channel return at once).
// Every dependency is a kernel boundary on the caller's stream: no workgroup
// waits for another.  Staging and pre rows live in the window buffer laW
// (rows [0, MAX) and [MAX, 2 MAX) of the channel's 2 LA_PT), so the windows
// are dropped: the host re-enters the per-block launch with la_all.
// The arithmetic per step is the full pass's, so the bits equal the per-block
// launches'.
#pragma once
#include <hip/hip_runtime.h>

#include "la.hpp"

namespace fftconv {

static_assert(2 * LA_BATCH_MAX <= 2 * LA_PT, "staging and pre rows fit the channel's windows");
// The walk's window slice and rows in flight per lane (H and X each).  The
// walk runs at the rate of its L2 misses; 16-step slices issue
// half the row requests of 8-step ones and miss less.  16 accumulators and
// the 19-row X ring take the 256 registers of two workgroups per CU (4 rows
// in flight spill 3).  A slice costs the same whatever part of it is live and
// the grid is half the 8-step one, so short grids and calls whose last 16-step
// slice is at most half full keep the 8-step slices (4 workgroups per CU, 2
// rows in flight: 3 spill 11 of the 128 registers): lab_wide.
constexpr int LAB_JW = 16, LAB_U = 3;
constexpr int LAB_WIDE_MIN_WG = 512;  // 16-step slices from two workgroups per CU up (profiles/batch_walk/ab_calls.txt)
static_assert(LA_BATCH_MAX % LAB_JW == 0 && LAB_JW % LA_NG == 0 && LA_JW % LA_NG == 0,
              "whole window slices, split evenly over the waves");
__host__ __device__ constexpr bool lab_wide(int channels, int nsl, int k) {
    return (k - 1) % LAB_JW >= LAB_JW / 2 &&
           (channels + 7) / 8 * 8 * nsl * ((k + LAB_JW - 1) / LAB_JW) >= LAB_WIDE_MIN_WG;
}

// staging row j (the spectrum of chunk step j) / pre row j of channel c
template <int LOG2B>
__device__ __forceinline__ float2 *lab_row(const ProcArgs &a, size_t c, int j, bool pre) {
#ifdef FFTCONV_DEBUG_BOUNDS
    if (!(c < (size_t)a.la_channels && j >= 0 && j < LA_BATCH_MAX)) {
        dbg_bounds(pre ? 6 : 5, (int)c, j, a.la_channels, 0);  // (sites 5 / 6: a staging / pre row index)
        c = 0; j = 0;
    }
#endif
    return a.laW + ((c * 2 * LA_PT + (pre ? LA_BATCH_MAX : 0) + j) << LOG2B);
}

// channel c's state word at the chunk's start (no launch before the finish
// writes it), wave-uniform; true if the chunk runs the channel
template <int LOG2B>
__device__ __forceinline__ bool lab_state(const ProcJob &J, int c, int4 &st) {
    const int4 v = J.state[c];
    st = make_int4(__builtin_amdgcn_readfirstlane(v.x), __builtin_amdgcn_readfirstlane(v.y),
                   __builtin_amdgcn_readfirstlane(v.z), __builtin_amdgcn_readfirstlane(v.w));
    return la_eligible<LOG2B>(st, J.n);
}
// ring row of the chunk's step j: current steps back once per block (:287-291)
__device__ __forceinline__ int lab_cur(int cur0, int j, int act) { return ((cur0 - j) % act + act) % act; }
// launch tag of chunk step j: the per-block launches alternate 1 / 2
__device__ __forceinline__ int lab_seq(const LaBatchArgs &bt, int j) { return (j & 1) ? 3 - bt.seq0 : bt.seq0; }

// ---------------------------------------------------------------------------
// 1. spectra: one wave per (channel, step)
// ---------------------------------------------------------------------------
template <int LOG2B>
struct LabSpectra {
    static constexpr int B = 1 << LOG2B;
    static constexpr size_t tw_bytes = 12 * (size_t)B;  // (LaStep::tw_bytes: the 1.5 B float2 the transforms index)
    static constexpr size_t bytes = tw_bytes + 4 * 2 * (size_t)B * sizeof(float2);
};
template <int LOG2B>
__global__ __launch_bounds__(LA_NT, 4) void la_batch_spectra_kernel(ProcArgs a, LaBatchArgs bt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int B = 1 << LOG2B;
    const ProcJob &J = a.job[0];
    const int c = (int)blockIdx.x;
    const int lane = (int)(threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int j = (int)blockIdx.y * 4 + wave;
    int4 st;
    const bool ok = lab_state<LOG2B>(J, c, st);
    if (blockIdx.y == 0 && threadIdx.x == 0) bt.resume[c] = ok ? bt.k : 0;  // (off the path: the fix-up runs every step)
    if (!ok || j >= bt.k) return;
    float2 *twl = reinterpret_cast<float2 *>(smem);
    float2 *bufA = reinterpret_cast<float2 *>(smem + LabSpectra<LOG2B>::tw_bytes) + (size_t)wave * 2 * B;
    float2 *bufB = bufA + B;
    const float *inc = J.in + (size_t)c * J.in_stride + (long long)j * bt.in_step;
    dma_f32<64>(reinterpret_cast<float *>(bufA), inc, B);  // x[0..B) as packed z[0..B/2)
    for (int m = B / 2 + lane; m < B; m += 64) bufA[m] = make_float2(0.f, 0.f);
    dma_16b<64>(twl, a.tw, (int)LabSpectra<LOG2B>::tw_bytes);  // (every wave: the same bytes, no barrier)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wave_sync();
    wave_r2c_post<LOG2B, 0, const float2 *, false, false>(bufA, bufB, twl, nullptr, lab_row<LOG2B>(a, (size_t)c, j, false));
}

// ---------------------------------------------------------------------------
// 2. walk
// ---------------------------------------------------------------------------
// la_walk_x's X source: ages >= 0 from the ring as it stands at the chunk's
// start (cur = the ring position one step before the chunk's first step:
// la_anchor_state's rebuild convention), ages < 0 -- blocks of this chunk --
// from the staging rows
template <int LOG2B>
struct LabX {
    RowStream ring, stg;
    int cur, act;
    template <bool NTL>
    __device__ __forceinline__ float4 ld(int voff, int age) const {
        constexpr int ROWB = (1 << LOG2B) * (int)sizeof(float2);
        const bool old = age >= 0;
        int r = cur + age;
        if (r >= act) r -= act;
        int row = old ? r : -age - 1;
#ifdef FFTCONV_DEBUG_BOUNDS
        if (!old && row >= LA_BATCH_MAX && voff != LA_OOB) {
            dbg_bounds(5, row, age, cur, act);  // (site 5: a staging row index)
            row = 0;
        }
#endif
        RowStream s = ring;
        if (!old) s = stg;
        return s.ld4<NTL>(voff, row * ROWB);
    }
};

template <int LOG2B, int JW>
struct LabWalk {
    // the groups' sums [NG][JW][FS] | W2 + W3 of the slice's steps [JW][FS] (float4): 5 KB per step
    static constexpr size_t red_bytes = (size_t)LA_NG * JW * LaGeo<LOG2B>::FS * 16;
    static constexpr size_t bytes = red_bytes + (size_t)JW * LaGeo<LOG2B>::FS * 16;
};
template <int LOG2B, int JW, int U, int WPC>
__global__ __launch_bounds__(LA_NT, WPC) void la_batch_walk_kernel(ProcArgs a, LaBatchArgs bt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using LG = LaGeo<LOG2B>;
    constexpr int B = LG::B, FS = LG::FS, NSL = LG::NSL, NG = LA_NG;
    constexpr int ROWB = B * (int)sizeof(float2);
    const ProcJob &J = a.job[0];
    // XCD-aware, as la_anchor_far: the workgroups of one (channel, bin slice)
    // sit 8 apart in the grid, on one XCD
    const int wga = NSL * ((bt.k + JW - 1) / JW);
    const int b = (int)blockIdx.x, x = b & 7, y = b >> 3;
    const int c = (y / wga) * 8 + x, r = y % wga;
    if (c >= a.la_channels) return;  // (padding of the last XCD round)
    int4 st;
    if (!lab_state<LOG2B>(J, c, st)) return;
    const int cur0 = st.x, act = st.y;
    const int h = r / NSL;  // window slice: chunk steps h*JW .. h*JW+JW-1
    const int tid = (int)threadIdx.x;
    const int l = __builtin_amdgcn_readfirstlane(tid / FS), fl = tid % FS;
    const int f = (r % NSL) * FS + fl;  // bin slice
    const size_t rows = (size_t)J.S * B;
    const size_t bytes = rows * sizeof(float2);
    const RowStream hs(J.H + (size_t)c * rows, bytes);
    const LabX<LOG2B> xs{RowStream(J.X + (size_t)c * rows, bytes),
                         RowStream(lab_row<LOG2B>(a, (size_t)c, 0, false), (size_t)LA_BATCH_MAX * ROWB),
                         cur0 + 1 == act ? 0 : cur0 + 1, act};
    float4 *red = reinterpret_cast<float4 *>(smem);  // [NG][JW][FS]
    // W3, then W2 + W3, of the JW / NG steps this wave combines (each entry is
    // written and read by one thread; in LDS to keep the walk's registers free)
    float4 *w23 = reinterpret_cast<float4 *>(smem + LabWalk<LOG2B, JW>::red_bytes);
    const int nlv = a.la_nlv;
    // phase 0: level 3, phase 1: level 2 (group l on wave l), phase 2: the
    // level-1 chain (wave 0) and the near chain (wave 1)
#pragma nounroll
    for (int ph = nlv == 3 ? 0 : 1; ph < 3; ++ph) {
        int lo = 0, hi = 0;
        bool asc = false;
        if (ph < 2) {
            la_group(3 - ph, l, act, lo, hi);
            asc = la_asc(l);
        } else if (l == 0) {
            lo = LA_D0 + 1;
            hi = la_hi(1, act);
        } else if (l == 1) {
            lo = 1;
            hi = LA_D0 + 1;
        }
        LaAcc acc[JW];
#pragma unroll
        for (int j = 0; j < JW; ++j) acc[j].zero();
        if (hi > lo) {
            if (asc) la_walk_x<LOG2B, true, false, JW, U>(acc, hs, xs, f * 16, f == 0, lo, hi, h * JW);
            else la_walk_x<LOG2B, false, false, JW, U>(acc, hs, xs, f * 16, f == 0, lo, hi, h * JW);
        }
        __syncthreads();  // (the previous phase's sums are read)
#pragma unroll
        for (int j = 0; j < JW; ++j) red[(l * JW + j) * FS + fl] = acc[j].get();
        __syncthreads();
#pragma unroll
        for (int t = 0; t < JW / NG; ++t) {
            const int j = (JW / NG) * l + t;
            if (ph < 2) {  // the level's groups in group order, as the anchors combine them
                float4 p = red[j * FS + fl];
#pragma unroll
                for (int q = 1; q < NG; ++q) p = vadd(p, red[(q * JW + j) * FS + fl]);
                w23[j * FS + fl] = (ph == 1 && nlv == 3) ? vadd(p, w23[j * FS + fl]) : p;
            } else {  // pre = near + (W1 + (W2 + W3))
                const float4 W1 = red[j * FS + fl], N0 = red[(JW + j) * FS + fl];
                const int w = h * JW + j;
                if (w < bt.k)  // (a partial last slice stores its live steps)
                    la_wst(reinterpret_cast<float4 *>(lab_row<LOG2B>(a, (size_t)c, w, true)) + f, vadd(N0, vadd(W1, w23[j * FS + fl])));
            }
        }
    }
}

// ---------------------------------------------------------------------------
// 3. finish
// ---------------------------------------------------------------------------
// c2r_rejects (step.hpp) for chunk step j before the ring holds the chunk's
// blocks: row i of the step's ring is staging row j - i, or for i > j the
// ring row (cur0 + i - j) % act, which no earlier step of the chunk rewrites
static __device__ __attribute__((noinline, unused)) bool lab_c2r_rejects(const float2 *Hc, const float2 *Xc,
                                                                         const float2 *Sc, int B, int cur0, int j,
                                                                         int act, float2 pre0, float2 x0, float2 h0) {
    if (!slot0_finite(x0) || !slot0_finite(h0)) return true;
    if (slot0_finite(pre0)) return false;
    for (int i = 1; i < act; ++i) {
        float2 xv;
        if (i <= j) {
            xv = Sc[(size_t)(j - i) * B];
        } else {
            int r = cur0 + i - j;
            if (r >= act) r -= act;
            xv = Xc[(size_t)r * B];
        }
        if (!slot0_finite(Hc[(size_t)i * B]) || !slot0_finite(xv)) return true;
    }
    return false;
}

template <int LOG2B>
struct LabFinish {
    static constexpr int B = 1 << LOG2B;
    static constexpr size_t tw_bytes = 12 * (size_t)B;
    static constexpr size_t wave_bytes = 2 * (size_t)B * sizeof(float2);  // conv / C2R ping-pong
    static constexpr size_t carry_off = tw_bytes + 4 * wave_bytes;        // the overlap handed on [B]
    static constexpr size_t err_off = carry_off + (size_t)B * sizeof(float);
    static constexpr size_t bytes = err_off + 16;
};
template <int LOG2B>
__global__ __launch_bounds__(LA_NT, 4) void la_batch_finish_kernel(ProcArgs a, LaBatchArgs bt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using LF = LabFinish<LOG2B>;
    constexpr int B = 1 << LOG2B, F = B / 2, NF = F / 64;
    constexpr float invN = 1.0f / (float)(2 * B);
    const ProcJob &J = a.job[0];
    const int c = (int)blockIdx.x;
    int4 st;
    if (!lab_state<LOG2B>(J, c, st)) return;
    const int cur0 = st.x, act = st.y, flags = st.w;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float2 *twl = reinterpret_cast<float2 *>(smem);
    float2 *Z = reinterpret_cast<float2 *>(smem + LF::tw_bytes + (size_t)wave * LF::wave_bytes), *P = Z + B;
    float *carry = reinterpret_cast<float *>(smem + LF::carry_off);
    int *errf = reinterpret_cast<int *>(smem + LF::err_off);
    const size_t rows = (size_t)J.S * B;
    const float2 *Hc = J.H + (size_t)c * rows;
    float2 *Xc = J.X + (size_t)c * rows;
    const float2 *Sc = lab_row<LOG2B>(a, (size_t)c, 0, false);
    float *ovc = J.overlap + (size_t)c * B;
    dma_16b<LA_NT>(twl, a.tw, (int)LF::tw_bytes);
    dma_f32<LA_NT>(carry, ovc, B);
    float4 h0r[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) h0r[i] = reinterpret_cast<const float4 *>(Hc)[lane + 64 * i];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int stop = bt.k;  // the first step whose C2R fails
    for (int j0 = 0; j0 < bt.k && stop == bt.k; j0 += 4) {
        const int j = j0 + wave;
        const bool live = j < bt.k;
        const int cj = live ? lab_cur(cur0, j, act) : 0;
        DBG_CHECK(cj >= 0 && cj < J.S, 2, c, cj, j, act);  // (site 2: a step chain's ring row)
        float4 xr[NF];
        bool bad = false;
        if (live) {  // conv = pre + X (.) H[0] (:256-261), then the C2R error check
            const float4 *pr = reinterpret_cast<const float4 *>(lab_row<LOG2B>(a, (size_t)c, j, true));
            const float4 *xq = reinterpret_cast<const float4 *>(lab_row<LOG2B>(a, (size_t)c, j, false));
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                const int f = lane + 64 * i;
                const float4 pv = pr[f];
                xr[i] = xq[f];
                const float4 cv = slot_mac(pv, xr[i], h0r[i], f);
                reinterpret_cast<float4 *>(Z)[f] = cv;
                if (f == 0 && !slot0_finite(cv) &&
                    lab_c2r_rejects(Hc, Xc, Sc, B, cur0, j, act, slot0_of(pv), slot0_of(xr[i]), slot0_of(h0r[0])))
                    bad = true;
            }
        }
        const bool err = __ballot(bad) != 0ull;
        if (lane == 0) errf[wave] = err ? 1 : 0;
        const float *y = nullptr;
        if (live && !err) {
            wave_sync();
            y = wave_c2r<LOG2B>(Z, P, Z, twl);
        }
        __syncthreads();  // every wave's C2R result and error word
        for (int w = 3; w >= 0; --w)
            if (errf[w]) stop = j0 + w;
        if (live && j <= stop) {
            // the block's spectrum into ring row `current`, in step order (the
            // barriers order the rounds; a failed step has written it too)
            float4 *xrow = reinterpret_cast<float4 *>(Xc + (size_t)cj * B);
#pragma unroll
            for (int i = 0; i < NF; ++i) xrow[lane + 64 * i] = xr[i];
        }
        float *outc = J.out + (size_t)c * J.out_stride + (long long)j * bt.out_step;
        if (live && j < stop) {  // overlap-add (:270-274): the overlap of step j - 1
            const float *yp = y - (LF::wave_bytes / sizeof(float));  // (the wave before this one: its result)
#pragma unroll
            for (int i = 0; i < B / 64; ++i) {
                const int m = lane + 64 * i;
                const float ov = wave == 0 ? carry[m] : yp[B + m] * invN;
                la_ost(outc + m, y[m] * invN + ov);
            }
        } else if (live && j == stop) {
            // output.fill(0); return (:264-267): the block stays in the input
            // buffer, fill / current unchanged (la_step's error path)
            const float *inc = J.in + (size_t)c * J.in_stride + (long long)j * bt.in_step;
            float *ibc = J.inbuf + (size_t)c * B;
            for (int m = lane; m < B; m += 64) {
                ibc[m] = inc[m];  // (before the output: a caller's output may alias its input)
                outc[m] = 0.f;
            }
        }
        __syncthreads();  // the overlaps above are read
        const int last = min(stop, min(bt.k, j0 + 4)) - 1;  // the last completed step
        if (live && j == last) {
#pragma unroll
            for (int i = 0; i < B / 64; ++i) carry[lane + 64 * i] = y[B + lane + 64 * i] * invN;  // :283-284
        }
    }
    __syncthreads();
    for (int m = tid; m < B; m += LA_NT) la_ost(ovc + m, carry[m]);
    if (tid == 0) {
        const int done = min(stop, bt.k);  // completed steps
        int nf = flags & ~(FLAG_INBUF | FLAG_PRE | LA_MASK | SEQ_MASK);
        if (done & 1) nf ^= FLAG_REV;
        if (stop < bt.k) {
            nf |= FLAG_INBUF | (lab_seq(bt, stop) << SEQ_SHIFT);
            bt.resume[c] = stop + 1;  // the fix-up runs the steps after the failed one
        } else {
            nf |= lab_seq(bt, bt.k - 1) << SEQ_SHIFT;
        }
        J.state[c] = make_int4(lab_cur(cur0, done, act), act, 0, nf);
    }
}

// ---------------------------------------------------------------------------
// 4. fix-up: steps [resume, k) of channel c, each exactly as a per-block
// launch without anchors runs a channel off the path: la_fallback (the
// generic step, or the lookahead step with the full pass once the channel is
// back on the path).  la_fallback reads its launch's arguments through a
// pointer; here that is a copy in LDS, behind the step's own LDS, in which
// thread 0 advances the block pointers and the launch tag from step to step.
// ---------------------------------------------------------------------------
template <int LOG2B>
struct LabFixup {
    static constexpr size_t gen = Geo<LOG2B, LA_NT>::lds_bytes, lsb = LaStep<LOG2B>::bytes;
    static constexpr size_t args_off = ((lsb > gen ? lsb : gen) + 15) / 16 * 16;
    static constexpr size_t bytes = args_off + (sizeof(ProcArgs) + 15) / 16 * 16;
};
// (out of line, the launch's arguments by their kernarg address: the workgroups
// with nothing to do -- every one in the common call -- leave before any of
// this is set up)
template <int LOG2B, bool NTL>
static __device__ __attribute__((noinline)) void lab_fixup(const ProcArgs *ap, LaBatchArgs bt, int c, int j0,
                                                          unsigned char *smem) {
    ProcArgs *al = reinterpret_cast<ProcArgs *>(smem + LabFixup<LOG2B>::args_off);
    for (int j = j0; j < bt.k; ++j) {
        if (threadIdx.x == 0) {
            if (j == j0) *al = *ap;  // (la_all < 0: no anchors, no window is opened)
            al->job[0].in = ap->job[0].in + (long long)j * bt.in_step;
            al->job[0].out = ap->job[0].out + (long long)j * bt.out_step;
            al->la_seq = lab_seq(bt, j);
        }
        __syncthreads();
        la_fallback<LOG2B, NTL, 0>(al, c, 1, smem);
        __syncthreads();  // (the next step reads what this one stored)
    }
}
template <int LOG2B, bool NTL>
__global__ __launch_bounds__(LA_NT, 4) void la_batch_fixup_kernel(ProcArgs a, LaBatchArgs bt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int c = (int)blockIdx.x;
    const int j0 = __builtin_amdgcn_readfirstlane(bt.resume[c]);
    if (j0 >= bt.k) return;
    lab_fixup<LOG2B, NTL>((const ProcArgs *)__builtin_amdgcn_kernarg_segment_ptr(), bt, c, j0, smem);
}

}  // namespace fftconv
