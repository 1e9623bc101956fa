// step.hpp -- device side of the generic step: FFTConvolver::process for one
// channel, from the launch geometry (Geo) to process_job.  Shared by the
// process / run kernels (process.hip), the lookahead fallback (la.hpp), the
// crossfade pair fallback (crossfade.hip) and the tail0 replay (tail0.hip).
//
// One workgroup owns one channel (one reference FFTConvolver instance) for
// the whole call, so every piece of per-channel state stays private to a CU
// and no inter-workgroup protocol is needed.
//
// HBM layout (per uniform batch: C channels, block B, S segments):
//   H   float2 [C][S][B]  packed IR segment spectra      (segments_ir)
//   X   float2 [C][S][B]  packed frequency-domain delay line (segments)
//   ovl float  [C][B]     overlap                        (overlap)
//   ib  float  [C][B]     input buffer, only touched for partial blocks
//   pre float2 [C][B]     pre_multiplied, only touched for partial blocks
//   st  int4   [C]        {current, active_seg_count, input_buffer_fill, flags}
// A packed row is B complex = 8B bytes (slot 0 = (DC, Nyquist)), so each
// channel's H and X are contiguous 8*S*B-byte streams read with 16-byte
// loads (float4 = 2 bins per lane).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "fft_lds.hpp"
#include "kernels.hpp"
#include "packed.hpp"

namespace fftconv {

// ---------------------------------------------------------------------------
// Geometry of the fused step kernel for a given block size
// ---------------------------------------------------------------------------
template <int LOG2B, int NT>
struct Geo {
    static constexpr int B = 1 << LOG2B;
    static constexpr int VEC = B >= 2 ? 2 : 1;          // complex bins per lane-slot
    static constexpr int F = B / VEC;                   // slots per row
    static constexpr int G = F >= NT ? 1 : NT / F;      // row groups (segment split)
    static constexpr int SPT = F >= NT ? F / NT : 1;    // slots per thread
    // rows in flight per thread (B 4096 on 512 threads: 2 rows measured no
    // faster than 1 -- its near-row MAC streams at the chip's rate, r5o)
    static constexpr int U = SPT == 1 ? 8 : (SPT == 2 ? 2 : 1);
    static constexpr size_t red_bytes = G > 1 ? (size_t)NT * VEC * sizeof(float2) : 0;
    // B <= 512: the prologue stages by LDS-DMA the twiddle table (2B float2),
    // H[0] (B float2), overlap, and the two tail slices (B floats each)
    static constexpr bool PREFETCH = LOG2B <= 9;
    static constexpr size_t tw_bytes = PREFETCH ? 2 * (size_t)B * sizeof(float2) : 0;
    static constexpr size_t pre_bytes = PREFETCH ? (size_t)B * sizeof(float2) + 3 * (size_t)B * sizeof(float) : 0;
    static constexpr size_t gen_bytes = ((2 * (size_t)B * sizeof(float2) + red_bytes + tw_bytes + pre_bytes + 15) / 16) * 16;
    // pipelined full-block step (pipelined_step): bufA | bufB | tw (2B) | H0 | H1 | pre | overlap | tail0 | tail1
    static constexpr bool PIPE = LOG2B >= 1 && LOG2B <= 9 && NT == 256;
    // the next block's pre is reduced and stored while the chain runs its C2R
    // (B <= 256): the reduction slots (4 waves x 64 lanes x 16 B x slots/lane)
    // after the chain's buffers; at B = 512 they reuse the front once the
    // chain is done (the process kernel's LDS stays below 40 KB there)
    static constexpr bool PIPE_EARLY = LOG2B <= 8;
    static constexpr size_t pipe_red = 4 * 64 * 16 * (size_t)(B >= 128 ? B / 128 : 1);
    static constexpr size_t pipe_bytes =
        PIPE ? (PIPE_EARLY ? 68 * (size_t)B + pipe_red : (68 * (size_t)B > pipe_red ? 68 * (size_t)B : pipe_red)) : 0;
    static constexpr size_t lds_bytes = (gen_bytes > pipe_bytes ? gen_bytes : pipe_bytes) + 16;
};

// a state word written by a non-lookahead step: no live window, this launch's tag
__device__ __forceinline__ int la_clear(int flags, const ProcArgs &a) {
    return (flags & ~(LA_MASK | SEQ_MASK)) | (a.la_seq << SEQ_SHIFT);
}

// realfft's C2R error (:264-267) once conv's slot 0 = pre0 + x0 (.) h0 came
// out non-finite.  The reference's DC / Nyquist imaginary parts are sums of
// re * 0 + 0 * re products (complex_multiply_accumulate on real bins): NaN
// exactly when one operand row's (DC, Nyquist) pair is not finite, and 0 when
// all are finite -- a finite overflow then runs the C2R on inf without an
// error.  pre0 was summed from rows 1..act-1 of H and of the ring, which are
// unchanged since (an update zeroes pre_multiplied), so only a non-finite pre0
// needs them scanned.  Rare path: one lane.
// (static: one copy per object; unused: not every includer runs the step)
static __device__ __attribute__((noinline, unused)) bool c2r_rejects(const float2 *Hc, const float2 *Xc, int B,
                                                                     int cur, int act, float2 pre0, float2 x0,
                                                                     float2 h0) {
    if (!slot0_finite(x0) || !slot0_finite(h0)) return true;
    if (slot0_finite(pre0)) return false;
    for (int i = 1; i < act; ++i) {
        const int xi = (cur + i) % act;  // index_audio (:248; current may exceed act after an update)
        if (!slot0_finite(Hc[(size_t)i * B]) || !slot0_finite(Xc[(size_t)xi * B])) return true;
    }
    return false;
}

// Buffer-resource streams (guide T8): one wave-uniform descriptor per channel
// stream, the row offset in an SGPR (soffset) when the row is wave-uniform,
// one shared per-lane voffset -- no per-load 64-bit address registers.
// aux 2 = nontemporal.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// FFTCONV_DEBUG_BOUNDS (debug builds only): DBG_CHECK (kernels.hpp) reports
// out-of-range stream rows and window/state indices with printf instead of
// touching the memory
struct RowStream {
    __amdgpu_buffer_rsrc_t r;
#ifdef FFTCONV_DEBUG_BOUNDS
    int nbytes;
#endif
    __device__ __forceinline__ RowStream(const float2 *base, size_t bytes) {
        r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2 *>(base), 0, (int)bytes, 0x00020000);
#ifdef FFTCONV_DEBUG_BOUNDS
        nbytes = (int)bytes;
#endif
    }
    // (an explicitly typed vector + memcpy: indexing the builtin's result
    // through __builtin_bit_cast made hipcc emit a single-dword load)
    template <bool NTL>
    __device__ __forceinline__ float4 ld4(int voff, int soff) const {
#ifdef FFTCONV_DEBUG_BOUNDS
        if (voff < nbytes && (soff < 0 || soff + voff + 16 > nbytes)) {
            dbg_bounds(3, voff, soff, nbytes, 0);  // (site 3: a stream row past the buffer)
            soff = 0;
        }
#endif
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, NTL ? 2 : 0);
        float4 f;
        __builtin_memcpy(&f, &v, sizeof(f));
        return f;
    }
    template <bool NTL>
    __device__ __forceinline__ float2 ld2(int voff, int soff) const {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, NTL ? 2 : 0);
        float2 f;
        __builtin_memcpy(&f, &v, sizeof(f));
        return f;
    }
    template <bool NTL>
    __device__ __forceinline__ float4 ld(int voff, int soff, float4 *) const { return ld4<NTL>(voff, soff); }
    template <bool NTL>
    __device__ __forceinline__ float2 ld(int voff, int soff, float2 *) const { return ld2<NTL>(voff, soff); }
};

// pre_multiplied = sum_{i=i0}^{i1-1} H[i] (.) X[(cur+i) % act] over this
// thread's slots (src/fft_convolver.rs:244-255; the whole sum is rows
// 1..act-1).  The rows are visited in scan order t = 0..i1-i0-1, group g
// taking t = g (mod G).  ZZ: every other block scans the rows backwards (rows
// read last by one step are read first by the next).  NTL: nontemporal loads.
template <int LOG2B, int NT, bool ZZ, bool NTL, class AccArr>
__device__ __forceinline__ void mac_rows(AccArr &acc, const float2 *Hc, const float2 *Xc, int S, int cur, int act,
                                         int i0, int i1, int flags, int f0, int g) {
    using Gm = Geo<LOG2B, NT>;
    constexpr int B = Gm::B, VEC = Gm::VEC, F = Gm::F, G = Gm::G, SPT = Gm::SPT, U = Gm::U;
    constexpr int ROWB = B * (int)sizeof(float2);  // bytes per row
    constexpr bool UNIFORM = F >= 64;              // a row group spans whole waves
    using vec_t = typename VecT<VEC>::type;
    const size_t bytes = (size_t)S * ROWB;
    const RowStream hs(Hc, bytes), xs(Xc, bytes);
    const int lane_off = f0 * VEC * (int)sizeof(float2);
#pragma unroll
    for (int s = 0; s < SPT; ++s) acc[s].zero();
    const bool rev = ZZ && (flags & FLAG_REV);
    const int di = rev ? -G : G;
    const int nr = i1 - i0;
    int t = g;
    int i = rev ? i1 - 1 - t : i0 + t;
    int xi = (cur + i) % act;  // index_audio = (current + i) % active
    for (; t + (U - 1) * G < nr; t += U * G) {
        vec_t hv[U][SPT], xv[U][SPT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int ho = i * ROWB, xo = xi * ROWB;
#pragma unroll
            for (int s = 0; s < SPT; ++s) {
                const int lo = lane_off + s * NT * VEC * (int)sizeof(float2);
                hv[u][s] = UNIFORM ? hs.ld<NTL>(lo, ho, (vec_t *)nullptr) : hs.ld<NTL>(lo + ho, 0, (vec_t *)nullptr);
                xv[u][s] = UNIFORM ? xs.ld<NTL>(lo, xo, (vec_t *)nullptr) : xs.ld<NTL>(lo + xo, 0, (vec_t *)nullptr);
            }
            i += di;
            xi += di;
            if (xi >= act) xi -= act;
            if (xi < 0) xi += act;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int s = 0; s < SPT; ++s) acc[s].mac(hv[u][s], xv[u][s]);
    }
    for (; t < nr; t += G) {
        const int ho = i * ROWB, xo = xi * ROWB;
#pragma unroll
        for (int s = 0; s < SPT; ++s) {
            const int lo = lane_off + s * NT * VEC * (int)sizeof(float2);
            const vec_t h = UNIFORM ? hs.ld<NTL>(lo, ho, (vec_t *)nullptr) : hs.ld<NTL>(lo + ho, 0, (vec_t *)nullptr);
            const vec_t x = UNIFORM ? xs.ld<NTL>(lo, xo, (vec_t *)nullptr) : xs.ld<NTL>(lo + xo, 0, (vec_t *)nullptr);
            acc[s].mac(h, x);
        }
        i += di;
        xi += di;
        if (xi >= act) xi -= act;
        if (xi < 0) xi += act;
    }
}

// Crossfade pair: the two convolvers' pre_multiplied from ONE read of the
// shared FDL (A and B see the same input, so while their ring states agree
// their FDL rows are equal).  Same row walk and per-accumulator order as
// mac_rows (non-zig-zag), so each sum is bit-identical to the unpaired one.
template <int LOG2B, int NT, bool NTL, class AccArr>
__device__ __forceinline__ void mac_rows_pair(AccArr &accA, AccArr &accB, const float2 *HA, const float2 *HB,
                                              const float2 *Xc, int S, int cur, int act, int f0, int g) {
    using Gm = Geo<LOG2B, NT>;
    constexpr int B = Gm::B, VEC = Gm::VEC, G = Gm::G, SPT = Gm::SPT;
    constexpr int U = SPT == 1 ? 8 : (SPT == 2 ? 4 : 2);
    constexpr int ROWB = B * (int)sizeof(float2);
    constexpr bool UNIFORM = Gm::F >= 64;
    using vec_t = typename VecT<VEC>::type;
    const size_t bytes = (size_t)S * ROWB;
    const RowStream ha(HA, bytes), hb(HB, bytes), xs(Xc, bytes);
    const int lane_off = f0 * VEC * (int)sizeof(float2);
#pragma unroll
    for (int s = 0; s < SPT; ++s) {
        accA[s].zero();
        accB[s].zero();
    }
    int t = g;
    int i = 1 + t;
    int xi = (cur + i) % act;
    for (; t + (U - 1) * G < act - 1; t += U * G) {
        vec_t av[U][SPT], bv[U][SPT], xv[U][SPT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int ho = i * ROWB, xo = xi * ROWB;
#pragma unroll
            for (int s = 0; s < SPT; ++s) {
                const int lo = lane_off + s * NT * VEC * (int)sizeof(float2);
                av[u][s] = UNIFORM ? ha.ld<NTL>(lo, ho, (vec_t *)nullptr) : ha.ld<NTL>(lo + ho, 0, (vec_t *)nullptr);
                bv[u][s] = UNIFORM ? hb.ld<NTL>(lo, ho, (vec_t *)nullptr) : hb.ld<NTL>(lo + ho, 0, (vec_t *)nullptr);
                xv[u][s] = UNIFORM ? xs.ld<NTL>(lo, xo, (vec_t *)nullptr) : xs.ld<NTL>(lo + xo, 0, (vec_t *)nullptr);
            }
            i += G;
            xi += G;
            if (xi >= act) xi -= act;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int s = 0; s < SPT; ++s) {
                accA[s].mac(av[u][s], xv[u][s]);
                accB[s].mac(bv[u][s], xv[u][s]);
            }
    }
    for (; t < act - 1; t += G) {
        const int ho = i * ROWB, xo = xi * ROWB;
#pragma unroll
        for (int s = 0; s < SPT; ++s) {
            const int lo = lane_off + s * NT * VEC * (int)sizeof(float2);
            const vec_t x = UNIFORM ? xs.ld<NTL>(lo, xo, (vec_t *)nullptr) : xs.ld<NTL>(lo + xo, 0, (vec_t *)nullptr);
            accA[s].mac(UNIFORM ? ha.ld<NTL>(lo, ho, (vec_t *)nullptr) : ha.ld<NTL>(lo + ho, 0, (vec_t *)nullptr), x);
            accB[s].mac(UNIFORM ? hb.ld<NTL>(lo, ho, (vec_t *)nullptr) : hb.ld<NTL>(lo + ho, 0, (vec_t *)nullptr), x);
        }
        i += G;
        xi += G;
        if (xi >= act) xi -= act;
    }
}

// Asynchronous global -> LDS copies (LDS-DMA, global_load_lds): lane l of a
// wave writes dst + l*W for a wave-uniform dst, no VGPR destination, drained
// by the next __syncthreads (s_waitcnt vmcnt(0) before s_barrier).
typedef __attribute__((address_space(1))) const void *gptr_t;
typedef __attribute__((address_space(3))) void *lptr_t;
template <int NT>
__device__ __forceinline__ void dma_f32(float *dst, const float *src, int count) {  // any alignment
    const int lane = threadIdx.x & 63;
    // NT threads copy: the caller's wave w of them starts at w (NT = 64: any single wave)
    for (int base = ((threadIdx.x >> 6) % (NT / 64)) * 64; base < count; base += NT)
        if (base + lane < count)
            __builtin_amdgcn_global_load_lds((gptr_t)(src + base + lane), (lptr_t)(dst + base), 4, 0, 0);
}
template <int NT>
__device__ __forceinline__ void dma_16b(void *dst, const void *src, int bytes) {  // 16-byte aligned, bytes % 16 == 0
    const int lane = threadIdx.x & 63;
    const char *s = static_cast<const char *>(src);
    char *d = static_cast<char *>(dst);
    for (int base = ((threadIdx.x >> 6) % (NT / 64)) * 1024; base < bytes; base += NT * 16)
        if (base + lane * 16 < bytes)
            __builtin_amdgcn_global_load_lds((gptr_t)(s + base + lane * 16), (lptr_t)(d + base), 16, 0, 0);
}

// TwoStageFFTConvolver::process sub-chunk (src/fft_convolver.rs:438-461) fused
// into the head job: output += precalculated0, then += precalculated (two
// separate adds, like the reference's two loops), and tail_input <- input.
// Generic form: a pass over the finished output.
template <int NT>
__device__ __forceinline__ void twostage_epilogue(const ProcJob &J, size_t c, float *outc, const float *inc, int n) {
    if (!J.add0 && !J.tin) return;
    __syncthreads();  // outc[] was written by other threads of this workgroup
    const float *p0 = J.add0 ? J.add0 + c * J.add_stride : nullptr;
    const float *p1 = J.add1 ? J.add1 + c * J.add_stride : nullptr;
    float *ti = J.tin ? J.tin + c * J.tin_stride : nullptr;
    for (int j = threadIdx.x; j < n; j += NT) {
        if (p0) {
            float v = outc[j];
            v += p0[j];
            if (p1) v += p1[j];
            outc[j] = v;
        }
        if (ti) ti[j] = inc[j];
    }
}

// FDL stream of the pipelined step: rows i = 2 + t of the NEXT block's
// pre_multiplied (block start `curp`) for t in [t_begin, t_end), split over
// nw waves (this is wave sw of them); a wave covers RPW rows at once when a
// row has fewer than 64 slots.  Accumulates into acc (not zeroed here).
template <int LOG2B, bool NTL, class AccArr>
__device__ __forceinline__ void mac_rows_range(AccArr &acc, const float2 *Hc, const float2 *Xc, int S, int curp,
                                               int act, int t_begin, int t_end, int nw, int sw, int rsub, int f0) {
    constexpr int B = 1 << LOG2B, F = B / 2;
    constexpr int RPW = F >= 64 ? 1 : 64 / F, SPL = F >= 64 ? F / 64 : 1;
    // (11 rows per half-wave in flight: cfg3's head stream -- 62 rows over 3
    // waves of 2 half-waves -- in one round trip instead of two: head step
    // 5.41 -> 5.05 us, cfg3 6.96 -> 6.86 us; 16 spills: 6.57 us; r4l A/B)
    constexpr int U = SPL == 1 ? 11 : (SPL == 2 ? 4 : 2);
    constexpr int ROWB = B * (int)sizeof(float2);
    constexpr bool UNIFORM = RPW == 1;  // one row per wave-iteration: row offset in an SGPR
    const int STEP = nw * RPW;
    const size_t bytes = (size_t)S * ROWB;
    const RowStream hs(Hc, bytes), xs(Xc, bytes);
    const int lane_off = f0 * 16;
    constexpr int OOB = 0x7ffffff0;  // a voffset past the stream: the load returns 0, no memory access
    int t = t_begin + sw * RPW + rsub;
    int i = 2 + t;
    int xi = (curp + i) % act;
    // batches of U rows, the last one partial: rows past t_end are loaded from
    // the out-of-range offset and not accumulated, so the last rows of a walk
    // are in flight together instead of one round trip each (cfg3 head, r3)
    for (; t < t_end; t += U * STEP) {
        float4 hv[U][SPL], xv[U][SPL];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = t + u * STEP < t_end;
            const int ho = in ? i * ROWB : 0, xo = in ? xi * ROWB : 0;
#pragma unroll
            for (int s = 0; s < SPL; ++s) {
                const int lo = in ? lane_off + s * 64 * 16 : OOB;
                hv[u][s] = UNIFORM ? hs.ld4<NTL>(lo, ho) : hs.ld4<NTL>(in ? lo + ho : OOB, 0);
                xv[u][s] = UNIFORM ? xs.ld4<NTL>(lo, xo) : xs.ld4<NTL>(in ? lo + xo : OOB, 0);
            }
            i += STEP;
            xi += STEP;
            if (xi >= act) xi -= act;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (t + u * STEP < t_end) {
#pragma unroll
                for (int s = 0; s < SPL; ++s) acc[s].mac(hv[u][s], xv[u][s]);
            }
    }
}

// mac_rows_range over a multi-call run's LDS copies of the IR rows (hl) and
// the FDL ring (xl): the same rows in the same order per slot, so the same
// bits -- without the HBM / L2 round trip the stream waves otherwise wait on
// every call (cfg3's head: 62 rows of H and X per call, ~1.6 us)
template <int LOG2B, class AccArr>
__device__ __forceinline__ void mac_rows_lds(AccArr &acc, const float2 *hl, const float2 *xl, int curp, int act,
                                             int t_begin, int t_end, int nw, int sw, int rsub, int f0) {
    constexpr int B = 1 << LOG2B, F = B / 2;
    constexpr int RPW = F >= 64 ? 1 : 64 / F, SPL = F >= 64 ? F / 64 : 1;
    // batches of U rows, every LDS read of a batch issued before its MACs
    // (one LDS round trip per batch, not per row); rows past t_end read row 0
    // and are not accumulated
    constexpr int U = SPL == 1 ? 12 : (SPL == 2 ? 6 : 3);
    const int STEP = nw * RPW;
    const float4 *h4 = reinterpret_cast<const float4 *>(hl), *x4 = reinterpret_cast<const float4 *>(xl);
    int t = t_begin + sw * RPW + rsub;
    int i = 2 + t;
    int xi = (curp + i) % act;
    for (; t < t_end; t += U * STEP) {
        float4 hv[U][SPL], xv[U][SPL];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = t + u * STEP < t_end;
            const int ho = in ? i * F : 0, xo = in ? xi * F : 0;
#pragma unroll
            for (int s = 0; s < SPL; ++s) {
                hv[u][s] = h4[ho + f0 + s * 64];
                xv[u][s] = x4[xo + f0 + s * 64];
            }
            i += STEP;
            xi += STEP;
            if (xi >= act) xi -= act;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (t + u * STEP < t_end) {
#pragma unroll
                for (int s = 0; s < SPL; ++s) acc[s].mac(hv[u][s], xv[u][s]);
            }
    }
}

// ProcArgs::sig: a tail step's workgroups arrive when their stores are done
// (each releases at agent scope, then one relaxed add; the last acquires them
// all and releases sig[1] = sig_val); a run waits for sig[1] >= sig_val
// (wrap-safe), acquires, and the workgroup's loads of the tail's output come
// after.  The wait is bounded (~100 ms, counted in sig[2]): the tail it waits
// for was enqueued a period earlier on a stream of its own, fits a CU beside
// a run workgroup, and in practice finished long before.
__device__ __forceinline__ void sig_arrive(const ProcArgs &a) {
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const unsigned n = gridDim.x * gridDim.y;
        const unsigned prev = __hip_atomic_fetch_add(a.sig, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == n - 1) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            __hip_atomic_store(a.sig, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.sig + 1, a.sig_val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
__device__ __forceinline__ void sig_wait(const ProcArgs &a) {
    if (threadIdx.x == 0) {
        const unsigned t0 = (unsigned)__builtin_amdgcn_s_memrealtime();
        while ((int)(__hip_atomic_load(a.sig + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - a.sig_val) < 0) {
            __builtin_amdgcn_s_sleep(8);
            if ((unsigned)__builtin_amdgcn_s_memrealtime() - t0 > 10000000u) {  // (100 MHz: 100 ms)
                __hip_atomic_fetch_add(a.sig + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
}

// launch timeline phase stamp k (0..3) of this wave of a process launch
// (FFTCONV_PROC_TRACE; job 0 only)
__device__ __forceinline__ void proc_stamp(const ProcArgs &a, int k) {
    if (a.la_trace && blockIdx.y == 0 && (threadIdx.x >> 6) < 4 && (threadIdx.x & 63) == 0) {
        int *p = reinterpret_cast<int *>(a.la_trace + ((size_t)a.la_trace_grid * 4 + (size_t)blockIdx.x * 4 + (threadIdx.x >> 6)));
        p[k] = (int)(unsigned)__builtin_amdgcn_s_memrealtime();
    }
}

// A multi-call launch's chain state between two calls of one channel
// (upols_run_kernel, pipelined steps at B <= 256): when the previous call ran
// the pipelined step without a C2R error (`hot`), the twiddles, H[0], H[1]
// and the next pre_multiplied are still in LDS, the next call's input block
// was prefetched into LDS stage[par] by a helper wave, and the overlap is in
// registers -- the call starts its R2C without a memory round trip.  The
// same values as the loads it replaces: bit-identical.
struct RunCarry {
    int hot;
    int par;                // stage buffer holding this call's input (hot)
    const float *next_in;   // the next call's input (null: the run's last call)
    float ov[4];            // overlap samples of the chain's lanes (B <= 256)
    int4 st;                // the state word the call stored (hot): the next call's, without a reload
    // the run's LDS copies of the IR rows and the FDL (ProcArgs::run_lds_rows;
    // null = the helpers stream the rows from memory): row r at hl / xl + r*B
    const float2 *hl;
    float2 *xl;
};

// Workgroup barrier for LDS data only: this wave's LDS operations complete,
// then s_barrier -- unlike __syncthreads, no wait for the wave's outstanding
// global stores (the pipelined step's chain has just issued its FDL row,
// tail_input and tail0 spectrum stores; nothing behind this barrier reads
// them, and the call's closing __syncthreads orders them for the next call).
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---------------------------------------------------------------------------
// Pipelined full-block step (2 <= B <= 512): the common call -- one whole
// block from an empty input buffer -- when pre[] already holds
// pre_multiplied for the block at `current` (FLAG_PRE).  The work of
// FFTConvolver::process (:215-295) is re-timed, not changed:
//   wave 0   : R2C of the block -> FDL row `current`; conv = pre + X.H[0];
//              C2R, x1/N; overlap-add and overlap save -- all out of LDS,
//              staged by its own LDS-DMA, synchronised at wave level; then
//              row 1 (H[1] (.) X_new) of the NEXT block's pre_multiplied,
//              then the last w0 = max(0, (S-2-lag)/4) FDL rows of it
//   waves 1-3: stream the other FDL rows of the NEXT block's pre_multiplied
// so the latency chain hides under the FDL stream instead of following it
// (lag ~ the chain's duration in rows of stream; set by the host).
// The next block's pre is reduced in a fixed order and stored (FLAG_PRE).
// B <= 256 (PIPE_EARLY): the chain parks its share of that pre right after
// the conv (row 1 needs only the new spectrum) and the helper waves, long
// done with their rows, reduce and store it and the state word while the
// chain runs its C2R -- the reduction leaves the launch's critical path
// (cfg3 head timeline, profiles/r3: it ran after the chain, 0.5 of 5.5 us).
// ---------------------------------------------------------------------------
template <int LOG2B, int NT, bool NTL, bool RUN = false>
__device__ __forceinline__ bool pipelined_step(const ProcArgs &a, const ProcJob &J, size_t c, int cur, int act,
                                               int flags, unsigned char *smem, RunCarry *rc = nullptr) {
    using Gm = Geo<LOG2B, NT>;
    constexpr int B = Gm::B, F = B / 2;
    constexpr int RPW = F >= 64 ? 1 : 64 / F, SPL = F >= 64 ? F / 64 : 1;
    constexpr int NSW = NT / 64 - 1;
    constexpr float invN = 1.0f / (float)(2 * B);
    float2 *bufA = reinterpret_cast<float2 *>(smem);
    float2 *bufB = bufA + B;
    float2 *twl = bufB + B;
    float2 *h0l = twl + 2 * B;
    float2 *h1l = h0l + B;
    float2 *prel = h1l + B;
    float *ovl = reinterpret_cast<float *>(prel + B);
    float *p0l = ovl + B;
    float *p1l = p0l + B;
    int &s_err = *reinterpret_cast<int *>(smem + Gm::lds_bytes - 16);
    // the next block's pre: partial sums [wave][slot/64][lane]
    float4 *red = reinterpret_cast<float4 *>(Gm::PIPE_EARLY ? reinterpret_cast<unsigned char *>(p1l + B) : smem);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t rows = (size_t)J.S * B;
    const float2 *Hc = J.H + c * rows;
    float2 *Xc = J.X + c * rows;
    float *ovc = J.overlap + c * B;
    float2 *prec = J.pre + c * B;
    float *outc = J.out + c * J.out_stride;
    const float *inc = J.in + c * J.in_stride;
    const int curp = cur > 0 ? cur - 1 : act - 1;  // current after this block (:287-291)
    const int rsub = F >= 64 ? 0 : lane / F;
    const int f0 = F >= 64 ? lane : lane % F;

    Acc2 acc[SPL];
#pragma unroll
    for (int s = 0; s < SPL; ++s) acc[s].zero();
    constexpr int CNB = (B + 63) / 64;  // the chain's samples per lane
    float ovr[CNB], p0r[CNB], p1r[CNB];
#pragma unroll
    for (int i = 0; i < CNB; ++i) ovr[i] = p0r[i] = p1r[i] = 0.f;
    float2 *Z = bufA, *Q = bufB;  // (the chain's transform buffers, across B1)
    bool err = false;
    constexpr bool RH = RUN && Gm::PIPE_EARLY && CNB <= 4;  // (run-carried state: B <= 256)
    float *stage[2] = {ovl, p0l};  // (a run's prefetched input blocks: LDS the step leaves unused)
    const bool hot = RH && rc->hot;
    // (a run: the spectra of the calls' blocks, double-buffered by stage
    // parity -- the last helper wave transforms the NEXT call's block while
    // the chain runs this call's C2R, so a hot call's chain starts at the
    // conv; then the helper's two transform buffers.  Past the step's LDS:
    // the run kernel allocates run_lds_bytes)
    float2 *nxs = reinterpret_cast<float2 *>(smem + Gm::lds_bytes);
    float2 *nfa = nxs + 2 * B, *nfb = nfa + B;
    // (a run: the state word this step stores when its block succeeds; every
    // thread holds it, so the next call starts without reloading it)
    if constexpr (RH) rc->st = make_int4(curp, act, 0, la_clear(((flags & ~FLAG_INBUF) ^ FLAG_REV) | FLAG_PRE, a));
    if (wave == 0) {
        // ---- critical chain, one wave: R2C, conv, the C2R error check ----
        if (hot) {
            // tw, H[0], H[1], pre and this block's spectrum in LDS already
        } else {
            dma_f32<64>(reinterpret_cast<float *>(bufA), inc, B);   // x[0..B) as packed z[0..B/2)
            for (int m = B / 2 + lane; m < B; m += 64) bufA[m] = make_float2(0.f, 0.f);
            dma_16b<64>(twl, a.tw, 2 * B * (int)sizeof(float2));
            dma_16b<64>(h0l, Hc, B * (int)sizeof(float2));
            if (act > 1) dma_16b<64>(h1l, Hc + B, B * (int)sizeof(float2));
            dma_16b<64>(prel, prec, B * (int)sizeof(float2));
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        wave_sync();
        // the overlap and the two-stage adds are read only by the overlap-add
        // at the chain's end: plain loads issued now arrive under the
        // transforms, instead of holding the R2C behind the prologue wait
        // (cfg3 head: the adds come from the tail buffers, HBM-cold)
#pragma unroll
        for (int i = 0; i < CNB; ++i) {
            const int j = lane + 64 * i;
            if (j < B) {
                if constexpr (RH) ovr[i] = hot ? rc->ov[i] : ovc[j];
                else ovr[i] = ovc[j];
                if (J.add0) p0r[i] = J.add0[c * J.add_stride + j];
                if (J.add1) p1r[i] = J.add1[c * J.add_stride + j];
            }
        }
        proc_stamp(a, 0);
        if (J.tin) {  // two-stage: append the block to tail_input (:459-461)
            const float *xb = hot ? stage[rc->par] : reinterpret_cast<const float *>(bufA);
            float *ti = J.tin + c * J.tin_stride;
            for (int j = lane; j < B; j += 64) ti[j] = xb[j];
        }
        float2 *Xcur = Xc + (size_t)cur * B;
        float2 *t0r = J.t0x ? J.t0x + c * J.t0x_stride : nullptr;  // (a run: tail0's copy of the spectrum)
        if (hot) {
            // the spectrum the last helper wave computed during the previous
            // call (the same transform, bit for bit): to the FDL row, tail0's row
            Q = nxs + rc->par * B;
            Z = bufA;
            float2 *xlc = rc->xl ? rc->xl + (size_t)cur * B : nullptr;  // (the run's LDS ring)
            for (int m = lane; m < B; m += 64) {
                const float2 v = Q[m];
                Xcur[m] = v;
                if (t0r) t0r[m] = v;
                if (xlc) xlc[m] = v;
            }
        } else {
            wave_sync();
            Z = lds_cfft<LOG2B, 64, false, true>(bufA, bufB, twl);  // :229-241
            Q = Z == bufA ? bufB : bufA;
            float2 *xlc = nullptr;
            if constexpr (RH) xlc = rc->xl ? rc->xl + (size_t)cur * B : nullptr;
            for (int m = lane; m < B; m += 64) {
                const float2 v = real_post<LOG2B, 64>(Z, m, twl);
                Q[m] = v;
                Xcur[m] = v;
                if (t0r) t0r[m] = v;
                if (xlc) xlc[m] = v;
            }
            wave_sync();
        }
        bool bad = false;  // conv = pre + X (.) H[0] (:256-261), then the C2R error check
        for (int f = lane; f < F; f += 64) {
            const float4 cv = slot_mac(reinterpret_cast<const float4 *>(prel)[f], reinterpret_cast<const float4 *>(Q)[f],
                                       reinterpret_cast<const float4 *>(h0l)[f], f);
            reinterpret_cast<float4 *>(Z)[f] = cv;
            if (f == 0 && !slot0_finite(cv) &&
                c2r_rejects(Hc, Xc, B, cur, act, slot0_of(reinterpret_cast<const float4 *>(prel)[0]),
                            slot0_of(reinterpret_cast<const float4 *>(Q)[0]), slot0_of(reinterpret_cast<const float4 *>(h0l)[0])))
                bad = true;
        }
        // row 1 of the next block's pre_multiplied: H[1] (.) X_new (X_new is row (curp+1) % act = cur)
        if (act > 1 && rsub == 0) {
#pragma unroll
            for (int s = 0; s < SPL; ++s) {
                const int f = f0 + s * 64;
                if (f < F) acc[s].mac(reinterpret_cast<const float4 *>(h1l)[f], reinterpret_cast<const float4 *>(Q)[f]);
            }
        }
        err = __ballot(bad) != 0ull;
        if constexpr (Gm::PIPE_EARLY) {
            // the chain's share of the next block's pre (row 1, and the last
            // w0 rows with a pipeline lag) to the reduction slots; the helper
            // waves reduce and store it, and the state, during the C2R below
            const int R = act > 2 ? act - 2 : 0;
            const int w0 = R > a.lag ? (R - a.lag) / (NSW + 1) : 0;
            if (w0 > 0) {
                bool inl = false;
                if constexpr (RH) inl = rc->xl != nullptr;
                if (inl) mac_rows_lds<LOG2B>(acc, rc->hl, rc->xl, curp, act, R - w0, R, 1, 0, rsub, f0);
                else mac_rows_range<LOG2B, NTL>(acc, Hc, Xc, J.S, curp, act, R - w0, R, 1, 0, rsub, f0);
            }
#pragma unroll
            for (int s = 0; s < SPL; ++s) red[s * 64 + lane] = acc[s].get(f0 + s * 64);
            if (lane == 0) s_err = err ? 1 : 0;
        }
    } else if constexpr (Gm::PIPE_EARLY) {
        // ---- helper waves: FDL rows 2..act-1 - w0 of the next block's pre ----
        // (a run: wave 1 first prefetches the next call's block into the other stage)
        if (RH && wave == 1 && rc->next_in) dma_f32<64>(stage[rc->par ^ 1], rc->next_in + c * J.in_stride, B);
        const int R = act > 2 ? act - 2 : 0;
        const int w0 = R > a.lag ? (R - a.lag) / (NSW + 1) : 0;
        bool inl = false;
        if constexpr (RH) inl = rc->xl != nullptr;
        if (inl) mac_rows_lds<LOG2B>(acc, rc->hl, rc->xl, curp, act, 0, R - w0, NSW, wave - 1, rsub, f0);
        else mac_rows_range<LOG2B, NTL>(acc, Hc, Xc, J.S, curp, act, 0, R - w0, NSW, wave - 1, rsub, f0);
#pragma unroll
        for (int s = 0; s < SPL; ++s) red[(wave * SPL + s) * 64 + lane] = acc[s].get(f0 + s * 64);
        // (the stage DMA has landed before B1: the last wave transforms it after B1)
        if constexpr (RH) {
            if (wave == 1 && rc->next_in) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        proc_stamp(a, 2);
    }
    // B1 (B <= 256): every wave at this one barrier -- the chain's share of
    // the next block's pre and its error flag, and the helpers' shares, are
    // in the reduction slots (LDS only: the chain's global stores stay in
    // flight across it)
    if constexpr (Gm::PIPE_EARLY) lds_barrier();
    if (wave == 0) {
        // ---- the chain's C2R and overlap-add ----
        wave_sync();
        proc_stamp(a, 1);
        if (!err) {
            for (int m = lane; m < B; m += 64) Q[m] = real_pre<LOG2B, 64>(Z, m, twl);
            wave_sync();
            const float *y = reinterpret_cast<const float *>(lds_cfft<LOG2B, 64, true, true>(Q, Z, twl));
#pragma unroll
            for (int i = 0; i < CNB; ++i) {  // overlap-add (:270-274) + two-stage adds (:439-454)
                const int j = lane + 64 * i;
                if (j >= B) continue;
                float v = y[j] * invN + ovr[i];
                if (J.add0) {
                    v += p0r[i];
                    if (J.add1) v += p1r[i];
                }
                outc[j] = v;
                ovc[j] = y[B + j] * invN;  // :283-284
                if constexpr (RH) rc->ov[i] = y[B + j] * invN;
            }
        } else {
            // output.fill(0); return (:264-267): the block stays in the input
            // buffer, fill / current unchanged, pre still describes this block
            float *ibc = J.inbuf + c * B;
#pragma unroll
            for (int i = 0; i < CNB; ++i) {
                const int j = lane + 64 * i;
                if (j >= B) continue;
                float v = 0.f;
                if (J.add0) {
                    v += p0r[i];
                    if (J.add1) v += p1r[i];
                }
                outc[j] = v;
                ibc[j] = inc[j];
            }
        }
        if (!Gm::PIPE_EARLY && lane == 0) s_err = err ? 1 : 0;
        proc_stamp(a, 2);  // (timelines: the chain's C2R and overlap-add done)
        if constexpr (Gm::PIPE_EARLY) return !err;
    }
    if constexpr (Gm::PIPE_EARLY) {
        // ---- helper waves: the next block's pre in its fixed-order
        // reduction, and the state, while the chain runs its C2R ----
        const int ht = tid - 64;
        if (s_err) {
            if (ht == 0) J.state[c] = make_int4(cur, act, 0, la_clear(flags | FLAG_INBUF, a));
            if constexpr (RH) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the stage DMA)
            return false;
        }
        for (int f = ht; f < F; f += NT - 64) {
            float4 p = red[f];
            for (int w = 0; w <= NSW; ++w)
                for (int r = (w == 0 ? 1 : 0); r < RPW; ++r) p = vadd(p, red[w * SPL * 64 + f + r * F]);
            reinterpret_cast<float4 *>(prec)[f] = p;
            if constexpr (RH) reinterpret_cast<float4 *>(prel)[f] = p;  // (the chain's C2R no longer reads prel)
        }
        if constexpr (RH) {
            // the last wave (never in the reduction at B <= 256): the R2C of the
            // next call's block (:229-241), from the stage wave 1 filled, into
            // the spectrum buffer of the other parity
            if (wave == NSW && rc->next_in) {
                const float *sg = stage[rc->par ^ 1];
                float *za = reinterpret_cast<float *>(nfa);
                for (int j = lane; j < B; j += 64) za[j] = sg[j];
                for (int m = B / 2 + lane; m < B; m += 64) nfa[m] = make_float2(0.f, 0.f);
                wave_sync();
                const float2 *Zn = lds_cfft<LOG2B, 64, false, true>(nfa, nfb, twl);
                float2 *qn = nxs + (rc->par ^ 1) * B;
                for (int m = lane; m < B; m += 64) qn[m] = real_post<LOG2B, 64>(Zn, m, twl);
            }
        }
        if (ht == 0) J.state[c] = make_int4(curp, act, 0, la_clear(((flags & ~FLAG_INBUF) ^ FLAG_REV) | FLAG_PRE, a));
        if constexpr (RH) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the stage DMA has landed)
        // (RunCarry::st above is this word)
        proc_stamp(a, 3);
        return true;
    }
    // ---- FDL rows 2..act-1 of the next block's pre: waves 1..NSW take
    // t in [0, R0), wave 0 (after its chain) the last w0 rows ----
    {
        const int R = act > 2 ? act - 2 : 0;
        const int w0 = R > a.lag ? (R - a.lag) / (NSW + 1) : 0;
        const int R0 = R - w0;
        if (wave == 0) mac_rows_range<LOG2B, NTL>(acc, Hc, Xc, J.S, curp, act, R0, R, 1, 0, rsub, f0);
        else mac_rows_range<LOG2B, NTL>(acc, Hc, Xc, J.S, curp, act, 0, R0, NSW, wave - 1, rsub, f0);
    }
    proc_stamp(a, 2);
    __syncthreads();
    if (s_err) {
        if (tid == 0) J.state[c] = make_int4(cur, act, 0, la_clear(flags | FLAG_INBUF, a));
        return false;
    }
    // next block's pre: every lane parks its partial sums in LDS (the whole
    // workgroup's staging is dead now), then slot f sums waves 0..NSW and
    // sub-rows in a fixed order -- deterministic for a given geometry and lag
#pragma unroll
    for (int s = 0; s < SPL; ++s) red[(wave * SPL + s) * 64 + lane] = acc[s].get(f0 + s * 64);
    __syncthreads();
    for (int f = tid; f < F; f += NT) {
        const int base = (f / 64) * 64 + f % 64;
        float4 p = red[base];
        for (int w = 0; w <= NSW; ++w)
            for (int r = (w == 0 ? 1 : 0); r < RPW; ++r) p = vadd(p, red[w * SPL * 64 + base + r * F]);
        reinterpret_cast<float4 *>(prec)[f] = p;
    }
    if (tid == 0) J.state[c] = make_int4(curp, act, 0, la_clear(((flags & ~FLAG_INBUF) ^ FLAG_REV) | FLAG_PRE, a));
    proc_stamp(a, 3);
    return false;  // (B = 512: no run-carried state)
}

// ---------------------------------------------------------------------------
// Fused UPOLS step: FFTConvolver::process (src/fft_convolver.rs:215-295) for
// one channel per workgroup, the whole chunk loop of one call on device.
//
// Latency structure: every load that does not depend on the MAC is issued in
// the prologue, so its round trip overlaps the FDL stream -- the twiddle table
// (into LDS), H[0], and for the common one-full-block call the input block,
// the overlap and the two-stage tail slices.  After the MAC the FFT / C2R /
// overlap-add tail then runs out of LDS and registers only.
// ---------------------------------------------------------------------------
// returns true when the call ran the pipelined step without a C2R error and
// left a multi-call launch's chain state in LDS (RunCarry::hot)
template <int LOG2B, int NT, bool ZZ, bool NTL, bool RUN = false>
__device__ __forceinline__ bool process_job(const ProcArgs &a, const ProcJob &J, const size_t c, const int4 st,
                                            unsigned char *smem, RunCarry *rc = nullptr) {
    using Gm = Geo<LOG2B, NT>;
    constexpr int B = Gm::B, VEC = Gm::VEC, F = Gm::F, G = Gm::G, SPT = Gm::SPT;
    constexpr float invN = 1.0f / (float)(2 * B);
    using vec_t = typename VecT<VEC>::type;

    float2 *bufA = reinterpret_cast<float2 *>(smem);
    float2 *bufB = bufA + B;
    vec_t *red = reinterpret_cast<vec_t *>(bufB + B);
    int &s_err = *reinterpret_cast<int *>(smem + Gm::lds_bytes - 16);

    const int tid = threadIdx.x;
    int cur = st.x;
    const int act = st.y;
    int fill = st.z;
    int flags = st.w;
    float *outc = J.out + c * J.out_stride;
    const float *inc = J.in + c * J.in_stride;
    const int n = J.n;

    if (act == 0) {  // :216-219 -- zero output, state untouched
        for (int j = tid; j < n; j += NT) outc[j] = 0.f;
        twostage_epilogue<NT>(J, c, outc, inc, n);
        return false;
    }

    if constexpr (Gm::PIPE) {
        if (a.pipe && fill == 0 && n == B && !(flags & FLAG_INBUF) && (flags & FLAG_PRE) && cur < act && !ZZ)
            return pipelined_step<LOG2B, NT, NTL, RUN>(a, J, c, cur, act, flags, smem, rc);
    }

    const size_t rows = (size_t)J.S * B;
    const float2 *Hc = J.H + c * rows;
    float2 *Xc = J.X + c * rows;
    float *ovc = J.overlap + c * B;
    float *ibc = J.inbuf + c * B;
    float2 *prec = J.pre + c * B;

    // slot ownership: the MAC splits rows over G groups; the owner of slot f
    // after the reduction is thread f (G > 1) or thread f % NT (G == 1).
    const int f0 = G > 1 ? tid % F : tid;
    // a row group spans whole waves when F >= 64: make g wave-uniform so the
    // row walk (i, xi, row addresses) lives in scalar registers
    const int g = G > 1 ? (F >= 64 ? __builtin_amdgcn_readfirstlane(tid / F) : tid / F) : 0;
    const bool owner = G > 1 ? tid < F : true;

    // ---- prologue: loads independent of the MAC ------------------------------
    constexpr bool PF = Gm::PREFETCH;
    float2 *twl = reinterpret_cast<float2 *>(smem + 2 * (size_t)B * sizeof(float2) + Gm::red_bytes);
    float2 *h0l = twl + 2 * B;
    float *ovl = reinterpret_cast<float *>(h0l + B);
    float *p0l = ovl + B;
    float *p1l = p0l + B;
    // the common call: exactly one full block from an empty input buffer
    const bool one_block = PF && fill == 0 && n == B && !(flags & FLAG_INBUF);
    const bool epi = J.add0 != nullptr || J.tin != nullptr;
    // far-row windows (B >= 1024): pre_multiplied is summed as
    // rows 1..sp-1 plus rows sp..act-1, in every launch of such a batch, so
    // the result does not depend on which steps read a window; a one-block
    // call of a channel whose window is live reads the far part from it
    constexpr bool GW = G == 1 && VEC == 2 && !ZZ && LOG2B >= 10;
    const int sp = GW && a.gw_p > 0 && act > a.gw_p ? a.gw_p : 0;
    const bool gwin = sp && a.gw && fill == 0 && n == B && !(flags & (FLAG_INBUF | FLAG_PRE)) && (flags & FLAG_GW);
    if constexpr (PF) {
        dma_16b<NT>(twl, a.tw, 2 * B * (int)sizeof(float2));
        if constexpr (B >= 2) dma_16b<NT>(h0l, Hc, B * (int)sizeof(float2));
        else dma_f32<NT>(reinterpret_cast<float *>(h0l), reinterpret_cast<const float *>(Hc), 2 * B);
        if (one_block) {
            // the zero-padded block, packed z[m] = (x[2m], x[2m+1]): x[0..B) lands
            // as raw floats in bufA[0..B/2), the padding half is zero
            dma_f32<NT>(reinterpret_cast<float *>(bufA), inc, B);
            if constexpr (B >= 2) {
                for (int m = B / 2 + tid; m < B; m += NT) bufA[m] = make_float2(0.f, 0.f);
            } else {
                if (tid == 0) bufA[0].y = 0.f;  // x[1] is padding when B == 1
            }
            dma_f32<NT>(ovl, ovc, B);
            if (J.add0) dma_f32<NT>(p0l, J.add0 + c * J.add_stride, B);
            if (J.add1) dma_f32<NT>(p1l, J.add1 + c * J.add_stride, B);
        }
    }
    const float2 *tw = PF ? twl : a.tw;
    const float2 *h0g = PF ? h0l : Hc;

    vec_t pacc[SPT];
    if (fill != 0 && owner) {  // a partial block carries pre_multiplied over
#pragma unroll
        for (int s = 0; s < SPT; ++s) pacc[s] = reinterpret_cast<const vec_t *>(prec)[f0 + s * NT];
    }

    int processed = 0;
    bool err = false, pre_next = false;
    bool t0w = false;  // (a run's two-stage head: this call wrote its block's spectrum to t0x)
    for (;;) {
        const bool was_empty = fill == 0;                               // :223
        const int k = min(n - processed, B - fill);                      // :224-227
        if (processed >= n) {
            // a full-block call that ended on a block boundary: one more MAC
            // pass (no transform) computes the next block's pre_multiplied so
            // the following full-block call takes pipelined_step
            if (!Gm::PIPE || ZZ || !a.pipe || n != B || !was_empty || (flags & FLAG_PRE) || cur >= act) break;
            pre_next = true;
        }

        if (was_empty && (flags & FLAG_PRE) && cur < act) {
            // pre[] already holds this block's pre_multiplied (computed at the
            // end of the previous block)
            if (owner) {
#pragma unroll
                for (int s = 0; s < SPT; ++s) pacc[s] = reinterpret_cast<const vec_t *>(prec)[f0 + s * NT];
            }
        } else if (was_empty) {                                          // :244-255
            AccT<VEC> acc[SPT];
            mac_rows<LOG2B, NT, ZZ, NTL>(acc, Hc, Xc, J.S, cur, act, 1, sp ? sp : act, flags, f0, g);
            if constexpr (GW) {
#pragma unroll
                for (int s = 0; s < SPT; ++s) pacc[s] = acc[s].get(f0 + s * NT);
                // far rows sp..act-1: this block's window row (the anchor
                // summed them, gw_anchor_kernel), else summed here; near +
                // far either way
                if (gwin) {
                    const int k = (int)(((long long)a.gw_t - 1 - (long long)c) % sp + sp) % sp;
                    DBG_CHECK(k >= 0 && k < sp, 40, k, a.gw_t, sp, (int)c);
                    const float4 *wr = reinterpret_cast<const float4 *>(a.gw + ((size_t)c * sp + k) * B);
#pragma unroll
                    for (int s = 0; s < SPT; ++s) pacc[s] = vadd(pacc[s], ntld4(wr + f0 + s * NT));
                } else if (sp) {  // (acc reused: one accumulator set live)
                    mac_rows<LOG2B, NT, ZZ, NTL>(acc, Hc, Xc, J.S, cur, act, sp, act, flags, f0, g);
#pragma unroll
                    for (int s = 0; s < SPT; ++s) pacc[s] = vadd(pacc[s], acc[s].get(f0 + s * NT));
                }
            } else if constexpr (G > 1) {
                red[g * F + f0] = acc[0].get(f0);
                __syncthreads();
                if (owner) {
                    vec_t p = red[f0];
#pragma unroll
                    for (int q = 1; q < G; ++q) p = vadd(p, red[q * F + f0]);
                    pacc[0] = p;
                }
            } else {
#pragma unroll
                for (int s = 0; s < SPT; ++s) pacc[s] = acc[s].get(f0 + s * NT);
            }
        }
        if (pre_next) {
            flags |= FLAG_PRE;
            break;
        }
        proc_stamp(a, 0);  // (timelines: pre_multiplied ready)

        // forward FFT of the zero-padded input buffer into segments[current]
        // (:229-241): x[i] = chunk sample, else the carried input buffer.
        if (one_block) {
            // the block is already in bufA (prologue DMA); two-stage: append it
            // to tail_input from LDS (:459-461)
            __syncthreads();
            if (J.tin) {
                const float *xb = reinterpret_cast<const float *>(bufA);
                float *ti = J.tin + c * J.tin_stride;
                for (int j = tid; j < B; j += NT) ti[j] = xb[j];
            }
        } else {
            for (int m = tid; m < B; m += NT) {
                float2 z = make_float2(0.f, 0.f);
                const int i0 = 2 * m, i1 = 2 * m + 1;
                if (i0 < B) {
                    z.x = (i0 >= fill && i0 < fill + k) ? inc[processed + i0 - fill]
                                                         : ((flags & FLAG_INBUF) ? ibc[i0] : 0.f);
                }
                if (i1 < B) {
                    z.y = (i1 >= fill && i1 < fill + k) ? inc[processed + i1 - fill]
                                                         : ((flags & FLAG_INBUF) ? ibc[i1] : 0.f);
                }
                bufA[m] = z;
            }
        }
        if (tid == 0) s_err = 0;
        __syncthreads();
        float2 *Z = lds_cfft<LOG2B, NT, false>(bufA, bufB, tw);
        float2 *Q = Z == bufA ? bufB : bufA;
        float2 *Xcur = Xc + (size_t)cur * B;
        // (a run's two-stage head: tail0's copy of a whole block's spectrum)
        float2 *t0r = J.t0x && fill == 0 && k == B ? J.t0x + c * J.t0x_stride : nullptr;
        t0w = t0w || t0r != nullptr;
        for (int m = tid; m < B; m += NT) {
            const float2 v = real_post<LOG2B, NT>(Z, m, tw);
            Q[m] = v;
            Xcur[m] = v;
            if (t0r) t0r[m] = v;
        }
        __syncthreads();
        proc_stamp(a, 1);  // (R2C done)

        // conv = pre_multiplied + segments[current] (.) segments_ir[0] (:256-261)
        if (owner) {
            const vec_t *q = reinterpret_cast<const vec_t *>(Q);
            vec_t *zc = reinterpret_cast<vec_t *>(Z);
#pragma unroll
            for (int s = 0; s < SPT; ++s) {
                const int f = f0 + s * NT;
                const vec_t cv = slot_mac(pacc[s], q[f], reinterpret_cast<const vec_t *>(h0g)[f], f);
                zc[f] = cv;
                // realfft's C2R rejects a non-zero DC/Nyquist imaginary part
                // (:264-267), which only a non-finite operand produces
                if (f == 0 && !slot0_finite(cv) &&
                    c2r_rejects(Hc, Xc, B, cur, act, slot0_of(pacc[s]), slot0_of(q[f]),
                                slot0_of(reinterpret_cast<const vec_t *>(h0g)[f])))
                    s_err = 1;
            }
        }
        __syncthreads();
        if (s_err) { err = true; break; }

        // inverse FFT (:264) with the 1/N of Fft::inverse (:44-46)
        for (int m = tid; m < B; m += NT) Q[m] = real_pre<LOG2B, NT>(Z, m, tw);
        __syncthreads();
        float2 *Y = lds_cfft<LOG2B, NT, true>(Q, Z, tw);
        const float *y = reinterpret_cast<const float *>(Y);
        proc_stamp(a, 2);  // (C2R done)

        // overlap-add (:270-274)
        if (one_block) {
            for (int j = tid; j < B; j += NT) {
                float v = y[j] * invN + ovl[j];
                if (J.add0) {  // two-stage sub-chunk adds (:439-454), same rounding order
                    v += p0l[j];
                    if (J.add1) v += p1l[j];
                }
                outc[j] = v;
            }
        } else {
            for (int j = tid; j < k; j += NT) outc[processed + j] = y[fill + j] * invN + ovc[fill + j];
        }
        const bool complete = fill + k == B;                              // :277-278
        if (complete) {
            if (!one_block) __syncthreads();  // every overlap read above is done
            for (int j = tid; j < B; j += NT) ovc[j] = y[B + j] * invN;  // :283-284
            if (flags & FLAG_INBUF)
                for (int j = tid; j < B; j += NT) ibc[j] = 0.f;           // :280
            flags &= ~(FLAG_INBUF | FLAG_PRE);
            flags ^= FLAG_REV;
            fill = 0;
            cur = cur > 0 ? cur - 1 : act - 1;                            // :287-291
        } else {
            for (int j = tid; j < k; j += NT) ibc[fill + j] = inc[processed + j];
            flags |= FLAG_INBUF;
            fill += k;
        }
        processed += k;
        __syncthreads();
    }

    if (err) {
        // output.fill(0); return -- state stays at the failing chunk: its
        // input is in the buffer, fill and current unchanged.
        const int k = min(n - processed, B - fill);
        for (int j = tid; j < k; j += NT) ibc[fill + j] = inc[processed + j];
        flags |= FLAG_INBUF;
        for (int j = tid; j < n; j += NT) outc[j] = 0.f;
    }
    if ((fill != 0 || err || pre_next) && owner) {
#pragma unroll
        for (int s = 0; s < SPT; ++s) reinterpret_cast<vec_t *>(prec)[f0 + s * NT] = pacc[s];
    }
    // (a live window stays live only across a step that read it and advanced)
    if (tid == 0) J.state[c] = make_int4(cur, act, fill, la_clear(flags, a) | (gwin && !err ? FLAG_GW : 0));
    // a run's call whose head buffer is out of step with tail_input wrote no
    // spectrum for tail0's pending block: the flush recomputes this channel's
    if (J.t0x && !t0w && tid == 0) J.t0m[c] = 1;
    if (epi && (!one_block || err)) twostage_epilogue<NT>(J, c, outc, inc, n);
    proc_stamp(a, 3);
    return false;
}

// threads per workgroup of the fused kernel: 256 up to B = 1024; larger
// blocks get more lanes so each owns <= 4 slots (no spills at 4 waves/SIMD)
// (B >= 2048 on 512 threads at 2 waves per SIMD: B 4096 197 VGPRs, no
// spills -- on 1024 threads the 128-VGPR cap spilled 34 (B 8192: 96).  A
// one-block step at 256 channels: B 2048 73.1 -> 70.3 us, B 4096 99.8 ->
// 92.2 us, B 8192 125.9 -> 117.5 us; bit-identical; r4e / r4f A/Bs)
constexpr int proc_nt(int log2b) { return log2b <= 10 ? 256 : 512; }

constexpr int kNT = 256;  // threads of the kernels with no geometry of their own (ir_segments_kernel)

}  // namespace fftconv
