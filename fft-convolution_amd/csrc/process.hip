// process.hip -- the generic step's kernels (one call, a run of calls, the
// 256-thread narrow form) and the far-row window anchors of B >= 1024, with
// their launchers.  The step itself is step.hpp's process_job.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "launch.hpp"
#include "step.hpp"

namespace fftconv {

// ---------------------------------------------------------------------------
// Far-row windows of the generic step (B >= 1024).  After step t
// of a batch, the channels of class t mod P (c = t mod P + P j) sum, for each
// of their next P blocks k = 0..P-1 (current = cur' - k, cur' = the state
// after step t), the far rows
//   W[k] = sum_{i=P}^{act-1} H[i] (.) X[(cur' - k + i) % act]
// (src/fft_convolver.rs:244-255 restricted to i >= P): rows written by block t
// or earlier, still in the ring at block t+1+k.  One pass over the far rows
// serves all P windows -- each X row meets P IR rows from a register ring.
// Each window accumulates its rows in the step's order with the step's
// arithmetic (Acc2), so near + W is bit-identical to the step summing the
// far rows itself.  A workgroup: one channel, 256 slots (512 bins).  Channels
// whose ring is off the block path (a buffered partial block, a failed C2R)
// or too short get no window: FLAG_GW cleared.
// long blocks (B > 2^kMaxLog2Fused): windows K0 .. K0+KH-1 of one slot, the
// far rows walked P at a time, software-pipelined (the next P rows' loads
// issued before this batch's MACs); each window sums its rows in the same
// order and arithmetic as the full walk below
#ifndef FFTCONV_GW_SPLIT
#define FFTCONV_GW_SPLIT 1  // threads per slot (2: window halves per thread, 41.9 vs 30.4 us at lgu, rejected)
#endif
template <int LOG2B, int K0, int KH>
__device__ __forceinline__ void gw_walk_long(Acc2 (&w)[KH], const float4 *H4, const float4 *X4, int cur, int act) {
    constexpr int F = (1 << LOG2B) / 2, P = kGwP;
    float4 xr[P];  // X at ring offset o (from cur') in xr[o % P]
#pragma unroll
    for (int o = 1; o < P; ++o) xr[o] = ntld4(X4 + (size_t)((cur + o) % act) * F);
    xr[0] = make_float4(0.f, 0.f, 0.f, 0.f);
    int i0 = P;
    float4 h[P], xn[P];
    if (i0 + P <= act) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
            h[j] = ntld4(H4 + (size_t)(i0 + j) * F);
            xn[j] = ntld4(X4 + (size_t)((cur + i0 + j) % act) * F);
        }
    }
    for (; i0 + P <= act; i0 += P) {
        float4 h2[P], x2[P];
        const bool more = i0 + 2 * P <= act;
        if (more) {
#pragma unroll
            for (int j = 0; j < P; ++j) {
                h2[j] = ntld4(H4 + (size_t)(i0 + P + j) * F);
                x2[j] = ntld4(X4 + (size_t)((cur + i0 + P + j) % act) * F);
            }
        }
#pragma unroll
        for (int j = 0; j < P; ++j)
#pragma unroll
            for (int kk = 0; kk < KH; ++kk) {
                const int k = K0 + kk;
                w[kk].mac(h[j], j >= k ? xn[j - k] : xr[j - k + P]);
            }
#pragma unroll
        for (int j = 0; j < P; ++j) {
            xr[j] = xn[j];
            if (more) {
                h[j] = h2[j];
                xn[j] = x2[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
        if (i0 + j < act) {
            const float4 hv = ntld4(H4 + (size_t)(i0 + j) * F);
            xr[j] = ntld4(X4 + (size_t)((cur + i0 + j) % act) * F);
#pragma unroll
            for (int kk = 0; kk < KH; ++kk) w[kk].mac(hv, xr[(j - (K0 + kk) + P) % P]);
        }
    }
}

template <int LOG2B>
__global__ __launch_bounds__(256) void gw_anchor_kernel(ProcArgs a) {
    constexpr int B = 1 << LOG2B, F = B / 2, P = kGwP;
    const ProcJob &J = a.job[0];
    const int cls = a.gw_t % P;
    const int c = cls + P * (int)blockIdx.y;
    if (c >= a.la_channels) return;
    const int4 st = J.state[c];
    const int cur = st.x, act = st.y;
    if (st.z != 0 || (st.w & (FLAG_INBUF | FLAG_PRE)) || act <= P) {
        if (blockIdx.x == 0 && threadIdx.x == 0) J.state[c].w = st.w & ~FLAG_GW;
        return;
    }
    const size_t rows = (size_t)J.S * B;
    if constexpr (LOG2B > kMaxLog2Fused) {
        // long blocks: FFTCONV_GW_SPLIT threads per slot, each summing P / SPLIT
        // of the windows (SPLIT 2 doubles the waves, one per SIMD at 1, but
        // measured slower: anchor 41.9 vs 30.4 us at lgu, r5ar)
        constexpr int SPLIT = FFTCONV_GW_SPLIT, KH = P / SPLIT, SL = 256 / SPLIT;
        static_assert(P % SPLIT == 0 && SL % 64 == 0, "window split");
        const int part = (int)threadIdx.x / SL;  // (wave-uniform)
        const int f = (int)blockIdx.x * SL + (int)threadIdx.x % SL;
        const float4 *H4 = reinterpret_cast<const float4 *>(J.H + (size_t)c * rows) + f;
        const float4 *X4 = reinterpret_cast<const float4 *>(J.X + (size_t)c * rows) + f;
        Acc2 w[KH];
#pragma unroll
        for (int k = 0; k < KH; ++k) w[k].zero();
        if constexpr (SPLIT == 1) {
            gw_walk_long<LOG2B, 0, KH>(w, H4, X4, cur, act);
        } else if constexpr (SPLIT == 2) {
            if (part == 0) gw_walk_long<LOG2B, 0, KH>(w, H4, X4, cur, act);
            else gw_walk_long<LOG2B, KH, KH>(w, H4, X4, cur, act);
        } else {
            static_assert(SPLIT <= 2, "window split");
        }
        float4 *W4 = reinterpret_cast<float4 *>(a.gw + (size_t)c * P * B) + f;
#pragma unroll
        for (int k = 0; k < KH; ++k) ntst4(W4 + (size_t)(part * KH + k) * F, w[k].get(f));
        if (blockIdx.x == 0 && threadIdx.x == 0) J.state[c].w = st.w | FLAG_GW;
        return;
    }
    const int f = (int)blockIdx.x * 256 + (int)threadIdx.x;  // float4 slot
    const float4 *H4 = reinterpret_cast<const float4 *>(J.H + (size_t)c * rows) + f;
    const float4 *X4 = reinterpret_cast<const float4 *>(J.X + (size_t)c * rows) + f;
    Acc2 w[P];
    float4 xr[P];  // X at ring offset o (from cur') in xr[o % P]
#pragma unroll
    for (int k = 0; k < P; ++k) w[k].zero();
#pragma unroll
    for (int o = 1; o < P; ++o) {
        DBG_CHECK((cur + o) % act < J.S, 41, cur, o, act, J.S);
        xr[o] = ntld4(X4 + (size_t)((cur + o) % act) * F);
    }
    // P rows in flight (B <= 8192: the two-stage tail's anchor beside the
    // head on few CUs -- the plain loop's lower register count measured
    // faster there than the pipelined walk of gw_walk_long)
    int i0 = P;
    for (; i0 + P <= act; i0 += P) {
        float4 h[P], xn[P];
#pragma unroll
        for (int j = 0; j < P; ++j) {
            h[j] = ntld4(H4 + (size_t)(i0 + j) * F);
            xn[j] = ntld4(X4 + (size_t)((cur + i0 + j) % act) * F);
        }
#pragma unroll
        for (int j = 0; j < P; ++j)
#pragma unroll
            for (int k = 0; k < P; ++k) w[k].mac(h[j], j >= k ? xn[j - k] : xr[j - k + P]);
#pragma unroll
        for (int j = 0; j < P; ++j) xr[j] = xn[j];
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
        if (i0 + j < act) {
            const float4 hv = ntld4(H4 + (size_t)(i0 + j) * F);
            xr[j] = ntld4(X4 + (size_t)((cur + i0 + j) % act) * F);
#pragma unroll
            for (int k = 0; k < P; ++k) w[k].mac(hv, xr[(j - k + P) % P]);
        }
    }
    float4 *W4 = reinterpret_cast<float4 *>(a.gw + (size_t)c * P * B) + f;
#pragma unroll
    for (int k = 0; k < P; ++k) ntst4(W4 + (size_t)k * F, w[k].get(f));
    if (blockIdx.x == 0 && threadIdx.x == 0) J.state[c].w = st.w | FLAG_GW;
}

template <int LOG2B, int NT, bool ZZ, bool NTL>
__global__ __launch_bounds__(NT, NT == 512 ? 2 : 4) void upols_process_kernel(ProcArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const size_t c = blockIdx.x;
    const ProcJob &J = a.job[blockIdx.y];
    unsigned t0 = 0;
    if (a.la_trace) t0 = (unsigned)__builtin_amdgcn_s_memrealtime();
    process_job<LOG2B, NT, ZZ, NTL>(a, J, c, J.state[c], smem);
    if (a.sig_mode == 1) sig_arrive(a);
    if (a.la_trace && blockIdx.y == 0 && (threadIdx.x >> 6) < 4 && (threadIdx.x & 63) == 0) {
        // launch timeline (FFTCONV_PROC_TRACE, tuning): role 6, as upols_la_kernel's record
        const unsigned t1 = (unsigned)__builtin_amdgcn_s_memrealtime();
        const unsigned hw = (unsigned)__builtin_amdgcn_s_getreg(0xF804);   // HW_REG_HW_ID
        const unsigned xcc = (unsigned)__builtin_amdgcn_s_getreg(0xF814);  // HW_REG_XCC_ID
        const int wave = (int)(threadIdx.x >> 6);
        a.la_trace[(size_t)blockIdx.x * 4 + wave] =
            make_int4(6 | (wave << 4), (int)((hw & 0xffffu) | ((xcc & 0xffu) << 24)), (int)t0, (int)t1);
    }
}

// ---------------------------------------------------------------------------
// A run of consecutive process() calls in ONE launch (process_device_steps of
// a TwoStageFFTConvolver inside one tail period): call k is job[0] with its
// input / output advanced by k steps and its two-stage slices (tail
// precalculated, tail_input) by k blocks.  Channels are independent, so each
// workgroup loops over its channel's calls with no grid-wide sync: call k+1
// reads the state, FDL row, pre_multiplied and overlap call k stored, which
// the barrier between calls makes visible to every wave of the workgroup.
// The body is process_job, the one-call kernel's, so the bits are the same.
// The kernel boundary between calls goes away (cfg3's head: ~1 us of its
// ~4.9 us per launch).  At most 2 workgroups per CU (256 VGPRs):
// the loop keeps its addresses live, and a 128-VGPR body spilled (r4p).
// ---------------------------------------------------------------------------
template <int LOG2B, int NT, bool NTL>
__global__ __launch_bounds__(NT, 2) void upols_run_kernel(ProcArgs a, RunSteps r) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const size_t c = blockIdx.x;
    ProcJob J = a.job[0];
    RunCarry rc{};
    // (issue priority over the waves of other kernels on the same SIMD: the
    // two-stage tail beside the run; 1 = the chain wave, 2 = every wave)
    if (a.prio == 2 || (a.prio == 1 && threadIdx.x < 64)) __builtin_amdgcn_s_setprio(3);
    if (a.sig_mode == 2) sig_wait(a);  // (the previous tail step's output, which the calls add)
    unsigned t0 = 0;
    using Gm = Geo<LOG2B, NT>;
    const int rl = a.run_lds_rows;  // (the IR rows and the FDL in LDS for the run: their row count)
    if (rl > 0) {
        float2 *hl = reinterpret_cast<float2 *>(smem + Gm::lds_bytes + 4 * (size_t)Gm::B * sizeof(float2));
        rc.hl = hl;
        rc.xl = hl + (size_t)rl * Gm::B;
        dma_16b<NT>(hl, J.H + c * (size_t)J.S * Gm::B, rl * Gm::B * (int)sizeof(float2));
    }
    for (int k = 0; k < r.n; ++k) {
        if (a.la_trace && k == r.n - 1) t0 = (unsigned)__builtin_amdgcn_s_memrealtime();  // (the last call's start)
        if (rl > 0 && !rc.hot) {
            // the FDL into LDS: at the run's start, and after a call that
            // did not run the pipelined step to its end (the generic step and
            // a failed C2R touch only the FDL in memory)
            dma_16b<NT>(rc.xl, J.X + c * (size_t)J.S * Gm::B, rl * Gm::B * (int)sizeof(float2));
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        rc.next_in = k + 1 < r.n ? J.in + r.in_step : nullptr;
        // (a hot call's state word is the one the previous call stored; the
        // reload stays behind the branch -- a speculated load would put a
        // memory round trip at the start of every call)
        int4 st = rc.st;
        if (!rc.hot) {
            asm volatile("" ::: "memory");
            st = J.state[c];
        }
        const bool kept = process_job<LOG2B, NT, false, NTL, true>(a, J, c, st, smem, &rc);
        rc.hot = kept && rc.next_in != nullptr;  // (the next call's block is in stage[par ^ 1])
        rc.par ^= 1;
        __syncthreads();
        J.in += r.in_step;
        J.out += r.out_step;
        if (J.add0) J.add0 += J.n;
        if (J.add1) J.add1 += J.n;
        if (J.tin) J.tin += J.n;
        if (J.t0x) J.t0x += J.n;
    }
    if (a.la_trace && (threadIdx.x >> 6) < 4 && (threadIdx.x & 63) == 0) {
        // launch timeline (FFTCONV_PROC_TRACE, tuning): the run's last call,
        // role 6 as upols_process_kernel's record (the phase stamps are that call's)
        const unsigned t1 = (unsigned)__builtin_amdgcn_s_memrealtime();
        const unsigned hw = (unsigned)__builtin_amdgcn_s_getreg(0xF804);   // HW_REG_HW_ID
        const unsigned xcc = (unsigned)__builtin_amdgcn_s_getreg(0xF814);  // HW_REG_XCC_ID
        const int wave = (int)(threadIdx.x >> 6);
        a.la_trace[(size_t)blockIdx.x * 4 + wave] =
            make_int4(6 | (wave << 4), (int)((hw & 0xffffu) | ((xcc & 0xffu) << 24)), (int)t0, (int)t1);
    }
}

template <int LOG2B>
static hipError_t launch_gw_anchor_t(const ProcArgs &a, int channels, hipStream_t s) {
    constexpr int F = (1 << LOG2B) / 2;
    constexpr int SL = LOG2B > kMaxLog2Fused ? 256 / FFTCONV_GW_SPLIT : 256;  // slots per workgroup
    static_assert(F % 256 == 0, "a workgroup covers 256 slots");
    const int cls = a.gw_t % kGwP;
    if (channels <= cls || a.gw == nullptr) return hipSuccess;
    ProcArgs args = a;
    args.la_channels = channels;
    const int ny = (channels - cls + kGwP - 1) / kGwP;
    return launch_dyn(gw_anchor_kernel<LOG2B>, dim3(F / SL, ny), dim3(256), 0, s, args);
}

hipError_t launch_gw_anchor(int log2b, const ProcArgs &a, int channels, hipStream_t s) {
    return dispatch_log2<10, kMaxLog2Block>(log2b, hipErrorInvalidValue,
                                            [&](auto L) { return launch_gw_anchor_t<L()>(a, channels, s); });
}

bool gw_supported(int log2b, int S) { return log2b >= 10 && log2b <= kMaxLog2Block && S >= 3 * kGwP; }

// The generic step on 256 threads for 2048 <= B <= 8192 (ProcArgs::narrow):
// one wave per SIMD and up to 512 VGPRs, so that the workgroup fits a CU
// beside a multi-call run's workgroup (4 waves of ~208 VGPRs) -- the
// 512-thread kernel's 2 waves per SIMD of ~200 VGPRs do not, and the cfg3
// tail then waited for the few CUs the run left free (227 us per period
// beside the run vs 44 us alone, profiles/r5/r5ai).  The MAC keeps each
// slot's row order and the transforms the same butterflies: same bits.
// (at most 256 registers: 2 waves per SIMD -- with a run workgroup's ~240 on
// the same SIMD; unbounded it took 255 VGPRs + 30 AGPRs, and beside the
// run's LDS-resident rows (237 VGPRs) it no longer fit: 200 us per tail
// step instead of 58, profiles/r6/r6h)
template <int LOG2B, bool ZZ, bool NTL>
__global__ __launch_bounds__(256, 2) void upols_narrow_kernel(ProcArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const size_t c = blockIdx.x;
    const ProcJob &J = a.job[blockIdx.y];
    process_job<LOG2B, 256, ZZ, NTL>(a, J, c, J.state[c], smem);
    if (a.sig_mode == 1) sig_arrive(a);
}

// One step launch of a kernel family kernel(ZZ, NTL) (zig-zag scan,
// nontemporal loads: the variant's bits 0 and 1) on NT threads.
template <int LOG2B, int NT, class Family>
static hipError_t launch_step_t(Family kernel, bool may_pipe, const ProcArgs &a, int channels, hipStream_t s) {
    using Y = std::true_type;
    using N = std::false_type;
    void (*const kern[4])(ProcArgs) = {kernel(N{}, N{}), kernel(Y{}, N{}), kernel(N{}, Y{}), kernel(Y{}, Y{})};
    const int var = pick_variant(Variant::current(), a, channels, LOG2B);
    ProcArgs args = a;
    args.pipe = may_pipe && !(var & VARIANT_NOPIPE) ? 1 : 0;
    args.lag = pipeline_lag();
    return launch_dyn(kern[var & 3], dim3(channels, a.njobs), dim3(NT), Geo<LOG2B, NT>::lds_bytes, s, args);
}

template <int LOG2B>
static hipError_t launch_process_t(const ProcArgs &a, int channels, hipStream_t s) {
    if constexpr (LOG2B >= 11 && LOG2B <= kMaxLog2Fused) {
        if (a.narrow)
            return launch_step_t<LOG2B, 256>(
                [](auto zz, auto ntl) { return upols_narrow_kernel<LOG2B, zz(), ntl()>; }, false, a, channels, s);
    }
    constexpr int PNT = proc_nt(LOG2B);
    return launch_step_t<LOG2B, PNT>(
        [](auto zz, auto ntl) { return upols_process_kernel<LOG2B, PNT, zz(), ntl()>; }, true, a, channels, s);
}

template <int LOG2B>
static hipError_t launch_run_t(const ProcArgs &a, const RunSteps &r, int channels, hipStream_t s) {
    if constexpr (LOG2B >= 6 && LOG2B <= 9) {
        constexpr int PNT = proc_nt(LOG2B);
        using Gm = Geo<LOG2B, PNT>;
        if (a.njobs != 1 || r.n < 1) return hipErrorInvalidValue;
        const int var = pick_variant(Variant::current(), a, channels, LOG2B);
        if (var & 1) return hipErrorInvalidValue;  // (zig-zag order: per-call launches only)
        ProcArgs args = a;
        args.pipe = (var & VARIANT_NOPIPE) ? 0 : 1;
        args.lag = pipeline_lag();
        auto kern = (var & VARIANT_NT) ? upols_run_kernel<LOG2B, PNT, true> : upols_run_kernel<LOG2B, PNT, false>;
        // (+ the run-carried spectra and the next block's transform buffers,
        // pipelined_step; + the IR rows and the FDL when they fit)
        const size_t lds = Gm::lds_bytes + 4 * (size_t)Gm::B * sizeof(float2) +
                           (size_t)a.run_lds_rows * 2 * Gm::B * sizeof(float2);
        if (a.run_lds_rows < 0 || lds > 160 * 1024) return hipErrorInvalidValue;
        return launch_dyn(kern, dim3(channels), dim3(PNT), lds, s, args, r);
    } else {
        return hipErrorNotSupported;
    }
}
// the row count of a run's LDS-resident IR rows + FDL (ProcArgs::run_lds_rows):
// S when a run workgroup's LDS stays within 96 KiB -- room left for a 64 KiB
// two-stage tail workgroup on the same CU (cfg3: B 64, S 64 -> 74 KiB) -- and
// only for the run-carried pipelined step (B <= 256); else 0
int run_lds_rows(int log2b, int S) {
    if (log2b < 6 || log2b > 8 || S < 2) return 0;
    if (Variant::current().has(VARIANT_NORUNLDS)) return 0;  // (not selectable through the ABI, variant.hpp)
    const size_t B = (size_t)1 << log2b;
    static_assert(proc_nt(8) == 256, "process_lds_bytes: the run kernels' 256 threads");
    const size_t base = process_lds_bytes(log2b) + 4 * B * sizeof(float2);
    return base + (size_t)S * 2 * B * sizeof(float2) <= 96 * 1024 ? S : 0;
}
bool run_supported(int log2b) {
    return log2b >= 6 && log2b <= 9 && !Variant::current().has(VARIANT_NORUN | VARIANT_ZIGZAG);
}
hipError_t launch_process_run(int log2b, const ProcArgs &a, const RunSteps &r, int channels, hipStream_t s) {
    if (channels <= 0) return hipSuccess;
    return dispatch_log2<6, 9>(log2b, hipErrorNotSupported,
                               [&](auto L) { return launch_run_t<L()>(a, r, channels, s); });
}

hipError_t launch_process(int log2b, const ProcArgs &a, int channels, hipStream_t s) {
    if (channels <= 0) return hipSuccess;
    if (log2b > kMaxLog2Fused) return launch_process_large(log2b, a, a.lg, a.lg_chunks, channels, s);
    return dispatch_fused(log2b, [&](auto L) { return launch_process_t<L()>(a, channels, s); });
}

size_t process_lds_bytes(int log2b) {
    return dispatch_log2<0, kMaxLog2Fused>(log2b, (size_t)0,
                                           [](auto L) -> size_t { return Geo<L(), proc_nt(L())>::lds_bytes; });
}

}  // namespace fftconv
