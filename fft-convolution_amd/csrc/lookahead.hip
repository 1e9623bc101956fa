// lookahead.hip -- the lookahead step (la.hpp: upols_la_kernel), the window
// rebuild after update / reset / init, the per-call batch of steps
// (la_batch.hpp), and their launchers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.hpp"
#include "la.hpp"
#include "la_batch.hpp"
#include "launch.hpp"

namespace fftconv {

// Lookahead geometry policy: block sizes whose row is whole waves of float4
// slots (128..512) and FDLs long enough that the anchor levels dominate.  A
// function of (B, S) only, never of the channel count.
int la_parts(int log2b, int S) {
    if (log2b < 7 || log2b > 9) return 0;
    if (Variant::current().has(VARIANT_NOLA)) return 0;
    if (S < 40) return 0;  // (channels whose active segments drop below D0 + 2 step generically)
    return 1;
}
LaDims la_dims(int log2b, int S, int jw) {
    LaDims d{};
    d.nlv = la_nlv(S);
    for (int lv = 1; lv <= 3; ++lv) d.per[lv - 1] = la_per(lv);
    const int nsl = log2b >= 7 ? (1 << (log2b - 1)) / 64 : 1;  // LaGeo::NSL
    d.wg[0] = log2b <= LA_MIDIN_MAXLOG ? 0 : 1;                // LaStep::MIDIN: level 1 in the step workgroups
    d.wg[1] = nsl * (LA_P2 / jw);
    d.wg[2] = d.nlv == 3 ? nsl * (LA_P3 / jw) : 0;
    d.pt = LA_PT;
    d.per_all = LA_PER;
    return d;
}

// anchor workgroups of a launch (ProcArgs::la_n): per level the scheduled
// channels of [c0, C) -- all of them when la_all > 0 -- in whole XCD rounds
// of 8 for the level 2/3 anchors (la_anchor_far)
// fold (ProcArgs::la_l1in2): level-1 anchors ride in the level-2 anchor
// workgroups (one each, after the level-2 walk), so the level-2 count covers
// the level-1 channels too.
static void la_counts(ProcArgs &a, int log2b, int S, int C, bool all, bool mid_wg, bool fold = false,
                      int jw = LA_JW) {
    const LaDims d = la_dims(log2b, S, jw);
    int n1 = 0;
    for (int lv = 1; lv <= 3; ++lv) {
        const int P = d.per[lv - 1];
        const int t0 = a.la_t % P;
        const int n = all ? C - a.la_c0 : (C > t0 ? (C - t0 + P - 1) / P : 0);
        if (lv == 1) {
            n1 = n;
            a.la_n[0] = mid_wg ? (n + 7) / 8 * 8 : 0;  // (whole rounds of 8: the XF 3 grid interleave)
        } else {
            a.la_n[lv - 1] = (lv <= d.nlv) ? (n + 7) / 8 * 8 * d.wg[lv - 1] : 0;
        }
    }
    if (fold) a.la_n[1] = std::max(a.la_n[1], (n1 + 7) / 8 * 8);
    a.la_l1in2 = fold ? 1 : 0;
    a.la_nlv = d.nlv;
}

template <int LOG2B>
static hipError_t launch_la_t(const ProcArgs &a, int channels, hipStream_t s) {
    if constexpr (LOG2B < 7 || LOG2B > 9) {
        return hipErrorNotSupported;
    } else {
        using LG = LaGeo<LOG2B>;
        const bool xf3 = a.la_mix == 3;
        const size_t lsb = xf3 ? LaStep<LOG2B, 3>::bytes : LaStep<LOG2B>::bytes;
        const int nch = xf3 ? 1 : LaStep<LOG2B>::NCH;  // channels per step workgroup
        constexpr size_t gen = Geo<LOG2B, LA_NT>::lds_bytes;
        const size_t lds0 = lsb > LG::anchor_bytes ? lsb : LG::anchor_bytes;
        const size_t lds1 = lds0 > gen ? lds0 : gen;
        const size_t lds = (lds1 + 15) / 16 * 16;
        if (!a.laW) return hipErrorInvalidValue;
        if (xf3 && (a.njobs != 2 || !a.laW2 || a.job[0].S != a.job[1].S || a.job[0].n != a.job[1].n ||
                    a.job[0].add0 || a.job[1].add0 || !a.mix.buf_a || !a.mix.buf_b))
            return hipErrorInvalidValue;
        // the full-pass streams: nontemporal once the whole H + FDL working
        // set exceeds the Infinity Cache
        const Variant v = Variant::current();
        const bool ntl = v.nt_stream(Variant::stream_bytes(channels, a.job[0].S, LOG2B));
        auto kern = a.la_mix == 1   ? (ntl ? upols_la_kernel<LOG2B, true, 1> : upols_la_kernel<LOG2B, false, 1>)
                    : a.la_mix == 2 ? (ntl ? upols_la_kernel<LOG2B, true, 2> : upols_la_kernel<LOG2B, false, 2>)
                    : xf3           ? (ntl ? upols_la_kernel<LOG2B, true, 3> : upols_la_kernel<LOG2B, false, 3>)
                                    : (ntl ? upols_la_kernel<LOG2B, true, 0> : upols_la_kernel<LOG2B, false, 0>);
        ProcArgs args = a;
        args.pipe = 0;
        args.lag = 0;
        args.la_channels = channels;
        args.la_c0 = 0;
        args.la_rebuild = 0;
        args.la_t = a.la_t % LA_PER;
        if (v.has(VARIANT_LAFULL)) args.la_all = -1;  // no anchors: every eligible step sums all its rows
        // standalone batches at B <= 256: level 1 in the level-2 anchor
        // workgroups (they finish their walks first); the crossfade launches
        // keep it in the step workgroups (LaStep::MIDIN)
        const bool fold = a.la_mix == 0 && LOG2B <= LA_MIDIN_MAXLOG;
        const bool midin = !fold && LOG2B <= LA_MIDIN_MAXLOG;
        la_counts(args, LOG2B, a.job[0].S, channels, args.la_all > 0, !fold && !midin, fold);
        if (args.la_all < 0) args.la_n[0] = args.la_n[1] = args.la_n[2] = 0;
        const int nstep = (channels + nch - 1) / nch;
        if (a.la_mix == 2 && a.job[0].add0) return hipErrorInvalidValue;  // (the fused mix uses the add buffers' LDS)
        const int xwg = a.la_mix == 1 ? LA_XWG : 0;  // A's launch: the mix_value walk workgroups
        const int nanch = (xf3 ? 2 : 1) * (args.la_n[0] + args.la_n[1] + args.la_n[2]);
        return launch_dyn(kern, dim3(nanch + nstep + xwg), dim3(LA_NT), lds, s, args);
    }
}

hipError_t launch_process_la(int log2b, const ProcArgs &a, int channels, hipStream_t s) {
    if (channels <= 0) return hipSuccess;
    if (a.njobs != (a.la_mix == 3 ? 2 : 1) || !a.laW) return hipErrorInvalidValue;
    return dispatch_fused(log2b, [&](auto L) { return launch_la_t<L()>(a, channels, s); });
}

int la_trace_grid(int log2b, int S, int channels) {  // (steady-state launches: la_t = 0 has the most anchors)
    if (log2b < 7 || log2b > 9) return 0;
    ProcArgs a{};
    la_counts(a, log2b, S, channels, false, true, true);
    return 2 * (a.la_n[0] + a.la_n[1] + a.la_n[2]) + channels + LA_XWG;  // (XF 3: A's and B's anchors)
}

// ---------------------------------------------------------------------------
// Window rebuild after update() / reset / init (FFTConvolver::update
// :174-213 keeps the FDL but replaces H, so every partial-sum window is
// stale).  Instead of the next process launch re-anchoring every channel on
// its latency-critical path, the update enqueues this anchors-only launch:
// each channel's windows of every level, as the anchors of the previous
// launch would have left them (la_anchor_state, la_rebuild), then the state
// words pointing at them.  The next process launch is a steady-state launch.
// ---------------------------------------------------------------------------
#ifndef FFTCONV_RB_WPC
#define FFTCONV_RB_WPC 4
#endif
#ifndef FFTCONV_RB_UF
#define FFTCONV_RB_UF LA_UF
#endif
// window steps per level-2/3 rebuild workgroup (LA_JW in the process launches):
// each workgroup walks its rows once for RB_JW steps, so the rows' L2
// requests scale with P / RB_JW; same rows in the same order per step
#ifndef FFTCONV_RB_JW
#define FFTCONV_RB_JW LA_JW
#endif
constexpr int RB_JW = FFTCONV_RB_JW;
static_assert(LA_JW == 8, "la_dims' default window slice (kernels.hpp)");
template <int LOG2B, bool NTL>
__global__ __launch_bounds__(LA_NT, FFTCONV_RB_WPC) void la_rebuild_kernel(ProcArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    la_anchor<LOG2B, NTL, FFTCONV_RB_UF, RB_JW>(a, 0, (int)blockIdx.x, smem);
}

// the state words of the rebuilt windows (same eligibility test as the
// anchors: both read the state word the update left)
template <int LOG2B>
__global__ void la_rebuild_state_kernel(ProcArgs a) {
    const int c = a.la_c0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= a.la_channels) return;
    const int4 st = a.job[0].state[c];
    // (vnext, when the host passes it: the next lookahead launch's copy of
    // every word, la.hpp la_anchor_state -- no separate refresh copy)
    int4 *vn = a.job[0].vnext;
    if (!la_eligible<LOG2B>(st, a.job[0].n)) {
        if (vn) vn[c] = st;
        return;
    }
    int nf = st.w & ~(LA_MASK | SEQ_MASK);  // (launch tag 0: no process launch wrote it)
    // (the anchors wrote the other window of each level: toggle its flag)
    for (int lv = 1; lv <= a.la_nlv; ++lv) nf = (nf ^ la_flag_win(lv)) | la_flag_live(lv);
    a.job[0].state[c].w = nf;
    if (vn) vn[c] = make_int4(st.x, st.y, st.z, nf);
}

template <int LOG2B>
static hipError_t launch_rebuild_t(const ProcArgs &a, int channels, hipStream_t s) {
    if constexpr (LOG2B < 7 || LOG2B > 9) {
        return hipErrorNotSupported;
    } else {
        using LG = LaGeo<LOG2B>;
        constexpr size_t anchor_bytes = (size_t)(LA_NG - 1) * RB_JW * LG::FS * 16;  // (LaGeo::anchor_bytes at RB_JW)
        constexpr size_t lds = (anchor_bytes + 15) / 16 * 16 + 16;
        if (!a.laW || a.njobs != 1 || a.job[0].n != (1 << LOG2B)) return hipErrorInvalidValue;
        const bool ntl = Variant::current().nt_stream(Variant::stream_bytes(channels, a.job[0].S, LOG2B));
        auto kern = ntl ? la_rebuild_kernel<LOG2B, true> : la_rebuild_kernel<LOG2B, false>;
        ProcArgs args = a;
        args.la_channels = channels;
        args.la_all = 1;
        args.la_rebuild = 1;
        args.la_seq = 0;
        args.la_t = a.la_t % LA_PER;
        const int nch = channels - a.la_c0;
        if (nch <= 0) return hipSuccess;
        la_counts(args, LOG2B, a.job[0].S, channels, true, true, false, RB_JW);  // (level 1 in workgroups of its own)
        if (hipError_t e = launch_dyn(kern, dim3(args.la_n[0] + args.la_n[1] + args.la_n[2]), dim3(LA_NT), lds, s, args);
            e != hipSuccess)
            return e;
        return launch_dyn(la_rebuild_state_kernel<LOG2B>, dim3((nch + 255) / 256), dim3(256), 0, s, args);
    }
}

hipError_t launch_la_rebuild(int log2b, const ProcArgs &a, int channels, hipStream_t s) {
    if (channels <= 0) return hipSuccess;
    return dispatch_fused(log2b, [&](auto L) { return launch_rebuild_t<L()>(a, channels, s); });
}

// ---------------------------------------------------------------------------
// A chunk of one-block steps in four launches (la_batch.hpp), all on stream s:
// each reads what the one before it wrote.
// ---------------------------------------------------------------------------
template <int LOG2B>
static hipError_t launch_batch_t(const ProcArgs &a, const LaBatchArgs &b, int channels, hipStream_t s) {
    if constexpr (LOG2B < 7 || LOG2B > 9) {
        return hipErrorNotSupported;
    } else {
        using LG = LaGeo<LOG2B>;
        if (!a.laW || !b.resume || a.njobs != 1 || a.job[0].n != (1 << LOG2B) || b.k < 1 || b.k > LA_BATCH_MAX ||
            (b.seq0 != 1 && b.seq0 != 2) || a.la_mix || a.job[0].add0 || a.job[0].tin || a.la_trace ||
            a.la_probe_cnt)
            return hipErrorInvalidValue;
        ProcArgs args = a;
        args.pipe = 0;
        args.lag = 0;
        args.la_channels = channels;
        args.la_c0 = 0;
        args.la_rebuild = 0;
        args.la_all = -1;
        args.la_n[0] = args.la_n[1] = args.la_n[2] = 0;
        args.la_l1in2 = 0;
        args.la_nlv = la_nlv(a.job[0].S);
        args.job[0].mcall = 1;
        args.job[0].mk = 0;
        args.job[0].sview = nullptr;
        args.job[0].vnext = nullptr;
        if (hipError_t e = launch_dyn(la_batch_spectra_kernel<LOG2B>, dim3(channels, (b.k + 3) / 4), dim3(LA_NT),
                                      LabSpectra<LOG2B>::bytes, s, args, b);
            e != hipSuccess)
            return e;
        const bool wide = lab_wide(channels, LG::NSL, b.k);
        const int wga = LG::NSL * (wide ? (b.k + LAB_JW - 1) / LAB_JW : (b.k + LA_JW - 1) / LA_JW);
        if (hipError_t e = wide ? launch_dyn(la_batch_walk_kernel<LOG2B, LAB_JW, LAB_U, 2>,
                                             dim3((channels + 7) / 8 * 8 * wga), dim3(LA_NT),
                                             LabWalk<LOG2B, LAB_JW>::bytes, s, args, b)
                                : launch_dyn(la_batch_walk_kernel<LOG2B, LA_JW, LA_UF, 4>,
                                             dim3((channels + 7) / 8 * 8 * wga), dim3(LA_NT),
                                             LabWalk<LOG2B, LA_JW>::bytes, s, args, b);
            e != hipSuccess)
            return e;
        if (hipError_t e = launch_dyn(la_batch_finish_kernel<LOG2B>, dim3(channels), dim3(LA_NT),
                                      LabFinish<LOG2B>::bytes, s, args, b);
            e != hipSuccess)
            return e;
        // the fix-up's steps are la_fallback's: the lookahead step of one
        // channel or the generic step
        constexpr size_t lds = LabFixup<LOG2B>::bytes;
        const bool ntl = Variant::current().nt_stream(Variant::stream_bytes(channels, a.job[0].S, LOG2B));
        auto fix = ntl ? la_batch_fixup_kernel<LOG2B, true> : la_batch_fixup_kernel<LOG2B, false>;
        return launch_dyn(fix, dim3(channels), dim3(LA_NT), lds, s, args, b);
    }
}

hipError_t launch_la_batch(int log2b, const ProcArgs &a, const LaBatchArgs &b, int channels, hipStream_t s) {
    if (channels <= 0) return hipSuccess;
    return dispatch_fused(log2b, [&](auto L) { return launch_batch_t<L()>(a, b, channels, s); });
}

}  // namespace fftconv
