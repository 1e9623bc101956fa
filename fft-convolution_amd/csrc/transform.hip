// transform.hip -- kernels beside the step: the IR partition transforms (init
// / update), the public Fft's rows, the two-stage sub-chunk accumulate and the
// state-word kernels, with their launchers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_lds.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "step.hpp"

namespace fftconv {

// IR transform (init / update): H rows stored nontemporal, so the window
// rebuild behind it finds them written out instead of dirty in L2 (cfg2
// update: rebuild 277 -> 261 us, cfg2u +1.1 %, profiles/r5/r5i_*)
#ifndef FFTCONV_IR_NTST
#define FFTCONV_IR_NTST 1
#endif

// ---------------------------------------------------------------------------
// IR partition: FFTConvolver::init (:131-142) / update (:190-212).
// grid (S, channels): workgroup (i, c) transforms segment i of channel
// chan0 + c; segments at or past ceil(len_active / B) are zeroed.
// ---------------------------------------------------------------------------
template <int LOG2B, int NT>
__global__ __launch_bounds__(NT) void ir_segments_kernel(IrArgs a) {
    constexpr int B = 1 << LOG2B;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *bufA = reinterpret_cast<float2 *>(smem);
    float2 *bufB = bufA + B;
    const int tid = threadIdx.x;
    const int i = blockIdx.x;
    const size_t c = a.chan0 + blockIdx.y;
    const size_t rows = (size_t)a.S * B;
    float2 *row = a.H + c * rows + (size_t)i * B;
    const long long active = (a.len_active + B - 1) / B;

    if (a.update_state && i == 0) {
        // update(): zero overlap / pre_multiplied / conv, set active (:185-190)
        for (int j = tid; j < B; j += NT) {
            a.overlap[c * B + j] = 0.f;
            a.pre[c * B + j] = make_float2(0.f, 0.f);
        }
        if (tid == 0) {
            a.state[c].y = (int)active;
            a.state[c].w &= ~(FLAG_PRE | LA_MASK | SEQ_MASK);  // the stored pre / window used the old response
        }
    }
    if (i >= active) {  // :210-212
        for (int j = tid; j < B; j += NT) row[j] = make_float2(0.f, 0.f);
        return;
    }
    const float *src = a.src + blockIdx.y * a.src_stride;
    const long long base = (long long)i * B;
    for (int m = tid; m < B; m += NT) {
        const long long i0 = base + 2 * m, i1 = base + 2 * m + 1;
        float2 z;
        z.x = (2 * m < B && i0 < a.len_data) ? src[i0] : 0.f;
        z.y = (2 * m + 1 < B && i1 < a.len_data) ? src[i1] : 0.f;
        bufA[m] = z;
    }
    __syncthreads();
    const float2 *Z = lds_cfft<LOG2B, NT, false>(bufA, bufB, a.tw);
    for (int m = tid; m < B; m += NT) row[m] = real_post<LOG2B, NT>(Z, m, a.tw);
}

// The same transforms one segment per wave (64 <= B <= 1024), each wave
// walking IR_SPW segments and loading the next segment's samples into
// registers while it transforms the current one (the transform was a
// dependent load -> FFT -> store chain per segment).  For B >= 128 (M = B
// complex points, the upper half the zero padding):
//  * stage 0 runs in registers from the loaded samples (wave_stage0_padded:
//    two of a butterfly's four inputs are padding), so neither the samples
//    nor the padding go through LDS;
//  * the middle stages read the per-stage twiddle table (TwStaged: gathered
//    once per workgroup, consecutive entries per stage -- the full table's
//    strided reads were the kernel's LDS bank conflicts);
//  * the last stage and realfft's post-twiddle run in registers with the
//    mirror bin fetched by __shfl (wave_r2c_post), straight to HBM.
// Same butterflies and twiddle values in the same order as
// ir_segments_kernel, so the same bits.
//  * B >= 128: the middle stages run in place (wave_stages_inplace), so a
//    wave needs one B-point buffer and a workgroup runs IR_NW = 8 waves --
//    twice the segment loads in flight per CU of the ping-pong layout.
// grid (ceil(S / (NW * IR_SPW)), channels); LDS: tw (2B) | NW x bufA (| bufB: B < 128)
#ifndef FFTCONV_IR_SPW
#define FFTCONV_IR_SPW 2
#endif
constexpr int IR_SPW = FFTCONV_IR_SPW;
// segments loaded ahead of the one being transformed (1: the next one only)
#ifndef FFTCONV_IR_PF
#define FFTCONV_IR_PF 1
#endif
constexpr int IR_PF = FFTCONV_IR_PF;
static_assert(IR_PF >= 1 && IR_PF <= IR_SPW, "prefetch depth");
template <int LOG2B>
constexpr int ir_nw() { return LOG2B >= 7 ? 8 : 4; }
template <int LOG2B>
constexpr size_t ir_wave_lds() { return (size_t)(2 + ir_nw<LOG2B>() * (LOG2B >= 7 ? 1 : 2)) * (1 << LOG2B) * sizeof(float2); }
template <int LOG2B>
__global__ __launch_bounds__(64 * ir_nw<LOG2B>()) void ir_segments_wave_kernel(IrArgs a) {
    constexpr int B = 1 << LOG2B;
    constexpr bool REG = LOG2B >= 7;                        // register stage 0 / __shfl last stage
    constexpr int NW = ir_nw<LOG2B>(), NT = 64 * NW;
    constexpr int NPL = REG ? stage0_per_lane<LOG2B>() : (B / 2 + 63) / 64;  // per lane: butterflies / points
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *twl = reinterpret_cast<float2 *>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float2 *bufA = twl + 2 * B + (size_t)wave * (REG ? 1 : 2) * B;
    float2 *bufB = bufA + B;
    const size_t c = a.chan0 + blockIdx.y;
    const size_t rows = (size_t)a.S * B;
    const long long active = (a.len_active + B - 1) / B;
    if constexpr (REG) tws_build<LOG2B, NT>(twl, a.tw, tid);
    else dma_16b<NT>(twl, a.tw, 2 * B * (int)sizeof(float2));
    if (a.update_state && blockIdx.x == 0) {
        // update(): zero overlap / pre_multiplied / conv, set active (:185-190)
        for (int j = tid; j < B; j += NT) {
            a.overlap[c * B + j] = 0.f;
            a.pre[c * B + j] = make_float2(0.f, 0.f);
        }
        if (tid == 0) {
            a.state[c].y = (int)active;
            a.state[c].w &= ~(FLAG_PRE | LA_MASK | SEQ_MASK);  // the stored pre / window used the old response
        }
    }
    const float *src = a.src + blockIdx.y * a.src_stride;
    // (a channel's response 8-byte aligned: a point inside the data is one
    // 8-byte load, half the load instructions of two 4-byte ones)
    const bool al8 = ((uintptr_t)src & 7) == 0;
    // copy_and_pad (:56-60) of segment i as packed points z[m] = (x[2m], x[2m+1]), m < B/2
    auto point = [&](long long base, int m) {
        const long long i0 = base + 2 * m, i1 = i0 + 1;
        if (al8 && 2 * m + 1 < B && i1 < a.len_data) return *reinterpret_cast<const float2 *>(src + i0);
        float2 z;
        z.x = (2 * m < B && i0 < a.len_data) ? src[i0] : 0.f;
        z.y = (2 * m + 1 < B && i1 < a.len_data) ? src[i1] : 0.f;
        return z;
    };
    // REG: lo[t] = z[j], hi[t] = z[j + B/4] for butterflies j = lane + 64 t < B/4;
    // else lo[u] = z[lane + 64 u]
    auto load = [&](int i, float2 (&lo)[NPL], float2 (&hi)[NPL]) {
        const long long base = (long long)i * B;
#pragma unroll
        for (int u = 0; u < NPL; ++u) {
            const int m = lane + 64 * u;
            if constexpr (REG) {
                if (m < B / 4) {
                    lo[u] = point(base, m);
                    hi[u] = point(base, m + B / 4);
                }
            } else {
                lo[u] = point(base, m);
            }
        }
    };
    const int i0 = (blockIdx.x * NW + wave) * IR_SPW;
    // a ring of IR_PF + 1 segments in registers: segment q + IR_PF is loaded
    // while segment q is transformed (the loop is unrolled, so every ring
    // index is a constant and no in-flight load is ever copied)
    constexpr int RING = IR_PF + 1;
    float2 rl[RING][NPL], rh[RING][NPL];
#pragma unroll
    for (int k = 0; k < IR_PF && k < IR_SPW; ++k)
        if (i0 + k < a.S && i0 + k < active) load(i0 + k, rl[k], rh[k]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // (the twiddle table)
#pragma unroll
    for (int q = 0; q < IR_SPW; ++q) {
        const int i = i0 + q;
        if (i >= a.S) break;
        float2 *row = a.H + c * rows + (size_t)i * B;
        if (q + IR_PF < IR_SPW && i + IR_PF < a.S && i + IR_PF < active)
            load(i + IR_PF, rl[(q + IR_PF) % RING], rh[(q + IR_PF) % RING]);  // (in flight under these FFTs)
        if (i >= active) {  // :210-212
            for (int m = lane; m < B; m += 64) row[m] = make_float2(0.f, 0.f);
            continue;
        }
        float2(&cur)[NPL] = rl[q % RING];
        if constexpr (REG) {
            wave_stage0_padded<LOG2B>(cur, rh[q % RING], bufA);
            wave_sync();
            wave_r2c_post<LOG2B, 1, TwStaged<LOG2B>, true, (FFTCONV_IR_NTST != 0)>(bufA, nullptr, TwStaged<LOG2B>{twl},
                                                                                 nullptr, row);
        } else {
#pragma unroll
            for (int u = 0; u < NPL; ++u) {
                const int m = lane + 64 * u;
                if (m < B) bufA[m] = m < B / 2 ? cur[u] : make_float2(0.f, 0.f);
            }
            for (int m = B / 2 + lane; m < B; m += 64) bufA[m] = make_float2(0.f, 0.f);
            wave_sync();
            const float2 *Z = lds_cfft<LOG2B, 64, false, true>(bufA, bufB, twl);
            for (int m = lane; m < B; m += 64) row[m] = real_post<LOG2B, 64>(Z, m, twl);
        }
        wave_sync();  // (the next segment overwrites both buffers)
    }
}

// ---------------------------------------------------------------------------
// Fft::forward / Fft::inverse as a batched API (src/fft_convolver.rs:36-49):
// realfft's even-length algorithm, the same butterflies and twiddles as the
// convolver's transforms, so an IR segment's spectrum here is bit-identical
// to the row the convolver holds for it.  Forward: N reals -> M+1 bins,
// unnormalised, DC / Nyquist imaginary parts exactly 0.  Inverse: M+1 bins ->
// N reals divided by N (:44-46); a non-zero DC / Nyquist imaginary part is
// realfft's FftError::InputValues -- flagged in status, and (like the oracle's
// restatement) the transform runs with those parts taken as 0.
// ---------------------------------------------------------------------------
template <int LOG2M, int NT, bool INV>
__global__ __launch_bounds__(NT) void fft_rows_kernel(FftArgs a) {
    constexpr int M = 1 << LOG2M;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *bufA = reinterpret_cast<float2 *>(smem);
    float2 *bufB = bufA + M;
    const int tid = threadIdx.x;
    const float *in = a.in + (size_t)blockIdx.x * a.in_stride;
    float *out = a.out + (size_t)blockIdx.x * a.out_stride;
    if constexpr (!INV) {
        for (int m = tid; m < M; m += NT) bufA[m] = make_float2(in[2 * m], in[2 * m + 1]);
        __syncthreads();
        const float2 *Z = lds_cfft<LOG2M, NT, false>(bufA, bufB, a.tw);
        for (int k = tid; k < M; k += NT) {
            const float2 v = real_post<LOG2M, NT>(Z, k, a.tw);
            if (k == 0) {  // packed (DC, Nyquist)
                out[0] = v.x;
                out[1] = 0.f;
                out[2 * M] = v.y;
                out[2 * M + 1] = 0.f;
            } else {
                out[2 * k] = v.x;
                out[2 * k + 1] = v.y;
            }
        }
    } else {
        constexpr float invN = 1.0f / (float)(2 * M);
        for (int k = tid; k < M; k += NT)
            bufA[k] = k == 0 ? make_float2(in[0], in[2 * M]) : make_float2(in[2 * k], in[2 * k + 1]);
        // FftError::InputValues: realfft still writes the transform (with the
        // imaginary parts as 0), and Fft::inverse returns through `?` (:42)
        // before its normalisation loop (:44-46) -- that row is not scaled
        const bool bad = in[1] != 0.f || in[2 * M + 1] != 0.f;
        if (tid == 0 && a.status) a.status[blockIdx.x] = bad ? 1 : 0;
        __syncthreads();
        for (int m = tid; m < M; m += NT) bufB[m] = real_pre<LOG2M, NT>(bufA, m, a.tw);
        __syncthreads();
        const float *y = reinterpret_cast<const float *>(lds_cfft<LOG2M, NT, true>(bufB, bufA, a.tw));
        const float sc = bad ? 1.0f : invN;
        for (int j = tid; j < 2 * M; j += NT) out[j] = y[j] * sc;  // (x / N: N is a power of two)
    }
}

template <int LOG2M>
static hipError_t launch_fft_t(bool inverse, const FftArgs &a, int rows, hipStream_t s) {
    constexpr int NT = LOG2M <= 6 ? 64 : 256;
    constexpr size_t lds = 2 * (size_t)(1 << LOG2M) * sizeof(float2) + 16;
    auto kern = inverse ? fft_rows_kernel<LOG2M, NT, true> : fft_rows_kernel<LOG2M, NT, false>;
    return launch_dyn(kern, dim3(rows), dim3(NT), lds, s, a);
}

// ---------------------------------------------------------------------------
// TwoStage sub-chunk (src/fft_convolver.rs:438-461): output += precalculated0
// then += precalculated (two passes, like the reference), and append the
// input to tail_input.
// ---------------------------------------------------------------------------
__global__ void twostage_accum_kernel(TwoStageAccumArgs a) {
    const size_t c = blockIdx.x;
    float *o = a.out + c * a.out_stride + a.sb;
    const float *p0 = a.p0 + c * a.T + a.pos;
    const float *p1 = a.p1 + c * a.T + a.pos;
    const float *x = a.in + c * a.in_stride + a.sb;
    float *ti = a.tail_input + c * a.T + a.fill;
    for (int j = threadIdx.x; j < a.cnt; j += blockDim.x) {
        float v = o[j];
        v += p0[j];
        v += p1[j];
        o[j] = v;
        ti[j] = x[j];
    }
}

// FFTConvolver::reset (src/fft_convolver.rs:296-306) scalar part: current = 0,
// input_buffer_fill = 0; active_seg_count is kept.
__global__ void reset_state_kernel(int4 *state, int channels) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < channels) {
        int4 s = state[c];
        state[c] = make_int4(0, s.y, 0, 0);
    }
}

template <int LOG2B>
static hipError_t launch_ir_t(const IrArgs &a, int channels, hipStream_t s) {
    if constexpr (LOG2B >= 6 && LOG2B <= 10) {
        if (!Variant::current().has(VARIANT_IRBLOCK)) {
            constexpr int NW = ir_nw<LOG2B>();
            return launch_dyn(ir_segments_wave_kernel<LOG2B>, dim3((a.S + NW * IR_SPW - 1) / (NW * IR_SPW), channels),
                              dim3(64 * NW), ir_wave_lds<LOG2B>(), s, a);
        }
    }
    constexpr size_t lds = 2 * (size_t)(1 << LOG2B) * sizeof(float2) + 16;
    return launch_dyn(ir_segments_kernel<LOG2B, kNT>, dim3(a.S, channels), dim3(kNT), lds, s, a);
}

hipError_t launch_ir_segments(int log2b, const IrArgs &a, int channels, hipStream_t s) {
    if (channels <= 0 || a.S <= 0) return hipSuccess;
    return dispatch_fused(log2b, [&](auto L) { return launch_ir_t<L()>(a, channels, s); });
}

hipError_t launch_fft_rows(int log2m, bool inverse, const FftArgs &a, int rows, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    return dispatch_fused(log2m, [&](auto L) { return launch_fft_t<L()>(inverse, a, rows, s); });
}

hipError_t launch_twostage_accum(const TwoStageAccumArgs &a, int channels, hipStream_t s) {
    if (channels <= 0 || a.cnt <= 0) return hipSuccess;
    return launch_dyn(twostage_accum_kernel, dim3(channels), dim3(a.cnt >= 256 ? 256 : 64), 0, s, a);
}

__global__ void state_flags_kernel(int4 *state, int channels, int set, int clear) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < channels) state[c].w = (state[c].w & ~clear) | set;
}

hipError_t launch_state_flags(int4 *state, int channels, int set, int clear, hipStream_t s) {
    if (channels <= 0) return hipSuccess;
    return launch_dyn(state_flags_kernel, dim3((channels + 255) / 256), dim3(256), 0, s, state, channels, set, clear);
}

hipError_t launch_reset_state(int4 *state, int channels, hipStream_t s) {
    if (channels <= 0) return hipSuccess;
    return launch_dyn(reset_state_kernel, dim3((channels + 255) / 256), dim3(256), 0, s, state, channels);
}

}  // namespace fftconv
