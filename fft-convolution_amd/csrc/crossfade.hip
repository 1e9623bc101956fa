// crossfade.hip -- CrossfadeConvolver: the stand-alone mix kernels and the
// pair step (both convolvers of a channel from one FDL stream), with their
// launchers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "launch.hpp"
#include "mix.hpp"
#include "step.hpp"

namespace fftconv {

__global__ void crossfade_mix_kernel(CrossfadeMixArgs a) {
    __shared__ float vtab[1025];
    const size_t c = blockIdx.x;
    const float *A = a.buf_a + c * a.buf_stride;
    const float *Bv = a.buf_b + c * a.buf_stride;
    float *o = a.out + c * a.out_stride;
    const bool tab = a.approaching && a.n <= 1024;
    if (tab) {
        if (threadIdx.x == 0) mix_walk(a, vtab);
        __syncthreads();
    }
    const float *vt = tab ? vtab : (a.approaching ? a.vtab : nullptr);
    for (int j = threadIdx.x; j < a.n; j += blockDim.x) o[j] = mix_sample(a, j, A[j], Bv[j], vt);
}

// the mix_value walk of a call longer than crossfade_mix_kernel's LDS table
// (n > 1024) into a device table, once (one lane), before the mix reads it
__global__ void crossfade_walk_kernel(CrossfadeMixArgs a, float *vtab) {
    if (threadIdx.x == 0) mix_walk(a, vtab);
}

// ---------------------------------------------------------------------------
// Crossfade pair step: CrossfadeConvolver::process (src/crossfade_convolver.rs
// :66-78) runs convolver_a and convolver_b on the same input block.  While
// the two ring states agree (and FLAG_XSYNC says they always have), their
// FDLs are equal row for row, so one workgroup per channel does both with
// one FDL stream (H_A, H_B, X: 24 instead of 32 B per bin-row), one forward
// transform written to both FDL rows, and the two C2Rs.  Each convolver's
// arithmetic is exactly the unpaired kernel's (same sum order): pairing never
// changes a result bit.  Any other call runs the two generic jobs in turn;
// if the states disagree the channel drops FLAG_XSYNC for good.
// B in [2, 512]; LDS: bufA | bufB | bufC | redA | redB | tw | H0a | H0b | ovA | ovB
// ---------------------------------------------------------------------------
template <int LOG2B, int NT>
struct PairGeo {
    using Gm = Geo<LOG2B, NT>;
    static constexpr int B = Gm::B;
    // ... | s_err[2] (16 B) | A's output (B floats) | mix_value walk (B + 1 floats)
    static constexpr size_t pair_bytes = 3 * 8 * (size_t)B + 2 * Gm::red_bytes + 16 * (size_t)B + 16 * (size_t)B +
                                         8 * (size_t)B + 16 + 4 * (size_t)B + 4 * ((size_t)B + 4);
    static constexpr size_t lds_bytes = pair_bytes > Gm::lds_bytes ? pair_bytes : Gm::lds_bytes;
};

template <int LOG2B, int NT, bool NTL>
__device__ __forceinline__ void pair_step(const ProcArgs &a, size_t c, int cur, int act, int flags,
                                          unsigned char *smem) {
    using Gm = Geo<LOG2B, NT>;
    constexpr int B = Gm::B, VEC = Gm::VEC, F = Gm::F, G = Gm::G, SPT = Gm::SPT;
    constexpr float invN = 1.0f / (float)(2 * B);
    using vec_t = typename VecT<VEC>::type;
    static_assert(VEC == 2 && B <= 512, "pair step: 2 <= B <= 512");
    float2 *bufA = reinterpret_cast<float2 *>(smem);
    float2 *bufB = bufA + B;
    float2 *bufC = bufB + B;
    vec_t *redA = reinterpret_cast<vec_t *>(bufC + B);
    vec_t *redB = reinterpret_cast<vec_t *>(reinterpret_cast<unsigned char *>(redA) + Gm::red_bytes);
    float2 *twl = reinterpret_cast<float2 *>(reinterpret_cast<unsigned char *>(redB) + Gm::red_bytes);
    float2 *h0[2] = {twl + 2 * B, twl + 3 * B};
    float *ovl[2] = {reinterpret_cast<float *>(twl + 4 * B), reinterpret_cast<float *>(twl + 4 * B) + B};
    int *s_err = reinterpret_cast<int *>(ovl[1] + B);  // [2]
    float *ya = reinterpret_cast<float *>(s_err + 4);   // A's output, for the fused mix
    float *vtab = ya + B;                               // mix_value walk
    const bool fuse = a.fuse_mix != 0;

    const ProcJob *Js[2] = {&a.job[0], &a.job[1]};
    const int tid = threadIdx.x;
    const size_t rows = (size_t)Js[0]->S * B;
    const float2 *Hc[2] = {Js[0]->H + c * rows, Js[1]->H + c * rows};
    const float *inc = Js[0]->in + c * Js[0]->in_stride;
    const int f0 = G > 1 ? tid % F : tid;
    const int g = G > 1 ? (F >= 64 ? __builtin_amdgcn_readfirstlane(tid / F) : tid / F) : 0;
    const bool owner = G > 1 ? tid < F : true;

    // prologue (LDS-DMA): twiddles, both H[0], the packed block, both overlaps
    dma_16b<NT>(twl, a.tw, 2 * B * (int)sizeof(float2));
    dma_16b<NT>(h0[0], Hc[0], B * (int)sizeof(float2));
    dma_16b<NT>(h0[1], Hc[1], B * (int)sizeof(float2));
    dma_f32<NT>(reinterpret_cast<float *>(bufA), inc, B);
    for (int m = B / 2 + tid; m < B; m += NT) bufA[m] = make_float2(0.f, 0.f);
    dma_f32<NT>(ovl[0], Js[0]->overlap + c * B, B);
    dma_f32<NT>(ovl[1], Js[1]->overlap + c * B, B);
    // the crossfader's mix_value walk (one lane; hides under the FDL stream)
    if (fuse && a.mix.approaching && tid == 0) mix_walk(a.mix, vtab);

    // both pre_multiplied from one FDL stream (:244-255)
    vec_t pacc[2][SPT];
    {
        AccT<VEC> accA[SPT], accB[SPT];
        mac_rows_pair<LOG2B, NT, NTL>(accA, accB, Hc[0], Hc[1], Js[0]->X + c * rows, Js[0]->S, cur, act, f0, g);
        if constexpr (G > 1) {
            redA[g * F + f0] = accA[0].get(f0);
            redB[g * F + f0] = accB[0].get(f0);
            __syncthreads();
            if (owner) {
                vec_t p = redA[f0], q = redB[f0];
#pragma unroll
                for (int r = 1; r < G; ++r) {
                    p = vadd(p, redA[r * F + f0]);
                    q = vadd(q, redB[r * F + f0]);
                }
                pacc[0][0] = p;
                pacc[1][0] = q;
            }
        } else {
#pragma unroll
            for (int s = 0; s < SPT; ++s) {
                pacc[0][s] = accA[s].get(f0 + s * NT);
                pacc[1][s] = accB[s].get(f0 + s * NT);
            }
        }
    }
    if (tid < 2) s_err[tid] = 0;
    __syncthreads();

    // one R2C (:229-241), written to both FDL rows `current`
    float2 *Z = lds_cfft<LOG2B, NT, false>(bufA, bufB, twl);
    float2 *W = Z == bufA ? bufB : bufA;
    float2 *XA = Js[0]->X + c * rows + (size_t)cur * B;
    float2 *XB = Js[1]->X + c * rows + (size_t)cur * B;
    for (int m = tid; m < B; m += NT) {
        const float2 v = real_post<LOG2B, NT>(Z, m, twl);
        bufC[m] = v;
        XA[m] = v;
        XB[m] = v;
    }
    __syncthreads();

    for (int j = 0; j < 2; ++j) {
        const ProcJob &J = *Js[j];
        // conv = pre + X (.) H[0] (:256-261), then the C2R error check
        if (owner) {
#pragma unroll
            for (int s = 0; s < SPT; ++s) {
                const int f = f0 + s * NT;
                const vec_t cv = slot_mac(pacc[j][s], reinterpret_cast<const vec_t *>(bufC)[f],
                                          reinterpret_cast<const vec_t *>(h0[j])[f], f);
                reinterpret_cast<vec_t *>(Z)[f] = cv;
                if (f == 0 && !slot0_finite(cv) &&
                    c2r_rejects(J.H + c * rows, Js[0]->X + c * rows, B, cur, act, slot0_of(pacc[j][s]),
                                slot0_of(reinterpret_cast<const vec_t *>(bufC)[f]),
                                slot0_of(reinterpret_cast<const vec_t *>(h0[j])[f])))
                    s_err[j] = 1;
            }
        }
        __syncthreads();
        float *outc = J.out + c * J.out_stride;
        if (!s_err[j]) {
            for (int m = tid; m < B; m += NT) W[m] = real_pre<LOG2B, NT>(Z, m, twl);
            __syncthreads();
            const float *y = reinterpret_cast<const float *>(lds_cfft<LOG2B, NT, true>(W, Z, twl));
            float *ovc = J.overlap + c * B;
            for (int k = tid; k < B; k += NT) {
                const float v = y[k] * invN + ovl[j][k];  // :270-274
                ovc[k] = y[B + k] * invN;                  // :283-284
                if (!fuse) {
                    outc[k] = v;
                } else if (j == 0) {
                    ya[k] = v;
                } else if (k < a.mix.n) {                  // crossfade_convolver.rs:75-77
                    a.mix.out[c * a.mix.out_stride + k] = mix_sample(a.mix, k, ya[k], v, vtab);
                }
            }
            if (tid == 0) J.state[c] = make_int4(cur > 0 ? cur - 1 : act - 1, act, 0, la_clear((flags & ~FLAG_INBUF) ^ FLAG_REV, a));
        } else {
            // output.fill(0); return (:264-267): block kept in the input buffer
            float *ibc = J.inbuf + c * B;
            for (int k = tid; k < B; k += NT) {
                if (!fuse) outc[k] = 0.f;
                else if (j == 0) ya[k] = 0.f;
                else if (k < a.mix.n) a.mix.out[c * a.mix.out_stride + k] = mix_sample(a.mix, k, ya[k], 0.f, vtab);
                ibc[k] = inc[k];
            }
            if (owner) {
#pragma unroll
                for (int s = 0; s < SPT; ++s) reinterpret_cast<vec_t *>(J.pre + c * B)[f0 + s * NT] = pacc[j][s];
            }
            if (tid == 0) J.state[c] = make_int4(cur, act, 0, la_clear(flags | FLAG_INBUF, a));
        }
        __syncthreads();  // Z / W are reused by the next convolver
    }
}

// the generic body for both jobs in turn, out of line: the rare fallback
// keeps its registers out of the pair step's allocation
template <int LOG2B, int NT, bool NTL>
__device__ __attribute__((noinline)) void pair_fallback(const ProcArgs &a, size_t c, int4 sa, int4 sb,
                                                        unsigned char *smem) {
    process_job<LOG2B, NT, false, NTL>(a, a.job[0], c, sa, smem);
    __syncthreads();
    process_job<LOG2B, NT, false, NTL>(a, a.job[1], c, sb, smem);
    if (a.fuse_mix) {  // the jobs wrote buf_a / buf_b (this workgroup's own stores)
        __threadfence_block();
        __syncthreads();
        const float *A = a.mix.buf_a + c * a.mix.buf_stride, *Bv = a.mix.buf_b + c * a.mix.buf_stride;
        for (int k = threadIdx.x; k < a.mix.n; k += NT)
            a.mix.out[c * a.mix.out_stride + k] = mix_sample(a.mix, k, A[k], Bv[k], nullptr);
    }
}

// (2 waves/SIMD suffice: C workgroups of 3 streams x 8 rows x 16 B per lane
// in flight; the rarely-taken generic fallback then needs no spills)
template <int LOG2B, int NT, bool NTL>
__global__ __launch_bounds__(NT, 2) void upols_pair_kernel(ProcArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const size_t c = blockIdx.x;
    int4 sa = a.job[0].state[c], sb = a.job[1].state[c];
    constexpr int KEY = FLAG_INBUF | FLAG_REV | FLAG_PRE;
    const bool same = sa.x == sb.x && sa.y == sb.y && sa.z == sb.z && ((sa.w ^ sb.w) & KEY) == 0;
    if (same && (sa.w & sb.w & FLAG_XSYNC) && sa.y > 0 && sa.z == 0 && a.job[0].n == (1 << LOG2B) &&
        !(sa.w & (FLAG_INBUF | FLAG_PRE)) && sa.x < sa.y) {
        pair_step<LOG2B, NT, NTL>(a, c, sa.x, sa.y, sa.w, smem);
        return;
    }
    if (!same) {  // the rings have diverged (a C2R error in one of them): never pair again
        sa.w &= ~FLAG_XSYNC;
        sb.w &= ~FLAG_XSYNC;
    }
    pair_fallback<LOG2B, NT, NTL>(a, c, sa, sb, smem);
}

hipError_t launch_crossfade_mix(const CrossfadeMixArgs &a, int channels, hipStream_t s) {
    if (channels <= 0 || a.n <= 0) return hipSuccess;
    return launch_dyn(crossfade_mix_kernel, dim3(channels), dim3(256), 0, s, a);
}

hipError_t launch_crossfade_walk(const CrossfadeMixArgs &a, float *vtab, hipStream_t s) {
    if (a.n <= 0 || !a.approaching) return hipSuccess;
    return launch_dyn(crossfade_walk_kernel, dim3(1), dim3(64), 0, s, a, vtab);
}

template <int LOG2B>
static hipError_t launch_pair_t(const ProcArgs &a, int channels, hipStream_t s) {
    if constexpr (LOG2B < 1 || LOG2B > 9) {
        return hipErrorNotSupported;
    } else {
        constexpr int PNT = proc_nt(LOG2B);
        using PG = PairGeo<LOG2B, PNT>;
        const int var = pick_variant(Variant::current(), a, channels, LOG2B);
        if (var & (VARIANT_ZIGZAG | VARIANT_NOPAIR)) return hipErrorNotSupported;  // the pair scan is the plain order only
        ProcArgs args = a;
        args.pipe = 0;
        args.lag = 0;
        auto kern = (var & VARIANT_NT) ? upols_pair_kernel<LOG2B, PNT, true> : upols_pair_kernel<LOG2B, PNT, false>;
        return launch_dyn(kern, dim3(channels), dim3(PNT), PG::lds_bytes, s, args);
    }
}

bool pair_supported(int log2b, int S) {
    // long FDLs only: there the step is HBM-bound and the shared stream saves
    // a quarter of the bytes; short ones are latency-bound and run better as
    // two pipelined workgroups
    return log2b >= 1 && log2b <= 9 && ((long long)S << log2b) > 16384 &&
           !Variant::current().has(VARIANT_ZIGZAG | VARIANT_NOPAIR);
}

hipError_t launch_process_pair(int log2b, const ProcArgs &a, int channels, hipStream_t s) {
    if (channels <= 0) return hipSuccess;
    if (a.njobs != 2) return hipErrorInvalidValue;
    return dispatch_fused(log2b, [&](auto L) { return launch_pair_t<L()>(a, channels, s); });
}

}  // namespace fftconv
