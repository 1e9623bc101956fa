// mix.hpp -- device helpers of the crossfade mix, shared by the stand-alone
// mix kernels (crossfade.hip) and the lookahead launches that fuse the mix
// (la.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace fftconv {

// ---------------------------------------------------------------------------
// Crossfade mix (src/crossfade_convolver.rs:75-77 + Crossfader::mix :242-278
// + RaisedCosineMixer :160-169), all channels in lockstep.  mix_value is
// walked by the same sequential f32 additions the reference performs (once
// per workgroup into LDS, or per sample for calls longer than 1024), so the
// gains are bit-identical to a serial walk.
// ---------------------------------------------------------------------------
// Crossfader::mix for sample j of the call.  vtab (if given) holds the
// sequential mix_value walk: vtab[k] = mix_value0 + step + ... (k adds).
// RaisedCosineMixer (:160-169): gain g1 = cos^2(pi/2 * v) of A, 1 - g1 of B
__device__ __forceinline__ float mix_gain(float v) {
    const float PI_HALF = 3.14159265358979323846f * 0.5f;
    const float rad = __fmul_rn(PI_HALF, v);
    const float cs = cosf(rad);
    return __fmul_rn(cs, cs);
}
__device__ __forceinline__ float mix_apply(float va, float vb, float g1) {
    const float g2 = __fsub_rn(1.0f, g1);
    return __fadd_rn(__fmul_rn(va, g1), __fmul_rn(vb, g2));
}

__device__ __forceinline__ float mix_sample(const CrossfadeMixArgs &a, int j, float va, float vb,
                                            const float *vtab) {
    if (!a.approaching) return a.target == 0 ? va : vb;
    const long long cj = a.counter0 + j + 1;
    if (cj <= 0) return a.target == 0 ? vb : va;                   // hold the previous target
    if (a.fading >= 1 && cj >= a.fading) return a.target == 0 ? va : vb;  // reached (snap)
    const long long inc = cj - (a.counter0 > 0 ? a.counter0 : 0);
    float v;
    if (vtab) {
        v = vtab[inc];
    } else {
        v = a.mix_value0;
        for (long long q = 0; q < inc; ++q) v = __fadd_rn(v, a.step);
    }
    return mix_apply(va, vb, mix_gain(v));
}

// Crossfader::mix for sample j as a selector word: MIX_SEL_A / MIX_SEL_B take
// that convolver's sample as is (hold, snap, not fading), anything else is the
// gain g1 in [0, 1] of the blend.  mix_select(va, vb, mix_selector(...)) is
// bit-identical to mix_sample.
constexpr float MIX_SEL_A = 2.0f, MIX_SEL_B = 3.0f;
__device__ __forceinline__ float mix_selector(const CrossfadeMixArgs &a, int j, const float *vtab) {
    const float sa = a.target == 0 ? MIX_SEL_A : MIX_SEL_B, sb = a.target == 0 ? MIX_SEL_B : MIX_SEL_A;
    if (!a.approaching) return sa;
    const long long cj = a.counter0 + j + 1;
    if (cj <= 0) return sb;                            // hold the previous target
    if (a.fading >= 1 && cj >= a.fading) return sa;    // reached (snap)
    return mix_gain(vtab[cj - (a.counter0 > 0 ? a.counter0 : 0)]);
}
__device__ __forceinline__ float mix_select(float va, float vb, float sel) {
    return sel == MIX_SEL_A ? va : (sel == MIX_SEL_B ? vb : mix_apply(va, vb, sel));
}

// The mix_value walk of one call into LDS: vtab[k] = v0 + step + ... + step
// (k sequential f32 additions, n + 1 entries), one thread, bit-identical to
// the reference's per-sample `mix_value += step` (:259).  The additions are a
// dependent chain on one lane; unrolled by 8 with the stores batched after
// them, the loop is little more than that chain (the rolled loop -- an
// address, a store and the loop test per add -- took ~9 us for 512 samples in
// the cfg5 step workgroups, more than their whole transform chain, r3).
__device__ __forceinline__ void mix_walk_lane(float *vtab, float v, float step, int n) {
    vtab[0] = v;
    int k = 1;
    for (; k + 7 <= n; k += 8) {
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            v = __fadd_rn(v, step);
            t[u] = v;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) vtab[k + u] = t[u];
    }
    for (; k <= n; ++k) {
        v = __fadd_rn(v, step);
        vtab[k] = v;
    }
}
__device__ __forceinline__ void mix_walk(const CrossfadeMixArgs &a, float *vtab) {
    mix_walk_lane(vtab, a.mix_value0, a.step, a.n);
}

}  // namespace fftconv
