// packed.hpp -- arithmetic and loads on packed spectrum rows: the reference's
// complex_multiply_accumulate (src/fft_convolver.rs:62-74) in the forms the
// kernels use.  Every path (uniform, lookahead, tail0, matrix, long-block)
// takes them from here, so they agree bit for bit.
//
// A packed row is B complex = 8B bytes; slot 0 holds (DC, Nyquist), two real
// bins multiplied component-wise.  Rows are read with 16-byte loads (float4 =
// 2 bins per lane-slot).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace fftconv {

template <int VEC> struct VecT;
template <> struct VecT<2> { using type = float4; };
template <> struct VecT<1> { using type = float2; };

// Complex multiply-accumulate over one lane-slot, complex_multiply_accumulate
// (src/fft_convolver.rs:62-74) for 2 bins.  dc/ny carry the products of the
// packed real bins so that slot 0 can be resolved as (DC, Nyquist).
struct Acc2 {
    float4 a;
    float dc, ny;
    __device__ __forceinline__ void zero() { a = make_float4(0.f, 0.f, 0.f, 0.f); dc = ny = 0.f; }
    __device__ __forceinline__ void mac(float4 h, float4 x) {
        a.x = fmaf(-h.y, x.y, fmaf(h.x, x.x, a.x));
        a.y = fmaf(h.y, x.x, fmaf(h.x, x.y, a.y));
        a.z = fmaf(-h.w, x.w, fmaf(h.z, x.z, a.z));
        a.w = fmaf(h.w, x.z, fmaf(h.z, x.w, a.w));
        dc = fmaf(h.x, x.x, dc);
        ny = fmaf(h.y, x.y, ny);
    }
    __device__ __forceinline__ float4 get(int slot) const {
        return slot == 0 ? make_float4(dc, ny, a.z, a.w) : a;
    }
};
struct Acc1 {  // B == 1: the only bin pair is (DC, Nyquist)
    float2 a;
    __device__ __forceinline__ void zero() { a = make_float2(0.f, 0.f); }
    __device__ __forceinline__ void mac(float2 h, float2 x) { a.x = fmaf(h.x, x.x, a.x); a.y = fmaf(h.y, x.y, a.y); }
    __device__ __forceinline__ float2 get(int) const { return a; }
};
template <int VEC> using AccT = std::conditional_t<VEC == 2, Acc2, Acc1>;

__device__ __forceinline__ float4 vadd(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float2 vadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
// streaming accesses (nontemporal): rows used once, which must not evict the
// working set of latency-bound launches running beside them (a two-stage head)
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ntld4(const float4 *p) {
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void ntst4(float4 *p, float4 v) {
    const f32x4 w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<f32x4 *>(p));
}

// conv = pre + x (.) h for one slot, packed-aware (slot 0 bin 0 is (DC, Nyquist)).
__device__ __forceinline__ float4 slot_mac(float4 pre, float4 x, float4 h, int slot) {
    float4 r;
    if (slot == 0) {
        r.x = fmaf(x.x, h.x, pre.x);
        r.y = fmaf(x.y, h.y, pre.y);
    } else {
        r.x = fmaf(-x.y, h.y, fmaf(x.x, h.x, pre.x));
        r.y = fmaf(x.y, h.x, fmaf(x.x, h.y, pre.y));
    }
    r.z = fmaf(-x.w, h.w, fmaf(x.z, h.z, pre.z));
    r.w = fmaf(x.w, h.z, fmaf(x.z, h.w, pre.w));
    return r;
}
__device__ __forceinline__ float2 slot_mac(float2 pre, float2 x, float2 h, int) {
    return make_float2(fmaf(x.x, h.x, pre.x), fmaf(x.y, h.y, pre.y));
}
__device__ __forceinline__ bool slot0_finite(float4 v) { return isfinite(v.x) && isfinite(v.y); }
__device__ __forceinline__ bool slot0_finite(float2 v) { return isfinite(v.x) && isfinite(v.y); }
__device__ __forceinline__ float2 slot0_of(float4 v) { return make_float2(v.x, v.y); }
__device__ __forceinline__ float2 slot0_of(float2 v) { return v; }
template <bool NTL>  // nontemporal or plain
__device__ __forceinline__ float4 ld4(const float4 *p) {
    if constexpr (NTL) {
        return ntld4(p);
    } else {
        return *p;
    }
}

// Packed-FMA form (v_pk_fma_f32) of the same sums: the lookahead anchors' and
// the deferred tail0's accumulator.
typedef float f2v __attribute__((ext_vector_type(2)));

// Per-row operands of one float4 slot (2 bins).  Bin 0 of slot 0 is the packed
// (DC, Nyquist) pair, multiplied component-wise; operand selection makes the
// same two packed FMAs do both (q0 = 0 adds a signed zero there).
struct LaH {
    f2v p0, q0, p1, q1;
};
__device__ __forceinline__ LaH la_ops(float4 h, bool z0) {
    LaH o;
    o.p0 = f2v{h.x, z0 ? h.y : h.x};
    o.q0 = z0 ? f2v{0.f, 0.f} : f2v{-h.y, h.y};
    o.p1 = f2v{h.z, h.z};
    o.q1 = f2v{-h.w, h.w};
    return o;
}
// complex_multiply_accumulate (src/fft_convolver.rs:62-74) over 2 bins:
// re = fma(-h.im, x.im, fma(h.re, x.re, re)), im = fma(h.im, x.re, fma(h.re, x.im, im))
struct LaAcc {
    f2v a01, a23;
    __device__ __forceinline__ void zero() { a01 = f2v{0.f, 0.f}; a23 = f2v{0.f, 0.f}; }
    __device__ __forceinline__ void mac(const LaH &h, float4 x) {
        a01 = __builtin_elementwise_fma(h.p0, f2v{x.x, x.y}, a01);
        a01 = __builtin_elementwise_fma(h.q0, f2v{x.y, x.x}, a01);
        a23 = __builtin_elementwise_fma(h.p1, f2v{x.z, x.w}, a23);
        a23 = __builtin_elementwise_fma(h.q1, f2v{x.w, x.z}, a23);
    }
    __device__ __forceinline__ float4 get() const { return make_float4(a01.x, a01.y, a23.x, a23.y); }
};

}  // namespace fftconv
