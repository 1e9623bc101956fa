// matrix_patch.hip -- gfx950 kernel of update_pairs: one launch
// patches the spectra H of one matrix for a listed set of (output, input)
// pairs, roles by block index.
//
//   [0, n_tr * gx)       gathered IR transform: workgroup (n, x) transforms
//                        segments of pair tr[n] from its response row -- the
//                        list position n (a direct update) or the pair index
//                        (rows kept in the crossfader's stored response) --
//                        into H[pair]: the bits launch_ir_segments writes for
//                        that pair.  gx = S (one segment per workgroup) or
//                        ceil(S / (NW * SPW)) (one segment per wave, 64 <= B <=
//                        1024), chosen by VARIANT_IRBLOCK like launch_ir_t.
//   then n_cp * cpb      gathered row copy: workgroup (n, x) copies 16-byte
//                        slots [x * NT * CP_U, ...) of the S * B float2 of pair
//                        cp[n] from Hsrc to H, all S rows.
//
// A pair is in at most one of the two lists, so no two workgroups write the
// same bytes; stream order and the kernel boundary are the only ordering.
//
// The wave form restates ir_segments_wave_kernel (transform.hip) on the
// building blocks of fft_lds.hpp with the pair and the source row gathered:
// same geometry (NW waves, SPW segments per wave, one segment loaded ahead),
// same butterflies and twiddles in the same order.  Change them together.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_lds.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "matrix.hpp"
#include "packed.hpp"
#include "step.hpp"

namespace fftconv {
namespace {

constexpr int PATCH_SPW = 2;  // segments per wave (transform.hip: IR_SPW)
constexpr int PATCH_PF = 1;   // segments loaded ahead (transform.hip: IR_PF)
constexpr int CP_U = 8;       // 16-byte slots in flight per thread of the copy
template <int LOG2B>
constexpr int patch_nw() { return LOG2B >= 7 ? 8 : 4; }  // (transform.hip: ir_nw)

template <int LOG2B, bool WAVE>
struct PGeo {
    static constexpr int B = 1 << LOG2B;
    static constexpr int NW = patch_nw<LOG2B>();
    static constexpr int NT = WAVE ? 64 * NW : matrix_nt(LOG2B);
    static constexpr size_t lds = WAVE ? (size_t)(2 + NW * (LOG2B >= 7 ? 1 : 2)) * B * sizeof(float2)
                                       : 2 * (size_t)B * sizeof(float2) + 16;
    static constexpr int seg_per_wg = WAVE ? NW * PATCH_SPW : 1;
};

// response row of list entry n
__device__ __forceinline__ const float *patch_src(const MatrixPatchArgs &a, int n, uint32_t pair) {
    const long long r = a.by_pair ? (long long)pair : (long long)a.row0 + n;
    return a.src + r * a.src_stride;
}

// ir_segments_kernel's transform of segment i of pair tr[n]
template <int LOG2B, int NT>
__device__ __forceinline__ void patch_ir_block(const MatrixPatchArgs &a, int n, int i, unsigned char *smem) {
    constexpr int B = 1 << LOG2B;
    float2 *bufA = reinterpret_cast<float2 *>(smem);
    float2 *bufB = bufA + B;
    const int tid = threadIdx.x;
    const uint32_t pair = a.tr[n];
    if (pair >= (uint32_t)a.pairs) return;  // (the host validated the list)
    float2 *row = a.H + ((size_t)pair * a.S + i) * B;
    const long long active = (a.len_active + B - 1) / B;
    if (i >= active) {
        for (int j = tid; j < B; j += NT) row[j] = make_float2(0.f, 0.f);
        return;
    }
    const float *src = patch_src(a, n, pair);
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

// ir_segments_wave_kernel's workgroup x of pair tr[n]
template <int LOG2B>
__device__ __forceinline__ void patch_ir_wave(const MatrixPatchArgs &a, int n, int x, unsigned char *smem) {
    constexpr int B = 1 << LOG2B;
    constexpr bool REG = LOG2B >= 7;  // register stage 0 / __shfl last stage
    constexpr int NW = patch_nw<LOG2B>(), NT = 64 * NW;
    constexpr int NPL = REG ? stage0_per_lane<LOG2B>() : (B / 2 + 63) / 64;
    float2 *twl = reinterpret_cast<float2 *>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float2 *bufA = twl + 2 * B + (size_t)wave * (REG ? 1 : 2) * B;
    float2 *bufB = bufA + B;
    const uint32_t pair = a.tr[n];
    if (pair >= (uint32_t)a.pairs) return;  // (uniform over the workgroup; the host validated the list)
    const size_t rows = (size_t)a.S * B;
    const long long active = (a.len_active + B - 1) / B;
    if constexpr (REG) tws_build<LOG2B, NT>(twl, a.tw, tid);
    else dma_16b<NT>(twl, a.tw, 2 * B * (int)sizeof(float2));
    const float *src = patch_src(a, n, pair);
    const bool al8 = ((uintptr_t)src & 7) == 0;
    auto point = [&](long long base, int m) {
        const long long i0 = base + 2 * m, i1 = i0 + 1;
        if (al8 && 2 * m + 1 < B && i1 < a.len_data) return *reinterpret_cast<const float2 *>(src + i0);
        float2 z;
        z.x = (2 * m < B && i0 < a.len_data) ? src[i0] : 0.f;
        z.y = (2 * m + 1 < B && i1 < a.len_data) ? src[i1] : 0.f;
        return z;
    };
    auto load = [&](int i, float2(&lo)[NPL], float2(&hi)[NPL]) {
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
    const int i0 = (x * NW + wave) * PATCH_SPW;
    constexpr int RING = PATCH_PF + 1;
    float2 rl[RING][NPL], rh[RING][NPL];
#pragma unroll
    for (int k = 0; k < PATCH_PF && k < PATCH_SPW; ++k)
        if (i0 + k < a.S && i0 + k < active) load(i0 + k, rl[k], rh[k]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // (the twiddle table)
#pragma unroll
    for (int q = 0; q < PATCH_SPW; ++q) {
        const int i = i0 + q;
        if (i >= a.S) break;
        float2 *row = a.H + (size_t)pair * rows + (size_t)i * B;
        if (q + PATCH_PF < PATCH_SPW && i + PATCH_PF < a.S && i + PATCH_PF < active)
            load(i + PATCH_PF, rl[(q + PATCH_PF) % RING], rh[(q + PATCH_PF) % RING]);
        if (i >= active) {
            for (int m = lane; m < B; m += 64) row[m] = make_float2(0.f, 0.f);
            continue;
        }
        float2(&cur)[NPL] = rl[q % RING];
        if constexpr (REG) {
            wave_stage0_padded<LOG2B>(cur, rh[q % RING], bufA);
            wave_sync();
            wave_r2c_post<LOG2B, 1, TwStaged<LOG2B>, true, true>(bufA, nullptr, TwStaged<LOG2B>{twl}, nullptr, row);
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

// slots [x * NT * CP_U, (x + 1) * NT * CP_U) of pair cp[n], Hsrc -> H
template <int LOG2B, int NT>
__device__ __forceinline__ void patch_copy(const MatrixPatchArgs &a, int n, int x) {
    constexpr int F = 1 << (LOG2B - 1);  // 16-byte slots per row
    const uint32_t pair = a.cp[n];
    if (pair >= (uint32_t)a.pairs) return;
    const size_t slots = (size_t)a.S * F;
    const float4 *s4 = reinterpret_cast<const float4 *>(a.Hsrc) + (size_t)pair * slots;
    float4 *d4 = reinterpret_cast<float4 *>(a.H) + (size_t)pair * slots;
    const size_t at = (size_t)x * (NT * CP_U) + threadIdx.x;
    float4 v[CP_U];
    if (a.nt_cp) {
#pragma unroll
        for (int u = 0; u < CP_U; ++u)
            if (at + (size_t)u * NT < slots) v[u] = ld4<true>(s4 + at + (size_t)u * NT);
    } else {
#pragma unroll
        for (int u = 0; u < CP_U; ++u)
            if (at + (size_t)u * NT < slots) v[u] = ld4<false>(s4 + at + (size_t)u * NT);
    }
#pragma unroll
    for (int u = 0; u < CP_U; ++u)
        if (at + (size_t)u * NT < slots) d4[at + (size_t)u * NT] = v[u];
}

template <int LOG2B, bool WAVE>
__global__ __launch_bounds__((PGeo<LOG2B, WAVE>::NT)) void matrix_patch_kernel(MatrixPatchArgs a) {
    using Pg = PGeo<LOG2B, WAVE>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x;
    const int tr_blocks = a.n_tr * a.gx;
    if (b < tr_blocks) {
        if constexpr (WAVE) patch_ir_wave<LOG2B>(a, b / a.gx, b % a.gx, smem);
        else patch_ir_block<LOG2B, Pg::NT>(a, b / a.gx, b % a.gx, smem);
        return;
    }
    const int c = b - tr_blocks;
    patch_copy<LOG2B, Pg::NT>(a, c / a.cpb, c % a.cpb);
}

template <int LOG2B, bool WAVE>
hipError_t launch_patch_t(MatrixPatchArgs a, hipStream_t s) {
    using Pg = PGeo<LOG2B, WAVE>;
    constexpr size_t per_wg = (size_t)Pg::NT * CP_U;
    a.gx = (a.S + Pg::seg_per_wg - 1) / Pg::seg_per_wg;
    const size_t slots = (size_t)a.S << (LOG2B - 1);
    a.cpb = (int)((slots + per_wg - 1) / per_wg);
    const long long grid = (long long)a.n_tr * a.gx + (long long)a.n_cp * a.cpb;
    if (grid > (long long)INT32_MAX) return hipErrorInvalidValue;
    return launch_dyn(matrix_patch_kernel<LOG2B, WAVE>, dim3((unsigned)grid), dim3(Pg::NT), Pg::lds, s, a);
}

template <int LOG2B>
hipError_t launch_patch_form(const MatrixPatchArgs &a, hipStream_t s) {
    if constexpr (LOG2B >= 6 && LOG2B <= 10) {
        if (!Variant::current().has(VARIANT_IRBLOCK)) return launch_patch_t<LOG2B, true>(a, s);
    }
    return launch_patch_t<LOG2B, false>(a, s);
}

}  // namespace

hipError_t launch_matrix_patch(int log2b, const MatrixPatchArgs &a, hipStream_t s) {
    if (a.n_tr < 0 || a.n_cp < 0 || a.S < 0 || a.pairs <= 0 || a.row0 < 0) return hipErrorInvalidValue;
    if (a.n_tr > kMatrixPatchChunk || a.n_cp > kMatrixPatchChunk) return hipErrorInvalidValue;
    if ((a.n_tr > 0 && (!a.tr || !a.H || (a.len_data > 0 && !a.src))) || (a.n_cp > 0 && (!a.cp || !a.H || !a.Hsrc)))
        return hipErrorInvalidValue;
    if (a.len_data < 0 || a.len_active < a.len_data) return hipErrorInvalidValue;
    if (a.S == 0 || a.n_tr + a.n_cp == 0) return hipSuccess;
    return dispatch_log2<5, kMaxLog2Fused>(log2b, hipErrorInvalidValue,
                                           [&](auto L) { return launch_patch_form<L()>(a, s); });
}

}  // namespace fftconv
