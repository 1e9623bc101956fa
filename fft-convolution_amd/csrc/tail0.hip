// tail0.hip -- the two-stage convolver's tail0 deferred to the end of its
// period: the five flush kernels, the fused kernel of B = 64, and their
// launcher.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "launch.hpp"
#include "step.hpp"

namespace fftconv {

// ---------------------------------------------------------------------------
// Two-stage tail0 deferred to the end of its period (Tail0Args, kernels.hpp).
// TwoStageFFTConvolver::process runs tail_convolver0 on every head block
// (src/fft_convolver.rs:464-472), but tail_output0 is first read after the
// period's swap (:473-475).  So the period's blocks are convolved together:
// one pass over tail0's IR rows and FDL serves all of them, instead of one
// pass per block (cfg3: 64 passes of 64 rows per period).  The state
// (FDL, overlap, current) is committed exactly as the per-block calls leave
// it.
// ---------------------------------------------------------------------------
// (1) copy_and_pad + Fft::forward (:229-241) of pending block k of channel c
// -- the step's own transform -- into xs[c][k]
template <int LOG2B>
__global__ __launch_bounds__(64) void tail0_r2c_kernel(Tail0Args t) {
    constexpr int B = 1 << LOG2B;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *bufA = reinterpret_cast<float2 *>(smem), *bufB = bufA + B, *twl = bufB + B;
    const ProcJob &J = t.pa.job[0];
    const size_t c = blockIdx.x;
    // grid.y: every pending block; blocks [0, k0) have their spectra from the
    // head's run unless the run missed some of this channel's (t.miss)
    const int k = (int)blockIdx.y, lane = threadIdx.x;
    if (k < t.k0 && !t.miss[c]) return;
    dma_f32<64>(reinterpret_cast<float *>(bufA), J.in + c * J.in_stride + (size_t)k * B, B);  // packed z[0..B/2)
    for (int m = B / 2 + lane; m < B; m += 64) bufA[m] = make_float2(0.f, 0.f);              // the padding half
    dma_16b<64>(twl, t.pa.tw, 2 * B * (int)sizeof(float2));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wave_sync();
    float2 *Z = lds_cfft<LOG2B, 64, false, true>(bufA, bufB, twl);
    float2 *xr = t.xs + ((size_t)c * t.nmax + k) * B;
    for (int m = lane; m < B; m += 64) xr[m] = real_post<LOG2B, 64>(Z, m, twl);
    if (k == 0) {  // the overlap before the period's blocks, for (3) (whose tiles overwrite it; k0 = 0)
        for (int j = lane; j < B; j += 64) t.ov0[c * B + j] = J.overlap[c * B + j];
    }
}

// (2) conv_k = sum_{i=1}^{act-1} H[i] (.) X_{k-i} + H[0] (.) X_k (:244-261,
// rows in the reference's order) for every pending block k, one slot chunk
// of FC float4 per workgroup.  X_m is pending block m (m >= 0) or, for m < 0,
// the FDL row (cur0 - m) % act of the previous period (untouched so far).
// The chunk's IR rows and every X row it meets are staged in LDS once; a
// thread owns one slot and J consecutive blocks and walks the rows with the
// X values in a register ring (one H and one X read per row for J MACs).
constexpr int T0_J = 8, T0_FC = 32;
template <int LOG2B>
__host__ __device__ constexpr size_t tail0_mac_lds(int act, int n) {
    return (size_t)(2 * act + 1 + n + T0_J) * T0_FC * 16;  // (+ zero rows: H[act], X[-1], X[nq..nq+J))
}
template <int LOG2B>
__global__ __launch_bounds__(256) void tail0_mac_kernel(Tail0Args t) {
    constexpr int B = 1 << LOG2B, F = B / 2, FC = F < T0_FC ? F : T0_FC, J = T0_J, RS = J + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const ProcJob &J0 = t.pa.job[0];
    const size_t c = blockIdx.x;
    const int fc0 = blockIdx.y * FC;
    const int tid = threadIdx.x, fl = tid % FC, g = tid / FC;
    const int4 st = J0.state[c];
    const int cur0 = st.x, act = st.y, n = t.n;
    if (t.k0 > 0 && blockIdx.y == 0) {
        // the overlap before the period's blocks, for (3) (tail0_r2c copies it
        // at block 0; with k0 > 0 the head's run made block 0's spectrum)
        for (int j = tid; j < B; j += 256) t.ov0[c * B + j] = J0.overlap[c * B + j];
    }
    if (act != t.act) {  // (not a geometry the LDS was sized for: the replay path runs it)
        if (tid == 0) t.err[c] = 1;
        return;
    }
    const size_t rows = (size_t)J0.S * B;
    const float4 *H = reinterpret_cast<const float4 *>(J0.H + c * rows) + fc0;
    const float4 *X = reinterpret_cast<const float4 *>(J0.X + c * rows) + fc0;
    const float4 *xs = reinterpret_cast<const float4 *>(t.xs + (size_t)c * t.nmax * B) + fc0;
    // LDS: H rows [0, act) and a zero row; then X rows q = m + act - 1 in
    // [-1, nq + J) (q = -1 and q >= nq zero), so the walk reads unguarded
    const int nq = act - 1 + n;
    float4 *Hs = reinterpret_cast<float4 *>(smem);  // [act + 1][FC]
    float4 *Xs = Hs + (size_t)(act + 2) * FC;        // Xs[q * FC], q >= -1
    for (int idx = tid; idx < FC; idx += 256) Hs[(size_t)act * FC + idx] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int idx = tid; idx < (J + 1) * FC; idx += 256) {
        const int q = idx < FC ? -1 : nq + idx / FC - 1;
        Xs[(size_t)q * FC + idx % FC] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // LDS-DMA of every row chunk (no VGPRs, all in flight): a wave copies
    // two rows per instruction, lanes 0..31 the first, 32..63 the second
    static_assert(FC == 32, "a row chunk is half a wave of 16-byte lanes");
    {
        const int wave = tid >> 6, lane = tid & 63, half = lane >> 5, f = lane & 31;
        for (int r2 = wave * 2; r2 < act; r2 += 8) {  // IR rows
            if (r2 + half < act)
                __builtin_amdgcn_global_load_lds((gptr_t)(H + (size_t)(r2 + half) * F + f),
                                                 (lptr_t)(Hs + (size_t)r2 * FC), 16, 0, 0);
        }
        for (int r2 = wave * 2; r2 < nq; r2 += 8) {  // X rows
            const int q = r2 + half;
            const float4 *src;
            if (q < act - 1) {
                int r = cur0 + act - 1 - q;
                if (r >= act) r -= act;
                src = X + (size_t)r * F;
            } else {
                src = xs + (size_t)(q - (act - 1)) * F;
            }
            if (q < nq)
                __builtin_amdgcn_global_load_lds((gptr_t)(src + f), (lptr_t)(Xs + (size_t)r2 * FC), 16, 0, 0);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int kb0 = g * J;
    if (kb0 >= n) return;
    auto xq = [&](int q) { return Xs[q * FC + fl]; };  // (q in [-1, nq + J): zero rows at the ends)
    LaAcc acc[J];  // (packed FMAs, packed.hpp)
#pragma unroll
    for (int j = 0; j < J; ++j) acc[j].zero();
    const bool z0 = fc0 + fl == 0;
    // load e of the walk is X at q = Q1 + J - 1 - e; row i = s + 1 of step s
    // meets, for block kb0 + j, load e = s + J - 1 - j
    const int Q1 = kb0 + act - 2;
    float4 xr[RS];
#pragma unroll
    for (int e = 0; e < J; ++e) xr[e] = xq(Q1 + J - 1 - e);
    float4 hn = Hs[(size_t)min(1, act) * FC + fl];
    const int ns = act - 1;
    for (int s0 = 0; s0 < ns; s0 += RS) {
#pragma unroll
        for (int u = 0; u < RS; ++u) {
            const int sidx = s0 + u;
            if (sidx >= ns) break;
            const float4 h = hn;
            xr[(u + J) % RS] = xq(Q1 - 1 - sidx);
            hn = Hs[(size_t)min(sidx + 2, act) * FC + fl];  // (row act is zero)
            const LaH ho = la_ops(h, z0);
#pragma unroll
            for (int j = 0; j < J; ++j) acc[j].mac(ho, xr[(u + J - 1 - j) % RS]);
        }
    }
    const float4 h0 = Hs[fl];
    const int f = fc0 + fl;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int k = kb0 + j;
        if (k < n) {
            const float4 cv = slot_mac(acc[j].get(), Xs[(size_t)(k + act - 1) * FC + fl], h0, f);
            reinterpret_cast<float4 *>(t.cv + ((size_t)c * t.nmax + k) * B)[f] = cv;
        }
    }
}

// (2b) the C2R of conv_k (:264, the 1/N applied by (3)), one wave per block;
// realfft's C2R error (a non-finite DC / Nyquist bin, :264-267) flags the
// channel for (4)
template <int LOG2B>
__global__ __launch_bounds__(64) void tail0_c2r_kernel(Tail0Args t) {
    constexpr int B = 1 << LOG2B;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *Z = reinterpret_cast<float2 *>(smem), *q = Z + B, *twl = q + B;
    const size_t c = blockIdx.x;
    const int k = blockIdx.y, lane = threadIdx.x;
    const float2 *cr = t.cv + ((size_t)c * t.nmax + k) * B;
    dma_16b<64>(Z, cr, B * (int)sizeof(float2));
    dma_16b<64>(twl, t.pa.tw, 2 * B * (int)sizeof(float2));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wave_sync();
    if (lane == 0 && !(isfinite(Z[0].x) && isfinite(Z[0].y))) t.err[c] = 1;
    for (int m = lane; m < B; m += 64) q[m] = real_pre<LOG2B, 64>(Z, m, twl);
    wave_sync();
    const float *y = reinterpret_cast<const float *>(lds_cfft<LOG2B, 64, true, true>(q, Z, twl));
    float *yr = t.ys + ((size_t)c * t.nmax + k) * 2 * B;
    for (int j = lane; j < 2 * B; j += 64) yr[j] = y[j];
}

// (3) overlap-add (:270-274) over a tile of pending blocks, the overlap
// save (:283-284) by the last tile, and the FDL rows (:229-241; block k at
// (cur0 - k) % act, the last act blocks stay) -- channels without a C2R error
template <int LOG2B>
__global__ __launch_bounds__(256) void tail0_commit_kernel(Tail0Args t) {
    constexpr int B = 1 << LOG2B, KT = 256 / (B / 2), NT = 256;
    constexpr float invN = 1.0f / (float)(2 * B);
    const ProcJob &J = t.pa.job[0];
    const size_t c = blockIdx.x;
    if (t.err[c]) return;  // (replayed by tail0_replay_kernel)
    const int tid = threadIdx.x, n = t.n;
    const int k0 = blockIdx.y * KT, k1 = min(n, k0 + KT);
    const int4 st = J.state[c];
    const int cur0 = st.x, act = st.y;
    const float *ys = t.ys + (size_t)c * t.nmax * 2 * B;
    float *outc = J.out + c * J.out_stride;
    for (int idx = k0 * B + tid; idx < k1 * B; idx += NT) {
        const int k = idx >> LOG2B, j = idx & (B - 1);
        const float ov = k == 0 ? t.ov0[c * B + j] : ys[(size_t)(k - 1) * 2 * B + B + j] * invN;
        outc[idx] = ys[(size_t)k * 2 * B + j] * invN + ov;
    }
    if (k1 == n) {  // (the input buffer is empty after a completed block, :280)
        for (int j = tid; j < B; j += NT) J.overlap[c * B + j] = ys[(size_t)(n - 1) * 2 * B + B + j] * invN;
        if (st.w & FLAG_INBUF)
            for (int j = tid; j < B; j += NT) J.inbuf[c * B + j] = 0.f;
    }
    const size_t rows = (size_t)J.S * B;
    float2 *Xc = J.X + c * rows;
    const float2 *xs = t.xs + (size_t)c * t.nmax * B;
    const int kf = max(k0, n - act);
    for (int idx = tid; idx < (k1 - kf) * B; idx += NT) {
        const int k = kf + (idx >> LOG2B), m = idx & (B - 1);
        int r = (cur0 - k) % act;
        if (r < 0) r += act;
        Xc[(size_t)r * B + m] = xs[(size_t)k * B + m];
    }
}

// (4) per channel: the state word of a committed channel (current, the
// flags of n completed blocks) -- or, for a channel whose C2R failed on a
// pending block, tail_convolver0.process block by block (:464-472) from the
// untouched state by the generic step, so the failing block leaves exactly
// the reference's state
template <int LOG2B>
constexpr int t0_replay_nt();
template <int LOG2B>
__global__ __launch_bounds__(LOG2B == 6 ? 512 : proc_nt(LOG2B)) void tail0_replay_kernel(Tail0Args t) {
    constexpr int B = 1 << LOG2B, NT = LOG2B == 6 ? 512 : proc_nt(LOG2B);  // (t0_replay_nt: the fused flush's)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const ProcJob &J = t.pa.job[0];
    const size_t c = blockIdx.x;
    const int n = t.n;
    if (threadIdx.x == 0) t.miss[c] = 0;  // (every pending spectrum was recomputed or is the run's)
    if (!t.err[c]) {
        if (threadIdx.x == 0) {
            const int4 st = J.state[c];
            const int act = st.y;
            int cur = (st.x - n) % act;
            if (cur < 0) cur += act;
            const int flags = (st.w & ~(FLAG_PRE | FLAG_INBUF)) ^ ((n & 1) ? FLAG_REV : 0);
            J.state[c] = make_int4(cur, act, 0, la_clear(flags, t.pa));
        }
        return;
    }
    for (int k = 0; k < n; ++k) {
        ProcJob Jk = J;
        Jk.in = J.in + (size_t)k * B;
        Jk.out = J.out + (size_t)k * B;
        Jk.n = B;
        __syncthreads();  // the previous block's state word is stored
        const int4 st = J.state[c];
        process_job<LOG2B, NT, false, false>(t.pa, Jk, c, st, smem);
    }
    __syncthreads();
    if (threadIdx.x == 0) t.err[c] = 0;
}

// The whole flush in ONE launch at B = 64 (cfg3's head; one slot chunk per
// channel), the default there: per channel one 512-thread workgroup
//   (0) every row by LDS-DMA: tail0's IR rows, the previous period's FDL rows,
//       the pending spectra the head's run wrote (blocks [0, k0)), the
//       overlap, and the inputs of the blocks still to transform;
//   (1) the R2C of blocks [r0, n) (r0 = k0, or 0 if the run missed some of
//       this channel's spectra) into their LDS X rows;
//   (2) the MAC of tail0_mac_kernel, conv rows to LDS; realfft's C2R error
//       (a non-finite DC / Nyquist of some block's conv) decided right here;
//   (3) the FDL rows committed, then each block's C2R;
//   (4) overlap-add, overlap save and the state -- or, on a C2R error, the
//       block-by-block replay of tail0_replay_kernel from the untouched state.
// The same arithmetic in the same order as the five kernels (bit-identical:
// a block's MAC sums its rows in the same order whatever the blocks per
// thread, and both replays run the generic step on 512 threads).
// The B = 64 transforms use 16 of a wave's 64 lanes (16 radix-4 butterflies
// per stage), so each wave runs FOUR blocks' transforms at once, one per
// 16-lane group, each in its own LDS buffers: the same butterflies per lane
// group.  (r4's fused kernel ran one at a time, 16 per wave: 46 us per
// flush; 256 threads with four groups per wave: 22.4 us per cfg3 flush --
// MAC 9.4, C2R 6.0, commit 3.4 -- r6o FFTCONV_T0_TRACE.)
// LDS: [H rows + zero | X rows (q >= -1) + zero rows] (the C2R outputs reuse
// the H rows once the MAC is done, the second 16 transform buffers the X
// rows once the FDL is committed) | tw | 16 groups x 2 B-point buffers |
// conv rows (the inputs to transform before the MAC) | overlap | flag
constexpr int T0F_NT = 512, T0F_J = 4, T0F_G = 16;  // threads; blocks per MAC thread; transform groups of waves 0-3
template <int LOG2B>
constexpr int t0_replay_nt() { return LOG2B == 6 ? T0F_NT : proc_nt(LOG2B); }
template <int LOG2B>
__host__ __device__ constexpr size_t tail0_fused_lds(int act, int n) {
    constexpr size_t B = (size_t)1 << LOG2B;
    return (size_t)(2 * act + 1 + n + T0F_J) * T0_FC * 16 + 2 * B * 8 + T0F_G * 2 * B * 8 + (size_t)n * (B / 2) * 16 +
           B * 4 + 16;
}
template <int LOG2B>
__host__ __device__ constexpr bool tail0_fused_fits(int act, int n) {
    constexpr size_t B = (size_t)1 << LOG2B;
    // (the C2R's second 16 transform buffers live in the X rows: 2 x 16 x B float2)
    return LOG2B == 6 && act >= 1 && n >= 1 && n <= (T0F_NT / T0_FC) * T0F_J && n <= act + 1 &&
           (size_t)(act + n + T0F_J) * T0_FC * 16 >= T0F_G * 2 * B * 8 && tail0_fused_lds<LOG2B>(act, n) <= 160 * 1024;
}
template <int LOG2B>
__global__ __launch_bounds__(T0F_NT) void tail0_fused_kernel(Tail0Args t) {
    constexpr int B = 1 << LOG2B, F = B / 2, FC = T0_FC, J = T0F_J, RS = J + 1, NT = T0F_NT, GL = 16;
    static_assert(F == FC && B / 4 == GL, "one slot chunk per channel, 16 butterflies per stage (B = 64)");
    constexpr float invN = 1.0f / (float)(2 * B);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const ProcJob &J0 = t.pa.job[0];
    const size_t c = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = wave * 4 + (lane >> 4), gl = lane & 15;  // this lane's transform group (0..31), its lane in it
    const int4 st = J0.state[c];
    const int cur0 = st.x, act = st.y, n = t.n;
    const size_t rows = (size_t)J0.S * B;
    float4 *Hs = reinterpret_cast<float4 *>(smem);   // [act + 1][FC]
    float4 *Xs = Hs + (size_t)(t.act + 2) * FC;       // Xs[q * FC], q >= -1
    unsigned char *rest = smem + (size_t)(2 * t.act + 1 + n + J) * FC * 16;
    float2 *twl = reinterpret_cast<float2 *>(rest);
    float2 *wb = twl + 2 * B;
    // groups 0-15: their buffers after tw; groups 16-31 (the C2R only): the X rows' region
    float2 *gA = grp < T0F_G ? wb + (size_t)grp * 2 * B : reinterpret_cast<float2 *>(Xs - FC) + (size_t)(grp - T0F_G) * 2 * B;
    float2 *gB = gA + B;
    float4 *cvs = reinterpret_cast<float4 *>(wb + (size_t)T0F_G * 2 * B);  // [n][F]
    float *ins = reinterpret_cast<float *>(cvs);       // [n][B] inputs to transform, before the MAC
    float *ovs = reinterpret_cast<float *>(cvs + (size_t)n * F);
    int &s_err = *reinterpret_cast<int *>(ovs + B);
    float *ys = reinterpret_cast<float *>(smem);       // [n][2B], over the H rows after the MAC
    const bool geo = act == t.act;  // (not the geometry the LDS was sized for: replay)
    const int r0 = t.miss[c] ? 0 : min(t.k0, n);      // blocks [r0, n) are transformed here
    // (FFTCONV_T0_TRACE, tuning: phase stamps of thread 0, s_memrealtime)
    int *tst = t.pa.la_trace ? reinterpret_cast<int *>(t.pa.la_trace) + c * 8 : nullptr;
    auto stamp = [&](int k) {
        if (tst && tid == 0) tst[k] = (int)(unsigned)__builtin_amdgcn_s_memrealtime();
    };
    stamp(0);

    // ---- (0) every row by LDS-DMA (no VGPRs, all in flight) ----
    const float4 *H = reinterpret_cast<const float4 *>(J0.H + c * rows);
    const float4 *X = reinterpret_cast<const float4 *>(J0.X + c * rows);
    const float4 *xs = reinterpret_cast<const float4 *>(t.xs + (size_t)c * t.nmax * B);
    const int nq = act - 1 + n;
    constexpr int NWV = NT / 64;
    if (tid == 0) s_err = geo ? 0 : 1;
    if (geo) {
        for (int idx = tid; idx < FC; idx += NT) Hs[(size_t)act * FC + idx] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int idx = tid; idx < (J + 1) * FC; idx += NT) {
            const int q = idx < FC ? -1 : nq + idx / FC - 1;
            Xs[(size_t)q * FC + idx % FC] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const int half = lane >> 5, f = lane & 31;
        for (int r2 = wave * 2; r2 < act; r2 += 2 * NWV)  // IR rows, two per wave instruction
            if (r2 + half < act)
                __builtin_amdgcn_global_load_lds((gptr_t)(H + (size_t)(r2 + half) * F + f),
                                                 (lptr_t)(Hs + (size_t)r2 * FC), 16, 0, 0);
        // X rows q < act - 1 + r0: the previous period's FDL rows, then the
        // spectra of pending blocks [0, r0) (the run's)
        for (int r2 = wave * 2; r2 < act - 1 + r0; r2 += 2 * NWV) {
            const int q = r2 + half;
            const float4 *src;
            if (q < act - 1) {
                int r = cur0 + act - 1 - q;
                if (r >= act) r -= act;
                src = X + (size_t)r * F;
            } else {
                src = xs + (size_t)(q - (act - 1)) * F;
            }
            if (q < act - 1 + r0)
                __builtin_amdgcn_global_load_lds((gptr_t)(src + f), (lptr_t)(Xs + (size_t)r2 * FC), 16, 0, 0);
        }
        dma_16b<NT>(twl, t.pa.tw, 2 * B * (int)sizeof(float2));
        dma_f32<NT>(ovs, J0.overlap + c * B, B);
        for (int k = r0 + wave; k < n; k += NWV)  // (tail_input blocks: the job's input, stride T)
            dma_f32<64>(ins + (size_t)k * B, J0.in + c * J0.in_stride + (size_t)k * B, B);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    stamp(1);
    if (!geo) goto replay;
    {
        // ---- (1) R2C of blocks [r0, n) (:229-241) into their X rows, 16 at a time (waves 0-3) ----
        if (grp < T0F_G) {
            for (int k0 = r0; k0 < n; k0 += T0F_G) {
                const int k = k0 + grp;
                const bool live = k < n;
                for (int m = gl; m < B; m += GL)
                    gA[m] = live && m < B / 2 ? make_float2(ins[(size_t)k * B + 2 * m], ins[(size_t)k * B + 2 * m + 1])
                                              : make_float2(0.f, 0.f);
                wave_sync();
                float2 *Z = lds_cfft<LOG2B, GL, false, true>(gA, gB, twl);
                if (live) {
                    float2 *xr = reinterpret_cast<float2 *>(Xs + (size_t)(k + act - 1) * FC);
                    for (int m = gl; m < B; m += GL) xr[m] = real_post<LOG2B, 64>(Z, m, twl);
                }
                wave_sync();
            }
        }
        __syncthreads();
        stamp(2);
        // ---- (2) the MAC of tail0_mac_kernel (J blocks per thread), conv rows to LDS ----
        const int fl = tid % FC, g = tid / FC, kb0 = g * J;
        if (kb0 < n) {
            auto xq = [&](int q) { return Xs[q * FC + fl]; };
            LaAcc acc[J];
#pragma unroll
            for (int j = 0; j < J; ++j) acc[j].zero();
            const bool z0 = fl == 0;
            const int Q1 = kb0 + act - 2;
            float4 xr[RS];
#pragma unroll
            for (int e = 0; e < J; ++e) xr[e] = xq(Q1 + J - 1 - e);
            float4 hn = Hs[(size_t)min(1, act) * FC + fl];
            const int ns = act - 1;
            for (int s0 = 0; s0 < ns; s0 += RS) {
#pragma unroll
                for (int u = 0; u < RS; ++u) {
                    const int sidx = s0 + u;
                    if (sidx >= ns) break;
                    const float4 h = hn;
                    xr[(u + J) % RS] = xq(Q1 - 1 - sidx);
                    hn = Hs[(size_t)min(sidx + 2, act) * FC + fl];
                    const LaH ho = la_ops(h, z0);
#pragma unroll
                    for (int j = 0; j < J; ++j) acc[j].mac(ho, xr[(u + J - 1 - j) % RS]);
                }
            }
            const float4 h0 = Hs[fl];
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int k = kb0 + j;
                if (k < n) cvs[(size_t)k * F + fl] = slot_mac(acc[j].get(), Xs[(size_t)(k + act - 1) * FC + fl], h0, fl);
            }
        }
        __syncthreads();
        stamp(3);
        // realfft's C2R error (:264-267): a block's conv DC / Nyquist not finite
        if (tid < n) {
            const float2 z = reinterpret_cast<const float2 *>(cvs + (size_t)tid * F)[0];
            if (!(isfinite(z.x) && isfinite(z.y))) s_err = 1;
        }
        __syncthreads();
        if (s_err) goto replay;
        // ---- (3) the FDL rows (block k at (cur0 - k) % act, the last act blocks stay) ----
        float2 *Xc = J0.X + c * rows;
        const int kf = max(0, n - act);
        for (int idx = tid; idx < (n - kf) * B; idx += NT) {
            const int k = kf + (idx >> LOG2B), m = idx & (B - 1);
            int r = (cur0 - k) % act;
            if (r < 0) r += act;
            Xc[(size_t)r * B + m] = reinterpret_cast<const float2 *>(Xs + (size_t)(k + act - 1) * FC)[m];
        }
        __syncthreads();  // (the X rows are read: groups 16-31 take their region)
        // ... then each block's C2R, 32 at a time
        for (int k0 = 0; k0 < n; k0 += 2 * T0F_G) {
            const int k = k0 + grp;
            const bool live = k < n;
            const float2 *Zc = reinterpret_cast<const float2 *>(cvs + (size_t)min(k, n - 1) * F);
            for (int m = gl; m < B; m += GL) gA[m] = real_pre<LOG2B, 64>(Zc, m, twl);
            wave_sync();
            const float *y = reinterpret_cast<const float *>(lds_cfft<LOG2B, GL, true, true>(gA, gB, twl));
            if (live) {
                float *yr = ys + (size_t)k * 2 * B;
                for (int j = gl; j < 2 * B; j += GL) yr[j] = y[j];
            }
            wave_sync();
        }
        __syncthreads();
        stamp(4);
        // ---- (4) overlap-add (:270-274), overlap save (:283-284), state ----
        float *outc = J0.out + c * J0.out_stride;
        for (int idx = tid; idx < n * B; idx += NT) {
            const int k = idx >> LOG2B, j = idx & (B - 1);
            const float ov = k == 0 ? ovs[j] : ys[(size_t)(k - 1) * 2 * B + B + j] * invN;
            outc[idx] = ys[(size_t)k * 2 * B + j] * invN + ov;
        }
        for (int j = tid; j < B; j += NT) J0.overlap[c * B + j] = ys[(size_t)(n - 1) * 2 * B + B + j] * invN;
        if (st.w & FLAG_INBUF)
            for (int j = tid; j < B; j += NT) J0.inbuf[c * B + j] = 0.f;
        if (tid == 0) {
            int cur = (cur0 - n) % act;
            if (cur < 0) cur += act;
            const int flags = (st.w & ~(FLAG_PRE | FLAG_INBUF)) ^ ((n & 1) ? FLAG_REV : 0);
            J0.state[c] = make_int4(cur, act, 0, la_clear(flags, t.pa));
            t.miss[c] = 0;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        stamp(5);
        return;
    }
replay:
    // tail_convolver0.process block by block from the untouched state (the
    // FDL, the overlap and the state word are not written above), on the
    // generic step of 512 threads, as tail0_replay_kernel at B = 64
    if (tid == 0) t.miss[c] = 0;
    for (int k = 0; k < n; ++k) {
        ProcJob Jk = J0;
        Jk.in = J0.in + (size_t)k * B;
        Jk.out = J0.out + (size_t)k * B;
        Jk.n = B;
        __syncthreads();  // (the LDS is the generic step's now; the previous block's state word is stored)
        const int4 sk = J0.state[c];
        process_job<LOG2B, NT, false, false>(t.pa, Jk, c, sk, smem);
    }
}

template <int LOG2B>
static hipError_t launch_tail0_t(const Tail0Args &a, int channels, hipStream_t s, hipEvent_t done) {
    if constexpr (LOG2B >= 6 && LOG2B <= 9) {
        constexpr int B = 1 << LOG2B, KT = 256 / (B / 2);
        if (a.n <= 0 || a.n > a.nmax) return hipErrorInvalidValue;
        Tail0Args t = a;
        const Variant v = Variant::current();
        const int var = pick_variant(v, a.pa, channels, LOG2B);
        t.pa.pipe = (var & VARIANT_NOPIPE) ? 0 : 1;  // (the replay path's generic step)
        t.pa.lag = pipeline_lag();
        // (every check before the first launch: a failure leaves the pending
        // blocks and tail0's state untouched)
        constexpr int F = B / 2, FC = F < T0_FC ? F : T0_FC;
        const size_t lds = tail0_mac_lds<LOG2B>(a.act, a.n);
        auto mk = tail0_mac_kernel<LOG2B>;
        if (lds > 160 * 1024 || (256 / FC) * T0_J < a.n) return hipErrorInvalidValue;
        if (hipError_t e = lds_attr(mk, lds); e != hipSuccess) return e;
        if constexpr (LOG2B == 6) {
            // (VARIANT_T0FUSED: the five kernels instead, bit-identical)
            if (tail0_fused_fits<LOG2B>(a.act, a.n) && !v.has(VARIANT_T0FUSED)) {
                const size_t fl = tail0_fused_lds<LOG2B>(a.act, a.n);
                auto fk = tail0_fused_kernel<LOG2B>;
                if (hipError_t e = hipFuncSetAttribute((const void *)fk, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       (int)fl);
                    e != hipSuccess)
                    return e;
                if (done) {  // (the event on the kernel's own completion: no marker packet of its own)
                    hipExtLaunchKernelGGL(fk, dim3(channels), dim3(T0F_NT), fl, s, nullptr, done, 0, t);
                    return hipGetLastError();
                }
                hipLaunchKernelGGL(fk, dim3(channels), dim3(T0F_NT), fl, s, t);
                return hipGetLastError();
            }
        }
        // (blocks [0, k0) have their spectra from the head's run; the overlap
        // copy tail0_r2c makes at block 0 is then tail0_mac's)
        if (t.k0 < 0 || t.k0 > a.n) return hipErrorInvalidValue;
        // (always: with k0 == n its workgroups only test the channel's miss flag)
        hipLaunchKernelGGL(tail0_r2c_kernel<LOG2B>, dim3(channels, a.n), dim3(64), 4 * B * sizeof(float2), s, t);
        hipLaunchKernelGGL(mk, dim3(channels, F / FC), dim3(256), lds, s, t);
        hipLaunchKernelGGL(tail0_c2r_kernel<LOG2B>, dim3(channels, a.n), dim3(64), 4 * B * sizeof(float2), s, t);
        hipLaunchKernelGGL(tail0_commit_kernel<LOG2B>, dim3(channels, (a.n + KT - 1) / KT), dim3(256), 0, s, t);
        constexpr int RNT = t0_replay_nt<LOG2B>();
        static_assert(RNT == (LOG2B == 6 ? 512 : proc_nt(LOG2B)), "tail0_replay_kernel's thread count");
        constexpr size_t rep_lds = Geo<LOG2B, RNT>::lds_bytes;  // (the generic step)
        if (done) {
            hipExtLaunchKernelGGL(tail0_replay_kernel<LOG2B>, dim3(channels), dim3(RNT), (std::uint32_t)rep_lds, s,
                                  nullptr, done, 0, t);
            return hipGetLastError();
        }
        hipLaunchKernelGGL(tail0_replay_kernel<LOG2B>, dim3(channels), dim3(RNT), rep_lds, s, t);
        return hipGetLastError();
    } else {
        return hipErrorNotSupported;
    }
}
bool tail0_defer_supported(int log2b, int act, int nmax) {
    if (log2b < 6 || log2b > 9 || act < 1 || nmax < 1) return false;
    const int F = (1 << log2b) / 2, FC = F < T0_FC ? F : T0_FC;
    return nmax <= (256 / FC) * T0_J && tail0_mac_lds<6>(act, nmax) <= 160 * 1024;
}
hipError_t launch_tail0_flush(int log2b, const Tail0Args &a, int channels, hipStream_t s, hipEvent_t done) {
    if (channels <= 0) return hipSuccess;
    return dispatch_log2<6, 9>(log2b, hipErrorNotSupported,
                               [&](auto L) { return launch_tail0_t<L()>(a, channels, s, done); });
}

}  // namespace fftconv
