// kernels.hpp -- host-visible kernel argument blocks and launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "variant.hpp"

// FFTCONV_DEBUG_BOUNDS (debug builds only, Makefile target debug-bounds):
// DBG_CHECK(cond, site, v0..v3) reports a failed index check with printf.
// One out-of-line report per translation unit (a printf inlined at each of
// the hundreds of inlined load sites made the debug build compile for hours).
#ifdef FFTCONV_DEBUG_BOUNDS
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
static __device__ __attribute__((noinline, unused)) void dbg_bounds(int site, int v0, int v1, int v2, int v3) {
    printf("BOUNDS site %d blk %d tid %d: %d %d %d %d\n", site, (int)blockIdx.x, (int)threadIdx.x, v0, v1, v2, v3);
}
#endif
#define DBG_CHECK(cond, site, v0, v1, v2, v3)          \
    do {                                               \
        if (!(cond)) dbg_bounds(site, v0, v1, v2, v3); \
    } while (0)
#else
#define DBG_CHECK(cond, site, v0, v1, v2, v3) do {} while (0)
#endif

namespace fftconv {

enum : int {
    FLAG_INBUF = 1,  // the HBM input buffer holds live samples
    FLAG_REV = 2,    // scan parity of the segment MAC (toggled per completed block)
    FLAG_PRE = 4,    // pre[] holds pre_multiplied of the block that starts at `current`
    FLAG_XSYNC = 8,  // crossfade pair: this FDL has always equalled its partner's
    // lookahead (time-blocked FDL, see la.hpp): per anchor level lv = 1..3 the
    // window of partial sums is live (FLAG_LA1 << 2(lv-1)) in window
    // FLAG_PW1 << 2(lv-1) of the two; a step at launch t reads the row at
    // position (t - 1 - c) mod P_lv.  Bits 24-25 = the launch tag of the last
    // process launch that wrote this state word
    FLAG_LA1 = 16,
    FLAG_PW1 = 32,
    FLAG_LA2 = 64,
    FLAG_PW2 = 128,
    FLAG_LA3 = 256,
    FLAG_PW3 = 512,
    // a multi-block call on the lookahead path (ProcJob::mcall > 1) is done
    // for this channel before its last launch: it ran the whole call by the
    // generic chunk loop in the first launch (off the lookahead path), or a
    // block's C2R failed (the call's output is zero-filled, :264-267); the
    // call's remaining launches skip it, the last one clears the flag
    FLAG_CALLDONE = 1 << 10,
    // far-row windows of the generic step (B >= 1024, gw_anchor_kernel): the
    // channel's P windows were anchored after the step of its class and every
    // step since read one and advanced
    FLAG_GW = 1 << 11,
    SEQ_SHIFT = 24,
    // lookahead: pre[] holds the near rows' sum (rows D0..1) of the block
    // that starts at `current`, left by the previous step (la.hpp)
    FLAG_NEAR = 1 << 26,
    LA_MASK = FLAG_LA1 | FLAG_LA2 | FLAG_LA3 | FLAG_NEAR | FLAG_GW,
    SEQ_MASK = 3 << SEQ_SHIFT,
};

// One convolver batch's call (FFTConvolver::process over `n` samples of every
// channel), optionally with the two-stage epilogue of the head block
// (src/fft_convolver.rs:438-461): out[j] += add0[j], then += add1[j], and
// tin[j] = in[j], applied after the call.
struct ProcJob {
    const float2 *H;       // [C][S][B] packed IR spectra
    float2 *X;             // [C][S][B] packed FDL
    float *overlap;        // [C][B]
    float *inbuf;          // [C][B]
    float2 *pre;           // [C][B]
    int4 *state;           // [C] {current, active, fill, flags}
    const float *in;
    long long in_stride;
    float *out;
    long long out_stride;
    const float *add0;     // tail_precalculated0 + precalculated_pos (or null)
    const float *add1;     // tail_precalculated  + precalculated_pos (or null)
    long long add_stride;
    float *tin;            // tail_input + tail_input_fill (or null)
    long long tin_stride;
    int S;                 // seg_count (row pitch of H and X in rows)
    int n;                 // output samples this call
    // lookahead launches of a multi-block call (n = mcall * B, one launch per
    // block, in / out advanced by mk * B): blocks of the whole call, this
    // launch's block (0 / 0 otherwise)
    int mcall, mk;
    // long-block path (B > 2^kMaxLog2Fused, large.hip): per channel the
    // call's progress {processed, done, C2R failed, arrival counter}, and the
    // [C][B] scratch between the row and the column passes of the inverse.
    // Lookahead launches (la.hpp, B <= 512: never long-block) use the same
    // two words for the channels' state words as of the end of the previous
    // launch, which the anchors read instead of `state` (the step of this
    // launch rewrites `state` while the anchors run), and the copy the steps
    // of this launch fill for the next one (null elsewhere).  (Shared words,
    // not new ones: a larger argument block measurably slows every launch,
    // +0.2 us per cfg2 step for 32 bytes, r6y.)
    union {
        int4 *lg_prog;
        const int4 *sview;
    };
    union {
        float2 *lg_v;
        int4 *vnext;
    };
    // two-stage head of a multi-call launch (upols_run_kernel): its block's
    // spectrum also goes to the deferred tail0's pending-block row
    // t0x + c * t0x_stride (the same R2C tail0_r2c_kernel would compute), so
    // the period's flush skips those blocks' transforms; null = none
    float2 *t0x;
    long long t0x_stride;
    // [C]: set by a run's call that did NOT write its block's spectrum to t0x
    // (a channel whose head buffer is out of step with tail_input, e.g. after
    // a C2R error on a partial call, :264-267): the flush recomputes that
    // channel's pending spectra from tail_input and clears the flag
    int *t0m;
};

// Twiddle tables of the long-block path (large.hip), f64-rounded f32:
// twN = W_N^k (k < N/2, the post/pre-twiddle), twM = W_M^j (j < M = N/2, the
// four-step's inner twiddle), twA / twB = W_{2 M1}^i / W_{2 M2}^i (the column
// and row FFTs), M = M1 x M2 (lg_split)
struct LgTab {
    const float2 *twN, *twM, *twA, *twB;
};

// Crossfader::mix over one call's samples (src/crossfade_convolver.rs:242-278),
// the crossfader state at the start of the call.
struct CrossfadeMixArgs {
    const float *buf_a;
    const float *buf_b;
    long long buf_stride;
    float *out;
    long long out_stride;
    int n;
    int approaching;       // FadingState::Approaching
    int target;            // 0 = A, 1 = B
    long long counter0;
    long long fading;
    float mix_value0;
    float step;
    const float *vtab;     // calls longer than 1024 samples: the mix_value walk (launch_crossfade_walk), or null
};

// Up to two jobs of the same block size in one launch (grid.y = job): the
// two-stage head and tail0 run together on the same input block.
struct ProcArgs {
    ProcJob job[2];
    const float2 *tw;      // W_N^k, k < N = 2B
    int njobs;
    int pipe;              // pipelined full-block step allowed (B <= 512)
    int lag;               // pipelined step: FDL rows wave 0 leaves to the stream waves
    int fuse_mix;          // crossfade pair launch: mix A and B into mix.out in-kernel
    CrossfadeMixArgs mix;  // (buf_a / buf_b unused then)
    // lookahead launch (launch_process_la; job[0] only)
    float2 *laW;           // [C][2 windows][LA_PT][B]: the partial-sum windows of levels 1..3
    float2 *laW2;          // job[1]'s windows (la_mix 3: the crossfade's B in the same launch)
    int la_n[3];           // anchor workgroups of levels 1..3 (grid: level 3, 2, 1, then the steps)
    int la_nlv;            // anchor levels: 3, or 2 when no FDL row reaches level 3 (S <= LA_R2 + 1)
    int la_all;            // 1: every channel is scheduled for anchors (entry launch); -1: none is
    int la_t;              // launch counter mod LA_PER: channel c anchors at period P when (c - t) % P == 0
    int la_seq;            // 1 or 2, alternating per lookahead launch; 0 in every other launch
    int la_channels;       // channels of the batch (step workgroups cover LaStep::NCH each)
    int la_l1in2;          // 1: level-1 anchor b runs in level-2 anchor workgroup b, after its walk
    // crossfade on the lookahead step (CrossfadeConvolver::process :72-77):
    // 1 = A's launch also writes this call's per-sample mix selectors to mix_tab;
    // 2 = B's launch mixes in its epilogue: out = mix(mix.buf_a, B's block);
    // 3 = ONE launch for A (job[0]) and B (job[1]): a step workgroup runs A's
    //     and B's chain of one channel and mixes in LDS (out = job[0].out)
    int la_mix;
    float *mix_tab;        // [n] mix_selector of each sample (la_mix 1 writes, 2 reads)
    // window rebuild (launch_la_rebuild, after update / reset / init): anchors
    // only, for channels [la_c0, la_channels), as if they had run in the
    // launch before the next one (la_t = that launch's counter)
    int la_rebuild;
    int la_c0;
    // launch timeline (tuning only, FFTCONV_LA_TRACE): per wave {role | wave
    // << 4, HW_ID low 16 bits | XCC_ID << 24, t0, t1} (s_memrealtime, 100 MHz)
    int4 *la_trace;        // this launch's record: [la_trace_grid][4 waves] + phase stamps after it
    int la_trace_grid;
    // state-word probe (tests only, FFTCONV_LA_PROBE at handle creation): the
    // anchors wait for the launch's steps and read the state past their L2,
    // so they observe the post-step word; each such observation is counted
    int *la_probe_cnt;
    // long-block path (launch_process with log2b > kMaxLog2Fused): the
    // geometry's tables and the chunks to run (an upper bound over channels)
    LgTab lg;
    int lg_chunks;
    // far-row windows of the generic step (B >= 1024, gw_anchor_kernel):
    // gw_p = the split row P (pre = rows 1..P-1 + rows P..act-1; 0 = one sum),
    // gw = [C][P][B] windows (null: no step of this launch reads one), gw_t =
    // the batch's one-block step count mod P (channel c reads row (gw_t-1-c) mod P)
    float2 *gw;
    int gw_p;
    int gw_t;
    // 2048 <= B <= 8192: 256-thread workgroups (upols_narrow_kernel) instead
    // of 512 -- a two-stage tail beside the head's multi-call run, so one
    // tail workgroup fits each CU next to a run workgroup (same bits)
    int narrow;
    // multi-call run (upols_run_kernel): the waves' issue priority (s_setprio;
    // 0 = the default) -- the latency-bound chain beside the two-stage tail
    int prio;
    // multi-call run: the FDL rows and IR rows held in LDS for the whole run
    // (the pipelined step's helpers stream them from LDS), when they fit: the
    // row count S of the job, 0 = off (the rows stream from HBM / L2)
    int run_lds_rows;
    // device-side ordering of a two-stage period's head after the previous
    // tail step, without a barrier packet on the head's stream: sig_mode 1
    // (the tail's step) -- every workgroup arrives on sig[0], the last one
    // releases sig[1] = sig_val; sig_mode 2 (a run) -- the workgroups start
    // once sig[1] has reached sig_val (acquire), or after a bounded wait that
    // counts in sig[2]
    unsigned *sig;
    unsigned sig_val;
    int sig_mode;
};

struct IrArgs {
    float2 *H;
    float *overlap;
    float2 *pre;
    int4 *state;
    const float *src;      // device IR samples of channel chan0 (+ src_stride per channel)
    long long src_stride;
    long long len_data;    // samples present in src
    long long len_active;  // length that sets active_seg_count = ceil(len_active / B)
    const float2 *tw;
    int S;
    int chan0;
    int update_state;      // 1: update() side effects (zero overlap/pre, set active)
};

struct TwoStageAccumArgs {
    float *out;
    long long out_stride;
    const float *p0;       // tail_precalculated0 [C][T]
    const float *p1;       // tail_precalculated  [C][T]
    long long T;
    int pos;               // precalculated_pos
    const float *in;
    long long in_stride;
    int sb;                // sub-chunk start within the call
    float *tail_input;     // [C][T]
    int fill;              // tail_input_fill before the append
    int cnt;               // samples in the sub-chunk
};


// Fft::forward / Fft::inverse (src/fft_convolver.rs:36-49) over rows of
// N = 2M reals / M+1 interleaved complex bins (the public Fft of the
// reference, fftconv_fft_*): one workgroup per row, the convolver's own
// transforms (lds_cfft + real_post / real_pre, the same twiddle table)
struct FftArgs {
    const float *in;
    long long in_stride;   // floats between rows
    float *out;
    long long out_stride;
    const float2 *tw;      // W_N^k, k < N
    int *status;           // inverse: per row 1 = FftError::InputValues (DC / Nyquist imag != 0), or null
};
hipError_t launch_fft_rows(int log2m, bool inverse, const FftArgs &a, int rows, hipStream_t s);

hipError_t launch_process(int log2b, const ProcArgs &a, int channels, hipStream_t s);
// a run of r.n consecutive one-job process() calls in one launch
// (upols_run_kernel, 64 <= B <= 512): call k = job[0] with in / out advanced
// by k * in_step / out_step floats and add0 / add1 / tin by k * n
struct RunSteps {
    long long in_step, out_step;
    int n;
};
bool run_supported(int log2b);
int run_lds_rows(int log2b, int S);  // a run's LDS-resident rows for this geometry (0 = none)
hipError_t launch_process_run(int log2b, const ProcArgs &a, const RunSteps &r, int channels, hipStream_t s);
hipError_t launch_ir_segments(int log2b, const IrArgs &a, int channels, hipStream_t s);
hipError_t launch_twostage_accum(const TwoStageAccumArgs &a, int channels, hipStream_t s);
hipError_t launch_crossfade_mix(const CrossfadeMixArgs &a, int channels, hipStream_t s);
hipError_t launch_reset_state(int4 *state, int channels, hipStream_t s);
// crossfade pair (A and B of one CrossfadeConvolver in one workgroup per channel)
bool pair_supported(int log2b, int S);
hipError_t launch_process_pair(int log2b, const ProcArgs &a, int channels, hipStream_t s);
hipError_t launch_state_flags(int4 *state, int channels, int set, int clear, hipStream_t s);
size_t process_lds_bytes(int log2b);
// lookahead: 1 if this geometry takes the lookahead step, else 0
int la_parts(int log2b, int S);
// the lookahead launch shape of a geometry (la.hpp): anchor levels, the
// workgroups per anchor of each level (level 1: 0 = run by the step
// workgroups), and the periods
struct LaDims {
    int nlv;
    int per[3];
    int wg[3];
    int pt;           // window rows per channel and window (all levels)
    int per_all;      // the stagger clock's modulus
};
LaDims la_dims(int log2b, int S, int jw = 8);  // (jw: window steps per level-2/3 anchor workgroup, LA_JW)
// launch timeline records per lookahead launch (FFTCONV_LA_TRACE): the largest grid
int la_trace_grid(int log2b, int S, int channels);
hipError_t launch_process_la(int log2b, const ProcArgs &a, int channels, hipStream_t s);
// every far and mid window of channels [a.la_c0, channels) rebuilt from the
// current H and FDL (anchors only), then their state words pointed at them
hipError_t launch_la_rebuild(int log2b, const ProcArgs &a, int channels, hipStream_t s);

// A chunk of k consecutive one-block lookahead steps whose blocks are all at
// hand (process_device_steps), in four launches (la_batch.hpp: spectra, walk,
// finish, fix-up) instead of k.  Step j is a.job[0] with in / out advanced by
// j * in_step / out_step floats.  The chunk's staging and pre rows take the
// window buffer a.laW, so it leaves no live window.
constexpr int LA_BATCH_MAX = 64;  // steps per chunk (2 x 64 rows of the channel's 2 x 84 window rows)
// the shortest call that takes the batch while the windows are live: below
// it the per-block launches' 36.5 row transfers per step cost less than the
// batch's one pass over H and the FDL spread over the call (cfg2, same
// process: 12-step calls 18.5 against 16.6 us per step per block, 16-step
// calls 14.5 against 16.6)
constexpr int LA_BATCH_MIN = 16;
struct LaBatchArgs {
    long long in_step, out_step;
    int k;                 // steps of the chunk, 1..LA_BATCH_MAX
    int seq0;              // the launch tag step 0 would carry (ProcArgs::la_seq), alternating per step
    int *resume;           // [C]: the first step the fix-up launch runs for the channel (k = none)
};
hipError_t launch_la_batch(int log2b, const ProcArgs &a, const LaBatchArgs &b, int channels, hipStream_t s);

// Two-stage tail0 deferred to the end of its period (src/fft_convolver.rs
// :464-475: tail_output0 is first read after the period's swap).  pa.job[0]
// is tail0's job with in = tail_input + off, out = tail_output0 + off (both
// stride T); the n pending blocks of every channel are transformed, summed
// against one pass of tail0's IR rows and FDL, inverted, and committed --
// or, for a channel whose C2R fails on any block (realfft's error path),
// replayed block by block by the generic step from the untouched state.
struct Tail0Args {
    ProcArgs pa;
    float2 *xs;            // [C][nmax][B]: spectra of the pending blocks
    float *ys;             // [C][nmax][2B]: their C2R outputs (not yet scaled)
    int *err;              // [C]: some pending block's C2R fails
    float *ov0;            // [C][B]: the overlap before the pending blocks
    float2 *cv;            // [C][nmax][B]: conv of each pending block
    int act;               // tail0's active segments (every channel: TwoStage never updates tail0)
    int n;                 // pending blocks
    int nmax;              // row pitch of xs / ys in blocks
    int k0;                // blocks [0, k0) already have their spectra in xs (the head's run wrote them)
    int *miss;             // [C]: 1 = the run missed some of this channel's spectra: recompute [0, n) (ProcJob::t0m)
};
bool tail0_defer_supported(int log2b, int act, int nmax);
// done (optional): an event recorded by the flush's last kernel itself (hipExtLaunchKernel)
hipError_t launch_tail0_flush(int log2b, const Tail0Args &a, int channels, hipStream_t s, hipEvent_t done = nullptr);

// The fused one-workgroup-per-channel kernels hold two B-point complex
// buffers in LDS: B <= 8192 (128 KiB).  Larger blocks, up to 2^22, take the
// four-step long-block path (large.hip).
constexpr int kMaxLog2Fused = 13;
constexpr int kMaxLog2Block = 22;
// far-row windows (gw_anchor_kernel): window rows per channel = the split row
constexpr int kGwP = 8;
// a batch of this geometry sums far rows through windows: 1024 <= B <= 8192
// and enough far rows to pay for the anchors
bool gw_supported(int log2b, int S);
// the windows of the channels of class a.gw_t mod kGwP, from the state after
// the step just launched (a.job[0]: H, X, state, S; a.la_channels channels)
hipError_t launch_gw_anchor(int log2b, const ProcArgs &a, int channels, hipStream_t s);
// M = 2^log2b = M1 x M2 of the long-block path; bin k of a spectrum row sits
// at position (k mod M1) * M2 + k / M1
void lg_split(int log2b, int *l1, int *l2);
size_t lg_position(int log2b, size_t k);
hipError_t launch_process_large(int log2b, const ProcArgs &a, const LgTab &t, int chunks, int channels,
                                hipStream_t s);
hipError_t launch_ir_large(int log2b, const IrArgs &a, const LgTab &t, int channels, hipStream_t s);
// the public Fft's rows through the same passes: rows in batches of `batch`,
// scratch [batch][N/2] complex
hipError_t launch_fft_large(int log2m, bool inverse, const FftArgs &a, const LgTab &t, float2 *scratch, int rows,
                            int batch, hipStream_t s);
// the public Fft of a length n that is not a power of two: Bluestein over
// P = 2^log2p >= 2n - 1 point FFTs (large.hip).  chirp[m] = exp(i pi m^2 / n)
// (m < n); filt = FFT_P of the chirp filter (natural order for P <= 8192,
// else the four-step's transposed order); twP = W_{2P}^i (P <= 8192); t =
// the four-step tables of P (P > 8192); scratch [batch][P] (P > 8192)
hipError_t launch_fft_bluestein(size_t n, int log2p, bool inverse, const FftArgs &a, const float2 *chirp,
                                const float2 *filt, const float2 *twP, const LgTab &t, float2 *scratch, int rows,
                                int batch, hipStream_t s);
// crossfade mix of calls longer than the in-LDS walk (n > 1024): the walk
// once into a device table (one lane), then the mix reading it
hipError_t launch_crossfade_walk(const CrossfadeMixArgs &a, float *vtab, hipStream_t s);

// MatrixConvolver (matrix.hip): one chunk -- k samples at offset `fill` of the
// block that starts at `current` -- of every input and output.  The host keeps
// {current, active, fill} and passes them by value.
struct MatrixArgs {
    const float2 *H;       // [O][I][S][B] packed IR spectra (pair o*I + i)
    float2 *X;             // [I][S][B] one FDL per input
    float *ovl;            // [O][B] summed overlap
    float *ib;             // [I][B] input buffers (zero past the fill)
    float2 *pre;           // [O][B] summed pre_multiplied of a block in progress
    float2 *part;          // [O][P][B] split-row partial sums
    const float2 *tw;      // W_N^k, k < N = 2B
    const float *in;       // chunk of input 0 (+ in_stride per input)
    long long in_stride;
    float *out;            // chunk of output 0 (+ out_stride per output)
    long long out_stride;
    int I, O, S;
    int P;                 // MAC parts (matrix_mac_parts)
    int rpp;               // rows per part = ceil(I * (act - 1) / P)
    int cur, act, fill, k;
    int nt_h;              // nontemporal loads of the H stream (Variant::nt_matrix; same bits either way)
};
// P for a geometry and its active segments: a function of these only
int matrix_mac_parts(int inputs, int log2b, int seg_count, int active);
// the rule itself -- about 64 rows per part, at most 64 parts -- for the host
// and for the sparse matrix's plan kernel (matrix_sp.hip): one definition
__host__ __device__ inline int matrix_parts_rule(long long inputs, int active) {
    const long long R = inputs * (active > 1 ? active - 1 : 0);
    const long long p = (R + 63) / 64;
    return (int)(p < 1 ? 1 : (p > 64 ? 64 : p));
}
// the chunk's two launches (32 <= B <= 8192): A = R2C of every input + the
// split-row MAC when the chunk starts a block, B = the outputs' finish
hipError_t launch_matrix_chunk(int log2b, const MatrixArgs &a, hipStream_t s);

// SparseMatrixConvolver (matrix_sp.hip): one chunk of a matrix
// that holds only its N listed (output, input) pairs, in CSR order.  `m` is the
// dense chunk with H = [N][S][B] (pair n = row n) and part = [sum P_o][B];
// m.P and m.rpp are unused -- every output has its own, from the plan.
struct MatrixSpArgs {
    MatrixArgs m;
    const int *rowptr;     // [O + 1] pairs of output o = [rowptr[o], rowptr[o + 1])
    const int *col;        // [N] input of pair n
    const int *plan;       // [O + 1] prefix sums of P_o = matrix_parts_rule(k_o, act)
    const int4 *wg;        // [PT] MAC workgroup m = plan[o] + p: {rowptr[o], k_o, p, P_o}
    int N;                 // pairs
    int PT;                // plan[O]: the MAC workgroups of launch A, rows of `part`
};
// plan[0..O] and wg[0..plan[O]) for `act` active segments, one workgroup on s
hipError_t launch_matrix_sp_plan(const int *rowptr, int *plan, int4 *wg, int O, int act, hipStream_t s);
// the chunk's two launches (32 <= B <= 8192)
hipError_t launch_matrix_sp_chunk(int log2b, const MatrixSpArgs &a, hipStream_t s);

// MatrixLookaheadConvolver (matrix_la.hip): one chunk of a dense
// matrix whose far rows (s >= kMatrixLaQ) are summed once every kMatrixLaQ
// blocks into a window of kMatrixLaQ future blocks.  `m` is the dense chunk
// with part = [O][Pn][B] over the near rows (m.P = Pn, m.rpp = near rows per
// part).  Block numbers are the handle's count of started blocks.
constexpr int kMatrixLaQ = 8;        // the period Q (fftconv_matrix_lookahead_period)
constexpr int kMatrixLaMaxLog2B = 9;  // one 16-byte slot per thread: B <= 512
struct MatrixLaArgs {
    MatrixArgs m;
    float2 *far;           // [O][Pf][Q][B] far partial sums, window row = block % Q
    int Pf;                // far parts (0: no far rows, active <= Q)
    int rppf;              // far rows per part = ceil(I * (act - Q) / Pf)
    long long t;           // the block this chunk belongs to
    long long tv;          // windows anchored before block tv are invalid (tv > t: every output sums in full)
};
// the part rule on a row count (matrix_parts_rule's, which takes inputs and active)
__host__ __device__ inline int matrix_la_parts(long long rows) {
    const long long p = (rows + 63) / 64;
    return (int)(p < 1 ? 1 : (p > 64 ? 64 : p));
}
// what output o does with its far rows in launch A of block t: 1 = anchor (the
// windows of blocks t .. t + Q - 1), 2 = full sum of block t alone, 0 = nothing
// (block t is served by the window of the output's latest anchor).  Output o
// anchors on blocks t = o (mod Q).
__host__ __device__ inline int matrix_la_role(long long t, long long tv, int o) {
    const int ph = (int)(((t - o) % kMatrixLaQ + kMatrixLaQ) % kMatrixLaQ);
    if (t - ph < tv) return 2;
    return ph == 0 ? 1 : 0;
}
// steady: every output that does not anchor has a window, so launch A holds far
// workgroups for the anchoring outputs t % Q, t % Q + Q, ... only (else for all)
__host__ __device__ inline bool matrix_la_steady(long long t, long long tv) { return t - (kMatrixLaQ - 1) >= tv; }
__host__ __device__ inline int matrix_la_far_outputs(long long t, long long tv, int O) {
    if (!matrix_la_steady(t, tv)) return O;
    const int t0 = (int)(t % kMatrixLaQ);
    return t0 < O ? (O - t0 + kMatrixLaQ - 1) / kMatrixLaQ : 0;
}
// the chunk's two launches (32 <= B <= 512)
hipError_t launch_matrix_la_chunk(int log2b, const MatrixLaArgs &a, hipStream_t s);

// SparseMatrixLookaheadConvolver (matrix_sp_la.hip): one chunk of a
// sparse matrix (MatrixSpArgs' H = [N][S][B], rowptr, col) with MatrixLaArgs'
// far-row windows, every output with its own part counts over its pair list:
//   Pn_o = matrix_la_parts(k_o * (min(Q, act) - 1))
//   Pf_o = matrix_la_parts(k_o * (act - Q)), 0 when act <= Q or k_o == 0
// m.part = [sum Pn_o][B] (output o's near parts at nplan[o]); m.P and m.rpp are
// unused.  The window rows of output o start at far row fplan[o].
struct MatrixSpLaArgs {
    MatrixArgs m;
    const int *rowptr;     // [O + 1] pairs of output o = [rowptr[o], rowptr[o + 1])
    const int *col;        // [N] input of pair n
    const int *nplan;      // [O + 1] prefix sums of Pn_o
    const int *fplan;      // [O + 1] prefix sums of Pf_o, in output order
    const int4 *nwg;       // [PnT] near workgroup m = nplan[o] + p: {rowptr[o], k_o, p, Pn_o}
    const int4 *fwg;       // [2 * PfT] far workgroups ordered by (o % Q, o, p), two entries each:
                           // {rowptr[o], k_o, o, p}, {Pf_o, fplan[o] + p, 0, 0}
    float2 *far;           // [PfT][Q][B] far partial sums, window row = block % Q
    int N;                 // pairs
    int PnT, PfT;          // nplan[O], fplan[O]
    int fbase, flen;       // the far workgroups of this launch: descriptors [fbase, fbase + flen)
    long long t, tv;       // as MatrixLaArgs
};
__host__ __device__ inline int matrix_sp_la_pn(long long ko, int act) {
    const int nm = act < kMatrixLaQ ? act : kMatrixLaQ;
    return matrix_la_parts(ko * (nm > 0 ? nm - 1 : 0));
}
__host__ __device__ inline int matrix_sp_la_pf(long long ko, int act) {
    return act > kMatrixLaQ && ko > 0 ? matrix_la_parts(ko * (act - kMatrixLaQ)) : 0;
}
// nplan, fplan, nwg, fwg and coff[0..Q] (the class offsets into fwg's pairs of
// entries) for `act` active segments, one workgroup on s
hipError_t launch_matrix_sp_la_plan(const int *rowptr, int *nplan, int *fplan, int4 *nwg, int4 *fwg, int *coff, int O,
                                    int act, hipStream_t s);
// the chunk's two launches (32 <= B <= 512)
hipError_t launch_matrix_sp_la_chunk(int log2b, const MatrixSpLaArgs &a, hipStream_t s);

// MatrixCrossfadeConvolver (matrix_xf.hip): one chunk of the two
// matrices A and B of a crossfaded handle while they are in step (equal
// {current, active, fill} at every call since creation, so X[0] and X[1], ib[0]
// and ib[1] are equal row for row).  [0] = convolver A, [1] = convolver B.
struct MatrixXfArgs {
    const float2 *H[2];    // [O][I][S][B] each
    float2 *X[2];          // [I][S][B] each; the chunk's row is written to both
    float *ovl[2];         // [O][B]
    float *ib[2];          // [I][B]; both maintained
    float2 *pre[2];        // [O][B]
    float2 *part[2];       // [O][P][B]
    const float2 *tw;      // W_N^k, k < N = 2B
    const float *in;       // chunk of input 0 (+ in_stride per input)
    long long in_stride;
    float *out;            // chunk of output 0 (+ out_stride per output)
    long long out_stride;
    int I, O, S;
    int P, rpp;            // as MatrixArgs
    int cur, act, fill, k;
    int nt_h;              // nontemporal H streams (Variant::nt_matrix of one H)
    int live;              // bit 0: A, bit 1: B -- an idle convolver (Crossfader Reached the other)
                           // keeps only its delay line: no MAC, no finish, no C2R
    int off;               // the chunk's offset in the call (mix sample index = off + j)
    CrossfadeMixArgs mix;  // the call's crossfader state; n = output_len, vtab = the device walk
                           // table while approaching (buf_a / buf_b unused)
    float *walk;           // the call's first chunk while approaching: mix.vtab, which one more
                           // workgroup of launch A fills (mix.n + 1 entries); null in every other chunk
};
// the chunk's two launches (32 <= B <= 8192)
hipError_t launch_matrix_xf_chunk(int log2b, const MatrixXfArgs &a, hipStream_t s);

// SparseMatrixCrossfadeConvolver (matrix_sp_xf.hip): one chunk of
// the two sparse matrices A and B of a crossfaded handle while they are in step
// -- MatrixXfArgs over the CSR pattern of MatrixSpArgs.  A and B have the same
// active_seg_count, so ONE plan serves both (A's).  [0] = A, [1] = B.
struct MatrixSpXfArgs {
    const float2 *H[2];    // [N][S][B] each
    float2 *X[2];          // [I][S][B] each; the chunk's row is written to both
    float *ovl[2];         // [O][B]
    float *ib[2];          // [I][B]; both maintained
    float2 *pre[2];        // [O][B]
    float2 *part[2];       // [sum P_o][B]
    const int *rowptr;     // as MatrixSpArgs
    const int *col;
    const int *plan;
    const int4 *wg;
    const float2 *tw;      // W_N^k, k < N = 2B
    const float *in;       // chunk of input 0 (+ in_stride per input)
    long long in_stride;
    float *out;            // chunk of output 0 (+ out_stride per output)
    long long out_stride;
    int I, O, S, N;
    int PT;                // plan[O]
    int cur, act, fill, k;
    int nt_h;              // nontemporal H streams (Variant::nt_matrix of one H)
    int live, off;         // as MatrixXfArgs
    CrossfadeMixArgs mix;
    float *walk;
};
// the chunk's two launches (32 <= B <= 8192)
hipError_t launch_matrix_sp_xf_chunk(int log2b, const MatrixSpXfArgs &a, hipStream_t s);

// MatrixLookaheadCrossfadeConvolver (matrix_la_xf.hip): one chunk of
// the two lookahead matrices A and B of a crossfaded handle while they are in
// step (MatrixXfArgs' condition, and equal block counts t) -- MatrixXfArgs with
// MatrixLaArgs' far-row windows, one set of windows and one tv per convolver.
// [0] = A, [1] = B.
struct MatrixLaXfArgs {
    const float2 *H[2];    // [O][I][S][B] each
    float2 *X[2];          // [I][S][B] each; the chunk's row is written to both
    float *ovl[2];         // [O][B]
    float *ib[2];          // [I][B]; both maintained
    float2 *pre[2];        // [O][B]
    float2 *part[2];       // [O][Pn][B] near partial sums
    float2 *far[2];        // [O][Pf][Q][B] far partial sums, window row = block % Q
    const float2 *tw;      // W_N^k, k < N = 2B
    const float *in;       // chunk of input 0 (+ in_stride per input)
    long long in_stride;
    float *out;            // chunk of output 0 (+ out_stride per output)
    long long out_stride;
    int I, O, S;
    int P, rpp;            // near parts and near rows per part, as MatrixLaArgs' m.P, m.rpp
    int Pf, rppf;          // as MatrixLaArgs (both convolvers have the same active_seg_count)
    int cur, act, fill, k;
    int nt_h;              // nontemporal H streams (Variant::nt_matrix of one H)
    int live, off;         // as MatrixXfArgs: an idle convolver makes no anchor and reads no window
    long long t;           // the block this chunk belongs to, the same for both convolvers
    long long tv[2];       // as MatrixLaArgs, per convolver (read for a live convolver only)
    CrossfadeMixArgs mix;
    float *walk;
};
// the far workgroups of launch A: per live convolver its far outputs x Pf
__host__ __device__ inline long long matrix_la_xf_far_groups(const MatrixLaXfArgs &a, int c) {
    return (a.live >> c) & 1 ? (long long)matrix_la_far_outputs(a.t, a.tv[c], a.O) * a.Pf : 0;
}
// the chunk's two launches (32 <= B <= 512)
hipError_t launch_matrix_la_xf_chunk(int log2b, const MatrixLaXfArgs &a, hipStream_t s);

// update_pairs (matrix_patch.hip): patch the spectra H of one matrix
// for listed pairs (pair = o * I + i) in one launch -- the pairs of `tr` are
// transformed from their response rows (the bits launch_ir_segments writes),
// the pairs of `cp` are copied, all S rows, from another matrix's spectra.  A
// pair is in at most one list.
constexpr int kMatrixPatchChunk = 32768;  // pairs per list and launch (as MatrixCore::ir_from_device)
struct MatrixPatchArgs {
    float2 *H;             // [O*I][S][B] the patched spectra
    const float2 *Hsrc;    // [O*I][S][B] the copy's source (unused when n_cp == 0)
    const float *src;      // response rows of the transform
    long long src_stride;  // floats between rows
    long long len_data;    // samples present in a row
    long long len_active;  // rows at or past ceil(len_active / B) are zeroed
    const float2 *tw;      // W_N^k, k < N = 2B
    const uint32_t *tr;    // [n_tr] pairs to transform
    const uint32_t *cp;    // [n_cp] pairs to copy
    int n_tr, n_cp;
    int row0;              // by_pair == 0: list entry n reads row row0 + n
    int by_pair;           // 1: list entry n reads row tr[n] (rows kept at the pairs' own positions)
    int S;
    int pairs;             // O * I
    int nt_cp;             // nontemporal loads of the copy (Variant::nt_matrix of one H)
    int gx, cpb;           // set by the launcher: transform / copy workgroups per pair
};
hipError_t launch_matrix_patch(int log2b, const MatrixPatchArgs &a, hipStream_t s);

// MatrixTwoStageConvolver (matrix_ts.hip): one aligned call -- a
// whole head block on a block boundary of the tail period -- of the head [0]
// and tail0 [1] matrices, which then have equal {current, active} and input
// buffer fill 0, and delay lines that are equal row for row.
struct MatrixTsArgs {
    const float2 *H[2];    // [O][I][S][B] each
    float2 *X[2];          // [I][S][B] each; the block's row is written to both
    float *ovl[2];         // [O][B]
    float2 *part[2];       // [O][P][B]
    const float2 *tw;      // W_N^k, k < N = 2B
    const float *in;       // the block of input 0 (+ in_stride per input)
    long long in_stride;
    float *out;            // the block of output 0 (+ out_stride per output)
    long long out_stride;
    float *tin;            // tail_input + tail_input_fill          (+ T per input)
    float *tout0;          // tail_output0 + tail_input_fill        (+ T per output)
    const float *p0;       // tail_precalculated0 + precalculated_pos (+ T per output)
    const float *p1;       // tail_precalculated + precalculated_pos, or null (no tail stage)
    long long T;
    int I, O, S;
    int P, rpp;            // as MatrixArgs
    int cur, act;
    int nt_h;              // nontemporal H streams (Variant::nt_matrix of one H)
};
// the call's two launches (32 <= B <= 8192)
hipError_t launch_matrix_ts_block(int log2b, const MatrixTsArgs &a, hipStream_t s);

// the two-stage matrix's sub-chunk on the composition path
// (src/fft_convolver.rs:438-461): out[o] = (out[o] + p0[o]) + p1[o] for every
// output, tail_input[i] <- in[i] for every input.
struct MatrixTsAccumArgs {
    float *out;
    long long out_stride;
    const float *p0;       // tail_precalculated0 [O][T], or null (no tail0 stage)
    const float *p1;       // tail_precalculated  [O][T], or null (no tail stage)
    long long T;
    int pos;               // precalculated_pos
    const float *in;
    long long in_stride;
    int sb;                // sub-chunk start within the call
    float *tail_input;     // [I][T]
    int fill;              // tail_input_fill before the append
    int cnt;               // samples in the sub-chunk
    int I, O;
};
hipError_t launch_matrix_ts_accum(const MatrixTsAccumArgs &a, hipStream_t s);

// SparseMatrixTwoStageConvolver (matrix_sp_ts.hip): one aligned
// call of the head [0] and tail0 [1] sparse matrices -- MatrixTsArgs over the
// CSR pattern of MatrixSpArgs.  Head and tail0 have the same pattern and, at an
// aligned call, the same active_seg_count, so ONE plan serves both (the head's).
struct MatrixSpTsArgs {
    const float2 *H[2];    // [N][S][B] each
    float2 *X[2];          // [I][S][B] each; the block's row is written to both
    float *ovl[2];         // [O][B]
    float2 *part[2];       // [sum P_o][B]
    const int *rowptr;     // as MatrixSpArgs
    const int *col;
    const int *plan;
    const int4 *wg;
    const float2 *tw;      // W_N^k, k < N = 2B
    const float *in;       // the block of input 0 (+ in_stride per input)
    long long in_stride;
    float *out;            // the block of output 0 (+ out_stride per output)
    long long out_stride;
    float *tin;            // as MatrixTsArgs
    float *tout0;
    const float *p0;
    const float *p1;
    long long T;
    int I, O, S, N;
    int PT;                // plan[O]
    int cur, act;
    int nt_h;              // nontemporal H streams (Variant::nt_matrix of one H)
};
// the call's two launches (32 <= B <= 8192)
hipError_t launch_matrix_sp_ts_block(int log2b, const MatrixSpTsArgs &a, hipStream_t s);

}  // namespace fftconv
