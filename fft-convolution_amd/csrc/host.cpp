// host.cpp -- C++ host side of the MI355X convolver and its C ABI (include/fftconv.h).
//
// The three reference types are mirrored as batches of device-resident
// channels:
//   UniformCore   <- FFTConvolver          (src/fft_convolver.rs:86-307)
//   TwoStageCore  <- TwoStageFFTConvolver  (src/fft_convolver.rs:323-512)
//   CrossfadeCore <- CrossfadeConvolver<FFTConvolver> (src/crossfade_convolver.rs:3-105)
// Per-channel block state lives on the device (the fused kernel advances it);
// the host only keeps what the reference keeps per *instance* and what all
// channels share in lockstep (two-stage fill/position, the crossfader).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/fftconv.h"
#include "block_walk.hpp"
#include "kernels.hpp"
#include "pair_book.hpp"

using namespace fftconv;

namespace {

thread_local std::string g_last_error;

void set_error(const std::string &m) { g_last_error = m; }

struct Status {
    int code = FFTCONV_OK;
    explicit operator bool() const { return code != FFTCONV_OK; }
};

int fail(int code, const std::string &m) {
    set_error(m);
    return code;
}

#define HIP_TRY(expr)                                                                    \
    do {                                                                                 \
        hipError_t e__ = (expr);                                                         \
        if (e__ != hipSuccess)                                                           \
            return fail(FFTCONV_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

size_t next_pow2(size_t v) {  // usize::next_power_of_two (0 -> 1)
    size_t p = 1;
    while (p < v) p <<= 1;
    return p;
}
int ilog2(size_t v) {
    int l = 0;
    while (((size_t)1 << l) < v) ++l;
    return l;
}
size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }  // == (a as f64 / b as f64).ceil()

// (tests: FFTCONV_POISON_ALLOC=1 fills every new buffer with 0xff bytes (NaN as
// float, -1 as an index), so a read of memory the path never wrote shows in the
// output instead of reading whatever the allocator recycled.  Every allocation
// of this file asks here: DevPtr, the shared twiddle / long-block / Bluestein
// tables, the public Fft's stream-ordered scratch and the pinned host stages.
// Read once per process; the first poisoned allocation says so on stderr, which
// is how tests/test_gpu_poison.py knows its child really ran poisoned.)
bool poison_alloc() {
    static const bool on = [] {
        const char *v = getenv("FFTCONV_POISON_ALLOC");
        const bool p = v && atoi(v) > 0;
        if (p) fputs("fftconv: FFTCONV_POISON_ALLOC on\n", stderr);
        return p;
    }();
    return on;
}
// a raw hipMalloc'd table, before its upload (which must cover all of it)
hipError_t poison_table(void *p, size_t bytes) {
    if (!poison_alloc()) return hipSuccess;
    const hipError_t e = hipMemset(p, 0xff, bytes);
    return e != hipSuccess ? e : hipDeviceSynchronize();
}

template <class T>
struct DevPtr {
    T *p = nullptr;
    size_t n = 0;
    DevPtr() = default;
    DevPtr(const DevPtr &) = delete;
    DevPtr &operator=(const DevPtr &) = delete;
    ~DevPtr() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    int alloc(size_t count) {
        reset();
        n = count;
        if (count == 0) return FFTCONV_OK;
        hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            n = 0;
            return fail(e == hipErrorOutOfMemory ? FFTCONV_E_NOMEM : FFTCONV_E_DEVICE,
                        std::string("hipMalloc: ") + hipGetErrorString(e));
        }
        if (poison_alloc()) {  // (done before any stream uses the buffer: null stream, then wait)
            if (hipMemset(p, 0xff, count * sizeof(T)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
                return fail(FFTCONV_E_DEVICE, "poison memset");
        }
        return FFTCONV_OK;
    }
    size_t bytes() const { return n * sizeof(T); }
};

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        (void)hipGetDevice(&prev);
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int now = -1;
        (void)hipGetDevice(&now);
        if (prev >= 0 && now != prev) (void)hipSetDevice(prev);
    }
};

int check_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(FFTCONV_E_DEVICE, "no HIP device available (the convolver has no CPU fallback)");
    if (device < 0 || device >= n) return fail(FFTCONV_E_DEVICE, "device index out of range");
    return FFTCONV_OK;
}

// Device scratch for the host-pointer entry points (grown on demand).
struct Scratch {
    DevPtr<float> in, out;
    int ensure(size_t nin, size_t nout) {
        if (in.n < nin) { if (int r = in.alloc(nin)) return r; }
        if (out.n < nout) { if (int r = out.alloc(nout)) return r; }
        return FFTCONV_OK;
    }
};

// Cross-stream ordering of one handle's work.  Asynchronous entry points take
// a caller stream; every call must still see the state the previous call left
// (the reference's calls are sequential on one instance).  `enter(s)` before
// enqueueing on s makes s wait for the stream of the handle's previous work
// when that was another stream (an event recorded there now -- so, as with a
// library handle's stream, a caller stream must stay valid until the handle's
// next call).  Host-synchronous entry points enter their own stream and wait
// for it alone: no device-wide synchronisation, so other handles' and other
// libraries' streams are never waited for.
struct StreamOrder {
    hipStream_t last = nullptr;
    bool any = false;
    hipEvent_t ev = nullptr;
    ~StreamOrder() {
        if (ev) (void)hipEventDestroy(ev);
    }
    int enter(hipStream_t s) {
        if (any && last != s) {
            if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(ev, last));
            HIP_TRY(hipStreamWaitEvent(s, ev, 0));
        }
        last = s;
        any = true;
        return FFTCONV_OK;
    }
    // every piece of the handle's work has finished, once `own` has drained
    int drain(hipStream_t own) {
        if (int r = enter(own)) return r;
        HIP_TRY(hipStreamSynchronize(own));
        return FFTCONV_OK;
    }
};

// Pinned host staging for host-memory IR uploads: update() copies the caller's
// response into it and returns once the H2D copy and the IR transform are
// enqueued (the next call on the handle is ordered behind them).  Reserved at
// init, so update() never allocates (src/lib.rs:8); `busy` guards its reuse.
// The reservation is capped by fftconv_set_host_stage_limit, and a failed one
// falls back to smaller sizes (down to one response row): then an
// update streams its rows through the stage in chunks, each chunk waiting for
// the previous one's copy out of it -- still no allocation, but the host
// waits for all but the last chunk's DMA.
static std::atomic<size_t> g_stage_limit{0};  // bytes, 0 = none (set / read from any thread)

struct PinnedStage {
    float *p = nullptr;
    size_t n = 0;
    hipEvent_t busy = nullptr;
    bool pending = false;
    PinnedStage() = default;
    PinnedStage(const PinnedStage &) = delete;
    PinnedStage &operator=(const PinnedStage &) = delete;
    ~PinnedStage() {
        if (busy) {
            if (pending) (void)hipEventSynchronize(busy);
            (void)hipEventDestroy(busy);
        }
        if (p) (void)hipHostFree(p);
    }
    // count floats wanted, at least min_count (one response row)
    int alloc(size_t count, size_t min_count) {
        if (count == 0) return FFTCONV_OK;
        min_count = std::max<size_t>(1, std::min(min_count, count));
        const size_t lim = g_stage_limit.load(std::memory_order_relaxed);
        if (lim) count = std::max(min_count, std::min(count, lim / sizeof(float)));
        hipError_t e = hipErrorOutOfMemory;
        for (;;) {
            e = hipHostMalloc((void **)&p, count * sizeof(float), hipHostMallocDefault);
            if (e == hipSuccess || count == min_count) break;
            (void)hipGetLastError();
            count = std::max(min_count, count / 4);
        }
        if (e != hipSuccess) {
            p = nullptr;
            return fail(FFTCONV_E_NOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
        }
        n = count;
        if (poison_alloc()) std::memset(p, 0xff, count * sizeof(float));
        HIP_TRY(hipEventCreateWithFlags(&busy, hipEventDisableTiming));
        return FFTCONV_OK;
    }
    // wait until the previous upload has left the buffer (normally long done)
    int acquire() {
        if (pending) HIP_TRY(hipEventSynchronize(busy));
        pending = false;
        return FFTCONV_OK;
    }
    int release(hipStream_t s) {  // after the H2D copy out of the buffer is enqueued on s
        HIP_TRY(hipEventRecord(busy, s));
        pending = true;
        return FFTCONV_OK;
    }
    // rows r of the caller's responses (src + r*stride, len floats each) to
    // device rows dst + r*dpitch, in as few chunks of whole rows as the stage
    // holds (one when it was reserved for the whole batch)
    int upload(const float *src, size_t rows, size_t len, size_t stride, float *dst, size_t dpitch, hipStream_t s) {
        if (len == 0 || rows == 0) return FFTCONV_OK;
        if (!p || n < len) return fail(FFTCONV_E_INVALID, "no host staging for this update");
        const size_t per = n / len;
        for (size_t r0 = 0; r0 < rows; r0 += per) {
            const size_t k = std::min(per, rows - r0);
            if (int r = acquire()) return r;
            for (size_t c = 0; c < k; ++c) std::memcpy(p + c * len, src + (r0 + c) * stride, len * sizeof(float));
            HIP_TRY(hipMemcpy2DAsync(dst + r0 * dpitch, dpitch * sizeof(float), p, len * sizeof(float),
                                     len * sizeof(float), k, hipMemcpyHostToDevice, s));
            if (int r = release(s)) return r;
        }
        return FFTCONV_OK;
    }
    // upload() with row r going to device row drow[r] (ascending): the rows are
    // staged once, one H2D copy per run of consecutive device rows
    int upload_scatter(const float *src, size_t rows, size_t len, size_t stride, float *dst, size_t dpitch,
                       const uint32_t *drow, hipStream_t s) {
        if (len == 0 || rows == 0) return FFTCONV_OK;
        if (!p || n < len) return fail(FFTCONV_E_INVALID, "no host staging for this update");
        const size_t per = n / len;
        for (size_t r0 = 0; r0 < rows; r0 += per) {
            const size_t k = std::min(per, rows - r0);
            if (int r = acquire()) return r;
            for (size_t c = 0; c < k; ++c) std::memcpy(p + c * len, src + (r0 + c) * stride, len * sizeof(float));
            for (size_t c0 = 0; c0 < k;) {
                size_t c1 = c0 + 1;
                while (c1 < k && drow[r0 + c1] == drow[r0 + c1 - 1] + 1) ++c1;
                HIP_TRY(hipMemcpy2DAsync(dst + (size_t)drow[r0 + c0] * dpitch, dpitch * sizeof(float), p + c0 * len,
                                         len * sizeof(float), len * sizeof(float), c1 - c0, hipMemcpyHostToDevice, s));
                c0 = c1;
            }
            if (int r = release(s)) return r;
        }
        return FFTCONV_OK;
    }
};

// The device pair lists of update_pairs (matrix_patch.hip) with their pinned
// host mirror, reserved at creation for O * I pairs each: [0, cap) the pairs to
// transform, [cap, 2 cap) the pairs to copy.  `busy` guards the mirror's reuse,
// as PinnedStage's.  `idx` is the host scratch of a call's validated list.
struct PairLists {
    DevPtr<uint32_t> d;
    uint32_t *h = nullptr;
    size_t cap = 0;
    hipEvent_t busy = nullptr;
    bool pending = false;
    std::vector<uint32_t> idx;
    PairLists() = default;
    PairLists(const PairLists &) = delete;
    PairLists &operator=(const PairLists &) = delete;
    ~PairLists() {
        if (busy) {
            if (pending) (void)hipEventSynchronize(busy);
            (void)hipEventDestroy(busy);
        }
        if (h) (void)hipHostFree(h);
    }
    int alloc(size_t pairs) {
        cap = pairs;
        if (pairs == 0) return FFTCONV_OK;
        idx.assign(pairs, 0);
        if (int r = d.alloc(2 * pairs)) return r;
        if (hipHostMalloc((void **)&h, 2 * pairs * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) {
            h = nullptr;
            return fail(FFTCONV_E_NOMEM, "hipHostMalloc: pair lists");
        }
        HIP_TRY(hipEventCreateWithFlags(&busy, hipEventDisableTiming));
        return FFTCONV_OK;
    }
    int acquire() {  // the previous call's lists have left the mirror (normally long done)
        if (pending) HIP_TRY(hipEventSynchronize(busy));
        pending = false;
        return FFTCONV_OK;
    }
    uint32_t *tr() { return h; }
    uint32_t *cp() { return h + cap; }
    int push(size_t n_tr, size_t n_cp, hipStream_t s) {
        if (n_tr) HIP_TRY(hipMemcpyAsync(d.p, h, n_tr * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        if (n_cp) HIP_TRY(hipMemcpyAsync(d.p + cap, h + cap, n_cp * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(busy, s));
        pending = true;
        return FFTCONV_OK;
    }
};

int pair_list_error(PairListError e) {
    return fail(FFTCONV_E_INVALID, e == PAIRS_RANGE ? "a pair index is out of range"
                                                    : "the pair list must be strictly ascending in (output, input)");
}

int lg_tables(int dev, int log2m, LgTab *out);

// What an owner adds to one UniformCore::process_device call (none by default)
struct StepOpts {
    // crossfade fusion on the lookahead step (ProcArgs::la_mix); the caller
    // only passes these when the call takes the lookahead launch
    int la_mix = 0;
    const CrossfadeMixArgs *mix = nullptr;
    float *mix_tab = nullptr;
    // recorded once the call's outputs are final, before the far-row window
    // anchor that follows a one-block step (the two-stage head reads the
    // tail's output, not its windows)
    hipEvent_t after_step = nullptr;
    bool narrow = false;  // 2048 <= B <= 8192: 256-thread step workgroups (ProcArgs::narrow)
    // a two-stage tail's one-block step: arrive on this signal with this
    // value (ProcArgs::sig, sig_mode 1); null = none
    unsigned *sig_arrive = nullptr;
    unsigned sig_arrive_val = 0;
};

// ---------------------------------------------------------------------------
// UniformCore -- a batch of FFTConvolver instances
// ---------------------------------------------------------------------------
struct UniformCore {
    int device = 0;
    size_t C = 0;         // channels
    size_t ir_len = 0;    // max_response_length (padded IR length)
    size_t B = 0;         // block_size.next_power_of_two()
    int log2b = 0;
    size_t S = 0;         // seg_count
    DevPtr<float2> H, X, pre, tw;
    DevPtr<float> overlap, inbuf, staging;
    DevPtr<int4> state;
    hipStream_t stream = nullptr;
    // an inner convolver (of a two-stage or a crossfade) runs on its owner's
    // stream: `parent_stream`, set before init / clone_from, is borrowed
    // instead of created, so a composite handle holds 2 HIP streams, not 5
    // (fewer streams sharing the process's hardware queues)
    hipStream_t parent_stream = nullptr;
    Scratch scratch;
    // host IR uploads (update_host), [C][ir_len]: only a standalone batch
    // owns one (own_stage, set before init).  A crossfade's a / b stage
    // through the crossfade's, and a two-stage's inner convolvers are never
    // updated (TwoStageFFTConvolver::update is todo!(), :408-410).
    PinnedStage hstage;
    bool own_stage = false;
    mutable StreamOrder order;     // (clone_from drains its source)
    // lookahead (la.hpp): standalone batches only (la_ok, set before init)
    bool la_ok = false;
    int la_W = 0;                 // far parts (partial rows per step), 0 = off
    DevPtr<float2> laW;           // windows of the three anchor levels [C][2][LA_PT][B]
    unsigned long long la_t = 0;  // lookahead launches so far (stagger clock)
    // launch timelines of the last `trace_slots` lookahead launches (tuning
    // only: FFTCONV_LA_TRACE=<slots>, written to FFTCONV_LA_TRACE_OUT at destroy)
    DevPtr<int4> trace;
    size_t trace_slots = 0, trace_grid = 0;
    std::vector<long long> trace_meta;  // per slot: la_t, grid
    int la_seq = 1;               // launch tag, alternating 1 / 2
    DevPtr<int> la_probe;         // (tests: FFTCONV_LA_PROBE) live words the anchors found rewritten
    // the anchors' copies of the state words [2][C] (ProcJob::sview / vnext):
    // copy la_seq & 1 is read by the next lookahead launch, the other filled
    // by its steps.  view_ok: that copy holds the current words -- true only
    // right after a lookahead launch; every other writer of the state words
    // (any launch built by job(), update, reset, init, clone) clears it, and
    // the next lookahead launch copies them first (la_view)
    DevPtr<int4> lav;
    mutable bool view_ok = false;
    bool la_all = true;           // next lookahead launch re-anchors every channel
    // the per-call batch of steps (la_batch.hpp): per channel the first step
    // its fix-up launch runs
    DevPtr<int> la_res;
    // long-block path (B > 2^kMaxLog2Fused, large.hip): per-call progress,
    // the inverse's scratch, the geometry's tables; lg_whole: every call
    // since init / reset was whole blocks, so every channel's buffer is empty
    // at a call's start (a failed C2R freezes fill at 0 then) and a call of
    // m blocks is exactly m chunks -- else one more chunk bounds any channel
    bool large = false;
    DevPtr<int4> lg_prog;
    DevPtr<float2> lg_v;
    LgTab lgt{};
    bool lg_whole = true;
    // far-row windows of the generic step (1024 <= B <= 8192):
    // standalone batches and the two-stage tail (gw_ok, set before init);
    // gw_p = the split row (0 = off), gwin = [C][P][B], gw_t = one-block
    // steps so far (the anchor class of the next one)
    bool gw_ok = false;
    int gw_p = 0;
    DevPtr<float2> gwin;
    unsigned long long gw_t = 0;

    ~UniformCore() {
        if (stream) {
            DeviceGuard g(device);
            (void)order.drain(stream);  // (work still queued on a caller stream reads these buffers)
            if (trace_slots) dump_trace();
            if (!parent_stream) (void)hipStreamDestroy(stream);
        }
    }

    void dump_trace() {
        static int dumps = 0;
        bool any = false;
        for (size_t k = 0; k < trace_slots; ++k) any = any || trace_meta[2 * k] >= 0;
        if (!any) return;
        std::vector<int4> h(trace.n);
        if (hipMemcpy(h.data(), trace.p, trace.bytes(), hipMemcpyDeviceToHost) != hipSuccess) return;
        const char *path = getenv("FFTCONV_LA_TRACE_OUT");
        const std::string fn = std::string(path ? path : "/tmp/la_trace.bin") + "." + std::to_string(dumps++);
        FILE *f = fopen(fn.c_str(), "wb");
        if (!f) return;
        const long long hdr[4] = {(long long)trace_slots, (long long)trace_grid, (long long)C, (long long)B};
        fwrite(hdr, sizeof(hdr), 1, f);
        fwrite(trace_meta.data(), sizeof(long long), trace_meta.size(), f);
        fwrite(h.data(), sizeof(int4), h.size(), f);
        fclose(f);
    }

    int alloc_geometry(int dev, size_t channels, size_t max_block_size, size_t max_len) {
        device = dev;
        C = channels;
        ir_len = max_len;
        B = next_pow2(max_block_size);                             // :115
        log2b = ilog2(B);
        if (log2b > kMaxLog2Block)
            return fail(FFTCONV_E_UNSUPPORTED, "block size " + std::to_string(B) + " exceeds 2^22");
        large = log2b > kMaxLog2Fused;
        S = ceil_div(ir_len, B);                                   // :117
        if (S * B > (size_t)INT32_MAX || C > (size_t)INT32_MAX)
            return fail(FFTCONV_E_UNSUPPORTED, "geometry exceeds 32-bit indexing");
        if (parent_stream) stream = parent_stream;
        else HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        if (int r = H.alloc(C * S * B)) return r;
        if (int r = X.alloc(C * S * B)) return r;
        if (int r = pre.alloc(C * B)) return r;
        if (int r = overlap.alloc(C * B)) return r;
        if (int r = inbuf.alloc(C * B)) return r;
        if (int r = state.alloc(C)) return r;
        if (int r = tw.alloc(2 * B)) return r;
        if (int r = staging.alloc(C * ir_len)) return r;  // update() never allocates
        if (own_stage)
            if (int r = hstage.alloc(C * ir_len, ir_len)) return r;
        if (large)
            if (int r = alloc_large()) return r;
        gw_p = gw_ok && gw_supported(log2b, (int)S) ? kGwP : 0;
        if (gw_p)
            if (int r = gwin.alloc(C * (size_t)gw_p * B)) return r;
        la_W = la_ok ? la_parts(log2b, (int)S) : 0;
        if (la_W) {
            const LaDims d = la_dims(log2b, (int)S);
            if (int r = laW.alloc(C * 2 * (size_t)d.pt * B)) return r;
            // (tests: FFTCONV_LA_POISON=1 fills the windows with NaN at init, so a
            // window row read before any anchor wrote it shows in the output)
            if (const char *e = getenv("FFTCONV_LA_POISON"); e && atoi(e) > 0)
                HIP_TRY(hipMemsetAsync(laW.p, 0xff, laW.bytes(), stream));
            if (int r = lav.alloc(2 * C)) return r;
            if (int r = la_res.alloc(C)) return r;
            view_ok = false;
            if (const char *e = getenv("FFTCONV_LA_PROBE"); e && atoi(e) > 0) {
                if (int r = la_probe.alloc(1)) return r;
                HIP_TRY(hipMemsetAsync(la_probe.p, 0, sizeof(int), stream));
            }
        }
        // launch timelines (tuning only): FFTCONV_LA_TRACE for the lookahead
        // launches of a batch that has them, FFTCONV_PROC_TRACE for the
        // process launches of one that has not (e.g. cfg3's head)
        if (const char *e = getenv(la_W ? "FFTCONV_LA_TRACE" : "FFTCONV_PROC_TRACE")) {
            trace_slots = (size_t)std::max(0, atoi(e));
            trace_grid = la_W ? (size_t)la_trace_grid(log2b, (int)S, (int)C) : C;
            if (trace_slots) {
                if (int r = trace.alloc(trace_slots * trace_grid * 8)) return r;
                HIP_TRY(hipMemsetAsync(trace.p, 0, trace.bytes(), stream));
                trace_meta.assign(2 * trace_slots, -1);
            }
        }
        // twiddles W_N^k in double, rounded to f32
        std::vector<float2> t(2 * B);
        const size_t N = 2 * B;
        for (size_t k = 0; k < N; ++k) {
            const double ang = -2.0 * M_PI * (double)k / (double)N;
            t[k] = make_float2((float)std::cos(ang), (float)std::sin(ang));
        }
        HIP_TRY(hipMemcpy(tw.p, t.data(), t.size() * sizeof(float2), hipMemcpyHostToDevice));
        return FFTCONV_OK;
    }

    // long-block path buffers (B > 2^kMaxLog2Fused); the tables are shared
    // per (device, geometry); W_N^k is the handle's own `tw`
    int alloc_large() {
        if (int r = lg_prog.alloc(C)) return r;
        if (C) HIP_TRY(hipMemsetAsync(lg_prog.p, 0, lg_prog.bytes(), stream));
        if (int r = lg_v.alloc(C * B)) return r;
        if (int r = lg_tables(device, log2b, &lgt)) return r;
        lgt.twN = tw.p;
        lg_whole = true;
        return FFTCONV_OK;
    }
    // chunks of an n-sample call, an upper bound over the channels
    int lg_chunks(size_t n) const {
        return (int)(lg_whole && n % B == 0 ? n / B : (n + B - 1) / B + 1);
    }
    void lg_note_call(size_t n) { lg_whole = lg_whole && n % B == 0; }

    // fresh state: zero FDL/overlap/buffers, {current 0, active S, fill 0}
    int zero_state() {
        if (X.n) HIP_TRY(hipMemsetAsync(X.p, 0, X.bytes(), stream));
        if (pre.n) HIP_TRY(hipMemsetAsync(pre.p, 0, pre.bytes(), stream));
        if (overlap.n) HIP_TRY(hipMemsetAsync(overlap.p, 0, overlap.bytes(), stream));
        if (inbuf.n) HIP_TRY(hipMemsetAsync(inbuf.p, 0, inbuf.bytes(), stream));
        std::vector<int4> st(C, make_int4(0, (int)S, 0, 0));
        if (C) HIP_TRY(hipMemcpyAsync(state.p, st.data(), C * sizeof(int4), hipMemcpyHostToDevice, stream));
        view_ok = false;
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }

    // run the IR partition FFT from device samples (channel c at src + c*stride)
    int ir_from_device(size_t chan0, size_t nch, const float *src, size_t stride, size_t len_data,
                       size_t len_active, bool update_state, hipStream_t s) {
        IrArgs a{};
        a.H = H.p; a.overlap = overlap.p; a.pre = pre.p; a.state = state.p;
        a.src = src; a.src_stride = (long long)stride;
        a.len_data = (long long)len_data; a.len_active = (long long)len_active;
        a.tw = tw.p; a.S = (int)S; a.chan0 = (int)chan0; a.update_state = update_state ? 1 : 0;
        if (update_state) view_ok = false;
        if (large) {
            HIP_TRY(launch_ir_large(log2b, a, lgt, (int)nch, s));
            return FFTCONV_OK;
        }
        HIP_TRY(launch_ir_segments(log2b, a, (int)nch, s));
        // the updated channels dropped their windows: rebuild them now, in
        // the update, so the next process launch stays a steady-state one
        if (update_state && !la_all) return la_rebuild(s, chan0, nch);
        return FFTCONV_OK;
    }

    // lookahead windows of channels [chan0, chan0+nch) from the current H and
    // FDL (launch_la_rebuild), as if anchored by the launch before the next
    // one; without the lookahead step (or with VARIANT_LAFULL) nothing to do
    int la_rebuild(hipStream_t s, size_t chan0, size_t nch) {
        if (!la_W || la_parts(log2b, (int)S) != la_W || Variant::current().has(VARIANT_LAFULL) || nch == 0)
            return FFTCONV_OK;
        const unsigned long long per = (unsigned long long)la_dims(log2b, (int)S).per_all;
        ProcArgs a{};
        a.job[0] = job(nullptr, 0, nullptr, 0, B);
        a.tw = tw.p;
        a.njobs = 1;
        a.laW = laW.p;
        a.la_c0 = (int)chan0;
        a.la_t = (int)((la_t + per - 1) % per);
        // a rebuild of every channel also fills the next lookahead launch's
        // copy of the state words (la_job then copies nothing)
        const bool whole = chan0 == 0 && nch == C && lav.p;
        if (whole) a.job[0].vnext = lav.p + (size_t)(la_seq & 1) * C;
        HIP_TRY(launch_la_rebuild(log2b, a, (int)(chan0 + nch), s));
        if (whole) view_ok = true;
        return FFTCONV_OK;
    }

    // upload host IRs (channel c at src + c*stride, len samples) into staging rows
    int upload(size_t chan0, size_t nch, const float *src, size_t len, size_t stride, hipStream_t s) {
        if (len == 0 || nch == 0) return FFTCONV_OK;
        float *dst = staging.p + chan0 * ir_len;
        if (stride == 0 || nch == 1) {
            HIP_TRY(hipMemcpyAsync(dst, src, len * sizeof(float), hipMemcpyHostToDevice, s));
        } else {
            HIP_TRY(hipMemcpy2DAsync(dst, ir_len * sizeof(float), src, stride * sizeof(float),
                                     len * sizeof(float), nch, hipMemcpyHostToDevice, s));
        }
        return FFTCONV_OK;
    }

    int init(int dev, size_t channels, const float *responses, size_t len, size_t stride, size_t max_block,
             size_t max_len) {
        if (max_len < len)                                          // :106-110
            return fail(FFTCONV_E_INVALID,
                        "max_response_length must be at least the length of the initial impulse response");
        if (int r = check_device(dev)) return r;
        DeviceGuard g(dev);
        if (int r = alloc_geometry(dev, channels, max_block, max_len)) return r;
        if (int r = zero_state()) return r;
        if (S > 0) {
            if (int r = upload(0, C, responses, len, stride == 0 ? 0 : stride, stream)) return r;
            // every channel reads its own staging row; a shared response reads row 0
            const size_t sst = (stride == 0 && C > 1) ? 0 : ir_len;
            if (int r = ir_from_device(0, C, staging.p, sst, len, ir_len, false, stream)) return r;
        }
        if (la_W && !Variant::current().has(VARIANT_LAFULL)) {  // the first process launch is a steady-state one too
            if (int r = la_rebuild(stream, 0, C)) return r;
            la_all = false;
        }
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }

    // FFTConvolver::update (:174-213) for channels [chan0, chan0+nch)
    int update_host(size_t chan0, size_t nch, const float *src, size_t len, size_t stride) {
        if (len > ir_len) return fail(FFTCONV_E_INVALID, "New impulse response is longer than initialized length");
        if (ir_len == 0) return FFTCONV_OK;                        // :181-183
        DeviceGuard g(device);
        // asynchronous: the response goes through the pinned stage; the copy
        // and the transform are enqueued behind the handle's previous work,
        // and every later call is ordered behind them (StreamOrder)
        if (int r = order.enter(stream)) return r;
        return update_host_on(chan0, nch, src, len, stride, stream, hstage);
    }
    // (the caller has ordered stream s behind the handle's previous work);
    // the response goes through `stage` into the staging rows
    int update_host_on(size_t chan0, size_t nch, const float *src, size_t len, size_t stride, hipStream_t s,
                       PinnedStage &stage) {
        if (len > ir_len) return fail(FFTCONV_E_INVALID, "New impulse response is longer than initialized length");
        if (ir_len == 0) return FFTCONV_OK;
        const bool shared = stride == 0 && nch > 1;  // one response for every channel: one staging row
        if (len && nch)
            if (int r = stage.upload(src, shared ? 1 : nch, len, stride, staging.p + chan0 * ir_len, ir_len, s)) return r;
        return ir_from_device(chan0, nch, staging.p + chan0 * ir_len, shared ? 0 : ir_len, len, len, true, s);
    }

    // update() from device samples, stream-ordered (used by the crossfade swap)
    int update_device(const float *src, size_t stride, size_t len, hipStream_t s) {
        if (len > ir_len) return fail(FFTCONV_E_INVALID, "New impulse response is longer than initialized length");
        if (ir_len == 0) return FFTCONV_OK;
        return ir_from_device(0, C, src, stride, len, len, true, s);
    }

    int reset(hipStream_t s) {  // :296-306
        if (X.n) HIP_TRY(hipMemsetAsync(X.p, 0, X.bytes(), s));
        if (overlap.n) HIP_TRY(hipMemsetAsync(overlap.p, 0, overlap.bytes(), s));
        if (inbuf.n) HIP_TRY(hipMemsetAsync(inbuf.p, 0, inbuf.bytes(), s));
        if (pre.n) HIP_TRY(hipMemsetAsync(pre.p, 0, pre.bytes(), s));
        HIP_TRY(launch_reset_state(state.p, (int)C, s));
        view_ok = false;
        lg_whole = true;
        if (la_W && !Variant::current().has(VARIANT_LAFULL)) {  // windows of the zeroed FDL, in the reset
            la_all = false;
            return la_rebuild(s, 0, C);
        }
        la_all = true;
        return FFTCONV_OK;
    }

    // a launch's job: any launch but a lookahead one may write the state
    // words, so the anchors' copy is stale after it (la_job for those)
    ProcJob job(const float *din, size_t is, float *dout, size_t os, size_t n) const {
        view_ok = false;
        return job_raw(din, is, dout, os, n);
    }
    ProcJob job_raw(const float *din, size_t is, float *dout, size_t os, size_t n) const {
        ProcJob j{};
        j.H = H.p; j.X = X.p; j.overlap = overlap.p; j.inbuf = inbuf.p; j.pre = pre.p; j.state = state.p;
        j.in = din; j.in_stride = (long long)is; j.out = dout; j.out_stride = (long long)os;
        j.S = (int)S; j.n = (int)n;
        j.lg_prog = lg_prog.p; j.lg_v = lg_v.p;
        return j;
    }
    // the long-block fields of a launch of this batch's n-sample call (the
    // call is counted: a launch failure after this leaves lg_whole pessimistic)
    void lg_fill(ProcArgs &a, size_t n) {
        if (!large) return;
        a.lg = lgt;
        a.lg_chunks = std::max(a.lg_chunks, lg_chunks(n));
        lg_note_call(n);
    }

    // a call of whole blocks takes the lookahead launch, one
    // launch per block
    bool la_ready(size_t n) const { return la_W && n > 0 && n % B == 0 && la_parts(log2b, (int)S) == la_W; }

    // this batch's lookahead fields of a launch: windows, stagger clock (the
    // launcher derives the anchor workgroups from them), and the timeline
    // record, when tracing
    int la_fill(ProcArgs &a, hipStream_t s) {
        a.laW = laW.p;
        a.la_all = la_all ? 1 : 0;
        a.la_t = (int)(la_t % (unsigned long long)la_dims(log2b, (int)S).per_all);  // (every period divides it)
        a.la_seq = la_seq;
        a.la_probe_cnt = la_probe.p;
        if (!la_all) return trace_fill(a, s);  // (steady-state launches only: the record is sized for them)
        return FFTCONV_OK;
    }
    // this launch's timeline record (slot = launch count mod trace_slots)
    int trace_fill(ProcArgs &a, hipStream_t s) {
        if (!trace_slots) return FFTCONV_OK;
        const size_t slot = (size_t)(la_t % trace_slots);
        a.la_trace = trace.p + slot * trace_grid * 8;
        a.la_trace_grid = (int)trace_grid;
        trace_meta[2 * slot] = (long long)la_t;
        trace_meta[2 * slot + 1] = -1;  // (grid: the analysis counts the records)
        HIP_TRY(hipMemsetAsync(a.la_trace, 0, trace_grid * 8 * sizeof(int4), s));
        return FFTCONV_OK;
    }
    void la_advance() {
        ++la_t;
        la_seq = 3 - la_seq;
        la_all = false;
    }
    // a lookahead launch's job: the anchors read copy la_seq & 1 of the state
    // words, the steps fill the other for the next launch (la.hpp
    // la_anchor_state); after any other writer the words are copied first
    int la_job(ProcJob &j, const float *din, size_t is, float *dout, size_t os, size_t n, hipStream_t s) {
        j = job_raw(din, is, dout, os, n);
        if (!lav.p) return fail(FFTCONV_E_DEVICE, "lookahead launch without the state copies");
        int4 *rd = lav.p + (size_t)(la_seq & 1) * C, *wr = lav.p + (size_t)((la_seq & 1) ^ 1) * C;
        if (!view_ok && C) HIP_TRY(hipMemcpyAsync(rd, state.p, C * sizeof(int4), hipMemcpyDeviceToDevice, s));
        view_ok = true;  // (the launch's steps fill `wr`; la_advance makes it the next read copy)
        j.sview = rd;
        j.vnext = wr;
        return FFTCONV_OK;
    }

    int process_device(const float *din, size_t is, float *dout, size_t os, size_t n, hipStream_t s,
                       const StepOpts &o = {}) {
        if (n > (size_t)INT32_MAX) return fail(FFTCONV_E_UNSUPPORTED, "process length exceeds 2^31-1");
        if (n == 0 || C == 0) return FFTCONV_OK;
        ProcArgs a{};
        a.job[0] = job_raw(din, is, dout, os, n);
        a.tw = tw.p;
        a.njobs = 1;
        if (la_ready(n)) {
            // lookahead launches, one per block of the call: the step
            // workgroups behind each launch's anchors (every channel on entry,
            // else the stagger classes (c - t) % period == 0).  A multi-block
            // call keeps the windows: each launch is the step of one block,
            // bit-identical to one call per block; a channel off the lookahead
            // path runs the whole call (:222-294) in the first launch
            const size_t m = n / B;
            if (m > 1 && o.la_mix) return fail(FFTCONV_E_INVALID, "crossfade lookahead launch of more than one block");
            for (size_t k = 0; k < m; ++k) {
                if (int r = la_job(a.job[0], din + k * B, is, dout + k * B, os, B, s)) return r;
                a.job[0].mcall = (int)m;
                a.job[0].mk = (int)k;
                if (int r = la_fill(a, s)) return r;
                if (o.la_mix && o.mix) {
                    a.la_mix = o.la_mix;
                    a.mix = *o.mix;
                    a.mix_tab = o.mix_tab;
                }
                HIP_TRY(launch_process_la(log2b, a, (int)C, s));
                la_advance();
            }
            if (o.after_step) HIP_TRY(hipEventRecord(o.after_step, s));
            return FFTCONV_OK;
        }
        if (la_W) la_all = true;  // this launch drops every window
        view_ok = false;          // (and writes the state words)
        if (trace_slots && !la_W && n == B) {  // (process timelines: one-block calls)
            if (int r = trace_fill(a, s)) return r;
            ++la_t;
        }
        lg_fill(a, n);
        a.narrow = o.narrow ? 1 : 0;
        a.gw_p = gw_p;  // (every launch: the split order)
        if (o.sig_arrive && n == B && !large) {
            a.sig = o.sig_arrive;
            a.sig_val = o.sig_arrive_val;
            a.sig_mode = 1;
        }
        if (gw_p && n == B && !Variant::current().has(VARIANT_NOGW)) {
            // a one-block step reads the live windows, then the channels of
            // class gw_t mod P anchor theirs for their next P blocks
            a.gw = gwin.p;
            a.gw_t = (int)(gw_t % (unsigned long long)gw_p);
            HIP_TRY(launch_process(log2b, a, (int)C, s));
            if (o.after_step) HIP_TRY(hipEventRecord(o.after_step, s));
            a.sig_mode = 0;  // (the anchor does not arrive)
            HIP_TRY(launch_gw_anchor(log2b, a, (int)C, s));
            ++gw_t;
            return FFTCONV_OK;
        }
        HIP_TRY(launch_process(log2b, a, (int)C, s));
        if (o.after_step) HIP_TRY(hipEventRecord(o.after_step, s));
        return FFTCONV_OK;
    }

    // `steps` one-block calls of a lookahead batch whose blocks are all at
    // hand: chunks of up to LA_BATCH_MAX steps, four launches each
    // (la_batch.hpp), the same bits as one launch per block.  Not for a
    // handle that is tracing or probing its per-block launches, nor under
    // VARIANT_NORUN (one launch per call) or VARIANT_LAFULL (the per-step
    // full pass, which tests compare against).  A chunk takes the window
    // buffer, so the per-block launch after it is an entry launch (la_all):
    // short calls stay per-block while the windows are live, and every call
    // takes the batch once they are dropped anyway.
    bool la_batch_ready(size_t n, size_t steps) const {
        const Variant v = Variant::current();
        return n == B && la_ready(n) && la_res.p && lav.p && !trace_slots && !la_probe.p &&
               !v.has(VARIANT_NORUN | VARIANT_LAFULL) && steps >= 1 && (steps >= (size_t)LA_BATCH_MIN || la_all);
    }
    int la_batch(const float *din, size_t is, size_t in_step, float *dout, size_t os, size_t out_step, size_t steps,
                 hipStream_t s) {
        for (size_t k0 = 0; k0 < steps; k0 += LA_BATCH_MAX) {
            const int k = (int)std::min<size_t>(LA_BATCH_MAX, steps - k0);
            ProcArgs a{};
            a.job[0] = job_raw(din + k0 * in_step, is, dout + k0 * out_step, os, B);
            a.tw = tw.p;
            a.njobs = 1;
            a.laW = laW.p;
            const LaBatchArgs b{(long long)in_step, (long long)out_step, k, la_seq, la_res.p};
            HIP_TRY(launch_la_batch(log2b, a, b, (int)C, s));
            // as k per-block launches leave the clocks; no window is live and
            // the anchors' copies of the state words are stale
            la_t += (unsigned long long)k;
            if (k & 1) la_seq = 3 - la_seq;
            la_all = true;
            view_ok = false;
        }
        return FFTCONV_OK;
    }

    // `steps` consecutive process() calls (fftconv_uniform_process_device_steps).
    // A batch on the generic / pipelined step (no lookahead, no far-row
    // windows, B <= 512) whose workgroups fit the chip twice over runs them
    // as ONE launch (upols_run_kernel: each channel loops over its calls,
    // process_job per call -- the same bits as one launch per call).
    int process_device_steps(const float *din, size_t is, size_t in_step, float *dout, size_t os, size_t out_step,
                             size_t n, size_t steps, hipStream_t s) {
        if (C && in_step <= (size_t)LLONG_MAX && out_step <= (size_t)LLONG_MAX && la_batch_ready(n, steps))
            return la_batch(din, is, in_step, dout, os, out_step, steps, s);
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) ncu = 0;
        if (steps >= 2 && n > 0 && n <= (size_t)INT32_MAX && !la_W && !large && !gw_p && !trace_slots &&
            C <= 2 * (size_t)ncu && steps <= (size_t)INT32_MAX && run_supported(log2b) &&
            in_step <= (size_t)LLONG_MAX && out_step <= (size_t)LLONG_MAX) {
            ProcArgs a{};
            a.job[0] = job(din, is, dout, os, n);
            a.tw = tw.p;
            a.njobs = 1;
            a.run_lds_rows = run_lds_rows(log2b, (int)S);
            RunSteps r{(long long)in_step, (long long)out_step, (int)steps};
            HIP_TRY(launch_process_run(log2b, a, r, (int)C, s));
            return FFTCONV_OK;
        }
        for (size_t k = 0; k < steps; ++k)
            if (int r = process_device(din + k * in_step, is, dout + k * out_step, os, n, s)) return r;
        return FFTCONV_OK;
    }

    int process_host(const float *in, size_t in_len, float *out, size_t out_len) {
        if (in_len < out_len) return fail(FFTCONV_E_INVALID, "input slice shorter than output (range end index out of range)");
        if (out_len == 0 || C == 0) return FFTCONV_OK;
        DeviceGuard g(device);
        if (int r = order.enter(stream)) return r;
        if (int r = scratch.ensure(C * out_len, C * out_len)) return r;
        HIP_TRY(hipMemcpy2DAsync(scratch.in.p, out_len * sizeof(float), in, in_len * sizeof(float),
                                 out_len * sizeof(float), C, hipMemcpyHostToDevice, stream));
        if (int r = process_device(scratch.in.p, out_len, scratch.out.p, out_len, out_len, stream)) return r;
        HIP_TRY(hipMemcpyAsync(out, scratch.out.p, C * out_len * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }

    // #[derive(Clone)]
    int clone_from(const UniformCore &o, bool with_stage = true) {
        DeviceGuard g(o.device);
        if (int r = o.order.drain(o.stream)) return r;
        device = o.device;
        C = o.C; ir_len = o.ir_len; B = o.B; log2b = o.log2b; S = o.S;
        if (parent_stream) stream = parent_stream;
        else HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        auto cp = [&](auto &dst, const auto &src) -> int {
            if (int r = dst.alloc(src.n)) return r;
            if (src.n) HIP_TRY(hipMemcpyAsync(dst.p, src.p, src.bytes(), hipMemcpyDeviceToDevice, stream));
            return FFTCONV_OK;
        };
        if (int r = cp(H, o.H)) return r;
        if (int r = cp(X, o.X)) return r;
        if (int r = cp(pre, o.pre)) return r;
        if (int r = cp(tw, o.tw)) return r;
        if (int r = cp(overlap, o.overlap)) return r;
        if (int r = cp(inbuf, o.inbuf)) return r;
        if (int r = cp(state, o.state)) return r;
        if (int r = cp(laW, o.laW)) return r;
        la_ok = o.la_ok; la_W = o.la_W; la_t = o.la_t; la_seq = o.la_seq; la_all = o.la_all;
        if (o.lav.n)
            if (int r = lav.alloc(o.lav.n)) return r;
        if (o.la_res.n)
            if (int r = la_res.alloc(o.la_res.n)) return r;
        view_ok = false;  // (copied from `state` before the clone's first lookahead launch)
        if (int r = cp(gwin, o.gwin)) return r;
        gw_ok = o.gw_ok; gw_p = o.gw_p; gw_t = o.gw_t;
        large = o.large;
        if (large) {  // (the progress words are zero between calls)
            if (int r = alloc_large()) return r;
            lg_whole = o.lg_whole;
        }
        if (o.trace_slots) {  // (tuning: a clone keeps its own timeline)
            trace_slots = o.trace_slots;
            trace_grid = o.trace_grid;
            if (int r = trace.alloc(trace_slots * trace_grid * 8)) return r;
            HIP_TRY(hipMemsetAsync(trace.p, 0, trace.bytes(), stream));
            trace_meta.assign(2 * trace_slots, -1);
        }
        if (int r = staging.alloc(o.staging.n)) return r;
        own_stage = with_stage && o.own_stage;
        if (own_stage)
            if (int r = hstage.alloc(o.hstage.n, ir_len)) return r;
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }

    // segments_ir[seg] of channel c as the reference holds it: B+1 bins,
    // interleaved (re, im), unpacked from the (DC, Nyquist) slot
    int ir_spectrum(size_t c, size_t seg, float *out) {
        if (c >= C || seg >= S) return fail(FFTCONV_E_INVALID, "channel or segment out of range");
        DeviceGuard g(device);
        if (int r = order.drain(stream)) return r;
        std::vector<float2> row(B);
        HIP_TRY(hipMemcpy(row.data(), H.p + (c * S + seg) * B, B * sizeof(float2), hipMemcpyDeviceToHost));
        out[0] = row[0].x;
        out[1] = 0.f;
        for (size_t k = 1; k < B; ++k) {
            const size_t p = large ? lg_position(log2b, k) : k;  // (long blocks: transposed bin order)
            out[2 * k] = row[p].x;
            out[2 * k + 1] = row[p].y;
        }
        out[2 * B] = row[0].y;
        out[2 * B + 1] = 0.f;
        return FFTCONV_OK;
    }

    int channel_state(size_t c, size_t out3[3]) {
        if (c >= C) return fail(FFTCONV_E_INVALID, "channel out of range");
        DeviceGuard g(device);
        if (int r = order.drain(stream)) return r;
        int4 st;
        HIP_TRY(hipMemcpy(&st, state.p + c, sizeof(int4), hipMemcpyDeviceToHost));
        out3[0] = (size_t)st.x; out3[1] = (size_t)st.y; out3[2] = (size_t)st.z;
        return FFTCONV_OK;
    }
};

// ---------------------------------------------------------------------------
// TailOrder -- the order between a two-stage's tail steps (side stream) and
// the head work that reads their output.
// The head of the period after a tail's period reads that tail's output.
// Instead of a barrier packet on the head's stream at every period end
// (hipStreamWaitEvent: ~7 us of cfg3's ~240 us period, r6p), the next run
// waits on the device (ProcArgs::sig): tail step k releases tsig[1] = k, and
// `pend` names the tail the next head work must follow (0 = none); every
// other path waits on that tail's event ev_tk[k & 1].
// ---------------------------------------------------------------------------
struct TailOrder {
    DevPtr<unsigned> tsig;  // {arrivals, last tail done, wait timeouts, -}
    // ev_main: the period's tail_input is complete (the tail may start);
    // ev_tk[k & 1]: tail k's step (its output, what the next period reads);
    // ev_tail_done: everything of the last tail, its window anchor included
    hipEvent_t ev_main = nullptr, ev_tk[2] = {nullptr, nullptr}, ev_tail_done = nullptr;
    bool tk_sig[2] = {false, false};  // tail k arrives on tsig
    unsigned tseq = 0, pend = 0;
    bool tail_in_flight = false;

    ~TailOrder() {
        for (hipEvent_t e : {ev_main, ev_tk[0], ev_tk[1], ev_tail_done})
            if (e) (void)hipEventDestroy(e);
    }

    // The events order kernels on this device only (no host wait reads what
    // they guard), so they carry no system-scope fence: with it, cfg3
    // one-launch-per-call periods ran at 21.5 us per call on one box (head
    // launches held for 456 us beside the tail), without it 6.6 us
    // (profiles/r6/r6b).
    int create(hipStream_t stream) {
        const unsigned evf = hipEventDisableTiming | hipEventDisableSystemFence;
        HIP_TRY(hipEventCreateWithFlags(&ev_main, evf));
        for (auto &e : ev_tk) HIP_TRY(hipEventCreateWithFlags(&e, evf));
        if (int r = tsig.alloc(4)) return r;
        HIP_TRY(hipMemsetAsync(tsig.p, 0, tsig.bytes(), stream));
        tseq = pend = 0;
        HIP_TRY(hipEventCreateWithFlags(&ev_tail_done, evf));
        return FFTCONV_OK;
    }

    // head work on stream s follows the pending tail: the event wait (every
    // path but a run)
    int follow(hipStream_t s) {
        if (pend) HIP_TRY(hipStreamWaitEvent(s, ev_tk[pend & 1], 0));
        pend = 0;
        return FFTCONV_OK;
    }
    // a run is about to launch on stream s: it waits for the pending tail on
    // the device when that tail arrives on tsig, else s takes the event wait
    int follow_in_run(ProcArgs &a, hipStream_t s) {
        if (pend && tk_sig[pend & 1]) {
            a.sig = tsig.p;
            a.sig_val = pend;
            a.sig_mode = 2;
            pend = 0;
            return FFTCONV_OK;
        }
        return follow(s);
    }

    // the period ended: the head work after this reads the tail in flight
    void period_ended() {
        if (tail_in_flight) pend = tseq;
    }

    // A tail step is about to be launched on stream ts, behind ev_main
    // (`recorded`: a kernel's completion on s records it, else a marker on s
    // here).  Fills the step's sequence number (never 0 = none), where it
    // arrives (`arrives`: on tsig, else on its event only) and the event
    // recorded after it.
    // (the next period waits for the tail's output only, not for its window
    // anchor: 19 us of cross-queue wait behind the anchor, r5p; starting the
    // tail before the flush gained nothing, r5s)
    int tail_begin(hipStream_t s, hipStream_t ts, bool recorded, bool arrives, StepOpts &o) {
        if (!recorded) HIP_TRY(hipEventRecord(ev_main, s));
        HIP_TRY(hipStreamWaitEvent(ts, ev_main, 0));
        const unsigned seq = tseq + 1 == 0 ? 1 : tseq + 1;
        o.sig_arrive = arrives ? tsig.p : nullptr;
        o.sig_arrive_val = seq;
        o.after_step = ev_tk[seq & 1];
        return FFTCONV_OK;
    }
    // that step (and its anchor) is enqueued on ts: commit what tail_begin handed out
    int tail_launched(hipStream_t ts, const StepOpts &o) {
        tk_sig[o.sig_arrive_val & 1] = o.sig_arrive != nullptr;
        tseq = o.sig_arrive_val;
        HIP_TRY(hipEventRecord(ev_tail_done, ts));
        tail_in_flight = true;
        return FFTCONV_OK;
    }

    // every tail has finished once `stream` has drained; a run that gave up
    // waiting for its tail (never expected) is an error
    int finish(hipStream_t stream) const {
        if (tail_in_flight) HIP_TRY(hipStreamWaitEvent(stream, ev_tail_done, 0));
        HIP_TRY(hipStreamSynchronize(stream));
        if (tsig.n) {
            unsigned to = 0;
            HIP_TRY(hipMemcpy(&to, tsig.p + 2, sizeof(unsigned), hipMemcpyDeviceToHost));
            if (to) return fail(FFTCONV_E_DEVICE, "a two-stage run timed out waiting for its tail step");
        }
        return FFTCONV_OK;
    }
    // (after finish: no tail to follow)
    void reset() {
        tail_in_flight = false;
        pend = 0;
    }
};

// ---------------------------------------------------------------------------
// TwoStageCore -- TwoStageFFTConvolver (src/fft_convolver.rs:323-512)
// ---------------------------------------------------------------------------
struct TwoStageCore {
    int device = 0;
    size_t C = 0, head_bs = 0, T = 0;
    std::unique_ptr<UniformCore> head, tail0, tail;  // null tail = Default (zeros)
    DevPtr<float> out0, pre0, out1, pre1;            // [C][T] each
    DevPtr<float> tin_buf[2];                        // tail_input, double-buffered per tail period
    int tin_idx = 0;
    float *tail_output0 = nullptr, *tail_precalculated0 = nullptr;
    float *tail_output = nullptr, *tail_precalculated = nullptr;
    size_t tail_input_fill = 0, precalculated_pos = 0;
    hipStream_t stream = nullptr;
    // The T-sized tail convolution runs on its own stream: its result is first
    // read one whole tail period later (after the next swap), which is the
    // reference's "might be done in some background thread" (:478).
    hipStream_t side = nullptr;
    TailOrder tord;  // which tail the next head work must follow, and how it waits
    // the tail's step on 256-thread workgroups, which fit beside the head's
    // (tests: FFTCONV_TAIL_NARROW=0 at creation for the 512-thread reference)
    bool tail_narrow = true;
    // the shortest run of calls taken as one launch: a one-call run (IR rows
    // and FDL loaded into LDS first) is slower than the per-call launch, 9.6 us
    // per cfg3 call against 7.1 (DESIGN.md "cfg3 per call", profiles/r6/r6g2)
    static constexpr size_t kRunMin = 2;
    // tail0 deferred to the end of its period (launch_tail0_flush): the
    // aligned calls' blocks [t0_off, t0_off + t0_n * head_bs) of tail_input
    // still to be convolved by tail_convolver0 (VARIANT_T0BLOCK: off, one
    // tail0 job per block)
    bool t0_defer = false;
    mutable size_t t0_off = 0, t0_n = 0;
    // pending blocks [0, t0_have) whose spectra a run already wrote to t0_xs
    mutable size_t t0_have = 0;
    size_t t0_nmax = 0;
    DevPtr<float2> t0_xs;
    DevPtr<float> t0_ys;
    DevPtr<int> t0_err;
    DevPtr<float> t0_ov;
    DevPtr<float2> t0_cv;
    // [C]: a run's call of this channel wrote no spectrum to t0_xs (its head
    // buffer out of step with tail_input); the flush recomputes and clears it
    DevPtr<int> t0_miss;
    DevPtr<int> t0_trace;  // (tuning, FFTCONV_T0_TRACE: the fused flush's phase stamps, [C][8], last flush)
    Scratch scratch;
    mutable StreamOrder order;

    ~TwoStageCore() {
        DeviceGuard g(device);
        if (t0_trace.n) {  // (FFTCONV_T0_TRACE: per-phase medians of the last flush, us)
            (void)hipDeviceSynchronize();
            std::vector<int> h(t0_trace.n);
            if (hipMemcpy(h.data(), t0_trace.p, t0_trace.bytes(), hipMemcpyDeviceToHost) == hipSuccess) {
                std::vector<double> ph[5];
                for (size_t c = 0; c < C; ++c)
                    for (int k = 0; k < 5; ++k) ph[k].push_back((double)(unsigned)(h[c * 8 + k + 1] - h[c * 8]) / 100.0);
                fprintf(stderr, "t0 flush phases (us from the workgroup's start, median over channels):");
                for (auto &v : ph) {
                    std::sort(v.begin(), v.end());
                    fprintf(stderr, " %.2f", v[v.size() / 2]);
                }
                fprintf(stderr, "\n");
            }
        }
        if (side) { (void)hipStreamSynchronize(side); (void)hipStreamDestroy(side); }
        if (stream) (void)order.drain(stream);
        head.reset(); tail0.reset(); tail.reset();  // (they borrow `stream`)
        if (stream) (void)hipStreamDestroy(stream);
    }

    float *tail_input() const { return tin_buf[tin_idx].p; }

    // every piece of the handle's work has finished: the caller-stream work
    // (StreamOrder) and the tail convolution on the side stream
    int quiesce() const {
        if (int r = order.enter(stream)) return r;
        return tord.finish(stream);
    }

    // The side stream is unmasked: the tail's step runs on 256-thread
    // workgroups that fit beside the head's.  Confined to the tail's byte
    // share of the CUs (a CU-masked stream), it held one handle's
    // one-launch-per-call head launches for 456 us at a time, 21.5-22.9 us per
    // cfg3 call against 7.55 unmasked (profiles/r6/r6b, r6c), and a long-block
    // tail's row pass ran at a fraction of the chip's bandwidth (head 512 /
    // IR 200,000: 59.6 us per step on 32 CUs, 21.4 unmasked;
    // profiles/r5/r5d_lgt_tail_units.log).
    // It has the device's highest stream priority: HIP maps streams onto at
    // most GPU_MAX_HW_QUEUES (4) hardware queues, and a normal-priority side
    // stream that shared its queue with the head's caller stream serialised
    // the tail behind the head (the third cfg3 handle of a process ran at
    // 5.1 us per call against 3.8); high-priority streams get queues of their
    // own (three handles 3.75 / 3.75 / 3.75 us, profiles/r6/r6m).
    int create_side_stream() {
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(hipStreamCreateWithPriority(&side, hipStreamNonBlocking, greatest));
        return FFTCONV_OK;
    }

    int alloc_buffers() {
        if (const char *e = getenv("FFTCONV_TAIL_NARROW")) tail_narrow = atoi(e) != 0;
        if (int r = create_side_stream()) return r;
        if (int r = tord.create(stream)) return r;
        for (auto *b : {&out0, &pre0, &out1, &pre1, &tin_buf[0], &tin_buf[1]}) {
            if (int r = b->alloc(C * T)) return r;
            if (b->n) HIP_TRY(hipMemsetAsync(b->p, 0, b->bytes(), stream));
        }
        tail_output0 = out0.p; tail_precalculated0 = pre0.p;
        tail_output = out1.p; tail_precalculated = pre1.p;
        tin_idx = 0;
        const bool defer = !Variant::current().has(VARIANT_T0BLOCK);  // (per-block tail0: tests)
        t0_nmax = T / std::max<size_t>(head_bs, 1);
        t0_defer = defer && tail0 && tail0->B == head_bs &&
                   tail0_defer_supported(tail0->log2b, (int)tail0->S, (int)t0_nmax);
        if (t0_defer) {
            if (int r = t0_xs.alloc(C * t0_nmax * head_bs)) return r;
            if (int r = t0_ys.alloc(C * t0_nmax * 2 * head_bs)) return r;
            if (int r = t0_err.alloc(C)) return r;
            if (int r = t0_ov.alloc(C * head_bs)) return r;
            if (int r = t0_cv.alloc(C * t0_nmax * head_bs)) return r;
            if (int r = t0_miss.alloc(C)) return r;
            if (getenv("FFTCONV_T0_TRACE"))
                if (int r = t0_trace.alloc(C * 16)) return r;  // (C x 4 int4: the replay's proc_stamp too)
            HIP_TRY(hipMemsetAsync(t0_err.p, 0, t0_err.bytes(), stream));
            if (t0_miss.n) HIP_TRY(hipMemsetAsync(t0_miss.p, 0, t0_miss.bytes(), stream));
        }
        t0_off = t0_n = t0_have = 0;
        return FFTCONV_OK;
    }

    // tail_convolver0.process (:464-472) of the deferred blocks, in one pass
    int flush_t0(hipStream_t s, hipEvent_t done = nullptr) const {
        if (t0_n == 0) return FFTCONV_OK;
        Tail0Args a{};
        a.pa.job[0] = tail0->job(tail_input() + t0_off, T, tail_output0 + t0_off, T, head_bs);
        a.pa.tw = tail0->tw.p;
        a.pa.njobs = 1;
        a.xs = t0_xs.p; a.ys = t0_ys.p; a.err = t0_err.p; a.ov0 = t0_ov.p; a.cv = t0_cv.p;
        a.act = (int)tail0->S;
        a.n = (int)t0_n; a.nmax = (int)t0_nmax;
        a.k0 = (int)std::min(t0_have, t0_n);
        a.miss = t0_miss.p;
        if (t0_trace.n) a.pa.la_trace = reinterpret_cast<int4 *>(t0_trace.p);  // (FFTCONV_T0_TRACE)
        HIP_TRY(launch_tail0_flush(tail0->log2b, a, (int)C, s, done));
        t0_n = t0_have = 0;  // (only once the flush is enqueued: a failed launch keeps the blocks pending)
        return FFTCONV_OK;
    }

    int init(int dev, size_t channels, const float *responses, size_t len, size_t stride, size_t block_size,
             size_t max_len) {
        head_bs = block_size;                                                   // :341
        T = fftconv_compute_tail_block_size(block_size, max_len);              // :342
        if (max_len < len)                                                      // :344-348
            return fail(FFTCONV_E_INVALID,
                        "max_response_length must be at least the length of the initial impulse response");
        if (int r = check_device(dev)) return r;
        if (ilog2(T) > kMaxLog2Block)
            return fail(FFTCONV_E_UNSUPPORTED, "tail block size " + std::to_string(T) + " exceeds 2^22");
        device = dev;
        C = channels;
        DeviceGuard g(dev);
        HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        // padded_ir = response zero-extended to max_len (:349-350); sub-ranges
        // are cut on the host so each stage sees exactly its reference slice
        const size_t sstride = stride == 0 ? 0 : stride;
        auto slice = [&](size_t off, size_t cnt, std::vector<float> &buf) -> size_t {
            const size_t rows = (sstride == 0) ? 1 : C;
            buf.assign(rows * std::max<size_t>(cnt, 1), 0.f);
            for (size_t c = 0; c < rows; ++c)
                for (size_t j = 0; j < cnt; ++j) {
                    const size_t p = off + j;
                    buf[c * cnt + j] = p < len ? responses[c * sstride + p] : 0.f;
                }
            return sstride == 0 ? 0 : cnt;
        };
        std::vector<float> tmp;
        const size_t head_ir_len = std::min(max_len, T);                        // :352-354
        head.reset(new (std::nothrow) UniformCore());
        if (!head) return fail(FFTCONV_E_NOMEM, "out of host memory");
        head->parent_stream = stream;
        size_t st = slice(0, head_ir_len, tmp);
        if (int r = head->init(dev, C, tmp.data(), head_ir_len, st, head_bs, head_ir_len)) return r;
        if (max_len > T) {                                                      // :356-368
            const size_t tl = std::min(max_len - T, T);
            tail0.reset(new (std::nothrow) UniformCore());
            if (!tail0) return fail(FFTCONV_E_NOMEM, "out of host memory");
            tail0->parent_stream = stream;
            st = slice(T, tl, tmp);
            if (int r = tail0->init(dev, C, tmp.data(), tl, st, head_bs, tl)) return r;
        }
        if (max_len > 2 * T) {                                                  // :373-384
            const size_t tl = max_len - 2 * T;
            tail.reset(new (std::nothrow) UniformCore());
            if (!tail) return fail(FFTCONV_E_NOMEM, "out of host memory");
            tail->parent_stream = stream;
            tail->gw_ok = true;  // one full-block call per period: far-row windows
            st = slice(2 * T, tl, tmp);
            if (int r = tail->init(dev, C, tmp.data(), tl, st, T, tl)) return r;
        }
        if (int r = alloc_buffers()) return r;
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }

    // fill reached T (:464-491): swap the tail0 buffers, swap the tail buffers,
    // and start the tail convolution of this period on the side stream.
    // (Starting the tail before the flush, beside it, was slower: 8.17 vs
    // 7.62 us per cfg3 step, profiles/r4/r4u_ab_cfg3_tail_early_rejected.log.)
    int end_of_period(hipStream_t s) {
        // ev_main (the tail may start) recorded by the flush kernel's own
        // completion (hipExtLaunchKernel) instead of a marker packet after it
        // (cfg3 A/B 3.669 -> 3.645 us per call, r6p)
        const bool ev_on_flush = t0_n > 0 && tail;
        if (int r = flush_t0(s, ev_on_flush ? tord.ev_main : nullptr)) return r;  // (tail_output0 is complete before the swap)
        std::swap(tail_precalculated0, tail_output0);                         // :473-475
        std::swap(tail_precalculated, tail_output);                           // :483
        // work after this point reads the swapped-in tail_precalculated: it is
        // the previous period's tail result, which the next head work waits for
        if (int r = tord.follow(s)) return r;  // (a period of one call: the previous one's)
        tord.period_ended();
        if (tail) {  // :484-485
            StepOpts o;
            o.narrow = tail_narrow && !tail->large;
            // (a long-block tail's passes do not arrive on the signal words)
            if (int r = tord.tail_begin(s, side, ev_on_flush, !tail->large, o)) return r;
            if (int r = tail->process_device(tail_input(), T, tail_output, T, T, side, o)) return r;
            if (int r = tord.tail_launched(side, o)) return r;
        }
        tin_idx ^= 1;  // the next period fills the other buffer while the tail reads this one
        tail_input_fill = 0;                                                   // :488-491
        precalculated_pos = 0;
        return FFTCONV_OK;
    }

    // An aligned call: a whole head block on a block boundary of the period
    // (one sub-chunk, and tail0 consumes exactly this block), with the
    // sub-chunk epilogue fused into the head's launch.
    bool aligned(size_t len) const {
        return len == head_bs && tail_input_fill % head_bs == 0 && tail_input_fill + len <= T &&
               head->log2b <= kMaxLog2Fused;
    }
    // the head launch of an aligned call (the first of a run's calls)
    ProcArgs aligned_args(const float *din, size_t is, float *dout, size_t os) const {
        ProcArgs a{};
        a.job[0] = head->job(din, is, dout, os, head_bs);                   // :417
        a.job[0].add0 = tail_precalculated0 + precalculated_pos;            // :439-445
        a.job[0].add1 = tail_precalculated + precalculated_pos;             // :448-454
        a.job[0].add_stride = (long long)T;
        a.job[0].tin = tail_input() + tail_input_fill;                     // :459-461
        a.job[0].tin_stride = (long long)T;
        a.njobs = 1;
        a.tw = head->tw.p;
        return a;
    }
    // (FFTCONV_PROC_TRACE timelines: a per-call launch, a run's last call per wave)
    int aligned_trace(ProcArgs &a, hipStream_t s) {
        if (!head->trace_slots || head->la_W) return FFTCONV_OK;
        if (int r = head->trace_fill(a, s)) return r;
        ++head->la_t;
        return FFTCONV_OK;
    }
    // the head launch of n aligned calls is enqueued (it writes their
    // tail_input, so tail0's deferred blocks are counted only now, :464-472);
    // a run that ends the period ends it as a per-call aligned call does
    int aligned_done(size_t n, hipStream_t s) {
        if (tail0 && t0_defer) {
            if (t0_n == 0) t0_off = tail_input_fill;
            t0_n += n;
        }
        precalculated_pos += n * head_bs;
        tail_input_fill += n * head_bs;
        if (tail_input_fill == T) return end_of_period(s);
        return FFTCONV_OK;
    }

    // TwoStageFFTConvolver::process (:412-495)
    int process_device(const float *din, size_t is, float *dout, size_t os, size_t len, hipStream_t s) {
        if (len > head_bs) return fail(FFTCONV_E_INVALID, "assertion failed: input.len() <= self.head_block_size");
        if (len == 0 || C == 0) return FFTCONV_OK;
        if (int r = tord.follow(s)) return r;
        if (aligned(len)) {
            // One launch: head (+ the sub-chunk epilogue) and tail0 as two jobs.
            ProcArgs a = aligned_args(din, is, dout, os);
            if (tail0 && !t0_defer) {                                           // :464-472
                a.job[1] = tail0->job(din, is, tail_output0 + tail_input_fill, T, head_bs);
                a.njobs = 2;
            }
            if (int r = aligned_trace(a, s)) return r;
            HIP_TRY(launch_process(head->log2b, a, (int)C, s));
            return aligned_done(1, s);
        }
        if (int r = flush_t0(s)) return r;  // (the sub-chunk loop runs tail0 per block)
        if (int r = head->process_device(din, is, dout, os, len, s)) return r;   // :417
        size_t processed = 0;
        while (processed < len) {                                                 // :427
            const size_t processing = std::min(len - processed, head_bs - (tail_input_fill % head_bs));
            if (tail_input_fill + processing > T)  // tail_input[fill..fill+processing] out of range (:459-460)
                return fail(FFTCONV_E_INVALID, "range end index out of range for slice of length tail_block_size");
            TwoStageAccumArgs a{};
            a.out = dout; a.out_stride = (long long)os;
            a.p0 = tail_precalculated0; a.p1 = tail_precalculated; a.T = (long long)T;
            a.pos = (int)precalculated_pos; a.in = din; a.in_stride = (long long)is;
            a.sb = (int)processed; a.tail_input = tail_input(); a.fill = (int)tail_input_fill;
            a.cnt = (int)processing;
            HIP_TRY(launch_twostage_accum(a, (int)C, s));                        // :438-461
            precalculated_pos += processing;
            tail_input_fill += processing;
            if (tail_input_fill % head_bs == 0 && tail0) {                        // :464-472
                const size_t off = tail_input_fill - head_bs;
                if (int r = tail0->process_device(tail_input() + off, T, tail_output0 + off, T, head_bs, s)) return r;
            }
            if (tail_input_fill == T) {
                if (int r = end_of_period(s)) return r;
            }
            processed += processing;
        }
        return FFTCONV_OK;
    }

    // `steps` consecutive process() calls (fftconv_twostage_process_device_steps).
    // Aligned head-block calls inside one tail period, with tail0 deferred,
    // run as ONE launch (upols_run_kernel: each channel loops over the calls,
    // process_job per call -- the same bits as one launch per call); the
    // period's end and every other call shape go through process_device.
    int process_device_steps(const float *din, size_t is, size_t in_step, float *dout, size_t os, size_t out_step,
                             size_t len, size_t steps, hipStream_t s) {
        size_t k = 0;
        while (k < steps) {
            const size_t left = aligned(len) ? (T - tail_input_fill) / head_bs : 0;
            const size_t nrun = std::min(steps - k, left);
            if (nrun >= kRunMin && t0_defer && tail0 && run_supported(head->log2b) &&
                nrun <= (size_t)INT32_MAX && in_step <= (size_t)LLONG_MAX && out_step <= (size_t)LLONG_MAX) {
                ProcArgs a = aligned_args(din + k * in_step, is, dout + k * out_step, os);
                // the run's block spectra double as tail0's pending-block
                // spectra while every pending block so far has one
                const bool t0spec = t0_have == t0_n && t0_n + nrun <= t0_nmax;
                if (t0spec) {
                    a.job[0].t0x = t0_xs.p + t0_n * head_bs;
                    a.job[0].t0x_stride = (long long)(t0_nmax * head_bs);
                    a.job[0].t0m = t0_miss.p;  // (a call that cannot write its spectrum flags the channel)
                }
                a.run_lds_rows = run_lds_rows(head->log2b, (int)head->S);
                if (int r = tord.follow_in_run(a, s)) return r;
                if (int r = aligned_trace(a, s)) return r;
                RunSteps r{(long long)in_step, (long long)out_step, (int)nrun};
                HIP_TRY(launch_process_run(head->log2b, a, r, (int)C, s));
                if (t0spec) t0_have += nrun;
                if (int r = aligned_done(nrun, s)) return r;
                k += nrun;
                continue;
            }
            if (int r = process_device(din + k * in_step, is, dout + k * out_step, os, len, s)) return r;
            ++k;
        }
        return FFTCONV_OK;
    }

    int process_host(const float *in, float *out, size_t len) {
        if (len > head_bs) return fail(FFTCONV_E_INVALID, "assertion failed: input.len() <= self.head_block_size");
        if (len == 0 || C == 0) return FFTCONV_OK;
        DeviceGuard g(device);
        if (int r = order.enter(stream)) return r;
        if (int r = scratch.ensure(C * len, C * len)) return r;
        HIP_TRY(hipMemcpyAsync(scratch.in.p, in, C * len * sizeof(float), hipMemcpyHostToDevice, stream));
        if (int r = process_device(scratch.in.p, len, scratch.out.p, len, len, stream)) return r;
        HIP_TRY(hipMemcpyAsync(out, scratch.out.p, C * len * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }

    int reset() {  // :497-511
        DeviceGuard g(device);
        if (int r = quiesce()) return r;
        if (int r = head->reset(stream)) return r;
        if (tail0) { if (int r = tail0->reset(stream)) return r; }
        if (tail) { if (int r = tail->reset(stream)) return r; }
        for (auto *b : {&out0, &pre0, &out1, &pre1, &tin_buf[0], &tin_buf[1]})
            if (b->n) HIP_TRY(hipMemsetAsync(b->p, 0, b->bytes(), stream));
        tail_input_fill = 0;
        precalculated_pos = 0;
        tord.reset();  // (quiesce waited for every tail)
        t0_n = t0_have = 0;  // (the deferred blocks' state is reset with everything else)
        if (t0_miss.n) HIP_TRY(hipMemsetAsync(t0_miss.p, 0, t0_miss.bytes(), stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }

    int clone_from(const TwoStageCore &o) {
        DeviceGuard g(o.device);
        if (int r = o.quiesce()) return r;
        if (o.t0_n) {  // the source's deferred tail0 blocks first: the copy starts with none
            if (int r = o.flush_t0(o.stream)) return r;
            HIP_TRY(hipStreamSynchronize(o.stream));
        }
        device = o.device; C = o.C; head_bs = o.head_bs; T = o.T;
        HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        auto cl = [&](std::unique_ptr<UniformCore> &dst, const std::unique_ptr<UniformCore> &src) -> int {
            if (!src) return FFTCONV_OK;
            dst.reset(new (std::nothrow) UniformCore());
            if (!dst) return fail(FFTCONV_E_NOMEM, "out of host memory");
            dst->parent_stream = stream;
            return dst->clone_from(*src);
        };
        if (int r = cl(head, o.head)) return r;
        if (int r = cl(tail0, o.tail0)) return r;
        if (int r = cl(tail, o.tail)) return r;
        if (int r = alloc_buffers()) return r;
        auto map = [&](const float *p) -> float * {  // same role, this instance's buffer
            if (p == o.out0.p) return out0.p;
            if (p == o.pre0.p) return pre0.p;
            if (p == o.out1.p) return out1.p;
            return pre1.p;
        };
        tail_output0 = map(o.tail_output0); tail_precalculated0 = map(o.tail_precalculated0);
        tail_output = map(o.tail_output); tail_precalculated = map(o.tail_precalculated);
        tin_idx = o.tin_idx;
        const std::pair<DevPtr<float> *, const DevPtr<float> *> pairs[] = {
            {&out0, &o.out0}, {&pre0, &o.pre0}, {&out1, &o.out1}, {&pre1, &o.pre1},
            {&tin_buf[0], &o.tin_buf[0]}, {&tin_buf[1], &o.tin_buf[1]}};
        for (auto &pr : pairs)
            if (pr.second->n)
                HIP_TRY(hipMemcpyAsync(pr.first->p, pr.second->p, pr.second->bytes(), hipMemcpyDeviceToDevice, stream));
        tail_input_fill = o.tail_input_fill;
        precalculated_pos = o.precalculated_pos;
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }
};

// ---------------------------------------------------------------------------
// Crossfader<RaisedCosineMixer> host state (src/crossfade_convolver.rs:192-279);
// the per-sample gains are evaluated on the device by crossfade_mix_kernel.
// ---------------------------------------------------------------------------
struct Crossfader {
    int64_t fading_samples = 0, hold_samples = 0, counter = 0;
    float mix_value_step = 0.f, mix_value = 0.f;
    bool approaching = false;
    int target = 0;  // 0 = A, 1 = B

    void init(size_t fading, size_t hold) {  // :204-214
        fading_samples = (int64_t)fading;
        hold_samples = (int64_t)hold;
        counter = 0;
        mix_value_step = 1.0f / (float)fading;
        mix_value = 0.f;
        approaching = false;
        target = 0;
    }
    void fade_into(int t) {  // :216-240
        if (target == t) return;
        if (!approaching) {
            counter = -hold_samples;
            approaching = true;
            target = t;
            mix_value_step = -mix_value_step;
        } else if (counter >= 0) {
            counter = fading_samples - counter;
            target = t;
            mix_value_step = -mix_value_step;
        } else {
            approaching = false;
            target = t;
        }
    }
    // advance the state machine over n samples exactly as n calls of mix() (:242-278)
    void advance(size_t n) {
        for (size_t i = 0; i < n && approaching; ++i) {
            counter += 1;
            if (counter <= 0) continue;
            volatile float v = mix_value + mix_value_step;  // one f32 rounding per step
            mix_value = v;
            if (counter == fading_samples) {
                approaching = false;
                mix_value = target == 0 ? 0.0f : 1.0f;
            }
        }
    }
};

// ---------------------------------------------------------------------------
// CrossfadeCore -- CrossfadeConvolver<FFTConvolver> (src/crossfade_convolver.rs:3-105)
// ---------------------------------------------------------------------------
struct CrossfadeCore {
    int device = 0;
    size_t C = 0, max_buffer_size = 0, stored_len = 0, stored_stride = 0;
    size_t stage_row = 0;  // hstage row: the stored response, or a direct update of a / b
    std::unique_ptr<UniformCore> a, b;
    Crossfader xf;
    DevPtr<float> buf_a, buf_b, stored;
    DevPtr<float> mix_tab;  // [max_buffer_size + 1] mix_value walk (lookahead-fused mix)
    bool response_pending = false;
    hipStream_t stream = nullptr;
    Scratch scratch;
    // crossfade pair launch (one FDL stream for A and B): allowed while A and B
    // have had the same active_seg_count at every call; act[] as far as the
    // host knows (-1: channels differ), sticky off once they disagree
    long long act[2] = {-1, -1};
    bool pair_ok = false;
    // A's launch of a fused crossfade step ran but B's failed: A is a block
    // ahead of B and the crossfader did not advance.  Every later call fails
    // instead of silently mixing convolvers that are out of step.
    bool poisoned = false;
    mutable StreamOrder order;
    PinnedStage hstage;  // host responses for the pending path (stored_response)
    // CrossfadeConvolver<TwoStageFFTConvolver> (the reference is generic over
    // Convolution, :11,45-49): convolver_a only.  B starts as A's clone and is
    // never switched to: every swap (:94-105) reaches TwoStageFFTConvolver::
    // update, todo!() (src/fft_convolver.rs:408-410), before fade_into, so the
    // crossfader stays Reached(A) and mix() returns A's sample (:244-247).  B
    // would run the same work on the same state and is never observable.
    std::unique_ptr<TwoStageCore> ts;
    int check_poisoned() const {
        return poisoned ? fail(FFTCONV_E_DEVICE, "crossfade handle unusable: an earlier process() failed between "
                                                  "its two convolvers' launches")
                        : FFTCONV_OK;
    }

    ~CrossfadeCore() {
        if (stream) {
            DeviceGuard g(device);
            (void)order.drain(stream);
            a.reset(); b.reset();  // (they borrow `stream`)
            (void)hipStreamDestroy(stream);
        }
    }

    // CrossfadeConvolver::new (:19-43)
    int init_new(const UniformCore &conv, size_t max_response_length, size_t mbs, size_t crossfade_samples) {
        device = conv.device;
        C = conv.C;
        DeviceGuard g(device);
        HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        a.reset(new (std::nothrow) UniformCore());
        b.reset(new (std::nothrow) UniformCore());
        if (!a || !b) return fail(FFTCONV_E_NOMEM, "out of host memory");
        a->parent_stream = b->parent_stream = stream;
        if (int r = a->clone_from(conv, false)) return r;  // (update() stages through hstage below)
        if (int r = b->clone_from(conv, false)) return r;
        // A and B start as copies: equal FDLs (FLAG_XSYNC), and one
        // active_seg_count if every channel of `conv` has the same
        if (C) {
            std::vector<int4> st(C);
            HIP_TRY(hipMemcpy(st.data(), a->state.p, C * sizeof(int4), hipMemcpyDeviceToHost));
            bool uniform = true;
            for (size_t c = 1; c < C; ++c) uniform = uniform && st[c].y == st[0].y;
            act[0] = act[1] = uniform ? st[0].y : -1;
            pair_ok = uniform && pair_supported(a->log2b, (int)a->S);
            HIP_TRY(launch_state_flags(a->state.p, (int)C, FLAG_XSYNC, 0, stream));
            HIP_TRY(launch_state_flags(b->state.p, (int)C, FLAG_XSYNC, 0, stream));
            a->view_ok = b->view_ok = false;
        }
        stored_len = max_response_length;
        stored_stride = stored_len;
        if (int r = stored.alloc(C * stored_len)) return r;
        if (stored.n) HIP_TRY(hipMemsetAsync(stored.p, 0, stored.bytes(), stream));
        stage_row = std::max(stored_len, a->ir_len);
        if (int r = hstage.alloc(C * stage_row, stage_row)) return r;
        xf.init(crossfade_samples, std::min(mbs, max_response_length));
        max_buffer_size = mbs;
        if (int r = buf_a.alloc(C * mbs)) return r;
        if (int r = buf_b.alloc(C * mbs)) return r;
        if (int r = mix_tab.alloc(mbs + 1)) return r;
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }

    // CrossfadeConvolver::<TwoStageFFTConvolver>::new (:19-43), taking
    // ownership of the (already cloned / freshly initialised) inner convolver
    int init_new_ts(std::unique_ptr<TwoStageCore> inner, size_t max_response_length, size_t mbs,
                    size_t crossfade_samples) {
        device = inner->device;
        C = inner->C;
        DeviceGuard g(device);
        HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        ts = std::move(inner);
        stored_len = max_response_length;  // (stored_response is never written: no swap can start)
        stored_stride = stored_len;
        xf.init(crossfade_samples, std::min(mbs, max_response_length));
        max_buffer_size = mbs;
        return buf_a.alloc(C * mbs);
    }

    int ts_update_unimplemented() const {
        return fail(FFTCONV_E_UNIMPLEMENTED, "not yet implemented (the swap calls TwoStageFFTConvolver::update, "
                                             "which is todo!())");
    }

    // :66-78 over a TwoStageFFTConvolver: convolver_a.process(input, buffer_a)
    // on max_buffer_size samples, then mix() = A's samples (Reached(A))
    int process_ts(const float *din, size_t is, float *dout, size_t os, size_t out_len, hipStream_t s) {
        const size_t m = max_buffer_size;
        if (m > ts->head_bs) return fail(FFTCONV_E_INVALID, "assertion failed: input.len() <= self.head_block_size");
        if (m == 0 || C == 0) return FFTCONV_OK;
        const bool direct = out_len == m;
        if (int r = ts->process_device(din, is, direct ? dout : buf_a.p, direct ? os : m, m, s)) return r;
        if (!direct && out_len)
            HIP_TRY(hipMemcpy2DAsync(dout, os * sizeof(float), buf_a.p, m * sizeof(float), out_len * sizeof(float), C,
                                     hipMemcpyDeviceToDevice, s));
        xf.advance(out_len);
        return FFTCONV_OK;
    }

    // every piece of the handle's work has finished (incl. a TwoStage inner's
    // tail convolution on its side stream)
    int quiesce() const {
        if (int r = order.drain(stream)) return r;
        return ts ? ts->quiesce() : FFTCONV_OK;
    }

    bool is_crossfading() const { return xf.approaching; }  // :85-92

    // swap (:94-105) from device samples
    int swap_device(const float *src, size_t stride, size_t len, hipStream_t s) {
        if (xf.target == 0) {
            if (int r = b->update_device(src, stride, len, s)) return r;
            note_update(1, len);
            xf.fade_into(1);
        } else {
            if (int r = a->update_device(src, stride, len, s)) return r;
            note_update(0, len);
            xf.fade_into(0);
        }
        return FFTCONV_OK;
    }

    // FFTConvolver::update sets active_seg_count = ceil(len / B) on every
    // channel (:185-190), unless the convolver is empty (:181-183)
    void note_update(int which, size_t len) {
        const UniformCore &u = which ? *b : *a;
        if (u.ir_len == 0) return;
        act[which] = (long long)ceil_div(len, u.B);
        if (act[0] < 0 || act[0] != act[1]) pair_ok = false;
    }

    // Convolution::update (:51-64); host samples, channel c at src + c*stride
    // (stride 0 = shared).  Asynchronous like FFTConvolver's: the response is
    // staged in pinned memory and the work enqueued behind the handle's.
    int update_host(const float *src, size_t len, size_t stride) {
        if (int r = check_poisoned()) return r;
        if (ts) return ts_update_unimplemented();
        DeviceGuard g(device);
        if (int r = order.enter(stream)) return r;
        if (!is_crossfading()) {
            UniformCore &t = xf.target == 0 ? *b : *a;
            if (len > t.ir_len) return fail(FFTCONV_E_INVALID, "New impulse response is longer than initialized length");
            if (int r = t.update_host_on(0, C, src, len, stride, stream, hstage)) return r;
            note_update(xf.target == 0 ? 1 : 0, len);
            xf.fade_into(xf.target == 0 ? 1 : 0);
            response_pending = false;
            return FFTCONV_OK;
        }
        if (len > stored_len) return fail(FFTCONV_E_INVALID, "assertion failed: response_len <= self.stored_response.len()");
        // stored_response[..len] = response; stored_response[len..] = 0
        if (stored.n) HIP_TRY(hipMemsetAsync(stored.p, 0, stored.bytes(), stream));
        if (len) {
            const bool shared = stride == 0 || C == 1;
            if (int r = hstage.upload(src, shared ? 1 : C, len, stride, stored.p, stored_len, stream)) return r;
            stored_stride = shared ? (C == 1 ? stored_len : 0) : stored_len;
        }
        response_pending = true;
        return FFTCONV_OK;
    }

    // Convolution::update (:51-64) from device samples, stream-ordered
    int update_device(const float *src, size_t len, size_t stride, hipStream_t s) {
        if (int r = check_poisoned()) return r;
        if (ts) return ts_update_unimplemented();
        if (!is_crossfading()) {
            UniformCore &t = xf.target == 0 ? *b : *a;
            if (len > t.ir_len) return fail(FFTCONV_E_INVALID, "New impulse response is longer than initialized length");
            if (int r = swap_device(src, stride, len, s)) return r;
            response_pending = false;
            return FFTCONV_OK;
        }
        if (len > stored_len) return fail(FFTCONV_E_INVALID, "assertion failed: response_len <= self.stored_response.len()");
        if (stored.n) HIP_TRY(hipMemsetAsync(stored.p, 0, stored.bytes(), s));
        if (len) {
            if (stride == 0 || C == 1) {
                HIP_TRY(hipMemcpyAsync(stored.p, src, len * sizeof(float), hipMemcpyDeviceToDevice, s));
                stored_stride = C == 1 ? stored_len : 0;
            } else {
                HIP_TRY(hipMemcpy2DAsync(stored.p, stored_len * sizeof(float), src, stride * sizeof(float),
                                         len * sizeof(float), C, hipMemcpyDeviceToDevice, s));
                stored_stride = stored_len;
            }
        }
        response_pending = true;
        return FFTCONV_OK;
    }

    CrossfadeMixArgs mix_args(float *dout, size_t os, size_t out_len) const {
        CrossfadeMixArgs x{};
        x.buf_a = buf_a.p; x.buf_b = buf_b.p; x.buf_stride = (long long)max_buffer_size;
        x.out = dout; x.out_stride = (long long)os; x.n = (int)out_len;
        x.approaching = xf.approaching ? 1 : 0; x.target = xf.target;
        x.counter0 = xf.counter; x.fading = xf.fading_samples;
        x.mix_value0 = xf.mix_value; x.step = xf.mix_value_step;
        return x;
    }

    // Convolution::process (:66-78)
    int process_device(const float *din, size_t is, float *dout, size_t os, size_t out_len, hipStream_t s) {
        if (int r = check_poisoned()) return r;
        if (out_len > max_buffer_size) return fail(FFTCONV_E_INVALID, "output longer than max_buffer_size (index out of bounds)");
        if (ts) return process_ts(din, is, dout, os, out_len, s);
        if (!is_crossfading() && response_pending) {                    // :67-70
            if (int r = swap_device(stored.p, stored_stride, stored_len, s)) return r;
            response_pending = false;
        }
        const size_t m = max_buffer_size;
        if (m > (size_t)INT32_MAX) return fail(FFTCONV_E_UNSUPPORTED, "process length exceeds 2^31-1");
        if (m > 0 && C > 0 && m == a->B && a->la_W && b->la_W && la_parts(a->log2b, (int)a->S) == a->la_W &&
            la_parts(b->log2b, (int)b->S) == b->la_W) {
            // :72-73 on the lookahead step: each convolver's full
            // block runs its own launch of far / mid anchors and steps; then
            // the mix (:75-77)
            const bool fuse_mix = out_len == m && !Variant::current().has(VARIANT_NOFMIX);
            if (fuse_mix && a->la_t == b->la_t && a->la_seq == b->la_seq &&
                a->la_all == b->la_all) {
                // :72-77 in ONE launch: A's and B's anchors, and per channel
                // one workgroup running A's and B's step (two chain waves)
                // that mixes the two blocks in LDS -- A's and B's clocks
                // agree (they step together), so one stagger serves both
                ProcArgs pa{};
                if (int r = a->la_job(pa.job[0], din, is, dout, os, m, s)) return r;
                if (int r = b->la_job(pa.job[1], din, is, nullptr, 0, m, s)) return r;
                pa.tw = a->tw.p;
                pa.njobs = 2;
                if (int r = a->la_fill(pa, s)) return r;
                pa.laW2 = b->laW.p;
                pa.la_mix = 3;
                pa.mix = mix_args(dout, os, out_len);  // (buf_a / buf_b: the generic-step fallback)
                HIP_TRY(launch_process_la(a->log2b, pa, (int)C, s));
                a->la_advance();
                b->la_advance();
                xf.advance(out_len);
                return FFTCONV_OK;
            }
            if (fuse_mix) {
                // the mix fused into B's launch: A's launch walks mix_value
                // once into mix_tab, B's epilogue mixes A's block (buf_a) with
                // its own straight into the output -- no mix launch, no buf_b
                const CrossfadeMixArgs mx = mix_args(dout, os, out_len);
                StepOpts o;
                o.mix = &mx;
                o.mix_tab = mix_tab.p;
                o.la_mix = 1;
                if (int r = a->process_device(din, is, buf_a.p, m, m, s, o)) return r;
                o.la_mix = 2;
                if (int r = b->process_device(din, is, dout, os, m, s, o)) {
                    poisoned = true;
                    return r;
                }
                xf.advance(out_len);
                return FFTCONV_OK;
            }
            if (int r = a->process_device(din, is, buf_a.p, m, m, s)) return r;
            if (int r = b->process_device(din, is, buf_b.p, m, m, s)) {
                poisoned = true;
                return r;
            }
            if (int r = launch_mix(dout, os, out_len, s)) return r;
            xf.advance(out_len);
            return FFTCONV_OK;
        }
        if (m > 0 && C > 0) {
            // :72-73 -- A and B are two jobs of ONE launch (same block size):
            // 2C workgroups fill the chip where C alone leaves it half occupied
            ProcArgs pa{};
            pa.job[0] = a->job(din, is, buf_a.p, m, m);
            pa.job[1] = b->job(din, is, buf_b.p, m, m);
            pa.njobs = 2;
            pa.tw = a->tw.p;
            // while A's and B's rings agree: one workgroup per channel reads
            // the FDL once for both (bit-identical to the two-job launch)
            pa.mix = mix_args(dout, os, out_len);
            if (pair_ok && pair_supported(a->log2b, (int)a->S) && m == a->B && out_len > 0) {
                // :72-77 in one launch: A, B and the mix (no buf_a / buf_b round trip)
                pa.fuse_mix = 1;
                HIP_TRY(launch_process_pair(a->log2b, pa, (int)C, s));
                xf.advance(out_len);
                return FFTCONV_OK;
            }
            a->lg_fill(pa, m);
            b->lg_fill(pa, m);
            HIP_TRY(launch_process(a->log2b, pa, (int)C, s));
        }
        if (int r = launch_mix(dout, os, out_len, s)) return r;  // :75-77
        xf.advance(out_len);
        return FFTCONV_OK;
    }

    // the stand-alone mix (:75-77); a call longer than the mix kernel's LDS
    // walk first walks mix_value once into mix_tab
    int launch_mix(float *dout, size_t os, size_t out_len, hipStream_t s) {
        CrossfadeMixArgs x = mix_args(dout, os, out_len);
        if (out_len > 1024 && x.approaching) {
            HIP_TRY(launch_crossfade_walk(x, mix_tab.p, s));
            x.vtab = mix_tab.p;
        }
        HIP_TRY(launch_crossfade_mix(x, (int)C, s));
        return FFTCONV_OK;
    }

    int process_host(const float *in, size_t in_len, float *out, size_t out_len) {
        if (in_len < max_buffer_size) return fail(FFTCONV_E_INVALID, "input shorter than max_buffer_size (range end index out of range)");
        if (ts && in_len > max_buffer_size)  // TwoStage: assert (:414), then output[i] past buffer_a (:441)
            return fail(FFTCONV_E_INVALID, in_len > ts->head_bs ? "assertion failed: input.len() <= self.head_block_size"
                                                                : "index out of bounds (input longer than max_buffer_size)");
        if (out_len > max_buffer_size) return fail(FFTCONV_E_INVALID, "output longer than max_buffer_size (index out of bounds)");
        if (C == 0) return FFTCONV_OK;
        DeviceGuard g(device);
        if (int r = order.enter(stream)) return r;
        const size_t m = max_buffer_size;
        if (int r = scratch.ensure(C * m, C * std::max<size_t>(out_len, 1))) return r;
        if (m)
            HIP_TRY(hipMemcpy2DAsync(scratch.in.p, m * sizeof(float), in, in_len * sizeof(float), m * sizeof(float), C,
                                     hipMemcpyHostToDevice, stream));
        if (int r = process_device(scratch.in.p, m, scratch.out.p, std::max<size_t>(out_len, 1), out_len, stream)) return r;
        if (out_len)
            HIP_TRY(hipMemcpy2DAsync(out, out_len * sizeof(float), scratch.out.p, out_len * sizeof(float),
                                     out_len * sizeof(float), C, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }

    int clone_from(const CrossfadeCore &o) {
        DeviceGuard g(o.device);
        if (int r = o.order.drain(o.stream)) return r;
        device = o.device; C = o.C; max_buffer_size = o.max_buffer_size;
        stored_len = o.stored_len; stored_stride = o.stored_stride;
        xf = o.xf; response_pending = o.response_pending;
        act[0] = o.act[0]; act[1] = o.act[1]; pair_ok = o.pair_ok; poisoned = o.poisoned;
        HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        if (o.ts) {
            ts.reset(new (std::nothrow) TwoStageCore());
            if (!ts) return fail(FFTCONV_E_NOMEM, "out of host memory");
            if (int r = ts->clone_from(*o.ts)) return r;
            return buf_a.alloc(o.buf_a.n);
        }
        a.reset(new (std::nothrow) UniformCore());
        b.reset(new (std::nothrow) UniformCore());
        if (!a || !b) return fail(FFTCONV_E_NOMEM, "out of host memory");
        a->parent_stream = b->parent_stream = stream;
        if (int r = a->clone_from(*o.a)) return r;
        if (int r = b->clone_from(*o.b)) return r;
        if (int r = buf_a.alloc(o.buf_a.n)) return r;
        if (int r = buf_b.alloc(o.buf_b.n)) return r;
        if (int r = mix_tab.alloc(o.mix_tab.n)) return r;
        if (int r = stored.alloc(o.stored.n)) return r;
        stage_row = o.stage_row;
        if (int r = hstage.alloc(o.hstage.n, stage_row)) return r;
        if (stored.n) HIP_TRY(hipMemcpyAsync(stored.p, o.stored.p, stored.bytes(), hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }
};

// ---------------------------------------------------------------------------
// What the matrix handles' cores share as free functions: `Core` is the
// handle's core (its process_device), `M` the matrix core that owns the
// geometry, the stream and the scratch (Core itself, or a lookahead core's m).
// ---------------------------------------------------------------------------
static_assert(kLookaheadPeriod == kMatrixLaQ, "block_walk.hpp's period is the kernels'");

// a clone's copy of one device buffer, enqueued on s
template <class T>
int clone_buffer(DevPtr<T> &dst, const DevPtr<T> &src, hipStream_t s) {
    if (int r = dst.alloc(src.n)) return r;
    if (src.n) HIP_TRY(hipMemcpyAsync(dst.p, src.p, src.bytes(), hipMemcpyDeviceToDevice, s));
    return FFTCONV_OK;
}

// process() from and to host memory: [I][in_len] -> [O][out_len], the host waits
template <class Core, class M>
int matrix_process_host(Core &c, M &m, const float *in, size_t in_len, float *out, size_t out_len) {
    if (in_len < out_len) return fail(FFTCONV_E_INVALID, "input slice shorter than output (range end index out of range)");
    if (out_len == 0) return FFTCONV_OK;
    DeviceGuard g(m.device);
    if (int r = m.order.enter(m.stream)) return r;
    if (int r = m.scratch.ensure(m.I * out_len, m.O * out_len)) return r;
    HIP_TRY(hipMemcpy2DAsync(m.scratch.in.p, out_len * sizeof(float), in, in_len * sizeof(float),
                             out_len * sizeof(float), m.I, hipMemcpyHostToDevice, m.stream));
    if (int r = c.process_device(m.scratch.in.p, out_len, m.scratch.out.p, out_len, out_len, m.stream)) return r;
    HIP_TRY(hipMemcpyAsync(out, m.scratch.out.p, m.O * out_len * sizeof(float), hipMemcpyDeviceToHost, m.stream));
    HIP_TRY(hipStreamSynchronize(m.stream));
    return FFTCONV_OK;
}

// `steps` process_device calls of n samples each, enqueued back to back
template <class Core>
int matrix_process_device_steps(Core &c, const float *din, size_t is, size_t in_step, float *dout, size_t os,
                                size_t out_step, size_t n, size_t steps, hipStream_t s) {
    for (size_t k = 0; k < steps; ++k)
        if (int r = c.process_device(din + k * in_step, is, dout + k * out_step, os, n, s)) return r;
    return FFTCONV_OK;
}

// ---------------------------------------------------------------------------
// MatrixBase -- what the dense and the sparse matrix share:
// P FFTConvolver instances in lockstep, one per (output, input) pair, P = O * I
// or the N pairs of a pattern.  Instance p processes its pair's input, output o
// is the sum over its pairs.  One FDL per input shared by all outputs, overlap /
// pre_multiplied summed per output, one inverse transform per output.  All
// instances are created, updated and reset together, so the reference's
// {current, active_seg_count, input_buffer_fill} (:215-295) is one triple
// (BlockWalk), advanced when a chunk is enqueued.  "Pair" is an index into H
// [P][S][B], the staging and the pair lists throughout.
// The concrete core D supplies, each called once per update, never per chunk:
//   int rebuild_plan(hipStream_t)    active_seg_count was set: what depends on it
//   int check_list(n, po, pi, idx)   an update_pairs list as ascending pair indices
// and its own process_device.
// ---------------------------------------------------------------------------
template <class D>
struct MatrixBase : BlockWalk {
    int device = 0;
    size_t I = 0, O = 0;
    size_t P = 0;         // pairs
    size_t ir_len = 0;    // max_response_length
    size_t B = 0;
    int log2b = 0;
    size_t S = 0;         // seg_count
    size_t last_len = 0;  // response_len of the last init / update: the length update_pairs pads to
    DevPtr<float2> H, X, pre, part, tw;  // part: the MAC parts' partial sums, sized by the concrete core
    DevPtr<float> ovl, ib, staging;
    hipStream_t stream = nullptr;
    bool own_stream = true;  // false: a crossfade's / MatrixTwoStageCore's convolver on its owner's stream
    Scratch scratch;
    PinnedStage hstage;
    PairLists lists;      // update_pairs (own_stream only: an owner brings its own)
    mutable StreamOrder order;

    D &self() { return static_cast<D &>(*this); }

    ~MatrixBase() {
        if (stream && own_stream) {
            DeviceGuard g(device);
            (void)order.drain(stream);
            (void)hipStreamDestroy(stream);
        }
    }

    // the sizes (:115-117) and the limits common to both matrices
    int set_geometry(int dev, size_t inputs, size_t outputs, size_t pairs, size_t max_block_size, size_t max_len) {
        device = dev;
        I = inputs;
        O = outputs;
        P = pairs;
        ir_len = max_len;
        B = next_pow2(max_block_size);                             // :115
        log2b = ilog2(B);
        if (B < 32 || B > 8192)
            return fail(FFTCONV_E_UNSUPPORTED, "matrix block size " + std::to_string(B) + " outside 32..8192");
        S = ceil_div(ir_len, B);                                   // :117
        if (S * B > (size_t)INT32_MAX || I * std::max<size_t>(S, 1) > (size_t)INT32_MAX)
            return fail(FFTCONV_E_UNSUPPORTED, "geometry exceeds 32-bit indexing");
        act = S;
        return FFTCONV_OK;
    }
    // the stream (`owner`: the matrix runs on that stream), the buffers of the
    // block walk (`part` of part_count spectra) and the twiddle table.  (The
    // order of the allocations is kept as it has always been: the buffers'
    // placement is worth a percent of a block's time.)
    int alloc_walk(hipStream_t owner, size_t part_count) {
        if (owner) {
            stream = owner;
            own_stream = false;
        } else {
            HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        }
        if (int r = H.alloc(P * S * B)) return r;
        if (int r = X.alloc(I * S * B)) return r;
        if (int r = pre.alloc(O * B)) return r;
        if (int r = part.alloc(part_count * B)) return r;
        if (int r = ovl.alloc(O * B)) return r;
        if (int r = ib.alloc(I * B)) return r;
        if (int r = tw.alloc(2 * B)) return r;
        std::vector<float2> t(2 * B);
        const size_t N = 2 * B;
        for (size_t k = 0; k < N; ++k) {
            const double ang = -2.0 * M_PI * (double)k / (double)N;
            t[k] = make_float2((float)std::cos(ang), (float)std::sin(ang));
        }
        HIP_TRY(hipMemcpy(tw.p, t.data(), t.size() * sizeof(float2), hipMemcpyHostToDevice));
        return FFTCONV_OK;
    }
    // what update() and update_pairs() stage through: update() never allocates
    int alloc_staging() {
        if (int r = staging.alloc(P * ir_len)) return r;
        if (int r = hstage.alloc(P * ir_len, ir_len)) return r;
        return own_stream ? lists.alloc(P) : FFTCONV_OK;
    }

    // the IR transform of every pair from device samples (pair p at src +
    // p * stride): rows at or past ceil(len_active / B) are zeroed (:210-212)
    int ir_from_device(const float *src, size_t stride, size_t len_data, size_t len_active, hipStream_t s) {
        const size_t step = 32768;  // (grid.y of the transform)
        for (size_t p0 = 0; p0 < P; p0 += step) {
            IrArgs a{};
            a.H = H.p;
            a.src = src + p0 * stride;
            a.src_stride = (long long)stride;
            a.len_data = (long long)len_data;
            a.len_active = (long long)len_active;
            a.tw = tw.p;
            a.S = (int)S;
            a.chan0 = (int)p0;
            a.update_state = 0;
            HIP_TRY(launch_ir_segments(log2b, a, (int)std::min(step, P - p0), s));
        }
        return FFTCONV_OK;
    }

    int zero_state(hipStream_t s) {  // :296-306
        if (X.n) HIP_TRY(hipMemsetAsync(X.p, 0, X.bytes(), s));
        if (ovl.n) HIP_TRY(hipMemsetAsync(ovl.p, 0, ovl.bytes(), s));
        if (ib.n) HIP_TRY(hipMemsetAsync(ib.p, 0, ib.bytes(), s));
        if (pre.n) HIP_TRY(hipMemsetAsync(pre.p, 0, pre.bytes(), s));
        cur = 0;
        fill = 0;
        return FFTCONV_OK;
    }
    int reset(hipStream_t s) { return zero_state(s); }

    // the end of init: the initial responses' transforms (:119-172), then the host waits
    int init_responses(const float *responses, size_t len, size_t stride) {
        last_len = len;
        if (S > 0) {
            const bool shared = stride == 0 && P > 1;
            if (len)
                if (int r = hstage.upload(responses, shared ? 1 : P, len, stride, staging.p, ir_len, stream)) return r;
            if (int r = ir_from_device(staging.p, shared ? 0 : ir_len, len, ir_len, stream)) return r;
        }
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }

    // update's side effects on the state (:186-190; current untouched)
    int set_active(size_t active, hipStream_t s) {
        if (pre.n) HIP_TRY(hipMemsetAsync(pre.p, 0, pre.bytes(), s));   // :187
        if (ovl.n) HIP_TRY(hipMemsetAsync(ovl.p, 0, ovl.bytes(), s));   // :188
        act = active;                                                   // :190
        return FFTCONV_OK;
    }

    // FFTConvolver::update (:174-213) of every instance; (the caller has
    // ordered s behind the handle's previous work)
    int update_device(const float *src, size_t stride, size_t len, hipStream_t s) {
        if (len > ir_len) return fail(FFTCONV_E_INVALID, "New impulse response is longer than initialized length");
        if (ir_len == 0) return FFTCONV_OK;                         // :181-183
        if (int r = set_active(ceil_div(len, B), s)) return r;
        last_len = len;
        if (int r = self().rebuild_plan(s)) return r;
        return ir_from_device(src, stride, len, len, s);
    }
    int update_host(const float *src, size_t len, size_t stride) {
        if (len > ir_len) return fail(FFTCONV_E_INVALID, "New impulse response is longer than initialized length");
        if (ir_len == 0) return FFTCONV_OK;
        DeviceGuard g(device);
        if (int r = order.enter(stream)) return r;
        const bool shared = stride == 0 && P > 1;
        if (len)
            if (int r = hstage.upload(src, shared ? 1 : P, len, stride, staging.p, ir_len, stream)) return r;
        return update_device(staging.p, shared ? 0 : ir_len, len, stream);
    }

    // One patch of H (matrix_patch.hip, generic in the pair index) from the
    // lists staged in L's mirror: the first n_tr pairs of L.tr() are
    // transformed from `src` (entry n reads row n, or -- by_pair -- the row of
    // its pair index), the first n_cp pairs of L.cp() are copied from Hsrc.
    // One launch up to kMatrixPatchChunk pairs per list.
    int patch_device(PairLists &L, size_t n_tr, size_t n_cp, const float2 *Hsrc, const float *src, size_t stride,
                     bool by_pair, size_t len_data, size_t len_active, hipStream_t s) {
        if (int r = L.push(n_tr, n_cp, s)) return r;
        const size_t step = (size_t)kMatrixPatchChunk;
        for (size_t c0 = 0; c0 < std::max(n_tr, n_cp); c0 += step) {
            MatrixPatchArgs a{};
            a.H = H.p;
            a.Hsrc = Hsrc;
            a.src = src;
            a.src_stride = (long long)stride;
            a.len_data = (long long)len_data;
            a.len_active = (long long)len_active;
            a.tw = tw.p;
            a.tr = L.d.p + c0;
            a.cp = L.d.p + L.cap + c0;
            a.n_tr = (int)(c0 < n_tr ? std::min(step, n_tr - c0) : 0);
            a.n_cp = (int)(c0 < n_cp ? std::min(step, n_cp - c0) : 0);
            a.row0 = (int)c0;
            a.by_pair = by_pair ? 1 : 0;
            a.S = (int)S;
            a.pairs = (int)P;
            a.nt_cp = Variant::current().nt_matrix(H.bytes()) ? 1 : 0;
            HIP_TRY(launch_matrix_patch(log2b, a, s));
        }
        return FFTCONV_OK;
    }

    // update(R'), R' = the responses this matrix holds with the n listed pairs
    // (ascending, in L.tr()) replaced by rows 0..n-1 of src, at the length of
    // the last init / update: update's side effects (the plan
    // included), and only the listed pairs are transformed -- every other
    // pair's rows are already the ones update(R') would write.
    int update_pairs_device(PairLists &L, size_t n, const float *src, size_t stride, size_t len, hipStream_t s) {
        if (len > last_len)
            return fail(FFTCONV_E_INVALID, "update_pairs: response longer than the length the response set was applied at");
        if (ir_len == 0) return FFTCONV_OK;
        if (int r = set_active(ceil_div(last_len, B), s)) return r;
        if (int r = self().rebuild_plan(s)) return r;
        return patch_device(L, n, 0, nullptr, src, stride, false, len, last_len, s);
    }
    // the C ABI's two variants: d_src == false -- host rows through the pinned staging
    int update_pairs(size_t n, const uint32_t *pair_out, const uint32_t *pair_in, const float *src, bool d_src,
                     size_t len, size_t stride, hipStream_t s) {
        if (int r = self().check_list(n, pair_out, pair_in, lists.idx.data())) return r;
        if (len > last_len)
            return fail(FFTCONV_E_INVALID, "update_pairs: response longer than the length the response set was applied at");
        DeviceGuard g(device);
        if (int r = order.enter(s)) return r;
        if (int r = lists.acquire()) return r;
        std::copy(lists.idx.begin(), lists.idx.begin() + n, lists.tr());
        if (!d_src && len && n && ir_len) {
            const bool shared = stride == 0 && n > 1;
            if (int r = hstage.upload(src, shared ? 1 : n, len, stride, staging.p, ir_len, s)) return r;
            return update_pairs_device(lists, n, staging.p, shared ? 0 : ir_len, len, s);
        }
        return update_pairs_device(lists, n, src, stride, len, s);
    }

    // What every process_device starts with.  *launch = false: nothing to
    // enqueue -- no samples, or active_seg_count == 0 (:216-219: zero output,
    // state untouched).
    int process_begin(float *dout, size_t os, size_t n, hipStream_t s, bool *launch) const {
        *launch = false;
        if (n > (size_t)INT32_MAX) return fail(FFTCONV_E_UNSUPPORTED, "process length exceeds 2^31-1");
        if (n == 0) return FFTCONV_OK;
        if (act == 0) {
            HIP_TRY(hipMemset2DAsync(dout, os * sizeof(float), 0, n * sizeof(float), O, s));
            return FFTCONV_OK;
        }
        *launch = true;
        return FFTCONV_OK;
    }
    // the call's part of a chunk launch's arguments (`part` and the part counts are the caller's)
    void call_args(MatrixArgs &a, size_t is, size_t os) const {
        a.H = H.p; a.X = X.p; a.ovl = ovl.p; a.ib = ib.p; a.pre = pre.p; a.tw = tw.p;
        a.in_stride = (long long)is;
        a.out_stride = (long long)os;
        a.I = (int)I; a.O = (int)O; a.S = (int)S;
        a.act = (int)act;
        a.nt_h = Variant::current().nt_matrix(H.bytes()) ? 1 : 0;
    }
    // the next chunk (:224-227) of a call with `done` of its n samples enqueued
    size_t chunk_args(MatrixArgs &a, const float *din, float *dout, size_t done, size_t n) const {
        const size_t k = chunk(n - done, B);
        a.in = din + done;
        a.out = dout + done;
        a.cur = (int)cur;
        a.fill = (int)fill;
        a.k = (int)k;
        return k;
    }

    int process_host(const float *in, size_t in_len, float *out, size_t out_len) {
        return matrix_process_host(self(), *this, in, in_len, out, out_len);
    }

    // What a crossfaded pair (MatrixCrossfadeCoreT) asks of its two convolvers
    // beyond the block walk; a matrix without windows has nothing to add.
    bool xf_in_step(const D &) const { return true; }
    void xf_swapped() {}
    template <class XfArgs>
    static void xf_chunk_begin(XfArgs &, D &, D &) {}
    static void xf_block_done(D &, D &) {}

    // #[derive(Clone)] of the base's part; `owner`: the clone is a crossfade's
    // convolver -- it runs on that stream and stages updates through its owner.
    // (The caller waits for the stream.)
    int clone_base(const MatrixBase &o, hipStream_t owner) {
        if (int r = o.order.drain(o.stream)) return r;
        device = o.device;
        I = o.I; O = o.O; P = o.P; ir_len = o.ir_len; B = o.B; log2b = o.log2b; S = o.S;
        cur = o.cur; act = o.act; fill = o.fill; last_len = o.last_len;
        if (owner) {
            stream = owner;
            own_stream = false;
        } else {
            HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
            if (int r = lists.alloc(P)) return r;
        }
        if (int r = clone_buffer(H, o.H, stream)) return r;
        if (int r = clone_buffer(X, o.X, stream)) return r;
        if (int r = clone_buffer(pre, o.pre, stream)) return r;
        if (int r = clone_buffer(tw, o.tw, stream)) return r;
        if (int r = clone_buffer(ovl, o.ovl, stream)) return r;
        return clone_buffer(ib, o.ib, stream);
    }
    // ... and what a clone reserves without copying, after the concrete core's own buffers
    int clone_reserve(const MatrixBase &o) {
        if (int r = part.alloc(o.part.n)) return r;  // (rewritten by every block before it is read)
        if (int r = staging.alloc(o.staging.n)) return r;
        return own_stream ? hstage.alloc(o.hstage.n, ir_len) : FFTCONV_OK;
    }
};

// ---------------------------------------------------------------------------
// MatrixCore -- the dense matrix (matrix.hip): pair (o, i) is
// o * I + i, every output sums all I inputs.
// ---------------------------------------------------------------------------
struct MatrixCore : MatrixBase<MatrixCore> {
    static constexpr const char *kName = "matrix";
    using XfArgs = MatrixXfArgs;
    using TsArgs = MatrixTsArgs;
    size_t Pmax = 1;      // MAC parts at active = S (the `part` rows per output)

    int mac_parts() const { return matrix_mac_parts((int)I, log2b, (int)S, (int)act); }
    int rebuild_plan(hipStream_t) { return FFTCONV_OK; }  // (the MAC grid is a function of active alone)

    int check_list(size_t n, const uint32_t *pair_out, const uint32_t *pair_in, uint32_t *idx) const {
        if (n && (!pair_out || !pair_in)) return fail(FFTCONV_E_INVALID, "null pair list");
        if (n > P) return fail(FFTCONV_E_INVALID, "the pair list must be strictly ascending in (output, input)");
        if (PairListError e = check_pairs(n, pair_out, pair_in, I, O, idx)) return pair_list_error(e);
        return FFTCONV_OK;
    }

    int alloc_geometry(int dev, size_t inputs, size_t outputs, size_t max_block_size, size_t max_len, hipStream_t owner) {
        if (int r = set_geometry(dev, inputs, outputs, inputs * outputs, max_block_size, max_len)) return r;
        if (I > (size_t)INT32_MAX || O > (size_t)INT32_MAX || O * 64 > (size_t)INT32_MAX)
            return fail(FFTCONV_E_UNSUPPORTED, "geometry exceeds 32-bit indexing");
        Pmax = (size_t)matrix_mac_parts((int)I, log2b, (int)S, (int)S);
        if (int r = alloc_walk(owner, O * Pmax)) return r;
        return alloc_staging();
    }

    // `owner`: the matrix is a stage of a MatrixTwoStageCore and runs on that stream
    int init(int dev, size_t inputs, size_t outputs, const float *responses, size_t len, size_t stride,
             size_t max_block, size_t max_len, hipStream_t owner = nullptr) {
        if (inputs == 0 || outputs == 0) return fail(FFTCONV_E_INVALID, "a matrix needs at least one input and one output");
        if (max_len < len)                                          // :106-110
            return fail(FFTCONV_E_INVALID,
                        "max_response_length must be at least the length of the initial impulse response");
        if (int r = check_device(dev)) return r;
        DeviceGuard g(dev);
        if (int r = alloc_geometry(dev, inputs, outputs, max_block, max_len, owner)) return r;
        if (int r = zero_state(stream)) return r;
        return init_responses(responses, len, stride);
    }

    int process_device(const float *din, size_t is, float *dout, size_t os, size_t n, hipStream_t s) {
        bool launch;
        if (int r = process_begin(dout, os, n, s, &launch); r || !launch) return r;
        MatrixArgs a{};
        call_args(a, is, os);
        a.part = part.p;
        a.P = mac_parts();
        a.rpp = (int)ceil_div(I * (act - 1), (size_t)a.P);
        for (size_t done = 0; done < n;) {                          // :222-294
            const size_t k = chunk_args(a, din, dout, done, n);
            HIP_TRY(launch_matrix_chunk(log2b, a, s));
            advance(k, B);
            done += k;
        }
        return FFTCONV_OK;
    }

    // the fused crossfade launch (matrix_xf.hip): what it takes beyond the shared arguments
    void xf_args(XfArgs &x) const {
        x.P = mac_parts();
        x.rpp = (int)ceil_div(I * (act - 1), (size_t)x.P);
    }
    static hipError_t launch_xf_chunk(int log2b, const XfArgs &x, hipStream_t s) { return launch_matrix_xf_chunk(log2b, x, s); }

    // the fused two-stage launch (matrix_ts.hip), this matrix being the head
    void ts_args(TsArgs &x) const {
        x.P = mac_parts();
        x.rpp = (int)ceil_div(I * (act - 1), (size_t)x.P);
    }
    bool ts_plan_equal(const MatrixCore &) const { return true; }  // (the MAC grid is a function of {I, S, active})
    static hipError_t launch_ts_block(int log2b, const TsArgs &x, hipStream_t s) { return launch_matrix_ts_block(log2b, x, s); }

    int clone_from(const MatrixCore &o, hipStream_t owner = nullptr) {  // #[derive(Clone)]
        DeviceGuard g(o.device);
        if (int r = clone_base(o, owner)) return r;
        Pmax = o.Pmax;
        if (int r = clone_reserve(o)) return r;
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }
};

// ---------------------------------------------------------------------------
// MatrixLookaheadCore -- the MatrixCore's I x O instances with one level of
// far-row windows (matrix_la.hip).  The dense core `m` owns the
// geometry, the buffers, the stream and {current, active, fill}; this core adds
// the near / far partial sums and the block clock that schedules the anchors.
// ---------------------------------------------------------------------------
struct MatrixLookaheadCore {
    static constexpr const char *kName = "lookahead matrix";
    static constexpr size_t Q = kMatrixLaQ;
    using XfArgs = MatrixLaXfArgs;
    MatrixCore m;
    DevPtr<float2> far;  // [O][Pf_max][Q][B]; the near partial sums use m.part (Pn <= the dense P)
    LookaheadClock clk;

    // rows (i, s) of one output: near 1 <= s < min(Q, active), far Q <= s < active
    size_t near_rows() const { return m.I * (std::min(m.act, Q) > 0 ? std::min(m.act, Q) - 1 : 0); }
    size_t far_rows() const { return m.act > Q ? m.I * (m.act - Q) : 0; }
    int near_parts() const { return matrix_la_parts((long long)near_rows()); }
    int far_parts() const { return far_rows() ? matrix_la_parts((long long)far_rows()) : 0; }
    // outputs that anchor when the next block starts
    int anchors() const {
        if (!clk.windows || m.act <= Q || m.cur >= m.act) return 0;
        const size_t t0 = (size_t)(clk.t % (long long)Q);
        return t0 < m.O ? (int)((m.O - t0 + Q - 1) / Q) : 0;
    }

    int alloc_extra() {
        const size_t pf = m.S > Q ? (size_t)matrix_la_parts((long long)m.I * (long long)(m.S - Q)) : 0;
        return far.alloc(m.O * pf * Q * m.B);
    }

    int init(int dev, size_t inputs, size_t outputs, const float *responses, size_t len, size_t stride,
             size_t max_block, size_t max_len) {
        if (inputs && outputs && max_len >= len && next_pow2(max_block) > ((size_t)1 << kMatrixLaMaxLog2B))
            return fail(FFTCONV_E_UNSUPPORTED, "matrix lookahead block size " + std::to_string(next_pow2(max_block)) +
                                                   " outside 32..512 (use the MatrixConvolver)");
        if (int r = m.init(dev, inputs, outputs, responses, len, stride, max_block, max_len)) return r;
        DeviceGuard g(dev);
        clk = LookaheadClock();
        return alloc_extra();
    }
    int update_device(const float *src, size_t stride, size_t len, hipStream_t s) {
        if (int r = m.update_device(src, stride, len, s)) return r;
        clk.invalidate(m.fill);
        return FFTCONV_OK;
    }
    int update_host(const float *src, size_t len, size_t stride) {
        if (int r = m.update_host(src, len, stride)) return r;
        clk.invalidate(m.fill);
        return FFTCONV_OK;
    }
    int reset(hipStream_t s) {
        const size_t fill = m.fill;  // (zero_state clears it)
        if (int r = m.zero_state(s)) return r;
        clk.reset(fill);
        return FFTCONV_OK;
    }

    int process_device(const float *din, size_t is, float *dout, size_t os, size_t n, hipStream_t s) {
        bool launch;
        if (int r = m.process_begin(dout, os, n, s, &launch); r || !launch) return r;
        MatrixLaArgs la{};
        MatrixArgs &a = la.m;
        // nt_h by the whole H, as the dense matrix: a block streams 1 / Q of the
        // far rows, but over Q blocks all of H passes through the cache (measured,
        // judging by a block's own bytes chose plain loads at M2 and lost 6 %)
        m.call_args(a, is, os);
        a.part = m.part.p;
        a.P = near_parts();
        a.rpp = (int)ceil_div(near_rows(), (size_t)a.P);
        la.far = far.p;
        la.Pf = far_parts();
        la.rppf = la.Pf ? (int)ceil_div(far_rows(), (size_t)la.Pf) : 0;
        for (size_t done = 0; done < n;) {                          // :222-294
            clk.begin_chunk(m.fill, m.cur, m.act);
            const size_t k = m.chunk_args(a, din, dout, done, n);
            la.t = clk.t;
            la.tv = clk.tv;
            HIP_TRY(launch_matrix_la_chunk(m.log2b, la, s));
            if (m.advance(k, m.B)) clk.block_done();
            done += k;
        }
        return FFTCONV_OK;
    }

    int process_host(const float *in, size_t in_len, float *out, size_t out_len) {
        return matrix_process_host(*this, m, in, in_len, out, out_len);
    }

    // The fused crossfade launch (matrix_la_xf.hip) of the pair (a, b), `x.live`
    // set: what it takes beyond the shared arguments, and the window rules of
    // DESIGN §4t -- a live convolver's clock runs as in process_device, an idle
    // one's windows are kept invalid, both count the block.
    void xf_args(XfArgs &x) const {
        x.P = near_parts();
        x.rpp = (int)ceil_div(near_rows(), (size_t)x.P);
        x.Pf = far_parts();
        x.rppf = x.Pf ? (int)ceil_div(far_rows(), (size_t)x.Pf) : 0;
    }
    bool xf_in_step(const MatrixLookaheadCore &o) const { return clk.t == o.clk.t; }
    void xf_swapped() { clk.invalidate(m.fill); }
    static void xf_chunk_begin(XfArgs &x, MatrixLookaheadCore &a, MatrixLookaheadCore &b) {
        MatrixLookaheadCore *cv[2] = {&a, &b};
        for (int c = 0; c < 2; ++c) {
            if ((x.live >> c) & 1)
                cv[c]->clk.begin_chunk(cv[c]->m.fill, cv[c]->m.cur, cv[c]->m.act);
            else
                cv[c]->clk.idle_chunk(cv[c]->m.fill);
            x.far[c] = cv[c]->far.p;
            x.tv[c] = cv[c]->clk.tv;
        }
        x.t = a.clk.t;
    }
    static void xf_block_done(MatrixLookaheadCore &a, MatrixLookaheadCore &b) {
        a.clk.block_done();
        b.clk.block_done();
    }
    static hipError_t launch_xf_chunk(int log2b, const XfArgs &x, hipStream_t s) { return launch_matrix_la_xf_chunk(log2b, x, s); }

    // #[derive(Clone)]: the windows and the clock too; `owner`: the clone is a
    // crossfade's convolver on that stream
    int clone_from(const MatrixLookaheadCore &o, hipStream_t owner = nullptr) {
        if (int r = m.clone_from(o.m, owner)) return r;
        DeviceGuard g(m.device);
        clk = o.clk;
        if (int r = clone_buffer(far, o.far, m.stream)) return r;
        HIP_TRY(hipStreamSynchronize(m.stream));
        return FFTCONV_OK;
    }
};

// ---------------------------------------------------------------------------
// SparseMatrixCore -- the matrix over a CSR pattern that is fixed for the life
// of the handle (matrix_sp.hip): pair n is the n-th listed (output,
// input), P = N.  Launch A's MAC grid is the compact sum of the outputs' P_o,
// found through a device plan that is rebuilt on the stream whenever
// active_seg_count is set (init, update, update_pairs).
// ---------------------------------------------------------------------------
struct SparseMatrixCore : MatrixBase<SparseMatrixCore> {
    static constexpr const char *kName = "sparse matrix";
    using XfArgs = MatrixSpXfArgs;
    using TsArgs = MatrixSpTsArgs;
    size_t PTmax = 0;     // sum of P_o at active = S (the rows of `part`)
    size_t PT = 0;        // sum of P_o at the current active
    std::vector<int> rowptr, col;  // the host's copy of the pattern
    DevPtr<int> d_rowptr, d_col, plan;
    DevPtr<int4> wg;      // [PTmax] the MAC workgroups' descriptors, rebuilt with the plan

    size_t pairs_of(size_t o) const { return (size_t)(rowptr[o + 1] - rowptr[o]); }
    int output_parts(size_t o) const { return matrix_mac_parts((int)pairs_of(o), log2b, (int)S, (int)act); }
    size_t total_parts(size_t active) const {
        size_t t = 0;
        for (size_t o = 0; o < O; ++o) t += (size_t)matrix_mac_parts((int)pairs_of(o), log2b, (int)S, (int)active);
        return t;
    }
    // the device plan for the current `act`, behind the stream's earlier work
    // (launches that read the previous plan) and ahead of its later launches
    int rebuild_plan(hipStream_t s) {
        PT = total_parts(act);
        HIP_TRY(launch_matrix_sp_plan(d_rowptr.p, plan.p, wg.p, (int)O, (int)act, s));
        return FFTCONV_OK;
    }

    static int check_pattern(size_t inputs, size_t outputs, size_t pairs, const uint32_t *po, const uint32_t *pi) {
        if (inputs == 0 || outputs == 0)
            return fail(FFTCONV_E_INVALID, "a matrix needs at least one input and one output");
        if (pairs == 0 || !po || !pi) return fail(FFTCONV_E_INVALID, "a sparse matrix needs at least one pair");
        if (inputs > (size_t)INT32_MAX || outputs > (size_t)INT32_MAX || pairs > (size_t)INT32_MAX)
            return fail(FFTCONV_E_UNSUPPORTED, "geometry exceeds 32-bit indexing");
        for (size_t n = 0; n < pairs; ++n) {
            if (po[n] >= outputs || pi[n] >= inputs)
                return fail(FFTCONV_E_INVALID, "pair " + std::to_string(n) + " is out of range");
            if (n > 0 && (po[n] < po[n - 1] || (po[n] == po[n - 1] && pi[n] <= pi[n - 1])))
                return fail(FFTCONV_E_INVALID, "the pair list is not strictly ascending in (output, input) at pair " +
                                                   std::to_string(n));
        }
        return FFTCONV_OK;
    }

    // the pair list of an update_pairs call as positions in the pattern's list
    int check_list(size_t n, const uint32_t *pair_out, const uint32_t *pair_in, uint32_t *idx) const {
        if (n && (!pair_out || !pair_in)) return fail(FFTCONV_E_INVALID, "null pair list");
        if (n > P) return fail(FFTCONV_E_INVALID, "the pair list must be strictly ascending in (output, input)");
        size_t bad = 0;
        const PairListError e = check_pairs_in_pattern(n, pair_out, pair_in, rowptr.data(), col.data(), I, O, idx, &bad);
        if (e == PAIRS_ABSENT)
            return fail(FFTCONV_E_INVALID, "pair (" + std::to_string(pair_out[bad]) + ", " + std::to_string(pair_in[bad]) +
                                               ") is not in the pattern");
        return e ? pair_list_error(e) : FFTCONV_OK;
    }

    int alloc_geometry(int dev, size_t inputs, size_t outputs, size_t pairs, size_t max_block_size, size_t max_len,
                       hipStream_t owner) {
        if (int r = set_geometry(dev, inputs, outputs, pairs, max_block_size, max_len)) return r;
        if (P * std::max<size_t>(S, 1) > (size_t)INT32_MAX)
            return fail(FFTCONV_E_UNSUPPORTED, "geometry exceeds 32-bit indexing");
        PTmax = total_parts(S);
        if (I + PTmax > (size_t)INT32_MAX) return fail(FFTCONV_E_UNSUPPORTED, "geometry exceeds 32-bit indexing");
        if (int r = alloc_walk(owner, PTmax)) return r;            // (P_o is largest at active = S)
        if (int r = d_rowptr.alloc(O + 1)) return r;
        if (int r = d_col.alloc(P)) return r;
        if (int r = plan.alloc(O + 1)) return r;
        if (int r = wg.alloc(PTmax)) return r;
        if (int r = alloc_staging()) return r;
        HIP_TRY(hipMemcpy(d_rowptr.p, rowptr.data(), d_rowptr.bytes(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_col.p, col.data(), d_col.bytes(), hipMemcpyHostToDevice));
        return FFTCONV_OK;
    }

    // `owner`: the matrix is a stage of a SparseMatrixTwoStageCore and runs on that stream
    int init(int dev, size_t inputs, size_t outputs, size_t pairs, const uint32_t *po, const uint32_t *pi,
             const float *responses, size_t len, size_t stride, size_t max_block, size_t max_len,
             hipStream_t owner = nullptr) {
        if (int r = check_pattern(inputs, outputs, pairs, po, pi)) return r;
        if (max_len < len)                                          // :106-110
            return fail(FFTCONV_E_INVALID,
                        "max_response_length must be at least the length of the initial impulse response");
        if (int r = check_device(dev)) return r;
        rowptr.assign(outputs + 1, 0);
        col.resize(pairs);
        for (size_t n = 0; n < pairs; ++n) {
            ++rowptr[po[n] + 1];
            col[n] = (int)pi[n];
        }
        for (size_t o = 0; o < outputs; ++o) rowptr[o + 1] += rowptr[o];
        DeviceGuard g(dev);
        if (int r = alloc_geometry(dev, inputs, outputs, pairs, max_block, max_len, owner)) return r;
        if (int r = zero_state(stream)) return r;
        if (int r = rebuild_plan(stream)) return r;
        return init_responses(responses, len, stride);
    }

    int process_device(const float *din, size_t is, float *dout, size_t os, size_t n, hipStream_t s) {
        bool launch;
        if (int r = process_begin(dout, os, n, s, &launch); r || !launch) return r;
        MatrixSpArgs a{};
        call_args(a.m, is, os);
        a.m.part = part.p;
        a.rowptr = d_rowptr.p; a.col = d_col.p; a.plan = plan.p; a.wg = wg.p;
        a.N = (int)P;
        a.PT = (int)PT;
        for (size_t done = 0; done < n;) {                          // :222-294
            const size_t k = chunk_args(a.m, din, dout, done, n);
            HIP_TRY(launch_matrix_sp_chunk(log2b, a, s));
            advance(k, B);
            done += k;
        }
        return FFTCONV_OK;
    }

    // the fused crossfade launch (matrix_sp_xf.hip): what it takes beyond the
    // shared arguments.  (In step, A and B have the same active_seg_count, so
    // their plans are equal.)
    void xf_args(XfArgs &x) const {
        x.rowptr = d_rowptr.p; x.col = d_col.p; x.plan = plan.p; x.wg = wg.p;
        x.N = (int)P;
        x.PT = (int)PT;
    }
    static hipError_t launch_xf_chunk(int log2b, const XfArgs &x, hipStream_t s) { return launch_matrix_sp_xf_chunk(log2b, x, s); }

    // the fused two-stage launch (matrix_sp_ts.hip), this matrix being the
    // head.  Head and tail0 hold the same pattern, so equal {S, active} give
    // equal plans; the part counts are compared all the same.
    void ts_args(TsArgs &x) const {
        x.rowptr = d_rowptr.p; x.col = d_col.p; x.plan = plan.p; x.wg = wg.p;
        x.N = (int)P;
        x.PT = (int)PT;
    }
    bool ts_plan_equal(const SparseMatrixCore &t) const { return PT == t.PT; }
    static hipError_t launch_ts_block(int log2b, const TsArgs &x, hipStream_t s) { return launch_matrix_sp_ts_block(log2b, x, s); }

    int clone_from(const SparseMatrixCore &o, hipStream_t owner = nullptr) {  // #[derive(Clone)]
        DeviceGuard g(o.device);
        if (int r = clone_base(o, owner)) return r;
        PTmax = o.PTmax; PT = o.PT;
        rowptr = o.rowptr;
        col = o.col;
        if (int r = clone_buffer(d_rowptr, o.d_rowptr, stream)) return r;
        if (int r = clone_buffer(d_col, o.d_col, stream)) return r;
        if (int r = clone_buffer(plan, o.plan, stream)) return r;
        if (int r = clone_buffer(wg, o.wg, stream)) return r;
        if (int r = clone_reserve(o)) return r;
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }
};

// ---------------------------------------------------------------------------
// SparseMatrixLookaheadCore -- the SparseMatrixCore's N instances with one
// level of far-row windows (matrix_sp_la.hip).  The sparse core `m`
// owns the geometry, the pattern, H, the delay lines, the stream, the IR
// transforms and {current, active, fill}, as MatrixLookaheadCore's dense core
// does; this core adds the near / far partial sums, its own plan (per output
// the near and far part counts over its pair list, the far workgroups ordered
// by anchor class) and the block clock that schedules the anchors.
// (m.part, m.plan and m.wg are the plain sparse walk's and unused here.)
// ---------------------------------------------------------------------------
struct SparseMatrixLookaheadCore {
    static constexpr size_t Q = kMatrixLaQ;
    SparseMatrixCore m;
    DevPtr<float2> npart;  // [sum Pn_o][B] at active = S
    DevPtr<float2> far;    // [sum Pf_o][Q][B] at active = S
    DevPtr<int> nplan, fplan, d_coff;
    DevPtr<int4> nwg, fwg;
    size_t PnT = 0, PfT = 0;   // for the current active
    int coff[Q + 1] = {};      // the host's copy of the class offsets, from its copy of rowptr
    int class_outputs[Q] = {}; // outputs with at least one pair, per anchor class
    LookaheadClock clk;

    int near_parts(size_t o) const { return matrix_sp_la_pn((long long)m.pairs_of(o), (int)m.act); }
    int far_parts(size_t o) const { return matrix_sp_la_pf((long long)m.pairs_of(o), (int)m.act); }
    // outputs with at least one pair that anchor when the next block starts
    int anchors() const {
        if (!clk.windows || m.act <= Q || m.cur >= m.act) return 0;
        return class_outputs[(size_t)(clk.t % (long long)Q)];
    }

    // the sums the plan kernel computes, from the host's copy of the pattern
    void count(size_t active, size_t *pn, size_t *pf, int *offsets) const {
        size_t n = 0, cls[Q] = {};
        for (size_t o = 0; o < m.O; ++o) {
            n += (size_t)matrix_sp_la_pn((long long)m.pairs_of(o), (int)active);
            cls[o % Q] += (size_t)matrix_sp_la_pf((long long)m.pairs_of(o), (int)active);
        }
        size_t f = 0;
        for (size_t c = 0; c < Q; ++c) {
            if (offsets) offsets[c] = (int)f;
            f += cls[c];
        }
        if (offsets) offsets[Q] = (int)f;
        *pn = n;
        *pf = f;
    }
    // the device plan for the current active, behind the stream's earlier work
    int rebuild_plan(hipStream_t s) {
        count(m.act, &PnT, &PfT, coff);
        HIP_TRY(launch_matrix_sp_la_plan(m.d_rowptr.p, nplan.p, fplan.p, nwg.p, fwg.p, d_coff.p, (int)m.O, (int)m.act, s));
        return FFTCONV_OK;
    }

    int alloc_extra() {
        size_t pn = 0, pf = 0;
        count(m.S, &pn, &pf, nullptr);  // (every count is largest at active = S)
        if (m.I + pn + pf > (size_t)INT32_MAX || 2 * pf > (size_t)INT32_MAX)
            return fail(FFTCONV_E_UNSUPPORTED, "geometry exceeds 32-bit indexing");
        if (int r = npart.alloc(pn * m.B)) return r;
        if (int r = far.alloc(pf * Q * m.B)) return r;
        if (int r = nplan.alloc(m.O + 1)) return r;
        if (int r = fplan.alloc(m.O + 1)) return r;
        if (int r = d_coff.alloc(Q + 1)) return r;
        if (int r = nwg.alloc(pn)) return r;
        if (int r = fwg.alloc(2 * pf)) return r;
        for (size_t c = 0; c < Q; ++c) class_outputs[c] = 0;
        for (size_t o = 0; o < m.O; ++o)
            if (m.pairs_of(o)) ++class_outputs[o % Q];
        return FFTCONV_OK;
    }

    int init(int dev, size_t inputs, size_t outputs, size_t pairs, const uint32_t *po, const uint32_t *pi,
             const float *responses, size_t len, size_t stride, size_t max_block, size_t max_len) {
        if (int r = SparseMatrixCore::check_pattern(inputs, outputs, pairs, po, pi)) return r;
        if (max_len >= len && next_pow2(max_block) > ((size_t)1 << kMatrixLaMaxLog2B))
            return fail(FFTCONV_E_UNSUPPORTED, "sparse matrix lookahead block size " + std::to_string(next_pow2(max_block)) +
                                                   " outside 32..512 (use the SparseMatrixConvolver)");
        if (int r = m.init(dev, inputs, outputs, pairs, po, pi, responses, len, stride, max_block, max_len)) return r;
        DeviceGuard g(dev);
        clk = LookaheadClock();
        if (int r = alloc_extra()) return r;
        if (int r = rebuild_plan(m.stream)) return r;
        HIP_TRY(hipStreamSynchronize(m.stream));
        return FFTCONV_OK;
    }
    int update_device(const float *src, size_t stride, size_t len, hipStream_t s) {
        if (int r = m.update_device(src, stride, len, s)) return r;
        if (m.ir_len == 0) return FFTCONV_OK;
        if (int r = rebuild_plan(s)) return r;
        clk.invalidate(m.fill);
        return FFTCONV_OK;
    }
    int update_host(const float *src, size_t len, size_t stride) {
        if (int r = m.update_host(src, len, stride)) return r;
        if (m.ir_len == 0) return FFTCONV_OK;
        DeviceGuard g(m.device);
        if (int r = rebuild_plan(m.stream)) return r;
        clk.invalidate(m.fill);
        return FFTCONV_OK;
    }
    // update(R') of the sparse core at the held length: active and the plan stay;
    // every window is dropped, the untouched outputs' too
    int update_pairs(size_t n, const uint32_t *pair_out, const uint32_t *pair_in, const float *src, bool d_src,
                     size_t len, size_t stride, hipStream_t s) {
        if (int r = m.update_pairs(n, pair_out, pair_in, src, d_src, len, stride, s)) return r;
        clk.invalidate(m.fill);
        return FFTCONV_OK;
    }
    int reset(hipStream_t s) {
        const size_t fill = m.fill;  // (zero_state clears it)
        if (int r = m.zero_state(s)) return r;
        clk.reset(fill);
        return FFTCONV_OK;
    }

    int process_device(const float *din, size_t is, float *dout, size_t os, size_t n, hipStream_t s) {
        bool launch;
        if (int r = m.process_begin(dout, os, n, s, &launch); r || !launch) return r;
        MatrixSpLaArgs la{};
        MatrixArgs &a = la.m;
        m.call_args(a, is, os);  // (nt_h by the whole H, as the dense lookahead matrix: DESIGN 4n)
        a.part = npart.p;
        la.rowptr = m.d_rowptr.p; la.col = m.d_col.p;
        la.nplan = nplan.p; la.fplan = fplan.p; la.nwg = nwg.p; la.fwg = fwg.p;
        la.far = far.p;
        la.N = (int)m.P;
        la.PnT = (int)PnT;
        la.PfT = (int)PfT;
        for (size_t done = 0; done < n;) {                          // :222-294
            clk.begin_chunk(m.fill, m.cur, m.act);
            const size_t k = m.chunk_args(a, din, dout, done, n);
            la.t = clk.t;
            la.tv = clk.tv;
            if (matrix_la_steady(clk.t, clk.tv)) {  // the anchoring class only (the launcher checks by the same predicate)
                const size_t c = (size_t)(clk.t % (long long)Q);
                la.fbase = coff[c];
                la.flen = coff[c + 1] - coff[c];
            } else {
                la.fbase = 0;
                la.flen = (int)PfT;
            }
            HIP_TRY(launch_matrix_sp_la_chunk(m.log2b, la, s));
            if (m.advance(k, m.B)) clk.block_done();
            done += k;
        }
        return FFTCONV_OK;
    }

    int process_host(const float *in, size_t in_len, float *out, size_t out_len) {
        return matrix_process_host(*this, m, in, in_len, out, out_len);
    }

    int clone_from(const SparseMatrixLookaheadCore &o) {  // #[derive(Clone)]: the windows, the plans and the clock too
        if (int r = m.clone_from(o.m)) return r;
        DeviceGuard g(m.device);
        clk = o.clk;
        PnT = o.PnT;
        PfT = o.PfT;
        std::copy(o.coff, o.coff + Q + 1, coff);
        std::copy(o.class_outputs, o.class_outputs + Q, class_outputs);
        if (int r = clone_buffer(far, o.far, m.stream)) return r;
        if (int r = clone_buffer(nplan, o.nplan, m.stream)) return r;
        if (int r = clone_buffer(fplan, o.fplan, m.stream)) return r;
        if (int r = clone_buffer(d_coff, o.d_coff, m.stream)) return r;
        if (int r = clone_buffer(nwg, o.nwg, m.stream)) return r;
        if (int r = clone_buffer(fwg, o.fwg, m.stream)) return r;
        if (int r = npart.alloc(o.npart.n)) return r;  // (rewritten by every block before it is read)
        HIP_TRY(hipStreamSynchronize(m.stream));
        return FFTCONV_OK;
    }
};

// where a handle's device, StreamOrder and stream (and a matrix's geometry,
// buffers and state) live: the core itself, or a lookahead core's matrix
template <class C>
const C &base(const C &c) { return c; }
template <class C>
C &base(C &c) { return c; }
inline const MatrixCore &base(const MatrixLookaheadCore &c) { return c.m; }
inline MatrixCore &base(MatrixLookaheadCore &c) { return c.m; }
inline const SparseMatrixCore &base(const SparseMatrixLookaheadCore &c) { return c.m; }
inline SparseMatrixCore &base(SparseMatrixLookaheadCore &c) { return c.m; }

// ---------------------------------------------------------------------------
// MatrixCrossfadeCoreT -- P CrossfadeConvolver<FFTConvolver> instances in
// lockstep, one per pair of a dense or a sparse (§4p) matrix: two
// Conv cores A and B on the handle's stream, ONE Crossfader and one
// response_pending for all of them, the mix applied to the per-output sums.
// "Pair" is Conv's pair index throughout (the PairBook, the lists, the stored
// response [P][stored_len]).
//   composition path: A.process_device -> buf_a, B.process_device -> buf_b,
//       crossfade_mix_kernel over the O outputs (always correct)
//   fused path (matrix_xf.hip / matrix_sp_xf.hip), while A and B are in step:
//       one R2C per input for both delay lines, the live convolvers' MAC from
//       one X stream, the finish of each live convolver and the mix in one
//       launch.  A convolver the crossfader has Reached away from is idle: its
//       output is never observed and the next thing that happens to it is
//       update(), which zeroes its pre_multiplied and overlap
//       (src/fft_convolver.rs:186-188), so it carries only its delay line and
//       input buffer forward.
// Conv supplies kName, check_list, rebuild_plan (a swap that changes the target
// convolver's active_seg_count rebuilds what depends on it before that
// convolver's next launch), and the fused launch: XfArgs, xf_args,
// launch_xf_chunk.  Conv's geometry, buffers and block walk are read through
// base(conv): Conv itself, or the matrix a lookahead core wraps,
// whose far-row windows follow the pair through the xf_* hooks -- xf_in_step,
// xf_swapped, xf_chunk_begin, xf_block_done, no-ops for a matrix without windows.
// ---------------------------------------------------------------------------
template <class Conv>
struct MatrixCrossfadeCoreT {
    int device = 0;
    size_t I = 0, O = 0, P = 0, max_buffer_size = 0, stored_len = 0, stored_stride = 0;
    size_t stage_row = 0;  // hstage row: the stored response, or a direct update of a / b
    std::unique_ptr<Conv> a, b;
    Crossfader xf;
    DevPtr<float> buf_a, buf_b, stored;  // stored [P][stored_len]
    DevPtr<float> mix_tab;               // [max_buffer_size + 1] mix_value walk of one call
    bool response_pending = false;
    // A and B have had equal {current, active, fill} and active > 0 at every
    // call since creation: their delay lines and input buffers are equal row
    // for row.  Sticky off (an update to another ceil(len / B) ends it for good).
    bool in_step = false;
    bool fused = true;  // fftconv_matrix[_sparse]_crossfade_set_fused
    // a launch failed between the two convolvers' work: they may be out of
    // step with the host's state.  Every later call fails.
    bool poisoned = false;
    hipStream_t stream = nullptr;
    Scratch scratch;
    mutable StreamOrder order;
    PinnedStage hstage;
    // update_pairs: the diff set D of A and B and the pending
    // partial update's list (host side, pair_book.hpp), the device lists
    PairBook book;
    PairLists lists;

    int check_poisoned() const {
        return poisoned ? fail(FFTCONV_E_DEVICE, std::string(Conv::kName) + " crossfade handle unusable: an earlier process() "
                                                                            "failed between its two convolvers' launches")
                        : FFTCONV_OK;
    }

    ~MatrixCrossfadeCoreT() {
        if (stream) {
            DeviceGuard g(device);
            (void)order.drain(stream);
            a.reset(); b.reset();  // (they borrow `stream`)
            (void)hipStreamDestroy(stream);
        }
    }

    // (Conv's geometry, buffers and block walk are its base()'s: Conv itself, or
    // the matrix a lookahead core wraps)
    bool states_agree() const {
        const auto &ma = base(*a), &mb = base(*b);
        return ma.cur == mb.cur && ma.act == mb.act && ma.fill == mb.fill && ma.act > 0 && a->xf_in_step(*b);
    }
    // the convolver that is not the crossfader's target, and the target
    Conv &other_conv() const { return xf.target == 0 ? *b : *a; }
    Conv &target_conv() const { return xf.target == 0 ? *a : *b; }

    int alloc_buffers(size_t hstage_count) {
        if (int r = stored.alloc(P * stored_len)) return r;
        if (int r = hstage.alloc(hstage_count, stage_row)) return r;
        if (int r = buf_a.alloc(O * max_buffer_size)) return r;
        if (int r = buf_b.alloc(O * max_buffer_size)) return r;
        if (int r = lists.alloc(P)) return r;
        book.init(P);
        return mix_tab.alloc(max_buffer_size + 1);
    }
    // A and B as clones of the two convolvers ca and cb, on this handle's new stream
    int clone_convolvers(const Conv &ca, const Conv &cb) {
        HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        a.reset(new (std::nothrow) Conv());
        b.reset(new (std::nothrow) Conv());
        if (!a || !b) return fail(FFTCONV_E_NOMEM, "out of host memory");
        if (int r = a->clone_from(ca, stream)) return r;
        return b->clone_from(cb, stream);
    }

    // CrossfadeConvolver::new (:19-43)
    int init_new(const Conv &conv, size_t max_response_length, size_t mbs, size_t crossfade_samples) {
        if (mbs > (size_t)INT32_MAX) return fail(FFTCONV_E_UNSUPPORTED, "max_buffer_size exceeds 2^31-1");
        device = base(conv).device;
        I = base(conv).I;
        O = base(conv).O;
        P = base(conv).P;
        DeviceGuard g(device);
        if (int r = clone_convolvers(conv, conv)) return r;
        in_step = states_agree();
        stored_len = max_response_length;
        stored_stride = stored_len;
        stage_row = std::max(stored_len, base(*a).ir_len);
        max_buffer_size = mbs;
        if (int r = alloc_buffers(P * stage_row)) return r;
        if (stored.n) HIP_TRY(hipMemsetAsync(stored.p, 0, stored.bytes(), stream));
        xf.init(crossfade_samples, std::min(mbs, max_response_length));
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }

    int quiesce() const { return order.drain(stream); }
    bool is_crossfading() const { return xf.approaching; }  // :85-92

    // swap (:94-105) from device samples: update the convolver that is not the
    // target (its plan included), then fade into it
    int swap_device(const float *src, size_t stride, size_t len, hipStream_t s) {
        const int to = xf.target == 0 ? 1 : 0;
        if (int r = other_conv().update_device(src, stride, len, s)) return r;
        xf.fade_into(to);
        book.whole_applied();  // every pair of A and B may differ now
        return FFTCONV_OK;
    }

    // The partial swap: update(R') of the convolver T that is
    // not the target, R' = the target's responses with the n listed pairs
    // (`lst`, ascending) replaced at len_active samples, then the fade into T.
    // T's spectra differ from the target's in the pairs of D only, so the pairs
    // of D minus lst are copied from the target's spectra, the listed ones are
    // transformed from `src` (entry k reads row k, or -- by_pair -- row lst[k]),
    // and D = lst.  T's active_seg_count becomes ceil(len_active / B); where
    // that changes it, T's plan is rebuilt behind the stream's earlier launches
    // and ahead of T's next one.  One patch launch; no allocation, no host wait
    // beyond the lists' mirror.
    int swap_pairs_device(const uint32_t *lst, size_t n, const float *src, size_t stride, bool by_pair,
                          size_t len_data, size_t len_active, hipStream_t s) {
        const int to = xf.target == 0 ? 1 : 0;
        auto &t = base(other_conv()), &other = base(target_conv());
        if (len_active > t.ir_len) return fail(FFTCONV_E_INVALID, "New impulse response is longer than initialized length");
        if (int r = lists.acquire()) return r;
        if (n) std::copy(lst, lst + n, lists.tr());
        const size_t n_cp = book.partial_applied(lst, n, lists.cp());
        if (t.ir_len != 0) {
            const size_t act0 = t.act;
            if (int r = t.set_active(ceil_div(len_active, t.B), s)) return r;   // update's side effects (:186-190)
            other_conv().xf_swapped();
            t.last_len = len_active;
            if (t.act != act0)
                if (int r = t.rebuild_plan(s)) return r;
            if (int r = t.patch_device(lists, n, n_cp, other.H.p, src, stride, by_pair, len_data, len_active, s)) return r;
        }
        xf.fade_into(to);
        return FFTCONV_OK;
    }

    // the pending response, whole or partial, into the convolver that is not the target
    int apply_pending(hipStream_t s) {
        if (!book.partial) return swap_device(stored.p, stored_stride, stored_len, s);
        const size_t n = book.pending_list(lists.idx.data());
        if (int r = swap_pairs_device(lists.idx.data(), n, stored.p, stored_len, true, stored_len, stored_len, s)) return r;
        book.clear_pending();
        return FFTCONV_OK;
    }

    // rows k of a listed update (`len` samples each, on the host or the device)
    // to the stored response's rows lst[k], zero-padded to stored_len
    int store_rows(const uint32_t *lst, size_t n, const float *src, bool d_src, size_t len, size_t stride, hipStream_t s) {
        for (size_t k0 = 0; k0 < n;) {
            size_t k1 = k0 + 1;
            while (k1 < n && lst[k1] == lst[k1 - 1] + 1) ++k1;
            float *dst = stored.p + (size_t)lst[k0] * stored_len;
            if (len < stored_len) HIP_TRY(hipMemsetAsync(dst, 0, (k1 - k0) * stored_len * sizeof(float), s));
            if (len && d_src) {
                if (stride >= len) {
                    HIP_TRY(hipMemcpy2DAsync(dst, stored_len * sizeof(float), src + k0 * stride, stride * sizeof(float),
                                             len * sizeof(float), k1 - k0, hipMemcpyDeviceToDevice, s));
                } else {  // (stride 0: one response for every listed pair)
                    for (size_t k = k0; k < k1; ++k)
                        HIP_TRY(hipMemcpyAsync(dst + (k - k0) * stored_len, src + k * stride, len * sizeof(float),
                                               hipMemcpyDeviceToDevice, s));
                }
            }
            k0 = k1;
        }
        if (len && !d_src) return hstage.upload_scatter(src, n, len, stride, stored.p, stored_len, lst, s);
        return FFTCONV_OK;
    }

    // update_pairs: update(R'), R' = the base set with the listed pairs replaced
    // (DESIGN §4o, §4p).  `s` is ordered behind the handle's previous work.
    int update_pairs(size_t n, const uint32_t *pair_out, const uint32_t *pair_in, const float *src, bool d_src,
                     size_t len, size_t stride, hipStream_t s) {
        if (int r = check_poisoned()) return r;
        uint32_t *lst = lists.idx.data();
        if (int r = base(*a).check_list(n, pair_out, pair_in, lst)) return r;
        auto &t = base(other_conv()), &tgt = base(target_conv());
        const bool fading = is_crossfading();
        DeviceGuard g(device);
        if (!fading && !response_pending) {
            // the base set is the target convolver's, at the length it was applied at
            const size_t lenp = tgt.last_len;
            if (len > lenp)
                return fail(FFTCONV_E_INVALID, "update_pairs: response longer than the length the response set was applied at");
            if (int r = order.enter(s)) return r;
            if (!d_src && len && n && t.ir_len) {
                const bool shared = stride == 0 && n > 1;
                if (int r = hstage.upload(src, shared ? 1 : n, len, stride, t.staging.p, t.ir_len, s)) return r;
                return swap_pairs_device(lst, n, t.staging.p, shared ? 0 : t.ir_len, false, len, lenp, s);
            }
            return swap_pairs_device(lst, n, src, stride, false, len, lenp, s);
        }
        // the base set is, or becomes, a stored response of stored_len samples
        if (len > stored_len)
            return fail(FFTCONV_E_INVALID, fading ? "assertion failed: response_len <= self.stored_response.len()"
                                                  : "update_pairs: response longer than the stored response");
        const bool whole = response_pending && !book.partial;
        if (!whole && ceil_div(stored_len, tgt.B) != tgt.act)
            return fail(FFTCONV_E_UNSUPPORTED, "update_pairs during a fade: the stored length gives another active segment "
                                               "count than the base convolver's, so zero-padding cannot reproduce update()");
        if (!fading && stored_len > t.ir_len)
            return fail(FFTCONV_E_INVALID, "New impulse response is longer than initialized length");
        if (int r = order.enter(s)) return r;
        if (whole && stored_stride == 0 && P > 1) {
            // a shared stored response: every pair gets its own row first
            for (size_t k = 1; k < P; k *= 2)
                HIP_TRY(hipMemcpyAsync(stored.p + k * stored_len, stored.p, std::min(k, P - k) * stored_len * sizeof(float),
                                       hipMemcpyDeviceToDevice, s));
            stored_stride = stored_len;
        }
        if (int r = store_rows(lst, n, src, d_src, len, stride, s)) return r;
        if (!whole) {
            book.merge_pending(lst, n);  // (a pair listed twice: the later rows have replaced the earlier ones)
            stored_stride = stored_len;
        }
        response_pending = true;
        if (!fading) {  // the fade has ended: update(R') swaps at once
            if (int r = apply_pending(s)) return r;
            response_pending = false;
        }
        return FFTCONV_OK;
    }

    // Convolution::update (:51-64) from host samples (pair p at src + p * stride,
    // stride 0 = one response for every pair); staged in pinned memory and
    // enqueued behind the handle's work: no allocation, no host wait
    int update_host(const float *src, size_t len, size_t stride) {
        if (int r = check_poisoned()) return r;
        DeviceGuard g(device);
        const bool shared = stride == 0 && P > 1;
        const size_t rows = shared ? 1 : P;
        if (!is_crossfading()) {
            auto &t = base(other_conv());
            if (len > t.ir_len) return fail(FFTCONV_E_INVALID, "New impulse response is longer than initialized length");
            if (int r = order.enter(stream)) return r;
            if (len)
                if (int r = hstage.upload(src, rows, len, stride, t.staging.p, t.ir_len, stream)) return r;
            if (int r = swap_device(t.staging.p, shared ? 0 : t.ir_len, len, stream)) return r;
            response_pending = false;
            book.clear_pending();
            return FFTCONV_OK;
        }
        if (len > stored_len) return fail(FFTCONV_E_INVALID, "assertion failed: response_len <= self.stored_response.len()");
        if (int r = order.enter(stream)) return r;
        // stored_response[..len] = response; stored_response[len..] = 0
        if (stored.n) HIP_TRY(hipMemsetAsync(stored.p, 0, stored.bytes(), stream));
        if (len)
            if (int r = hstage.upload(src, rows, len, stride, stored.p, stored_len, stream)) return r;
        stored_stride = shared ? 0 : stored_len;
        response_pending = true;
        book.clear_pending();  // (a whole response replaces a pending partial one)
        return FFTCONV_OK;
    }

    // Convolution::update (:51-64) from device samples, stream-ordered (the
    // caller has ordered s behind the handle's previous work)
    int update_device(const float *src, size_t stride, size_t len, hipStream_t s) {
        if (int r = check_poisoned()) return r;
        if (!is_crossfading()) {
            if (int r = swap_device(src, stride, len, s)) return r;
            response_pending = false;
            book.clear_pending();
            return FFTCONV_OK;
        }
        if (len > stored_len) return fail(FFTCONV_E_INVALID, "assertion failed: response_len <= self.stored_response.len()");
        const bool shared = stride == 0 && P > 1;
        if (stored.n) HIP_TRY(hipMemsetAsync(stored.p, 0, stored.bytes(), s));
        if (len)
            HIP_TRY(hipMemcpy2DAsync(stored.p, stored_len * sizeof(float), src, (shared ? len : std::max(stride, len)) * sizeof(float),
                                     len * sizeof(float), shared ? 1 : P, hipMemcpyDeviceToDevice, s));
        stored_stride = shared ? 0 : stored_len;
        response_pending = true;
        book.clear_pending();  // (a whole response replaces a pending partial one)
        return FFTCONV_OK;
    }

    CrossfadeMixArgs mix_args(float *dout, size_t os, size_t out_len) const {
        CrossfadeMixArgs x{};
        x.buf_a = buf_a.p; x.buf_b = buf_b.p; x.buf_stride = (long long)max_buffer_size;
        x.out = dout; x.out_stride = (long long)os; x.n = (int)out_len;
        x.approaching = xf.approaching ? 1 : 0; x.target = xf.target;
        x.counter0 = xf.counter; x.fading = xf.fading_samples;
        x.mix_value0 = xf.mix_value; x.step = xf.mix_value_step;
        return x;
    }

    // 0 = composition, 1 = fused with both convolvers live, 2 = fused with one
    // idle: a function of the handle's state only
    int path_now() const {
        if (!fused || !in_step || !states_agree()) return 0;
        return xf.approaching ? 1 : 2;
    }
    // the path the next process() takes: a pending swap is applied first, and
    // the path follows from the updated convolver's NEW active_seg_count
    int path_next() const {
        if (!is_crossfading() && response_pending) {
            const auto &t = base(other_conv()), &other = base(target_conv());
            if (t.ir_len == 0 || stored_len > t.ir_len) return path_now();  // (the update changes nothing)
            const size_t act = ceil_div(stored_len, t.B);
            return fused && in_step && act > 0 && act == other.act && t.cur == other.cur && t.fill == other.fill &&
                           a->xf_in_step(*b)
                       ? 1
                       : 0;
        }
        return path_now();
    }

    // Convolution::process (:66-78): both convolvers advance by max_buffer_size
    // samples, the first out_len mixed samples are written
    int process_device(const float *din, size_t is, float *dout, size_t os, size_t out_len, hipStream_t s) {
        if (int r = check_poisoned()) return r;
        if (out_len > max_buffer_size) return fail(FFTCONV_E_INVALID, "output longer than max_buffer_size (index out of bounds)");
        if (!is_crossfading() && response_pending) {                    // :67-70
            if (int r = apply_pending(s)) return r;
            response_pending = false;
        }
        const size_t m = max_buffer_size;
        if (m == 0) return FFTCONV_OK;
        in_step = in_step && states_agree();
        CrossfadeMixArgs mx = mix_args(dout, os, out_len);
        if (path_now() == 0) {
            if (int r = a->process_device(din, is, buf_a.p, m, m, s)) return r;    // :72
            if (int r = b->process_device(din, is, buf_b.p, m, m, s)) {            // :73
                poisoned = true;
                return r;
            }
            if (out_len > 1024 && mx.approaching) {
                HIP_TRY(launch_crossfade_walk(mx, mix_tab.p, s));
                mx.vtab = mix_tab.p;
            }
            HIP_TRY(launch_crossfade_mix(mx, (int)O, s));                          // :75-77
            xf.advance(out_len);
            return FFTCONV_OK;
        }
        if (mx.approaching) mx.vtab = mix_tab.p;  // the call's mix_value walk: launch A of the first chunk fills it
        typename Conv::XfArgs x{};
        auto &ma = base(*a), &mb = base(*b);
        const decltype(&ma) cv[2] = {&ma, &mb};
        for (int c = 0; c < 2; ++c) {
            x.H[c] = cv[c]->H.p; x.X[c] = cv[c]->X.p; x.ovl[c] = cv[c]->ovl.p; x.ib[c] = cv[c]->ib.p;
            x.pre[c] = cv[c]->pre.p; x.part[c] = cv[c]->part.p;
        }
        x.tw = ma.tw.p;
        x.in_stride = (long long)is;
        x.out_stride = (long long)os;
        x.I = (int)I; x.O = (int)O; x.S = (int)ma.S;
        x.act = (int)ma.act;
        x.nt_h = Variant::current().nt_matrix(ma.H.bytes()) ? 1 : 0;
        x.live = xf.approaching ? 3 : (xf.target == 0 ? 1 : 2);
        x.mix = mx;
        a->xf_args(x);
        for (size_t done = 0; done < m;) {                              // FFTConvolver::process :222-294, A and B at once
            const size_t k = ma.chunk(m - done, ma.B);
            x.in = din + done;
            x.out = dout + done;
            x.cur = (int)ma.cur;
            x.fill = (int)ma.fill;
            x.k = (int)k;
            x.off = (int)done;
            x.walk = done == 0 && mx.approaching ? mix_tab.p : nullptr;
            Conv::xf_chunk_begin(x, *a, *b);
            if (hipError_t e = Conv::launch_xf_chunk(ma.log2b, x, s); e != hipSuccess) {
                poisoned = true;
                HIP_TRY(e);
            }
            if (ma.advance(k, ma.B)) Conv::xf_block_done(*a, *b);
            mb.fill = ma.fill;
            mb.cur = ma.cur;
            done += k;
        }
        xf.advance(out_len);
        return FFTCONV_OK;
    }

    int process_host(const float *in, size_t in_len, float *out, size_t out_len) {
        if (in_len < max_buffer_size) return fail(FFTCONV_E_INVALID, "input shorter than max_buffer_size (range end index out of range)");
        if (out_len > max_buffer_size) return fail(FFTCONV_E_INVALID, "output longer than max_buffer_size (index out of bounds)");
        if (int r = check_poisoned()) return r;
        DeviceGuard g(device);
        if (int r = order.enter(stream)) return r;
        const size_t m = max_buffer_size, on = std::max<size_t>(out_len, 1);
        if (int r = scratch.ensure(I * std::max<size_t>(m, 1), O * on)) return r;
        if (m)
            HIP_TRY(hipMemcpy2DAsync(scratch.in.p, m * sizeof(float), in, in_len * sizeof(float), m * sizeof(float), I,
                                     hipMemcpyHostToDevice, stream));
        if (int r = process_device(scratch.in.p, m, scratch.out.p, on, out_len, stream)) return r;
        if (out_len && m)
            HIP_TRY(hipMemcpy2DAsync(out, out_len * sizeof(float), scratch.out.p, on * sizeof(float),
                                     out_len * sizeof(float), O, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }

    int clone_from(const MatrixCrossfadeCoreT &o) {
        DeviceGuard g(o.device);
        if (int r = o.order.drain(o.stream)) return r;
        device = o.device; I = o.I; O = o.O; P = o.P; max_buffer_size = o.max_buffer_size;
        stored_len = o.stored_len; stored_stride = o.stored_stride; stage_row = o.stage_row;
        xf = o.xf; response_pending = o.response_pending;
        in_step = o.in_step; fused = o.fused; poisoned = o.poisoned;
        if (int r = clone_convolvers(*o.a, *o.b)) return r;
        if (int r = alloc_buffers(o.hstage.n)) return r;
        book.copy_from(o.book);
        if (stored.n) HIP_TRY(hipMemcpyAsync(stored.p, o.stored.p, stored.bytes(), hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }
};
using MatrixCrossfadeCore = MatrixCrossfadeCoreT<MatrixCore>;
using SparseMatrixCrossfadeCore = MatrixCrossfadeCoreT<SparseMatrixCore>;
// (A and B are lookahead matrices; the fused launch is matrix_la_xf.hip's)
using MatrixLookaheadCrossfadeCore = MatrixCrossfadeCoreT<MatrixLookaheadCore>;


// ---------------------------------------------------------------------------
// MatrixTwoStageCoreT -- P TwoStageFFTConvolver instances in lockstep, one per
// pair of the matrix Conv (the dense matrix's O * I pairs; §4r: the
// N listed pairs of a sparse pattern): up to three Convs (head, tail0, tail) on
// the handle's stream, ONE {tail_input_fill, precalculated_pos} for all of
// them, the four tail buffers summed per output [O][T], tail_input per input
// [I][T].
//   composition path: TwoStageCore::process_device's sub-chunk loop
//       (src/fft_convolver.rs:412-495) with matrices for convolvers (always
//       correct)
//   fused path (matrix_ts.hip / matrix_sp_ts.hip), at an aligned call: head, the
//       sub-chunk's sums and copy, and tail0 in the plain matrix's two launches,
//       every delay-line row streamed once for both responses.  Head and tail0
//       count samples modulo B from the same start, so at an aligned call their
//       last S rows are transforms of the same input blocks whatever ragged
//       calls came before.
// Everything is enqueued on one stream in stream order; the tail's block-T
// convolution at the end of a period is enqueued inline, where the reference
// runs it (:479-486).
// Conv supplies kName, init / clone_from with an owner stream, and the fused
// launch: TsArgs, ts_args, ts_plan_equal (head and tail0 walk the same MAC
// grid), launch_ts_block.
// ---------------------------------------------------------------------------
template <class Conv>
struct MatrixTwoStageCoreT {
    int device = 0;
    size_t I = 0, O = 0, P = 0, head_bs = 0, T = 0;  // P: pairs
    std::unique_ptr<Conv> head, tail0, tail;  // null = the reference's Default convolver (zeros): skipped
    DevPtr<float> out0, pre0, out1, pre1;           // [O][T] each
    DevPtr<float> tin;                              // tail_input [I][T]
    float *tail_output0 = nullptr, *tail_precalculated0 = nullptr;
    float *tail_output = nullptr, *tail_precalculated = nullptr;
    size_t tail_input_fill = 0, precalculated_pos = 0;
    bool fused = true;  // fftconv_matrix[_sparse]_twostage_set_fused
    // a launch failed inside a call: the stages may be out of step with the
    // host's scalars.  Every later call fails.
    bool poisoned = false;
    hipStream_t stream = nullptr;
    Scratch scratch;
    mutable StreamOrder order;

    ~MatrixTwoStageCoreT() {
        if (stream) {
            DeviceGuard g(device);
            (void)order.drain(stream);
            head.reset(); tail0.reset(); tail.reset();  // (they borrow `stream`)
            (void)hipStreamDestroy(stream);
        }
    }

    int check_poisoned() const {
        return poisoned ? fail(FFTCONV_E_DEVICE, std::string(Conv::kName) + " two-stage handle unusable: an earlier "
                                                                            "process() failed between its stages' launches")
                        : FFTCONV_OK;
    }

    int alloc_buffers() {
        for (auto *b : {&out0, &pre0, &out1, &pre1}) {
            if (int r = b->alloc(O * T)) return r;
            HIP_TRY(hipMemsetAsync(b->p, 0, b->bytes(), stream));
        }
        if (int r = tin.alloc(I * T)) return r;
        HIP_TRY(hipMemsetAsync(tin.p, 0, tin.bytes(), stream));
        tail_output0 = out0.p; tail_precalculated0 = pre0.p;
        tail_output = out1.p; tail_precalculated = pre1.p;
        return FFTCONV_OK;
    }

    // TwoStageFFTConvolver::init (:340-406) of every instance.  The dense
    // matrix: pair (o, i) = o * I + i.
    int init(int dev, size_t inputs, size_t outputs, const float *responses, size_t len, size_t stride,
             size_t block_size, size_t max_len) {
        if (inputs == 0 || outputs == 0) return fail(FFTCONV_E_INVALID, "a matrix needs at least one input and one output");
        return init_stages(dev, inputs, outputs, inputs * outputs, responses, len, stride, block_size, max_len,
                           [&](Conv &m, const float *rows, size_t cnt, size_t row_stride, size_t block) {
                               return m.init(dev, I, O, rows, cnt, row_stride, block, cnt, stream);
                           });
    }
    // The sparse matrix: the listed pairs, responses in list order.
    int init(int dev, size_t inputs, size_t outputs, size_t pairs, const uint32_t *po, const uint32_t *pi,
             const float *responses, size_t len, size_t stride, size_t block_size, size_t max_len) {
        if (int r = Conv::check_pattern(inputs, outputs, pairs, po, pi)) return r;
        return init_stages(dev, inputs, outputs, pairs, responses, len, stride, block_size, max_len,
                           [&](Conv &m, const float *rows, size_t cnt, size_t row_stride, size_t block) {
                               return m.init(dev, I, O, pairs, po, pi, rows, cnt, row_stride, block, cnt, stream);
                           });
    }

    // `stage_init(m, rows, cnt, row_stride, block)`: Conv::init of one stage from its slices
    template <class StageInit>
    int init_stages(int dev, size_t inputs, size_t outputs, size_t pairs, const float *responses, size_t len,
                    size_t stride, size_t block_size, size_t max_len, StageInit stage_init) {
        if (max_len < len)                                                      // :344-348
            return fail(FFTCONV_E_INVALID,
                        "max_response_length must be at least the length of the initial impulse response");
        head_bs = block_size;                                                   // :341
        T = fftconv_compute_tail_block_size(block_size, max_len);              // :342
        const size_t B = next_pow2(block_size);
        if (B < 32 || B > 8192)
            return fail(FFTCONV_E_UNSUPPORTED, "matrix block size " + std::to_string(B) + " outside 32..8192");
        if (T > 8192)  // (the tail is a matrix of block T)
            return fail(FFTCONV_E_UNSUPPORTED, "matrix tail block size " + std::to_string(T) + " exceeds 8192");
        if (inputs > (size_t)INT32_MAX / T || outputs > (size_t)INT32_MAX / T)
            return fail(FFTCONV_E_UNSUPPORTED, "geometry exceeds 32-bit indexing");
        if (int r = check_device(dev)) return r;
        device = dev;
        I = inputs;
        O = outputs;
        P = pairs;
        DeviceGuard g(dev);
        HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        // padded_ir = each pair's response zero-extended to max_len (:349-350);
        // the sub-ranges are cut on the host, one row per pair, so each stage
        // sees its reference slice
        const bool shared = stride == 0 && pairs > 1;
        std::vector<float> tmp;
        auto stage = [&](std::unique_ptr<Conv> &m, size_t off, size_t cnt, size_t block) -> int {
            const size_t rows = shared ? 1 : pairs;
            tmp.assign(rows * std::max<size_t>(cnt, 1), 0.f);
            for (size_t p = 0; p < rows; ++p)
                for (size_t j = 0; j < cnt && off + j < len; ++j) tmp[p * cnt + j] = responses[p * stride + off + j];
            m.reset(new (std::nothrow) Conv());
            if (!m) return fail(FFTCONV_E_NOMEM, "out of host memory");
            return stage_init(*m, tmp.data(), cnt, shared ? 0 : cnt, block);
        };
        if (int r = stage(head, 0, std::min(max_len, T), head_bs)) return r;             // :352-354
        if (max_len > T)                                                                  // :356-368
            if (int r = stage(tail0, T, std::min(max_len - T, T), head_bs)) return r;
        if (max_len > 2 * T)                                                              // :373-384
            if (int r = stage(tail, 2 * T, max_len - 2 * T, T)) return r;
        if (int r = alloc_buffers()) return r;
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }

    // 1 = the next process() of `len` samples takes the fused path: the call
    // is aligned (a whole power-of-two head block on a block boundary of the
    // period, both input buffers empty), tail0 exists, and head and tail0 walk
    // the same rows.  A function of the geometry, the calls so far and `fused`,
    // never of `outputs`.
    int path(size_t len) const {
        if (!fused || !tail0) return 0;
        const Conv &h = *head, &t = *tail0;
        return len == head_bs && head_bs == h.B && tail_input_fill % h.B == 0 && tail_input_fill + len <= T &&
                       h.fill == 0 && t.fill == 0 && h.S == t.S && h.act == t.act && h.act > 0 && h.cur == t.cur &&
                       h.ts_plan_equal(t)
                   ? 1
                   : 0;
    }

    // fill reached T (:473-491): both swaps, then the tail's block-T convolution
    // of this period, inline
    int end_of_period(hipStream_t s) {
        std::swap(tail_precalculated0, tail_output0);                           // :473-475
        std::swap(tail_precalculated, tail_output);                             // :483
        if (tail)                                                               // :484-485
            if (int r = tail->process_device(tin.p, T, tail_output, T, T, s)) return r;
        tail_input_fill = 0;                                                    // :488-491
        precalculated_pos = 0;
        return FFTCONV_OK;
    }

    int process_composed(const float *din, size_t is, float *dout, size_t os, size_t len, hipStream_t s) {
        if (int r = head->process_device(din, is, dout, os, len, s)) return r;     // :417
        size_t processed = 0;
        while (processed < len) {                                                   // :427
            const size_t processing = std::min(len - processed, head_bs - (tail_input_fill % head_bs));
            if (tail_input_fill + processing > T)  // tail_input[fill..fill+processing] out of range (:459-460)
                return fail(FFTCONV_E_INVALID, "range end index out of range for slice of length tail_block_size");
            MatrixTsAccumArgs a{};
            a.out = dout; a.out_stride = (long long)os;
            a.p0 = tail0 ? tail_precalculated0 : nullptr;
            a.p1 = tail ? tail_precalculated : nullptr;
            a.T = (long long)T; a.pos = (int)precalculated_pos;
            a.in = din; a.in_stride = (long long)is; a.sb = (int)processed;
            a.tail_input = tin.p; a.fill = (int)tail_input_fill; a.cnt = (int)processing;
            a.I = (int)I; a.O = (int)O;
            HIP_TRY(launch_matrix_ts_accum(a, s));                                  // :438-461
            precalculated_pos += processing;
            tail_input_fill += processing;
            if (tail_input_fill % head_bs == 0 && tail0) {                          // :464-472
                const size_t off = tail_input_fill - head_bs;
                if (int r = tail0->process_device(tin.p + off, T, tail_output0 + off, T, head_bs, s)) return r;
            }
            if (tail_input_fill == T)
                if (int r = end_of_period(s)) return r;
            processed += processing;
        }
        return FFTCONV_OK;
    }

    int process_fused(const float *din, size_t is, float *dout, size_t os, hipStream_t s) {
        Conv &h = *head, &t = *tail0;
        typename Conv::TsArgs x{};
        const Conv *cv[2] = {&h, &t};
        for (int c = 0; c < 2; ++c) {
            x.H[c] = cv[c]->H.p; x.X[c] = cv[c]->X.p; x.ovl[c] = cv[c]->ovl.p; x.part[c] = cv[c]->part.p;
        }
        x.tw = h.tw.p;
        x.in = din; x.in_stride = (long long)is;
        x.out = dout; x.out_stride = (long long)os;
        x.tin = tin.p + tail_input_fill;                                        // :459-461
        x.tout0 = tail_output0 + tail_input_fill;                               // :468-472
        x.p0 = tail_precalculated0 + precalculated_pos;                         // :439-445
        x.p1 = tail ? tail_precalculated + precalculated_pos : nullptr;         // :448-454
        x.T = (long long)T;
        x.I = (int)I; x.O = (int)O; x.S = (int)h.S;
        h.ts_args(x);
        x.cur = (int)h.cur;
        x.act = (int)h.act;
        x.nt_h = Variant::current().nt_matrix(h.H.bytes()) ? 1 : 0;
        HIP_TRY(Conv::launch_ts_block(h.log2b, x, s));
        // a whole block (:277-291 of both); the fused path is taken at h.fill == 0 only (path()),
        // so this always completes the block and steps `current`
        h.advance(h.B, h.B);
        t.cur = h.cur;
        precalculated_pos += head_bs;
        tail_input_fill += head_bs;
        if (tail_input_fill == T) return end_of_period(s);
        return FFTCONV_OK;
    }

    // TwoStageFFTConvolver::process (:412-495) of every instance
    int process_device(const float *din, size_t is, float *dout, size_t os, size_t len, hipStream_t s) {
        if (int r = check_poisoned()) return r;
        if (len > head_bs) return fail(FFTCONV_E_INVALID, "assertion failed: input.len() <= self.head_block_size");
        if (len == 0) return FFTCONV_OK;
        const int r = path(len) ? process_fused(din, is, dout, os, s) : process_composed(din, is, dout, os, len, s);
        if (r == FFTCONV_E_DEVICE) poisoned = true;
        return r;
    }

    int process_device_steps(const float *din, size_t is, size_t in_step, float *dout, size_t os, size_t out_step,
                             size_t len, size_t steps, hipStream_t s) {
        for (size_t k = 0; k < steps; ++k)
            if (int r = process_device(din + k * in_step, is, dout + k * out_step, os, len, s)) return r;
        return FFTCONV_OK;
    }

    int process_host(const float *in, float *out, size_t len) {
        if (int r = check_poisoned()) return r;
        if (len > head_bs) return fail(FFTCONV_E_INVALID, "assertion failed: input.len() <= self.head_block_size");
        if (len == 0) return FFTCONV_OK;
        DeviceGuard g(device);
        if (int r = order.enter(stream)) return r;
        if (int r = scratch.ensure(I * len, O * len)) return r;
        HIP_TRY(hipMemcpyAsync(scratch.in.p, in, I * len * sizeof(float), hipMemcpyHostToDevice, stream));
        if (int r = process_device(scratch.in.p, len, scratch.out.p, len, len, stream)) return r;
        HIP_TRY(hipMemcpyAsync(out, scratch.out.p, O * len * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }

    int reset() {  // :497-511
        if (int r = check_poisoned()) return r;
        DeviceGuard g(device);
        if (int r = order.enter(stream)) return r;
        for (auto *m : {head.get(), tail0.get(), tail.get()})
            if (m)
                if (int r = m->zero_state(stream)) return r;
        for (auto *b : {&out0, &pre0, &out1, &pre1, &tin}) HIP_TRY(hipMemsetAsync(b->p, 0, b->bytes(), stream));
        tail_input_fill = 0;
        precalculated_pos = 0;
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }

    // #[derive(Clone)]: a deep device-side copy, including which buffer
    // currently plays tail_output* / tail_precalculated*
    int clone_from(const MatrixTwoStageCoreT &o) {
        DeviceGuard g(o.device);
        if (int r = o.order.drain(o.stream)) return r;
        device = o.device; I = o.I; O = o.O; P = o.P; head_bs = o.head_bs; T = o.T;
        fused = o.fused; poisoned = o.poisoned;
        HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        auto cl = [&](std::unique_ptr<Conv> &dst, const std::unique_ptr<Conv> &src) -> int {
            if (!src) return FFTCONV_OK;
            dst.reset(new (std::nothrow) Conv());
            if (!dst) return fail(FFTCONV_E_NOMEM, "out of host memory");
            return dst->clone_from(*src, stream);
        };
        if (int r = cl(head, o.head)) return r;
        if (int r = cl(tail0, o.tail0)) return r;
        if (int r = cl(tail, o.tail)) return r;
        if (int r = alloc_buffers()) return r;
        auto map = [&](const float *p) -> float * {  // same role, this instance's buffer
            if (p == o.out0.p) return out0.p;
            if (p == o.pre0.p) return pre0.p;
            if (p == o.out1.p) return out1.p;
            return pre1.p;
        };
        tail_output0 = map(o.tail_output0); tail_precalculated0 = map(o.tail_precalculated0);
        tail_output = map(o.tail_output); tail_precalculated = map(o.tail_precalculated);
        const std::pair<DevPtr<float> *, const DevPtr<float> *> bufs[] = {
            {&out0, &o.out0}, {&pre0, &o.pre0}, {&out1, &o.out1}, {&pre1, &o.pre1}, {&tin, &o.tin}};
        for (auto &b : bufs)
            HIP_TRY(hipMemcpyAsync(b.first->p, b.second->p, b.second->bytes(), hipMemcpyDeviceToDevice, stream));
        tail_input_fill = o.tail_input_fill;
        precalculated_pos = o.precalculated_pos;
        HIP_TRY(hipStreamSynchronize(stream));
        return FFTCONV_OK;
    }
};
using MatrixTwoStageCore = MatrixTwoStageCoreT<MatrixCore>;
using SparseMatrixTwoStageCore = MatrixTwoStageCoreT<SparseMatrixCore>;

// W_N^k tables of the stand-alone Fft entry points, one per (device, N),
// built on first use in f64 and kept for the process (the handles keep
// their own); the same values as every handle's table for that N.  The first
// use uploads on the caller's stream and waits for that stream only (no
// legacy-stream synchronisation).
int fft_twiddles(int dev, int log2n, hipStream_t s, const float2 **out) {
    static std::mutex mu;
    static std::map<std::pair<int, int>, float2 *> tabs;
    std::lock_guard<std::mutex> lk(mu);
    auto it = tabs.find({dev, log2n});
    if (it != tabs.end()) {
        *out = it->second;
        return FFTCONV_OK;
    }
    const size_t N = (size_t)1 << log2n;
    std::vector<float2> t(N);
    for (size_t k = 0; k < N; ++k) {
        const double ang = -2.0 * M_PI * (double)k / (double)N;
        t[k] = make_float2((float)std::cos(ang), (float)std::sin(ang));
    }
    float2 *p = nullptr;
    HIP_TRY(hipMalloc((void **)&p, N * sizeof(float2)));
    hipError_t e = poison_table(p, N * sizeof(float2));
    if (e == hipSuccess) e = hipMemcpyAsync(p, t.data(), N * sizeof(float2), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // (t is freed on return)
    if (e != hipSuccess) {
        (void)hipFree(p);
        return fail(FFTCONV_E_DEVICE, std::string("twiddle upload: ") + hipGetErrorString(e));
    }
    tabs[{dev, log2n}] = p;
    *out = p;
    return FFTCONV_OK;
}

// The long-block path's tables for M = 2^log2m (lg_split: M = M1 x M2), one
// set per (device, M), built in f64 and rounded to f32 like every other
// table: W_M^j (j < M), W_{2 M1}^i (i < 2 M1), W_{2 M2}^i (i < 2 M2).  The
// caller sets twN (its W_N table).  Synchronous upload on first use.
int lg_tables(int dev, int log2m, LgTab *out) {
    static std::mutex mu;
    static std::map<std::pair<int, int>, float2 *> tabs;
    std::lock_guard<std::mutex> lk(mu);
    int l1 = 0, l2 = 0;
    lg_split(log2m, &l1, &l2);
    const size_t M = (size_t)1 << log2m, A = (size_t)2 << l1, Bt = (size_t)2 << l2;
    auto it = tabs.find({dev, log2m});
    float2 *p = nullptr;
    if (it != tabs.end()) {
        p = it->second;
    } else {
        std::vector<float2> t(M + A + Bt);
        auto fill = [&](float2 *dst, size_t n, size_t period) {
            for (size_t k = 0; k < n; ++k) {
                const double ang = -2.0 * M_PI * (double)k / (double)period;
                dst[k] = make_float2((float)std::cos(ang), (float)std::sin(ang));
            }
        };
        fill(t.data(), M, M);
        fill(t.data() + M, A, A);
        fill(t.data() + M + A, Bt, Bt);
        HIP_TRY(hipMalloc((void **)&p, t.size() * sizeof(float2)));
        hipError_t e = poison_table(p, t.size() * sizeof(float2));
        if (e == hipSuccess) e = hipMemcpy(p, t.data(), t.size() * sizeof(float2), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return fail(FFTCONV_E_DEVICE, std::string("twiddle upload: ") + hipGetErrorString(e));
        }
        tabs[{dev, log2m}] = p;
    }
    out->twN = nullptr;
    out->twM = p;
    out->twA = p + M;
    out->twB = p + M + A;
    return FFTCONV_OK;
}

// Bluestein tables of a length n that is not a power of two (the public Fft
// of any length, launch_fft_bluestein): the chirp w_m = exp(i pi m^2 / n)
// (m^2 mod 2n in integers, the angle in f64) and the spectrum of the chirp
// filter b (b_m = b_{P-m} = w_m, m < n) by an f64 FFT on the host, both
// rounded to f32 once; the filter in the device FFT's bin order.  One set per
// (device, n) in a cache of at most kBluesteinCacheBytes of device memory:
// the least recently used sets are freed when a new length would pass it.
// The caller holds bluestein_mutex() from this lookup until its kernels are
// enqueued, so a set being freed was last used by work already on a stream,
// and the eviction waits for that device before hipFree.  The first use of a
// length uploads on the caller's stream and waits for that stream only.
constexpr size_t kMaxBluestein = (size_t)1 << 21;  // P = 2^22 at most
constexpr size_t kBluesteinCacheBytes = (size_t)256 << 20;
std::mutex &bluestein_mutex() {
    static std::mutex mu;
    return mu;
}
int bluestein_tables(int dev, size_t n, int log2p, hipStream_t s, const float2 **chirp, const float2 **filt) {
    struct Tab { float2 *p; size_t bytes; unsigned long long used; };
    static std::map<std::pair<int, size_t>, Tab> tabs;
    static size_t total = 0;
    static unsigned long long clock = 0;
    const size_t P = (size_t)1 << log2p;
    auto it = tabs.find({dev, n});
    if (it == tabs.end()) {
        const size_t bytes = (n + P) * sizeof(float2);
        while (!tabs.empty() && total + bytes > kBluesteinCacheBytes) {
            auto lru = tabs.begin();
            for (auto j = tabs.begin(); j != tabs.end(); ++j)
                if (j->second.used < lru->second.used) lru = j;
            DeviceGuard g(lru->first.first);
            (void)hipDeviceSynchronize();  // kernels enqueued with this set have finished
            (void)hipFree(lru->second.p);
            total -= lru->second.bytes;
            tabs.erase(lru);
        }
        std::vector<double> wr(n), wi(n);
        for (size_t m = 0; m < n; ++m) {
            const unsigned long long q = ((unsigned long long)m * m) % (2ull * n);
            const double ang = M_PI * (double)q / (double)n;
            wr[m] = std::cos(ang);
            wi[m] = std::sin(ang);
        }
        std::vector<double> br(P, 0.0), bi(P, 0.0);
        for (size_t m = 0; m < n; ++m) {
            br[m] = wr[m];
            bi[m] = wi[m];
            if (m) {
                br[P - m] = wr[m];
                bi[P - m] = wi[m];
            }
        }
        // forward DFT of b in f64: iterative radix-2, exp(-2 pi i / len) per stage
        for (size_t i = 1, j = 0; i < P; ++i) {
            size_t bit = P >> 1;
            for (; j & bit; bit >>= 1) j ^= bit;
            j ^= bit;
            if (i < j) {
                std::swap(br[i], br[j]);
                std::swap(bi[i], bi[j]);
            }
        }
        for (size_t len = 2; len <= P; len <<= 1) {
            const size_t h = len / 2;
            for (size_t k = 0; k < h; ++k) {
                const double ang = -2.0 * M_PI * (double)k / (double)len;
                const double c = std::cos(ang), sn = std::sin(ang);
                for (size_t b0 = 0; b0 < P; b0 += len) {
                    const size_t u = b0 + k, v = u + h;
                    const double tr = br[v] * c - bi[v] * sn, ti = br[v] * sn + bi[v] * c;
                    br[v] = br[u] - tr;
                    bi[v] = bi[u] - ti;
                    br[u] += tr;
                    bi[u] += ti;
                }
            }
        }
        std::vector<float2> t(n + P);
        for (size_t m = 0; m < n; ++m) t[m] = make_float2((float)wr[m], (float)wi[m]);
        for (size_t k = 0; k < P; ++k) {
            const size_t pos = log2p > kMaxLog2Fused ? lg_position(log2p, k) : k;
            t[n + pos] = make_float2((float)br[k], (float)bi[k]);
        }
        float2 *d = nullptr;
        HIP_TRY(hipMalloc((void **)&d, bytes));
        hipError_t e = poison_table(d, bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(d, t.data(), bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);  // (t is freed on return)
        if (e != hipSuccess) {
            (void)hipFree(d);
            return fail(FFTCONV_E_DEVICE, std::string("Bluestein tables: ") + hipGetErrorString(e));
        }
        it = tabs.emplace(std::make_pair(dev, n), Tab{d, bytes, 0}).first;
        total += bytes;
    }
    it->second.used = ++clock;
    *chirp = it->second.p;
    *filt = it->second.p + n;
    return FFTCONV_OK;
}

// Fft::forward / inverse on device rows (src/fft_convolver.rs:36-49)
int fft_rows(int device, size_t n, size_t rows, const float *din, size_t is, float *dout, size_t os, int *status,
             bool inverse, hipStream_t s) {
    if (int r = check_device(device)) return r;
    const bool pow2 = n >= 2 && !(n & (n - 1));
    if (n < 1 || (pow2 && n > ((size_t)2 << kMaxLog2Block)) || (!pow2 && n > kMaxBluestein))
        return fail(FFTCONV_E_UNSUPPORTED, "Fft length must be 1..2^21, or a power of two up to 2^23");
    const size_t nbf = 2 * (n / 2 + 1);  // floats of the n/2 + 1 interleaved bins
    const size_t cin = inverse ? nbf : n, cout = inverse ? n : nbf;
    if (rows > (size_t)INT32_MAX || (rows > 1 && (is < cin || os < cout)))
        return fail(FFTCONV_E_INVALID, "row strides shorter than a row");
    if (rows == 0) return FFTCONV_OK;
    DeviceGuard g(device);
    const float2 *tw = nullptr;
    if (pow2)
        if (int r = fft_twiddles(device, ilog2(n), s, &tw)) return r;
    FftArgs a{};
    a.in = din; a.in_stride = (long long)is; a.out = dout; a.out_stride = (long long)os; a.tw = tw; a.status = status;
    if (!pow2) {
        // any other length: Bluestein over P >= 2n - 1 point FFTs (large.hip)
        const size_t P = std::max<size_t>(2, next_pow2(2 * n - 1));
        const int lp = ilog2(P);
        const float2 *chirp = nullptr, *filt = nullptr, *twP = nullptr;
        std::lock_guard<std::mutex> lk(bluestein_mutex());  // until the kernels are enqueued
        if (int r = bluestein_tables(device, n, lp, s, &chirp, &filt)) return r;
        LgTab t{};
        float2 *scr = nullptr;
        size_t batch = rows;
        if (lp > kMaxLog2Fused) {
            if (int r = lg_tables(device, lp, &t)) return r;
            batch = std::max<size_t>(1, std::min(rows, ((size_t)64 << 20) / (P * sizeof(float2))));
            HIP_TRY(hipMallocAsync((void **)&scr, batch * P * sizeof(float2), s));
            if (poison_alloc()) HIP_TRY(hipMemsetAsync(scr, 0xff, batch * P * sizeof(float2), s));
        } else {
            if (int r = fft_twiddles(device, lp + 1, s, &twP)) return r;  // W_{2P}
        }
        const hipError_t e = launch_fft_bluestein(n, lp, inverse, a, chirp, filt, twP, t, scr, (int)rows, (int)batch, s);
        if (scr) HIP_TRY(hipFreeAsync(scr, s));
        HIP_TRY(e);
        return FFTCONV_OK;
    }
    const int log2m = ilog2(n) - 1;
    if (log2m > kMaxLog2Fused) {
        // the long-block passes (large.hip) through a stream-ordered scratch
        // of up to 64 MiB of rows (the public Fft is not the real-time path)
        LgTab t{};
        if (int r = lg_tables(device, log2m, &t)) return r;
        t.twN = tw;
        const size_t m = n / 2;
        const size_t batch = std::max<size_t>(1, std::min(rows, ((size_t)64 << 20) / (m * sizeof(float2))));
        float2 *scr = nullptr;
        HIP_TRY(hipMallocAsync((void **)&scr, batch * m * sizeof(float2), s));
        if (poison_alloc()) HIP_TRY(hipMemsetAsync(scr, 0xff, batch * m * sizeof(float2), s));
        const hipError_t e = launch_fft_large(log2m, inverse, a, t, scr, (int)rows, (int)batch, s);
        HIP_TRY(hipFreeAsync(scr, s));
        HIP_TRY(e);
        return FFTCONV_OK;
    }
    HIP_TRY(launch_fft_rows(log2m, inverse, a, (int)rows, s));
    return FFTCONV_OK;
}

// host-memory form: rows packed ([rows][n] reals, [rows][n + 2] bin floats),
// through temporary device buffers on a private stream; synchronous
int fft_rows_host(int device, size_t n, size_t rows, const float *in, float *out, int *status, bool inverse) {
    if (int r = check_device(device)) return r;
    if (rows == 0) return FFTCONV_OK;
    DeviceGuard g(device);
    const size_t nbf = 2 * (n / 2 + 1);
    const size_t cin = inverse ? nbf : n, cout = inverse ? n : nbf;
    DevPtr<float> din, dout;
    DevPtr<int> dst;
    if (int r = din.alloc(rows * cin)) return r;
    if (int r = dout.alloc(rows * cout)) return r;
    if (status) { if (int r = dst.alloc(rows)) return r; }
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    struct Del { hipStream_t s; ~Del() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } del{s};
    HIP_TRY(hipMemcpyAsync(din.p, in, rows * cin * sizeof(float), hipMemcpyHostToDevice, s));
    if (int r = fft_rows(device, n, rows, din.p, cin, dout.p, cout, status ? dst.p : nullptr, inverse, s)) return r;
    HIP_TRY(hipMemcpyAsync(out, dout.p, rows * cout * sizeof(float), hipMemcpyDeviceToHost, s));
    if (status) HIP_TRY(hipMemcpyAsync(status, dst.p, rows * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FFTCONV_OK;
}

template <class T>
T *make_or_null(int r, T *p) {
    if (r != FFTCONV_OK) {
        delete p;
        return nullptr;
    }
    return p;
}

}  // namespace

// The process-wide tuning knobs (variant.hpp; like g_stage_limit above, but
// read by the launchers of every kernel file).  Relaxed atomics: set / read
// from any thread; a launcher reads each once.
namespace fftconv {
static std::atomic<int> g_variant{VARIANT_AUTO};
static std::atomic<int> g_lag{-1};

void set_variant(int v) { g_variant.store(v < 0 ? VARIANT_AUTO : (v & 4095), std::memory_order_relaxed); }
Variant Variant::current() { return Variant{g_variant.load(std::memory_order_relaxed)}; }
int get_variant() {
    const Variant v = Variant::current();
    return v.is_auto() ? -1 : v.bits;
}
void set_pipeline_lag(int rows) { g_lag.store(rows < 0 ? -1 : rows, std::memory_order_relaxed); }
int get_pipeline_lag() { return g_lag.load(std::memory_order_relaxed); }
}  // namespace fftconv

// ===========================================================================
// C ABI
// A caller's stream argument: NULL is HIP's null (legacy default) stream, as
// in every HIP API (fftconv.h "Streams"); StreamOrder orders it after the
// handle's own non-blocking streams, and nothing on it runs ahead of them.
// ===========================================================================
struct fftconv_uniform { UniformCore core; };
struct fftconv_twostage { TwoStageCore core; };
struct fftconv_crossfade { CrossfadeCore core; };
struct fftconv_matrix { MatrixCore core; };
struct fftconv_matrix_sparse { SparseMatrixCore core; };
struct fftconv_matrix_lookahead { MatrixLookaheadCore core; };
struct fftconv_matrix_sparse_lookahead { SparseMatrixLookaheadCore core; };
struct fftconv_matrix_crossfade { MatrixCrossfadeCore core; };
struct fftconv_matrix_sparse_crossfade { SparseMatrixCrossfadeCore core; };
struct fftconv_matrix_lookahead_crossfade { MatrixLookaheadCrossfadeCore core; };
struct fftconv_matrix_twostage { MatrixTwoStageCore core; };
struct fftconv_matrix_sparse_twostage { SparseMatrixTwoStageCore core; };

// The wrappers the handle types repeat, over the handle struct H (the matrix
// handles use all of them, the others those whose shape they share).
namespace {

template <class H, class... A>
H *abi_init(A... args) {
    set_error("");
    auto *h = new (std::nothrow) H();
    if (!h) { set_error("out of host memory"); return nullptr; }
    return make_or_null(h->core.init(args...), h);
}
template <class H>
int abi_update(H *h, const float *responses, size_t len, size_t stride) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return h->core.update_host(responses, len, stride);
}
// a stream-ordered call: on the handle's device, with the caller's stream
// ordered behind the handle's previous work, f(core, stream)
template <class H, class F>
int abi_on_stream(H *h, void *hip_stream, F f) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    const auto &b = base(h->core);
    DeviceGuard g(b.device);
    hipStream_t s = (hipStream_t)hip_stream;
    if (int r = b.order.enter(s)) return r;
    return f(h->core, s);
}
template <class H>
int abi_update_device(H *h, const float *d_responses, size_t len, size_t stride, void *hip_stream) {
    return abi_on_stream(h, hip_stream, [&](auto &c, hipStream_t s) { return c.update_device(d_responses, stride, len, s); });
}
// both update_pairs variants: d_src == false -- host rows, on the handle's own stream
template <class H>
int abi_update_pairs(H *h, size_t n, const uint32_t *pair_out, const uint32_t *pair_in, const float *src, bool d_src,
                     size_t len, size_t stride, void *hip_stream) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return h->core.update_pairs(n, pair_out, pair_in, src, d_src, len, stride,
                                d_src ? (hipStream_t)hip_stream : base(h->core).stream);
}
template <class H>
int abi_reset(H *h) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    const auto &b = base(h->core);
    DeviceGuard g(b.device);
    if (int r = b.order.enter(b.stream)) return r;
    if (int r = h->core.reset(b.stream)) return r;
    HIP_TRY(hipStreamSynchronize(b.stream));
    return FFTCONV_OK;
}
template <class H>
int abi_process(H *h, const float *input, size_t input_len, float *output, size_t output_len) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return h->core.process_host(input, input_len, output, output_len);
}
template <class H>
int abi_process_device(H *h, const float *d_in, size_t is, float *d_out, size_t os, size_t len, void *hip_stream) {
    return abi_on_stream(h, hip_stream, [&](auto &c, hipStream_t s) { return c.process_device(d_in, is, d_out, os, len, s); });
}
template <class H>
int abi_process_device_steps(H *h, const float *d_in, size_t is, size_t in_step, float *d_out, size_t os, size_t out_step,
                             size_t len, size_t steps, void *hip_stream) {
    return abi_on_stream(h, hip_stream, [&](auto &c, hipStream_t s) {
        return matrix_process_device_steps(c, d_in, is, in_step, d_out, os, out_step, len, steps, s);
    });
}
template <class H>
H *abi_clone(const H *h) {
    if (!h) { set_error("null handle"); return nullptr; }
    auto *c = new (std::nothrow) H();
    if (!c) { set_error("out of host memory"); return nullptr; }
    return make_or_null(c->core.clone_from(h->core), c);
}
template <class H>
int abi_synchronize(H *h) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    const auto &b = base(h->core);
    DeviceGuard g(b.device);
    return b.order.drain(b.stream);
}
template <class H>
int abi_state(const H *h, size_t out3[3]) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    const auto &b = base(h->core);
    out3[0] = b.cur; out3[1] = b.act; out3[2] = b.fill;
    return FFTCONV_OK;
}
// the crossfaded matrices' CrossfadeConvolver::new and the rest of their own calls
template <class H, class M>
H *abi_crossfade_new(const M *convolver, size_t max_response_length, size_t max_buffer_size, size_t crossfade_samples) {
    if (!convolver) { set_error("null handle"); return nullptr; }
    auto *h = new (std::nothrow) H();
    if (!h) { set_error("out of host memory"); return nullptr; }
    return make_or_null(h->core.init_new(convolver->core, max_response_length, max_buffer_size, crossfade_samples), h);
}
template <class H>
int abi_last_patch(const H *h, size_t out2[2]) {
    if (!h || !out2) return fail(FFTCONV_E_INVALID, "null handle");
    out2[0] = h->core.book.last[0];
    out2[1] = h->core.book.last[1];
    return FFTCONV_OK;
}
template <class H>
int abi_crossfade_reset(H *h) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return fail(FFTCONV_E_UNIMPLEMENTED, "not yet implemented (CrossfadeConvolver::reset is todo!())");
}

}  // namespace

extern "C" {

int fftconv_abi_version(void) { return FFTCONV_ABI_VERSION; }
const char *fftconv_last_error(void) { return g_last_error.c_str(); }
int fftconv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
size_t fftconv_complex_size(size_t size) { return size / 2 + 1; }

// ---- Fft (src/fft_convolver.rs:7-50) ---------------------------------------
int fftconv_fft_forward(int device, size_t n, size_t rows, const float *d_in, size_t in_stride, float *d_out,
                        size_t out_stride, void *hip_stream) {
    return fft_rows(device, n, rows, d_in, in_stride, d_out, out_stride, nullptr, false, (hipStream_t)hip_stream);
}
int fftconv_fft_inverse(int device, size_t n, size_t rows, const float *d_in, size_t in_stride, float *d_out,
                        size_t out_stride, int *d_status, void *hip_stream) {
    return fft_rows(device, n, rows, d_in, in_stride, d_out, out_stride, d_status, true, (hipStream_t)hip_stream);
}
int fftconv_fft_forward_host(int device, size_t n, size_t rows, const float *input, float *output) {
    return fft_rows_host(device, n, rows, input, output, nullptr, false);
}
int fftconv_fft_inverse_host(int device, size_t n, size_t rows, const float *input, float *output, int *status) {
    return fft_rows_host(device, n, rows, input, output, status, true);
}

// compute_tail_block_size, src/fft_convolver.rs:514-526, in f32 exactly as written
size_t fftconv_compute_tail_block_size(size_t head_len, size_t response_len) {
    const volatile float FFT_K = 1.5f;
    const volatile float ln2 = logf(2.0f);
    volatile float kn = (FFT_K * (float)head_len);
    kn = kn / (2.0f * ln2);
    volatile float kk = kn * kn;
    volatile float lh = (float)response_len * (float)head_len;
    volatile float sum = kk + lh;
    volatile float b = -kn + sqrtf(sum);
    const float h = (float)head_len;
    float bb = (b != b) ? h : (b > h ? b : h);
    size_t bi;
    if (!(bb > 0.0f)) bi = 0;
    else if (bb >= 18446744073709551615.0f) bi = SIZE_MAX;
    else bi = (size_t)bb;
    return next_pow2(bi);
}

int fftconv_set_kernel_variant(int variant) {
    if (variant > 4095 || variant < -1) return fail(FFTCONV_E_INVALID, "variant must be 0..4095 (or -1 = auto)");
    set_variant(variant);
    return FFTCONV_OK;
}
int fftconv_get_kernel_variant(void) { return get_variant(); }
int fftconv_set_pipeline_lag(int rows) {
    set_pipeline_lag(rows);
    return FFTCONV_OK;
}
int fftconv_get_pipeline_lag(void) { return get_pipeline_lag(); }
int fftconv_set_host_stage_limit(size_t bytes) {
    g_stage_limit.store(bytes, std::memory_order_relaxed);
    return FFTCONV_OK;
}
size_t fftconv_get_host_stage_limit(void) { return g_stage_limit.load(std::memory_order_relaxed); }

// ---- uniform --------------------------------------------------------------
fftconv_uniform *fftconv_uniform_init(const float *response, size_t response_len, size_t max_block_size,
                                      size_t max_response_length) {
    return fftconv_uniform_init_batch(0, 1, response, response_len, response_len, max_block_size,
                                      max_response_length);
}

fftconv_uniform *fftconv_uniform_init_batch(int device, size_t channels, const float *responses,
                                            size_t response_len, size_t response_stride, size_t max_block_size,
                                            size_t max_response_length) {
    set_error("");
    auto *h = new (std::nothrow) fftconv_uniform();
    if (!h) { set_error("out of host memory"); return nullptr; }
    h->core.la_ok = true;
    h->core.gw_ok = true;
    h->core.own_stage = true;
    int r = h->core.init(device, channels, responses, response_len, response_stride, max_block_size,
                         max_response_length);
    return make_or_null(r, h);
}

int fftconv_uniform_update(fftconv_uniform *h, const float *response, size_t len) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return h->core.update_host(0, h->core.C, response, len, 0);
}
int fftconv_uniform_update_batch(fftconv_uniform *h, const float *responses, size_t len, size_t stride) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return h->core.update_host(0, h->core.C, responses, len, h->core.C == 1 ? 0 : stride);
}
int fftconv_uniform_update_channel(fftconv_uniform *h, size_t channel, const float *response, size_t len) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    if (channel >= h->core.C) return fail(FFTCONV_E_INVALID, "channel out of range");
    return h->core.update_host(channel, 1, response, len, 0);
}
int fftconv_uniform_update_device(fftconv_uniform *h, const float *d_responses, size_t len, size_t stride,
                                  void *hip_stream) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    DeviceGuard g(h->core.device);
    hipStream_t s = (hipStream_t)hip_stream;
    if (int r = h->core.order.enter(s)) return r;
    return h->core.update_device(d_responses, h->core.C == 1 ? 0 : stride, len, s);
}
int fftconv_uniform_reset(fftconv_uniform *h) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    DeviceGuard g(h->core.device);
    if (int r = h->core.order.enter(h->core.stream)) return r;
    if (int r = h->core.reset(h->core.stream)) return r;
    HIP_TRY(hipStreamSynchronize(h->core.stream));
    return FFTCONV_OK;
}
int fftconv_uniform_process(fftconv_uniform *h, const float *input, size_t input_len, float *output,
                            size_t output_len) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return h->core.process_host(input, input_len, output, output_len);
}
int fftconv_uniform_process_device(fftconv_uniform *h, const float *d_input, size_t in_stride, float *d_output,
                                   size_t out_stride, size_t len, void *hip_stream) {
    return abi_process_device(h, d_input, in_stride, d_output, out_stride, len, hip_stream);
}
int fftconv_uniform_process_device_steps(fftconv_uniform *h, const float *d_input, size_t in_stride, size_t in_step,
                                   float *d_output, size_t out_stride, size_t out_step, size_t len, size_t steps,
                                   void *hip_stream) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    DeviceGuard g(h->core.device);
    hipStream_t s = (hipStream_t)hip_stream;
    if (int r = h->core.order.enter(s)) return r;
    return h->core.process_device_steps(d_input, in_stride, in_step, d_output, out_stride, out_step, len, steps, s);
}
fftconv_uniform *fftconv_uniform_clone(const fftconv_uniform *h) { return abi_clone(h); }
void fftconv_uniform_destroy(fftconv_uniform *h) { delete h; }
int fftconv_uniform_synchronize(fftconv_uniform *h) { return abi_synchronize(h); }
size_t fftconv_uniform_channels(const fftconv_uniform *h) { return h ? h->core.C : 0; }
int fftconv_uniform_lookahead_parts(const fftconv_uniform *h) { return h ? h->core.la_W : 0; }
int fftconv_uniform_far_windows(const fftconv_uniform *h) { return h ? h->core.gw_p : 0; }
int fftconv_uniform_lookahead_probe(const fftconv_uniform *h) {
    if (!h || !h->core.la_probe.p) return -1;
    DeviceGuard g(h->core.device);
    if (h->core.order.drain(h->core.stream) != FFTCONV_OK) return -1;
    int n = 0;
    if (hipMemcpy(&n, h->core.la_probe.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return n;
}
size_t fftconv_uniform_block_size(const fftconv_uniform *h) { return h ? h->core.B : 0; }
size_t fftconv_uniform_seg_count(const fftconv_uniform *h) { return h ? h->core.S : 0; }
int fftconv_uniform_ir_spectrum(const fftconv_uniform *h, size_t channel, size_t segment, float *out) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return const_cast<UniformCore &>(h->core).ir_spectrum(channel, segment, out);
}
int fftconv_uniform_channel_state(const fftconv_uniform *h, size_t channel, size_t out3[3]) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return const_cast<UniformCore &>(h->core).channel_state(channel, out3);
}

// ---- two-stage ------------------------------------------------------------
fftconv_twostage *fftconv_twostage_init(const float *response, size_t response_len, size_t max_block_size,
                                        size_t max_response_length) {
    return fftconv_twostage_init_batch(0, 1, response, response_len, response_len, max_block_size,
                                       max_response_length);
}
fftconv_twostage *fftconv_twostage_init_batch(int device, size_t channels, const float *responses,
                                              size_t response_len, size_t response_stride, size_t max_block_size,
                                              size_t max_response_length) {
    set_error("");
    auto *h = new (std::nothrow) fftconv_twostage();
    if (!h) { set_error("out of host memory"); return nullptr; }
    int r = h->core.init(device, channels, responses, response_len, channels == 1 ? response_len : response_stride,
                         max_block_size, max_response_length);
    return make_or_null(r, h);
}
int fftconv_twostage_update(fftconv_twostage *h, const float *, size_t) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return fail(FFTCONV_E_UNIMPLEMENTED, "not yet implemented (TwoStageFFTConvolver::update is todo!())");
}
int fftconv_twostage_reset(fftconv_twostage *h) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return h->core.reset();
}
int fftconv_twostage_process(fftconv_twostage *h, const float *input, float *output, size_t len) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return h->core.process_host(input, output, len);
}
int fftconv_twostage_process_device(fftconv_twostage *h, const float *d_input, size_t in_stride, float *d_output,
                                    size_t out_stride, size_t len, void *hip_stream) {
    return abi_process_device(h, d_input, in_stride, d_output, out_stride, len, hip_stream);
}
int fftconv_twostage_process_device_steps(fftconv_twostage *h, const float *d_input, size_t in_stride, size_t in_step,
                                   float *d_output, size_t out_stride, size_t out_step, size_t len, size_t steps,
                                   void *hip_stream) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    DeviceGuard g(h->core.device);
    hipStream_t s = (hipStream_t)hip_stream;
    if (int r = h->core.order.enter(s)) return r;
    return h->core.process_device_steps(d_input, in_stride, in_step, d_output, out_stride, out_step, len, steps, s);
}
fftconv_twostage *fftconv_twostage_clone(const fftconv_twostage *h) { return abi_clone(h); }
void fftconv_twostage_destroy(fftconv_twostage *h) { delete h; }
int fftconv_twostage_synchronize(fftconv_twostage *h) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    DeviceGuard g(h->core.device);
    return h->core.quiesce();
}
size_t fftconv_twostage_tail_block_size(const fftconv_twostage *h) { return h ? h->core.T : 0; }

// ---- crossfade ------------------------------------------------------------
fftconv_crossfade *fftconv_crossfade_init(const float *response, size_t response_len, size_t max_block_size,
                                          size_t max_response_length) {
    return fftconv_crossfade_init_batch(0, 1, response, response_len, response_len, max_block_size,
                                        max_response_length);
}
fftconv_crossfade *fftconv_crossfade_init_batch(int device, size_t channels, const float *responses,
                                                size_t response_len, size_t response_stride, size_t max_block_size,
                                                size_t max_response_length) {
    set_error("");
    fftconv_uniform *conv = fftconv_uniform_init_batch(device, channels, responses, response_len, response_stride,
                                                       max_block_size, max_response_length);
    if (!conv) return nullptr;
    // Convolution::init (src/crossfade_convolver.rs:46-49)
    fftconv_crossfade *h = fftconv_crossfade_new(conv, response_len, max_block_size, response_len);
    fftconv_uniform_destroy(conv);
    return h;
}
fftconv_crossfade *fftconv_crossfade_new(const fftconv_uniform *convolver, size_t max_response_length,
                                         size_t max_buffer_size, size_t crossfade_samples) {
    if (!convolver) { set_error("null handle"); return nullptr; }
    auto *h = new (std::nothrow) fftconv_crossfade();
    if (!h) { set_error("out of host memory"); return nullptr; }
    int r = h->core.init_new(convolver->core, max_response_length, max_buffer_size, crossfade_samples);
    return make_or_null(r, h);
}
// CrossfadeConvolver<TwoStageFFTConvolver>: init (:46-49) / new (:19-43)
fftconv_crossfade *fftconv_crossfade_init_twostage(const float *response, size_t response_len, size_t max_block_size,
                                                   size_t max_response_length) {
    return fftconv_crossfade_init_twostage_batch(0, 1, response, response_len, response_len, max_block_size,
                                                 max_response_length);
}
fftconv_crossfade *fftconv_crossfade_init_twostage_batch(int device, size_t channels, const float *responses,
                                                         size_t response_len, size_t response_stride,
                                                         size_t max_block_size, size_t max_response_length) {
    set_error("");
    std::unique_ptr<TwoStageCore> inner(new (std::nothrow) TwoStageCore());
    auto *h = new (std::nothrow) fftconv_crossfade();
    if (!inner || !h) { delete h; set_error("out of host memory"); return nullptr; }
    int r = inner->init(device, channels, responses, response_len, channels == 1 ? response_len : response_stride,
                        max_block_size, max_response_length);
    if (r == FFTCONV_OK) r = h->core.init_new_ts(std::move(inner), response_len, max_block_size, response_len);
    return make_or_null(r, h);
}
fftconv_crossfade *fftconv_crossfade_new_twostage(const fftconv_twostage *convolver, size_t max_response_length,
                                                  size_t max_buffer_size, size_t crossfade_samples) {
    if (!convolver) { set_error("null handle"); return nullptr; }
    std::unique_ptr<TwoStageCore> inner(new (std::nothrow) TwoStageCore());
    auto *h = new (std::nothrow) fftconv_crossfade();
    if (!inner || !h) { delete h; set_error("out of host memory"); return nullptr; }
    int r = inner->clone_from(convolver->core);
    if (r == FFTCONV_OK) r = h->core.init_new_ts(std::move(inner), max_response_length, max_buffer_size, crossfade_samples);
    return make_or_null(r, h);
}
int fftconv_crossfade_update(fftconv_crossfade *h, const float *response, size_t len) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return h->core.update_host(response, len, 0);
}
int fftconv_crossfade_update_batch(fftconv_crossfade *h, const float *responses, size_t len, size_t stride) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return h->core.update_host(responses, len, h->core.C == 1 ? 0 : stride);
}
int fftconv_crossfade_update_device(fftconv_crossfade *h, const float *d_responses, size_t len, size_t stride,
                                    void *hip_stream) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    DeviceGuard g(h->core.device);
    hipStream_t s = (hipStream_t)hip_stream;
    if (int r = h->core.order.enter(s)) return r;
    return h->core.update_device(d_responses, len, h->core.C == 1 ? 0 : stride, s);
}
int fftconv_crossfade_reset(fftconv_crossfade *h) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return fail(FFTCONV_E_UNIMPLEMENTED, "not yet implemented (CrossfadeConvolver::reset is todo!())");
}
int fftconv_crossfade_process(fftconv_crossfade *h, const float *input, size_t input_len, float *output,
                              size_t output_len) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return h->core.process_host(input, input_len, output, output_len);
}
int fftconv_crossfade_process_device(fftconv_crossfade *h, const float *d_input, size_t in_stride, float *d_output,
                                     size_t out_stride, size_t output_len, void *hip_stream) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    DeviceGuard g(h->core.device);
    hipStream_t s = (hipStream_t)hip_stream;
    if (int r = h->core.order.enter(s)) return r;
    return h->core.process_device(d_input, in_stride, d_output, out_stride, output_len, s);
}
int fftconv_crossfade_is_crossfading(const fftconv_crossfade *h) { return h && h->core.is_crossfading() ? 1 : 0; }
int fftconv_crossfade_process_device_steps(fftconv_crossfade *h, const float *d_input, size_t in_stride, size_t in_step,
                                   float *d_output, size_t out_stride, size_t out_step, size_t len, size_t steps,
                                   void *hip_stream) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    DeviceGuard g(h->core.device);
    hipStream_t s = (hipStream_t)hip_stream;
    if (int r = h->core.order.enter(s)) return r;
    for (size_t k = 0; k < steps; ++k) {
        if (int r = h->core.process_device(d_input + k * in_step, in_stride, d_output + k * out_step, out_stride, len, s))
            return r;
    }
    return FFTCONV_OK;
}
fftconv_crossfade *fftconv_crossfade_clone(const fftconv_crossfade *h) { return abi_clone(h); }
void fftconv_crossfade_destroy(fftconv_crossfade *h) { delete h; }
int fftconv_crossfade_synchronize(fftconv_crossfade *h) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    DeviceGuard g(h->core.device);
    return h->core.quiesce();
}

// ---- matrix -----------------------------------------------------
fftconv_matrix *fftconv_matrix_init(int device, size_t inputs, size_t outputs, const float *responses,
                                    size_t response_len, size_t response_stride, size_t max_block_size,
                                    size_t max_response_length) {
    return abi_init<fftconv_matrix>(device, inputs, outputs, responses, response_len, response_stride, max_block_size,
                                    max_response_length);
}
int fftconv_matrix_update(fftconv_matrix *h, const float *responses, size_t response_len, size_t response_stride) {
    return abi_update(h, responses, response_len, response_stride);
}
int fftconv_matrix_update_device(fftconv_matrix *h, const float *d_responses, size_t response_len,
                                 size_t response_stride, void *hip_stream) {
    return abi_update_device(h, d_responses, response_len, response_stride, hip_stream);
}
int fftconv_matrix_update_pairs(fftconv_matrix *h, size_t n_pairs, const uint32_t *pair_out, const uint32_t *pair_in,
                                const float *responses, size_t response_len, size_t response_stride) {
    return abi_update_pairs(h, n_pairs, pair_out, pair_in, responses, false, response_len, response_stride, nullptr);
}
int fftconv_matrix_update_pairs_device(fftconv_matrix *h, size_t n_pairs, const uint32_t *pair_out,
                                       const uint32_t *pair_in, const float *d_responses, size_t response_len,
                                       size_t response_stride, void *hip_stream) {
    return abi_update_pairs(h, n_pairs, pair_out, pair_in, d_responses, true, response_len, response_stride, hip_stream);
}
int fftconv_matrix_reset(fftconv_matrix *h) { return abi_reset(h); }
int fftconv_matrix_process(fftconv_matrix *h, const float *input, size_t input_len, float *output,
                           size_t output_len) {
    return abi_process(h, input, input_len, output, output_len);
}
int fftconv_matrix_process_device(fftconv_matrix *h, const float *d_input, size_t in_stride, float *d_output,
                                  size_t out_stride, size_t len, void *hip_stream) {
    return abi_process_device(h, d_input, in_stride, d_output, out_stride, len, hip_stream);
}
int fftconv_matrix_process_device_steps(fftconv_matrix *h, const float *d_input, size_t in_stride, size_t in_step,
                                        float *d_output, size_t out_stride, size_t out_step, size_t len,
                                        size_t steps, void *hip_stream) {
    return abi_process_device_steps(h, d_input, in_stride, in_step, d_output, out_stride, out_step, len, steps, hip_stream);
}
fftconv_matrix *fftconv_matrix_clone(const fftconv_matrix *h) { return abi_clone(h); }
void fftconv_matrix_destroy(fftconv_matrix *h) { delete h; }
int fftconv_matrix_synchronize(fftconv_matrix *h) { return abi_synchronize(h); }
size_t fftconv_matrix_inputs(const fftconv_matrix *h) { return h ? h->core.I : 0; }
size_t fftconv_matrix_outputs(const fftconv_matrix *h) { return h ? h->core.O : 0; }
size_t fftconv_matrix_block_size(const fftconv_matrix *h) { return h ? h->core.B : 0; }
size_t fftconv_matrix_seg_count(const fftconv_matrix *h) { return h ? h->core.S : 0; }
int fftconv_matrix_mac_parts(const fftconv_matrix *h) { return h ? h->core.mac_parts() : 0; }
int fftconv_matrix_state(const fftconv_matrix *h, size_t out3[3]) { return abi_state(h, out3); }

// ---- matrix with far-row windows ---------------------------------
fftconv_matrix_lookahead *fftconv_matrix_lookahead_init(int device, size_t inputs, size_t outputs,
                                                        const float *responses, size_t response_len,
                                                        size_t response_stride, size_t max_block_size,
                                                        size_t max_response_length) {
    return abi_init<fftconv_matrix_lookahead>(device, inputs, outputs, responses, response_len, response_stride,
                                              max_block_size, max_response_length);
}
int fftconv_matrix_lookahead_update(fftconv_matrix_lookahead *h, const float *responses, size_t response_len,
                                    size_t response_stride) {
    return abi_update(h, responses, response_len, response_stride);
}
int fftconv_matrix_lookahead_update_device(fftconv_matrix_lookahead *h, const float *d_responses, size_t response_len,
                                           size_t response_stride, void *hip_stream) {
    return abi_update_device(h, d_responses, response_len, response_stride, hip_stream);
}
int fftconv_matrix_lookahead_reset(fftconv_matrix_lookahead *h) { return abi_reset(h); }
int fftconv_matrix_lookahead_process(fftconv_matrix_lookahead *h, const float *input, size_t input_len, float *output,
                                     size_t output_len) {
    return abi_process(h, input, input_len, output, output_len);
}
int fftconv_matrix_lookahead_process_device(fftconv_matrix_lookahead *h, const float *d_input, size_t in_stride,
                                            float *d_output, size_t out_stride, size_t len, void *hip_stream) {
    return abi_process_device(h, d_input, in_stride, d_output, out_stride, len, hip_stream);
}
int fftconv_matrix_lookahead_process_device_steps(fftconv_matrix_lookahead *h, const float *d_input, size_t in_stride,
                                                  size_t in_step, float *d_output, size_t out_stride, size_t out_step,
                                                  size_t len, size_t steps, void *hip_stream) {
    return abi_process_device_steps(h, d_input, in_stride, in_step, d_output, out_stride, out_step, len, steps, hip_stream);
}
fftconv_matrix_lookahead *fftconv_matrix_lookahead_clone(const fftconv_matrix_lookahead *h) { return abi_clone(h); }
void fftconv_matrix_lookahead_destroy(fftconv_matrix_lookahead *h) { delete h; }
int fftconv_matrix_lookahead_synchronize(fftconv_matrix_lookahead *h) { return abi_synchronize(h); }
size_t fftconv_matrix_lookahead_inputs(const fftconv_matrix_lookahead *h) { return h ? h->core.m.I : 0; }
size_t fftconv_matrix_lookahead_outputs(const fftconv_matrix_lookahead *h) { return h ? h->core.m.O : 0; }
size_t fftconv_matrix_lookahead_block_size(const fftconv_matrix_lookahead *h) { return h ? h->core.m.B : 0; }
size_t fftconv_matrix_lookahead_seg_count(const fftconv_matrix_lookahead *h) { return h ? h->core.m.S : 0; }
int fftconv_matrix_lookahead_state(const fftconv_matrix_lookahead *h, size_t out3[3]) { return abi_state(h, out3); }
int fftconv_matrix_lookahead_period(void) { return kMatrixLaQ; }
int fftconv_matrix_lookahead_near_parts(const fftconv_matrix_lookahead *h) { return h ? h->core.near_parts() : 0; }
int fftconv_matrix_lookahead_far_parts(const fftconv_matrix_lookahead *h) { return h ? h->core.far_parts() : 0; }
int fftconv_matrix_lookahead_set_windows(fftconv_matrix_lookahead *h, int on) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    h->core.clk.windows = on != 0;
    return FFTCONV_OK;
}
int fftconv_matrix_lookahead_anchors(const fftconv_matrix_lookahead *h) { return h ? h->core.anchors() : 0; }

// ---- sparse matrix ----------------------------------------------
fftconv_matrix_sparse *fftconv_matrix_sparse_init(int device, size_t inputs, size_t outputs, size_t pairs,
                                                  const uint32_t *pair_out, const uint32_t *pair_in,
                                                  const float *responses, size_t response_len,
                                                  size_t response_stride, size_t max_block_size,
                                                  size_t max_response_length) {
    return abi_init<fftconv_matrix_sparse>(device, inputs, outputs, pairs, pair_out, pair_in, responses, response_len,
                                           response_stride, max_block_size, max_response_length);
}
int fftconv_matrix_sparse_update(fftconv_matrix_sparse *h, const float *responses, size_t response_len,
                                 size_t response_stride) {
    return abi_update(h, responses, response_len, response_stride);
}
int fftconv_matrix_sparse_update_device(fftconv_matrix_sparse *h, const float *d_responses, size_t response_len,
                                        size_t response_stride, void *hip_stream) {
    return abi_update_device(h, d_responses, response_len, response_stride, hip_stream);
}
int fftconv_matrix_sparse_update_pairs(fftconv_matrix_sparse *h, size_t n_pairs, const uint32_t *pair_out,
                                       const uint32_t *pair_in, const float *responses, size_t response_len,
                                       size_t response_stride) {
    return abi_update_pairs(h, n_pairs, pair_out, pair_in, responses, false, response_len, response_stride, nullptr);
}
int fftconv_matrix_sparse_update_pairs_device(fftconv_matrix_sparse *h, size_t n_pairs, const uint32_t *pair_out,
                                              const uint32_t *pair_in, const float *d_responses, size_t response_len,
                                              size_t response_stride, void *hip_stream) {
    return abi_update_pairs(h, n_pairs, pair_out, pair_in, d_responses, true, response_len, response_stride, hip_stream);
}
int fftconv_matrix_sparse_reset(fftconv_matrix_sparse *h) { return abi_reset(h); }
int fftconv_matrix_sparse_process(fftconv_matrix_sparse *h, const float *input, size_t input_len, float *output,
                                  size_t output_len) {
    return abi_process(h, input, input_len, output, output_len);
}
int fftconv_matrix_sparse_process_device(fftconv_matrix_sparse *h, const float *d_input, size_t in_stride,
                                         float *d_output, size_t out_stride, size_t len, void *hip_stream) {
    return abi_process_device(h, d_input, in_stride, d_output, out_stride, len, hip_stream);
}
int fftconv_matrix_sparse_process_device_steps(fftconv_matrix_sparse *h, const float *d_input, size_t in_stride,
                                               size_t in_step, float *d_output, size_t out_stride, size_t out_step,
                                               size_t len, size_t steps, void *hip_stream) {
    return abi_process_device_steps(h, d_input, in_stride, in_step, d_output, out_stride, out_step, len, steps, hip_stream);
}
fftconv_matrix_sparse *fftconv_matrix_sparse_clone(const fftconv_matrix_sparse *h) { return abi_clone(h); }
void fftconv_matrix_sparse_destroy(fftconv_matrix_sparse *h) { delete h; }
int fftconv_matrix_sparse_synchronize(fftconv_matrix_sparse *h) { return abi_synchronize(h); }
size_t fftconv_matrix_sparse_inputs(const fftconv_matrix_sparse *h) { return h ? h->core.I : 0; }
size_t fftconv_matrix_sparse_outputs(const fftconv_matrix_sparse *h) { return h ? h->core.O : 0; }
size_t fftconv_matrix_sparse_pairs(const fftconv_matrix_sparse *h) { return h ? h->core.P : 0; }
size_t fftconv_matrix_sparse_block_size(const fftconv_matrix_sparse *h) { return h ? h->core.B : 0; }
size_t fftconv_matrix_sparse_seg_count(const fftconv_matrix_sparse *h) { return h ? h->core.S : 0; }
int fftconv_matrix_sparse_output_parts(const fftconv_matrix_sparse *h, size_t output) {
    return h && output < h->core.O ? h->core.output_parts(output) : 0;
}
int fftconv_matrix_sparse_state(const fftconv_matrix_sparse *h, size_t out3[3]) { return abi_state(h, out3); }

// ---- sparse matrix with far-row windows ---------------------------
fftconv_matrix_sparse_lookahead *fftconv_matrix_sparse_lookahead_init(int device, size_t inputs, size_t outputs,
                                                                      size_t pairs, const uint32_t *pair_out,
                                                                      const uint32_t *pair_in, const float *responses,
                                                                      size_t response_len, size_t response_stride,
                                                                      size_t max_block_size,
                                                                      size_t max_response_length) {
    return abi_init<fftconv_matrix_sparse_lookahead>(device, inputs, outputs, pairs, pair_out, pair_in, responses,
                                                     response_len, response_stride, max_block_size, max_response_length);
}
int fftconv_matrix_sparse_lookahead_update(fftconv_matrix_sparse_lookahead *h, const float *responses,
                                           size_t response_len, size_t response_stride) {
    return abi_update(h, responses, response_len, response_stride);
}
int fftconv_matrix_sparse_lookahead_update_device(fftconv_matrix_sparse_lookahead *h, const float *d_responses,
                                                  size_t response_len, size_t response_stride, void *hip_stream) {
    return abi_update_device(h, d_responses, response_len, response_stride, hip_stream);
}
int fftconv_matrix_sparse_lookahead_update_pairs(fftconv_matrix_sparse_lookahead *h, size_t n_pairs,
                                                 const uint32_t *pair_out, const uint32_t *pair_in,
                                                 const float *responses, size_t response_len, size_t response_stride) {
    return abi_update_pairs(h, n_pairs, pair_out, pair_in, responses, false, response_len, response_stride, nullptr);
}
int fftconv_matrix_sparse_lookahead_update_pairs_device(fftconv_matrix_sparse_lookahead *h, size_t n_pairs,
                                                        const uint32_t *pair_out, const uint32_t *pair_in,
                                                        const float *d_responses, size_t response_len,
                                                        size_t response_stride, void *hip_stream) {
    return abi_update_pairs(h, n_pairs, pair_out, pair_in, d_responses, true, response_len, response_stride, hip_stream);
}
int fftconv_matrix_sparse_lookahead_reset(fftconv_matrix_sparse_lookahead *h) { return abi_reset(h); }
int fftconv_matrix_sparse_lookahead_process(fftconv_matrix_sparse_lookahead *h, const float *input, size_t input_len,
                                            float *output, size_t output_len) {
    return abi_process(h, input, input_len, output, output_len);
}
int fftconv_matrix_sparse_lookahead_process_device(fftconv_matrix_sparse_lookahead *h, const float *d_input,
                                                   size_t in_stride, float *d_output, size_t out_stride, size_t len,
                                                   void *hip_stream) {
    return abi_process_device(h, d_input, in_stride, d_output, out_stride, len, hip_stream);
}
int fftconv_matrix_sparse_lookahead_process_device_steps(fftconv_matrix_sparse_lookahead *h, const float *d_input,
                                                         size_t in_stride, size_t in_step, float *d_output,
                                                         size_t out_stride, size_t out_step, size_t len, size_t steps,
                                                         void *hip_stream) {
    return abi_process_device_steps(h, d_input, in_stride, in_step, d_output, out_stride, out_step, len, steps, hip_stream);
}
fftconv_matrix_sparse_lookahead *fftconv_matrix_sparse_lookahead_clone(const fftconv_matrix_sparse_lookahead *h) {
    return abi_clone(h);
}
void fftconv_matrix_sparse_lookahead_destroy(fftconv_matrix_sparse_lookahead *h) { delete h; }
int fftconv_matrix_sparse_lookahead_synchronize(fftconv_matrix_sparse_lookahead *h) { return abi_synchronize(h); }
size_t fftconv_matrix_sparse_lookahead_inputs(const fftconv_matrix_sparse_lookahead *h) { return h ? h->core.m.I : 0; }
size_t fftconv_matrix_sparse_lookahead_outputs(const fftconv_matrix_sparse_lookahead *h) { return h ? h->core.m.O : 0; }
size_t fftconv_matrix_sparse_lookahead_pairs(const fftconv_matrix_sparse_lookahead *h) { return h ? h->core.m.P : 0; }
size_t fftconv_matrix_sparse_lookahead_block_size(const fftconv_matrix_sparse_lookahead *h) {
    return h ? h->core.m.B : 0;
}
size_t fftconv_matrix_sparse_lookahead_seg_count(const fftconv_matrix_sparse_lookahead *h) {
    return h ? h->core.m.S : 0;
}
int fftconv_matrix_sparse_lookahead_state(const fftconv_matrix_sparse_lookahead *h, size_t out3[3]) {
    return abi_state(h, out3);
}
int fftconv_matrix_sparse_lookahead_near_parts(const fftconv_matrix_sparse_lookahead *h, size_t output) {
    return h && output < h->core.m.O ? h->core.near_parts(output) : 0;
}
int fftconv_matrix_sparse_lookahead_far_parts(const fftconv_matrix_sparse_lookahead *h, size_t output) {
    return h && output < h->core.m.O ? h->core.far_parts(output) : 0;
}
int fftconv_matrix_sparse_lookahead_set_windows(fftconv_matrix_sparse_lookahead *h, int on) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    h->core.clk.windows = on != 0;
    return FFTCONV_OK;
}
int fftconv_matrix_sparse_lookahead_anchors(const fftconv_matrix_sparse_lookahead *h) {
    return h ? h->core.anchors() : 0;
}

// ---- matrix crossfade ---------------------------------------------
fftconv_matrix_crossfade *fftconv_matrix_crossfade_init(int device, size_t inputs, size_t outputs,
                                                        const float *responses, size_t response_len,
                                                        size_t response_stride, size_t max_block_size,
                                                        size_t max_response_length) {
    fftconv_matrix *conv = fftconv_matrix_init(device, inputs, outputs, responses, response_len, response_stride,
                                               max_block_size, max_response_length);
    if (!conv) return nullptr;
    // Convolution::init (src/crossfade_convolver.rs:46-49)
    fftconv_matrix_crossfade *h = fftconv_matrix_crossfade_new(conv, response_len, max_block_size, response_len);
    fftconv_matrix_destroy(conv);
    return h;
}
fftconv_matrix_crossfade *fftconv_matrix_crossfade_new(const fftconv_matrix *convolver, size_t max_response_length,
                                                       size_t max_buffer_size, size_t crossfade_samples) {
    return abi_crossfade_new<fftconv_matrix_crossfade>(convolver, max_response_length, max_buffer_size, crossfade_samples);
}
int fftconv_matrix_crossfade_update(fftconv_matrix_crossfade *h, const float *responses, size_t response_len,
                                    size_t response_stride) {
    return abi_update(h, responses, response_len, response_stride);
}
int fftconv_matrix_crossfade_update_device(fftconv_matrix_crossfade *h, const float *d_responses, size_t response_len,
                                           size_t response_stride, void *hip_stream) {
    return abi_update_device(h, d_responses, response_len, response_stride, hip_stream);
}
int fftconv_matrix_crossfade_update_pairs(fftconv_matrix_crossfade *h, size_t n_pairs, const uint32_t *pair_out,
                                          const uint32_t *pair_in, const float *responses, size_t response_len,
                                          size_t response_stride) {
    return abi_update_pairs(h, n_pairs, pair_out, pair_in, responses, false, response_len, response_stride, nullptr);
}
int fftconv_matrix_crossfade_update_pairs_device(fftconv_matrix_crossfade *h, size_t n_pairs, const uint32_t *pair_out,
                                                 const uint32_t *pair_in, const float *d_responses,
                                                 size_t response_len, size_t response_stride, void *hip_stream) {
    return abi_update_pairs(h, n_pairs, pair_out, pair_in, d_responses, true, response_len, response_stride, hip_stream);
}
size_t fftconv_matrix_crossfade_diff_pairs(const fftconv_matrix_crossfade *h) { return h ? h->core.book.nd : 0; }
int fftconv_matrix_crossfade_last_patch(const fftconv_matrix_crossfade *h, size_t out2[2]) {
    return abi_last_patch(h, out2);
}
int fftconv_matrix_crossfade_reset(fftconv_matrix_crossfade *h) { return abi_crossfade_reset(h); }
int fftconv_matrix_crossfade_process(fftconv_matrix_crossfade *h, const float *input, size_t input_len, float *output,
                                     size_t output_len) {
    return abi_process(h, input, input_len, output, output_len);
}
int fftconv_matrix_crossfade_process_device(fftconv_matrix_crossfade *h, const float *d_input, size_t in_stride,
                                            float *d_output, size_t out_stride, size_t output_len, void *hip_stream) {
    return abi_process_device(h, d_input, in_stride, d_output, out_stride, output_len, hip_stream);
}
int fftconv_matrix_crossfade_process_device_steps(fftconv_matrix_crossfade *h, const float *d_input, size_t in_stride,
                                                  size_t in_step, float *d_output, size_t out_stride, size_t out_step,
                                                  size_t output_len, size_t steps, void *hip_stream) {
    return abi_process_device_steps(h, d_input, in_stride, in_step, d_output, out_stride, out_step, output_len, steps,
                                    hip_stream);
}
int fftconv_matrix_crossfade_is_crossfading(const fftconv_matrix_crossfade *h) {
    return h && h->core.is_crossfading() ? 1 : 0;
}
fftconv_matrix_crossfade *fftconv_matrix_crossfade_clone(const fftconv_matrix_crossfade *h) { return abi_clone(h); }
void fftconv_matrix_crossfade_destroy(fftconv_matrix_crossfade *h) { delete h; }
int fftconv_matrix_crossfade_synchronize(fftconv_matrix_crossfade *h) { return abi_synchronize(h); }
size_t fftconv_matrix_crossfade_inputs(const fftconv_matrix_crossfade *h) { return h ? h->core.I : 0; }
size_t fftconv_matrix_crossfade_outputs(const fftconv_matrix_crossfade *h) { return h ? h->core.O : 0; }
int fftconv_matrix_crossfade_set_fused(fftconv_matrix_crossfade *h, int on) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    h->core.fused = on != 0;
    return FFTCONV_OK;
}
int fftconv_matrix_crossfade_path(const fftconv_matrix_crossfade *h) { return h ? h->core.path_next() : 0; }

// ---- matrix crossfade with far-row windows -------------------------
fftconv_matrix_lookahead_crossfade *fftconv_matrix_lookahead_crossfade_init(int device, size_t inputs, size_t outputs,
                                                                            const float *responses, size_t response_len,
                                                                            size_t response_stride, size_t max_block_size,
                                                                            size_t max_response_length) {
    set_error("");
    if (inputs && outputs && max_response_length >= response_len &&
        next_pow2(max_block_size) > ((size_t)1 << kMatrixLaMaxLog2B)) {
        (void)fail(FFTCONV_E_UNSUPPORTED, "matrix lookahead crossfade block size " + std::to_string(next_pow2(max_block_size)) +
                                              " outside 32..512 (use the MatrixCrossfadeConvolver)");
        return nullptr;
    }
    fftconv_matrix_lookahead *conv = fftconv_matrix_lookahead_init(device, inputs, outputs, responses, response_len,
                                                                   response_stride, max_block_size, max_response_length);
    if (!conv) return nullptr;
    // Convolution::init (src/crossfade_convolver.rs:46-49)
    fftconv_matrix_lookahead_crossfade *h =
        fftconv_matrix_lookahead_crossfade_new(conv, response_len, max_block_size, response_len);
    fftconv_matrix_lookahead_destroy(conv);
    return h;
}
fftconv_matrix_lookahead_crossfade *fftconv_matrix_lookahead_crossfade_new(const fftconv_matrix_lookahead *convolver,
                                                                           size_t max_response_length,
                                                                           size_t max_buffer_size,
                                                                           size_t crossfade_samples) {
    return abi_crossfade_new<fftconv_matrix_lookahead_crossfade>(convolver, max_response_length, max_buffer_size,
                                                                 crossfade_samples);
}
int fftconv_matrix_lookahead_crossfade_update(fftconv_matrix_lookahead_crossfade *h, const float *responses,
                                              size_t response_len, size_t response_stride) {
    return abi_update(h, responses, response_len, response_stride);
}
int fftconv_matrix_lookahead_crossfade_update_device(fftconv_matrix_lookahead_crossfade *h, const float *d_responses,
                                                     size_t response_len, size_t response_stride, void *hip_stream) {
    return abi_update_device(h, d_responses, response_len, response_stride, hip_stream);
}
int fftconv_matrix_lookahead_crossfade_update_pairs(fftconv_matrix_lookahead_crossfade *h, size_t n_pairs,
                                                    const uint32_t *pair_out, const uint32_t *pair_in,
                                                    const float *responses, size_t response_len, size_t response_stride) {
    return abi_update_pairs(h, n_pairs, pair_out, pair_in, responses, false, response_len, response_stride, nullptr);
}
int fftconv_matrix_lookahead_crossfade_update_pairs_device(fftconv_matrix_lookahead_crossfade *h, size_t n_pairs,
                                                           const uint32_t *pair_out, const uint32_t *pair_in,
                                                           const float *d_responses, size_t response_len,
                                                           size_t response_stride, void *hip_stream) {
    return abi_update_pairs(h, n_pairs, pair_out, pair_in, d_responses, true, response_len, response_stride, hip_stream);
}
size_t fftconv_matrix_lookahead_crossfade_diff_pairs(const fftconv_matrix_lookahead_crossfade *h) {
    return h ? h->core.book.nd : 0;
}
int fftconv_matrix_lookahead_crossfade_last_patch(const fftconv_matrix_lookahead_crossfade *h, size_t out2[2]) {
    return abi_last_patch(h, out2);
}
int fftconv_matrix_lookahead_crossfade_reset(fftconv_matrix_lookahead_crossfade *h) { return abi_crossfade_reset(h); }
int fftconv_matrix_lookahead_crossfade_process(fftconv_matrix_lookahead_crossfade *h, const float *input, size_t input_len,
                                               float *output, size_t output_len) {
    return abi_process(h, input, input_len, output, output_len);
}
int fftconv_matrix_lookahead_crossfade_process_device(fftconv_matrix_lookahead_crossfade *h, const float *d_input,
                                                      size_t in_stride, float *d_output, size_t out_stride,
                                                      size_t output_len, void *hip_stream) {
    return abi_process_device(h, d_input, in_stride, d_output, out_stride, output_len, hip_stream);
}
int fftconv_matrix_lookahead_crossfade_process_device_steps(fftconv_matrix_lookahead_crossfade *h, const float *d_input,
                                                            size_t in_stride, size_t in_step, float *d_output,
                                                            size_t out_stride, size_t out_step, size_t output_len,
                                                            size_t steps, void *hip_stream) {
    return abi_process_device_steps(h, d_input, in_stride, in_step, d_output, out_stride, out_step, output_len, steps,
                                    hip_stream);
}
int fftconv_matrix_lookahead_crossfade_is_crossfading(const fftconv_matrix_lookahead_crossfade *h) {
    return h && h->core.is_crossfading() ? 1 : 0;
}
fftconv_matrix_lookahead_crossfade *fftconv_matrix_lookahead_crossfade_clone(const fftconv_matrix_lookahead_crossfade *h) {
    return abi_clone(h);
}
void fftconv_matrix_lookahead_crossfade_destroy(fftconv_matrix_lookahead_crossfade *h) { delete h; }
int fftconv_matrix_lookahead_crossfade_synchronize(fftconv_matrix_lookahead_crossfade *h) { return abi_synchronize(h); }
size_t fftconv_matrix_lookahead_crossfade_inputs(const fftconv_matrix_lookahead_crossfade *h) { return h ? h->core.I : 0; }
size_t fftconv_matrix_lookahead_crossfade_outputs(const fftconv_matrix_lookahead_crossfade *h) { return h ? h->core.O : 0; }
int fftconv_matrix_lookahead_crossfade_set_fused(fftconv_matrix_lookahead_crossfade *h, int on) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    h->core.fused = on != 0;
    return FFTCONV_OK;
}
int fftconv_matrix_lookahead_crossfade_path(const fftconv_matrix_lookahead_crossfade *h) {
    return h ? h->core.path_next() : 0;
}
int fftconv_matrix_lookahead_crossfade_set_windows(fftconv_matrix_lookahead_crossfade *h, int on) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    h->core.a->clk.windows = h->core.b->clk.windows = on != 0;
    return FFTCONV_OK;
}
int fftconv_matrix_lookahead_crossfade_anchors(const fftconv_matrix_lookahead_crossfade *h, int which) {
    if (!h || which < 0 || which > 1) return 0;
    // (an idle convolver -- the fused path with the crossfader Reached at the other one -- makes no anchor)
    if (h->core.path_next() == 2 && which != h->core.xf.target) return 0;
    return (which == 0 ? h->core.a : h->core.b)->anchors();
}

// ---- sparse matrix crossfade ---------------------------------------
fftconv_matrix_sparse_crossfade *fftconv_matrix_sparse_crossfade_init(int device, size_t inputs, size_t outputs,
                                                                      size_t pairs, const uint32_t *pair_out,
                                                                      const uint32_t *pair_in, const float *responses,
                                                                      size_t response_len, size_t response_stride,
                                                                      size_t max_block_size,
                                                                      size_t max_response_length) {
    fftconv_matrix_sparse *conv = fftconv_matrix_sparse_init(device, inputs, outputs, pairs, pair_out, pair_in, responses,
                                                             response_len, response_stride, max_block_size,
                                                             max_response_length);
    if (!conv) return nullptr;
    // Convolution::init (src/crossfade_convolver.rs:46-49)
    fftconv_matrix_sparse_crossfade *h =
        fftconv_matrix_sparse_crossfade_new(conv, response_len, max_block_size, response_len);
    fftconv_matrix_sparse_destroy(conv);
    return h;
}
fftconv_matrix_sparse_crossfade *fftconv_matrix_sparse_crossfade_new(const fftconv_matrix_sparse *convolver,
                                                                     size_t max_response_length,
                                                                     size_t max_buffer_size,
                                                                     size_t crossfade_samples) {
    return abi_crossfade_new<fftconv_matrix_sparse_crossfade>(convolver, max_response_length, max_buffer_size,
                                                              crossfade_samples);
}
int fftconv_matrix_sparse_crossfade_update(fftconv_matrix_sparse_crossfade *h, const float *responses,
                                           size_t response_len, size_t response_stride) {
    return abi_update(h, responses, response_len, response_stride);
}
int fftconv_matrix_sparse_crossfade_update_device(fftconv_matrix_sparse_crossfade *h, const float *d_responses,
                                                  size_t response_len, size_t response_stride, void *hip_stream) {
    return abi_update_device(h, d_responses, response_len, response_stride, hip_stream);
}
int fftconv_matrix_sparse_crossfade_update_pairs(fftconv_matrix_sparse_crossfade *h, size_t n_pairs,
                                                 const uint32_t *pair_out, const uint32_t *pair_in,
                                                 const float *responses, size_t response_len,
                                                 size_t response_stride) {
    return abi_update_pairs(h, n_pairs, pair_out, pair_in, responses, false, response_len, response_stride, nullptr);
}
int fftconv_matrix_sparse_crossfade_update_pairs_device(fftconv_matrix_sparse_crossfade *h, size_t n_pairs,
                                                        const uint32_t *pair_out, const uint32_t *pair_in,
                                                        const float *d_responses, size_t response_len,
                                                        size_t response_stride, void *hip_stream) {
    return abi_update_pairs(h, n_pairs, pair_out, pair_in, d_responses, true, response_len, response_stride, hip_stream);
}
size_t fftconv_matrix_sparse_crossfade_diff_pairs(const fftconv_matrix_sparse_crossfade *h) {
    return h ? h->core.book.nd : 0;
}
int fftconv_matrix_sparse_crossfade_last_patch(const fftconv_matrix_sparse_crossfade *h, size_t out2[2]) {
    return abi_last_patch(h, out2);
}
int fftconv_matrix_sparse_crossfade_reset(fftconv_matrix_sparse_crossfade *h) { return abi_crossfade_reset(h); }
int fftconv_matrix_sparse_crossfade_process(fftconv_matrix_sparse_crossfade *h, const float *input, size_t input_len,
                                            float *output, size_t output_len) {
    return abi_process(h, input, input_len, output, output_len);
}
int fftconv_matrix_sparse_crossfade_process_device(fftconv_matrix_sparse_crossfade *h, const float *d_input,
                                                   size_t in_stride, float *d_output, size_t out_stride,
                                                   size_t output_len, void *hip_stream) {
    return abi_process_device(h, d_input, in_stride, d_output, out_stride, output_len, hip_stream);
}
int fftconv_matrix_sparse_crossfade_process_device_steps(fftconv_matrix_sparse_crossfade *h, const float *d_input,
                                                         size_t in_stride, size_t in_step, float *d_output,
                                                         size_t out_stride, size_t out_step, size_t output_len,
                                                         size_t steps, void *hip_stream) {
    return abi_process_device_steps(h, d_input, in_stride, in_step, d_output, out_stride, out_step, output_len, steps,
                                    hip_stream);
}
int fftconv_matrix_sparse_crossfade_is_crossfading(const fftconv_matrix_sparse_crossfade *h) {
    return h && h->core.is_crossfading() ? 1 : 0;
}
fftconv_matrix_sparse_crossfade *fftconv_matrix_sparse_crossfade_clone(const fftconv_matrix_sparse_crossfade *h) {
    return abi_clone(h);
}
void fftconv_matrix_sparse_crossfade_destroy(fftconv_matrix_sparse_crossfade *h) { delete h; }
int fftconv_matrix_sparse_crossfade_synchronize(fftconv_matrix_sparse_crossfade *h) { return abi_synchronize(h); }
size_t fftconv_matrix_sparse_crossfade_inputs(const fftconv_matrix_sparse_crossfade *h) { return h ? h->core.I : 0; }
size_t fftconv_matrix_sparse_crossfade_outputs(const fftconv_matrix_sparse_crossfade *h) { return h ? h->core.O : 0; }
size_t fftconv_matrix_sparse_crossfade_pairs(const fftconv_matrix_sparse_crossfade *h) { return h ? h->core.P : 0; }
int fftconv_matrix_sparse_crossfade_set_fused(fftconv_matrix_sparse_crossfade *h, int on) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    h->core.fused = on != 0;
    return FFTCONV_OK;
}
int fftconv_matrix_sparse_crossfade_path(const fftconv_matrix_sparse_crossfade *h) {
    return h ? h->core.path_next() : 0;
}


// ---- matrix two-stage ---------------------------------------------
fftconv_matrix_twostage *fftconv_matrix_twostage_init(int device, size_t inputs, size_t outputs,
                                                      const float *responses, size_t response_len,
                                                      size_t response_stride, size_t max_block_size,
                                                      size_t max_response_length) {
    set_error("");
    auto *h = new (std::nothrow) fftconv_matrix_twostage();
    if (!h) { set_error("out of host memory"); return nullptr; }
    int r = h->core.init(device, inputs, outputs, responses, response_len, response_stride, max_block_size,
                         max_response_length);
    return make_or_null(r, h);
}
int fftconv_matrix_twostage_update(fftconv_matrix_twostage *h, const float *, size_t, size_t) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return fail(FFTCONV_E_UNIMPLEMENTED, "not yet implemented (TwoStageFFTConvolver::update is todo!())");
}
int fftconv_matrix_twostage_reset(fftconv_matrix_twostage *h) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return h->core.reset();
}
int fftconv_matrix_twostage_process(fftconv_matrix_twostage *h, const float *input, float *output, size_t len) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return h->core.process_host(input, output, len);
}
int fftconv_matrix_twostage_process_device(fftconv_matrix_twostage *h, const float *d_input, size_t in_stride,
                                           float *d_output, size_t out_stride, size_t len, void *hip_stream) {
    return abi_process_device(h, d_input, in_stride, d_output, out_stride, len, hip_stream);
}
int fftconv_matrix_twostage_process_device_steps(fftconv_matrix_twostage *h, const float *d_input, size_t in_stride,
                                                 size_t in_step, float *d_output, size_t out_stride, size_t out_step,
                                                 size_t len, size_t steps, void *hip_stream) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    DeviceGuard g(h->core.device);
    hipStream_t s = (hipStream_t)hip_stream;
    if (int r = h->core.order.enter(s)) return r;
    return h->core.process_device_steps(d_input, in_stride, in_step, d_output, out_stride, out_step, len, steps, s);
}
fftconv_matrix_twostage *fftconv_matrix_twostage_clone(const fftconv_matrix_twostage *h) { return abi_clone(h); }
void fftconv_matrix_twostage_destroy(fftconv_matrix_twostage *h) { delete h; }
int fftconv_matrix_twostage_synchronize(fftconv_matrix_twostage *h) { return abi_synchronize(h); }
size_t fftconv_matrix_twostage_inputs(const fftconv_matrix_twostage *h) { return h ? h->core.I : 0; }
size_t fftconv_matrix_twostage_outputs(const fftconv_matrix_twostage *h) { return h ? h->core.O : 0; }
size_t fftconv_matrix_twostage_tail_block_size(const fftconv_matrix_twostage *h) { return h ? h->core.T : 0; }
int fftconv_matrix_twostage_set_fused(fftconv_matrix_twostage *h, int on) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    h->core.fused = on != 0;
    return FFTCONV_OK;
}
int fftconv_matrix_twostage_path(const fftconv_matrix_twostage *h, size_t len) { return h ? h->core.path(len) : 0; }

// ---- sparse matrix two-stage ---------------------------------------
fftconv_matrix_sparse_twostage *fftconv_matrix_sparse_twostage_init(int device, size_t inputs, size_t outputs,
                                                                    size_t pairs, const uint32_t *pair_out,
                                                                    const uint32_t *pair_in, const float *responses,
                                                                    size_t response_len, size_t response_stride,
                                                                    size_t max_block_size, size_t max_response_length) {
    return abi_init<fftconv_matrix_sparse_twostage>(device, inputs, outputs, pairs, pair_out, pair_in, responses,
                                                    response_len, response_stride, max_block_size, max_response_length);
}
int fftconv_matrix_sparse_twostage_update(fftconv_matrix_sparse_twostage *h, const float *, size_t, size_t) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return fail(FFTCONV_E_UNIMPLEMENTED, "not yet implemented (TwoStageFFTConvolver::update is todo!())");
}
int fftconv_matrix_sparse_twostage_reset(fftconv_matrix_sparse_twostage *h) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return h->core.reset();
}
int fftconv_matrix_sparse_twostage_process(fftconv_matrix_sparse_twostage *h, const float *input, float *output,
                                           size_t len) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    return h->core.process_host(input, output, len);
}
int fftconv_matrix_sparse_twostage_process_device(fftconv_matrix_sparse_twostage *h, const float *d_input,
                                                  size_t in_stride, float *d_output, size_t out_stride, size_t len,
                                                  void *hip_stream) {
    return abi_process_device(h, d_input, in_stride, d_output, out_stride, len, hip_stream);
}
int fftconv_matrix_sparse_twostage_process_device_steps(fftconv_matrix_sparse_twostage *h, const float *d_input,
                                                        size_t in_stride, size_t in_step, float *d_output,
                                                        size_t out_stride, size_t out_step, size_t len, size_t steps,
                                                        void *hip_stream) {
    return abi_process_device_steps(h, d_input, in_stride, in_step, d_output, out_stride, out_step, len, steps, hip_stream);
}
fftconv_matrix_sparse_twostage *fftconv_matrix_sparse_twostage_clone(const fftconv_matrix_sparse_twostage *h) {
    return abi_clone(h);
}
void fftconv_matrix_sparse_twostage_destroy(fftconv_matrix_sparse_twostage *h) { delete h; }
int fftconv_matrix_sparse_twostage_synchronize(fftconv_matrix_sparse_twostage *h) { return abi_synchronize(h); }
size_t fftconv_matrix_sparse_twostage_inputs(const fftconv_matrix_sparse_twostage *h) { return h ? h->core.I : 0; }
size_t fftconv_matrix_sparse_twostage_outputs(const fftconv_matrix_sparse_twostage *h) { return h ? h->core.O : 0; }
size_t fftconv_matrix_sparse_twostage_pairs(const fftconv_matrix_sparse_twostage *h) { return h ? h->core.P : 0; }
size_t fftconv_matrix_sparse_twostage_tail_block_size(const fftconv_matrix_sparse_twostage *h) { return h ? h->core.T : 0; }
int fftconv_matrix_sparse_twostage_set_fused(fftconv_matrix_sparse_twostage *h, int on) {
    if (!h) return fail(FFTCONV_E_INVALID, "null handle");
    h->core.fused = on != 0;
    return FFTCONV_OK;
}
int fftconv_matrix_sparse_twostage_path(const fftconv_matrix_sparse_twostage *h, size_t len) {
    return h ? h->core.path(len) : 0;
}

}  // extern "C"
