// variant.hpp -- the kernel-variant setting (fftconv_set_kernel_variant) and
// every rule that reads it.  Host side only.
#pragma once
#include <stddef.h>

namespace fftconv {

// One row per bit.  "launch": read by every launch (one snapshot each);
// "create": read when a handle is created, later changes do not reach it.
//
//   bit  value  name       read    set means (default = the "else")
//   0    1      ZIGZAG     launch  zig-zag segment scan on alternate blocks (else plain order; changes the
//                                  summation order, so opt-in only)
//   1    2      NT         launch  nontemporal H / X loads (else plain loads)
//   2    4      NOPIPE     launch  no pipelined full-block step
//                                  -- bits 0-2 are the scan bits: they replace the automatic load / step
//                                     policy only when one of them is set (Variant::scan_set)
//   3    8      NOPAIR     launch  no crossfade pair launch (A and B stream the shared FDL separately)
//   4    16     NOLA       both    no lookahead step (create: no windows are allocated; every call
//                                  re-checks it and leaves the lookahead step when it no longer matches)
//   5    32     LAFULL     launch  lookahead launches without anchors: every step sums all rows itself (tests)
//   6    64     NOFMIX     launch  crossfade on the lookahead step: stand-alone mix kernel (else B's epilogue)
//   7    128    IRBLOCK    launch  IR transforms one segment per workgroup (else one per wave, 64 <= B <= 1024)
//   8    256    T0BLOCK    create  two-stage tail0 per block (else deferred to the end of its period)
//   9    512    T0FUSED    launch  deferred tail0 at B = 64: the five-kernel flush (else the ONE fused kernel;
//                                  bit-identical -- despite its name the bit turns the fusion off)
//   10   1024   NOGW       launch  B >= 1024: no far-row windows, every step sums its far rows itself (tests)
//   11   2048   NORUN      launch  process_device_steps: one launch per call (else a run of calls per launch,
//                                  or on the lookahead step a batch of steps in four launches, la_batch.hpp)
//   12   4096   NORUNLDS   launch  runs stream the FDL / IR rows from memory (else from LDS copies; same bits).
//                                  NOT selectable: the ABI accepts 0..4095 and set_variant masks with 4095,
//                                  so the branch that reads it never runs
enum : int {
    VARIANT_ZIGZAG = 1, VARIANT_NT = 2, VARIANT_NOPIPE = 4, VARIANT_NOPAIR = 8, VARIANT_NOLA = 16,
    VARIANT_LAFULL = 32, VARIANT_NOFMIX = 64, VARIANT_IRBLOCK = 128, VARIANT_T0BLOCK = 256, VARIANT_T0FUSED = 512,
    VARIANT_NOGW = 1024, VARIANT_NORUN = 2048, VARIANT_NORUNLDS = 4096,
    VARIANT_AUTO = 0x7fffffff
};
void set_variant(int v);  // v < 0: automatic, else v & 4095
int get_variant();        // -1 = automatic
void set_pipeline_lag(int rows);
int get_pipeline_lag();

// One snapshot of the process-wide setting: a launcher takes it once and
// decides everything from it (a setter on another thread cannot change the
// setting between two of its tests).
struct Variant {
    int bits;  // VARIANT_AUTO, or the bits set

    static Variant current();  // (one relaxed load, host.cpp)

    bool is_auto() const { return bits == VARIANT_AUTO; }
    bool has(int bit) const { return !is_auto() && (bits & bit) != 0; }
    bool scan_set() const { return has(7); }

    // Nontemporal loads of a per-step H + X stream of `bytes`.  A stream
    // larger than the 256 MiB Infinity Cache is re-read from HBM every step
    // whatever the load policy, and there nontemporal loads stream 12-14 %
    // faster (measured, cfg2: 137 -> 121 us); a stream that stays
    // cache-resident across steps is 1.5x faster with plain loads (S = 8: 9.5
    // vs 14.3 us).  Both perform identical arithmetic, so the choice never
    // changes a result bit.
    bool nt_stream(double bytes) const {
        return scan_set() ? (bits & VARIANT_NT) != 0 : bytes > 192.0 * 1024 * 1024;
    }
    // the H + X stream of a uniform batch's step
    static double stream_bytes(int channels, int S, int log2b) {
        return 16.0 * (double)channels * (double)S * (double)(1 << log2b);
    }
    // The MatrixConvolver's H loads.  Unlike nt_stream it weighs H alone
    // against the cache's whole 256 MiB, and ANY set variant decides by its NT
    // bit, variant 0 included: the matrix tests select each instantiation by
    // name that way (variant 0 = plain loads at every size).
    bool nt_matrix(size_t h_bytes) const {
        return is_auto() ? h_bytes > ((size_t)256 << 20) : (bits & VARIANT_NT) != 0;
    }

    // The step's variant bits for a launch streaming `bytes` per step whose
    // longest FDL holds `fdl_bins` bins: the setting itself when a scan bit is
    // set, else the automatic policy with the setting's feature bits.
    //
    // Zig-zag (+0.6 % on top of NT) changes the summation order and is
    // therefore opt-in only, keeping channel shards bit-identical whatever
    // the shard size.
    //
    // The pipelined full-block step pays off where a channel's FDL stream is
    // short next to its transform chain (cfg3's head, S*B = 4096: 1630 -> 1860
    // MS/s) and costs ~3 % on long ones (cfg2, S*B = 48128: the other resident
    // workgroups' streams already cover each chain, and three stream waves
    // issue fewer loads than four).  It changes the summation order, so it is
    // chosen per channel geometry (never by channel count): shards stay
    // bit-identical.
    int step_bits(double bytes, long long fdl_bins) const {
        if (scan_set()) return bits;
        return (nt_stream(bytes) ? VARIANT_NT : 0) | (fdl_bins > 16384 ? VARIANT_NOPIPE : 0) | (is_auto() ? 0 : bits);
    }
};

}  // namespace fftconv
