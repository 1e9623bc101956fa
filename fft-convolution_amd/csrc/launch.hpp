// launch.hpp -- host-side helpers of the launchers (every .hip file): run-time
// log2 -> template argument, the launch sequence of a kernel with dynamic LDS,
// and the step launches' share of the variant policy.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <algorithm>
#include <type_traits>

#include "kernels.hpp"

namespace fftconv {

// f(std::integral_constant<int, v>) for LO <= v <= HI, else `out_of_range`
// (the callers' error codes differ).  In f, `L()` is the constant.
template <int LO, int HI, class R, class F>
R dispatch_log2(int v, R out_of_range, F &&f) {
    if constexpr (LO > HI) {
        return out_of_range;
    } else {
        if (v == LO) return f(std::integral_constant<int, LO>{});
        return dispatch_log2<LO + 1, HI>(v, out_of_range, f);
    }
}

// more than 64 KiB of dynamic LDS has to be allowed per kernel function (one
// call per launch: not cached)
template <class K>
hipError_t lds_attr(K kern, size_t lds) {
    if (lds > 64 * 1024)
        return hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    return hipSuccess;
}

template <class K, class... Args>
hipError_t launch_dyn(K kern, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args &...args) {
    if (hipError_t e = lds_attr(kern, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, block, lds, s, args...);
    return hipGetLastError();
}

// the fused kernels' block sizes: 1 <= B <= 8192
template <class F>
hipError_t dispatch_fused(int log2b, F &&f) {
    return dispatch_log2<0, kMaxLog2Fused>(log2b, hipErrorInvalidValue, f);
}

// Pipelined step: FDL rows the three stream waves take alone while wave 0
// runs the transform chain.  Auto: all of them -- wave 0 never streams (cfg3
// head, S = 64, swept in-process: lag 0 1527, 16 1586, 32 1635, 48 1754,
// >= 62 1844 MS/s; the chain is the critical path, any row given to wave 0
// lengthens it).  Never a function of the channel count, so channel shards
// of any size stay bit-identical.
inline int pipeline_lag() {
    const int lag = get_pipeline_lag();
    return lag >= 0 ? lag : (1 << 30);
}

// the step's variant bits for a launch of a.njobs jobs (Variant::step_bits)
inline int pick_variant(Variant v, const ProcArgs &a, int channels, int log2b) {
    double stream = 0.0;
    long long rows = 0;
    for (int j = 0; j < a.njobs; ++j) {
        stream += Variant::stream_bytes(channels, a.job[j].S, log2b);
        rows = std::max(rows, (long long)a.job[j].S);
    }
    return v.step_bits(stream, rows << log2b);
}

}  // namespace fftconv
