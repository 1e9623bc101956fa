// launch.hpp -- host-side helpers of the launchers (kernels.hip, large.hip,
// matrix.hip): run-time log2 -> template argument, and the launch sequence of
// a kernel with dynamic LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <type_traits>

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

}  // namespace fftconv
