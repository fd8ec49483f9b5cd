// launch.h -- host-side launch helpers shared by passes.hip and the dense matrix-core files: the dynamic-LDS attribute, the
// checked launch, and run-time value -> template argument.
#pragma once
#include "common.h"
#include <type_traits>

namespace oriana {

// run-time variant -> template argument: f(std::integral_constant<int, v>) for the v of the list, ORIANA_EINVAL for any other
template <int... Vs, typename F>
static int with_variant(int v, F &&f) {
    int rc = ORIANA_EINVAL;
    (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return rc;
}

template <typename KernelT>
static int set_lds(KernelT kern, size_t bytes) {
    if (bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return -1000 - (int)e;
    }
    return 0;
}

// set_lds, then the launch; the arguments convert to the kernel's parameter types (nullptr, 0)
template <typename... P, typename... A>
static int launch(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, const A &...args) {
    const int rc = set_lds(kern, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(kern, grid, block, lds, s, static_cast<P>(args)...);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

}  // namespace oriana
