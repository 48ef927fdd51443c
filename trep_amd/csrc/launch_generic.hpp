// launch_generic.hpp -- what every translation unit of generic kernels does to launch one (host only): trepamd.hip, trepamd_par.hip,
// trepamd_project.hip, trepamd_equilibrium.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "mvi_core.hpp"

namespace tg_detail {
int fail(int code, const std::string &msg);

// One 64-thread workgroup per grid entry with `lds` bytes of dynamic LDS; above 64 KiB a kernel has to opt in first.
template <class... Params, class... Args>
int launch_kernel(void (*kernel)(Params...), int grid, size_t lds, hipStream_t stream, const Args &...args) {
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return fail(TG_ERR_HIP, std::string("hipFuncSetAttribute failed: ") + hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), lds, stream, args...);
    return TG_SUCCESS;
}

// f(IntTag<TEAM>()) for the team size of the system: 64, 16, 4 or 1 lanes per trajectory
template <class F>
int dispatch_team(int team, F &&f) {
    return team == 64 ? f(tg::IntTag<64>()) : (team == 16 ? f(tg::IntTag<16>()) : (team == 4 ? f(tg::IntTag<4>()) : f(tg::IntTag<1>())));
}
}  // namespace tg_detail
