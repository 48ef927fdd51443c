// trepamd_project.hip -- k_project: the constraint-projection kernel (mvi_project.hpp, MODE_PROJECT; tg_batch_project_constraints).
//
// Launch geometry of the generic kernels (trepamd.hip): one 64-thread workgroup holds 64 / TEAM teams, one trajectory per team; the
// team's LDS slice is the rollout slice plus the projection's scratch (ProjectArgs::lds_per_team).  Generic only: constraints do not
// depend on masses, gravity or damping, so there is no parameter-table twin and no specialised one.  A translation unit of its own so
// that it compiles beside trepamd.hip.
#include <hip/hip_runtime.h>

#include <string>

#include "mvi_project.hpp"

namespace tg_detail {
int fail(int code, const std::string &msg);
}

namespace {

template <int TEAM, bool SPRINGS>
__global__ __launch_bounds__(64, 1) void k_project(const tg::DevProg *__restrict__ Pg, const tg::RunArgs A, const tg::ProjectArgs J) {
    double *lds = tg_lds_base();
    tg::CProg &P = *(tg::CProg *)Pg;
    const int team = threadIdx.x / TEAM, lane = threadIdx.x % TEAM;
    const int traj = tg::tg_remap_trajectory(A, (int)blockIdx.x * (64 / TEAM) + team);
    tg::run_project<TEAM, SPRINGS>(P, A, J, lds + (size_t)team * J.lds_per_team, lane, traj);
}

template <int TEAM, bool SPRINGS>
int launch_variant(const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::ProjectArgs &J, int grid, size_t lds, hipStream_t stream) {
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(&k_project<TEAM, SPRINGS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return tg_detail::fail(TG_ERR_HIP, "hipFuncSetAttribute failed");
    hipLaunchKernelGGL((k_project<TEAM, SPRINGS>), dim3(grid), dim3(64), lds, stream, d_prog, A, J);
    return TG_SUCCESS;
}

template <int TEAM>
int launch_team(bool springs, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::ProjectArgs &J, int grid, size_t lds, hipStream_t stream) {
    return springs ? launch_variant<TEAM, true>(d_prog, A, J, grid, lds, stream) : launch_variant<TEAM, false>(d_prog, A, J, grid, lds, stream);
}

}  // namespace

namespace tg_detail {
int launch_project(int team, bool springs, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::ProjectArgs &J, int grid, size_t lds, hipStream_t stream) {
#if defined(TG_PROFILE)   // the diagnostic build instruments the default kernels only
    (void)team; (void)springs; (void)d_prog; (void)A; (void)J; (void)grid; (void)lds; (void)stream;
    return fail(TG_ERR_UNSUPPORTED, "the profiling build has no projection kernel");
#else
    return team == 64 ? launch_team<64>(springs, d_prog, A, J, grid, lds, stream)
           : (team == 16 ? launch_team<16>(springs, d_prog, A, J, grid, lds, stream)
              : (team == 4 ? launch_team<4>(springs, d_prog, A, J, grid, lds, stream) : launch_team<1>(springs, d_prog, A, J, grid, lds, stream)));
#endif
}
}  // namespace tg_detail
