// trepamd_project.hip -- k_project: the constraint-projection kernel (mvi_project.hpp, MODE_PROJECT; tg_batch_project_constraints).
//
// Launch geometry of the generic kernels (trepamd.hip): one 64-thread workgroup holds 64 / TEAM teams, one trajectory per team; the
// team's LDS slice is the rollout slice plus the projection's scratch (ProjectArgs::lds_per_team).  Generic only: constraints do not
// depend on masses, gravity or damping, so there is no parameter-table twin and no specialised one.  A translation unit of its own so
// that it compiles beside trepamd.hip.
#include <hip/hip_runtime.h>

#include "launch_generic.hpp"
#include "mvi_project.hpp"

namespace {

template <int TEAM, bool SPRINGS>
__global__ __launch_bounds__(64, 1) void k_project(const tg::DevProg *__restrict__ Pg, const tg::RunArgs A, const tg::ProjectArgs J) {
    double *lds = tg_lds_base();
    tg::CProg &P = *(tg::CProg *)Pg;
    const int team = threadIdx.x / TEAM, lane = threadIdx.x % TEAM;
    const int traj = tg::tg_remap_trajectory(A, (int)blockIdx.x * (64 / TEAM) + team);
    tg::run_project<TEAM, SPRINGS>(P, A, J, lds + (size_t)team * J.lds_per_team, lane, traj);
}

}  // namespace

namespace tg_detail {
int launch_project(int team, bool springs, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::ProjectArgs &J, int grid, size_t lds, hipStream_t stream) {
#if defined(TG_PROFILE)   // the diagnostic build instruments the default kernels only
    (void)team; (void)springs; (void)d_prog; (void)A; (void)J; (void)grid; (void)lds; (void)stream;
    return fail(TG_ERR_UNSUPPORTED, "the profiling build has no projection kernel");
#else
    return dispatch_team(team, [&](auto team_tag) {
        constexpr int TEAM = decltype(team_tag)::value;
        return launch_kernel(springs ? &k_project<TEAM, true> : &k_project<TEAM, false>, grid, lds, stream, d_prog, A, J);
    });
#endif
}
}  // namespace tg_detail
