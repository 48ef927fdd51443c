// trepamd_dyn_inverse.hip -- k_dyn_inverse: the computed-torque kernel (mvi_dyn_inverse.hpp, MODE_DYN_INVERSE; tg_batch_dynamics_inverse).
//
// Launch geometry of the generic kernels (trepamd.hip): one 64-thread workgroup holds 64 / TEAM teams; here a team is one state of one
// trajectory, team index b * n_states + s, and its LDS slice is the rollout slice plus the solve's scratch
// (DynInverseArgs::lds_per_team).  Generic only, with a parameter-table twin (PAR): the residual depends on masses, gravity and
// damping, so a set table is honoured, trajectory b using row b / group.  A translation unit of its own so that it compiles beside
// trepamd.hip.
#include <hip/hip_runtime.h>

#include "launch_generic.hpp"
#include "mvi_dyn_inverse.hpp"

namespace {

template <int TEAM, bool SPRINGS, bool PAR>
__global__ __launch_bounds__(64, 1) void k_dyn_inverse(const tg::DevProg *__restrict__ Pg, const tg::RunArgs A, const tg::DynInverseArgs J, const tg::ParTable T) {
    double *lds = tg_lds_base();
    tg::CProg &P = *(tg::CProg *)Pg;
    const int team = threadIdx.x / TEAM, lane = threadIdx.x % TEAM;
    const long long index = (long long)blockIdx.x * (64 / TEAM) + team;
    tg::run_dyn_inverse<TEAM, SPRINGS, PAR>(P, A, J, T, lds + (size_t)team * J.lds_per_team, lane, index);
}

}  // namespace

namespace tg_detail {
int launch_dyn_inverse(int team, bool springs, bool par, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::DynInverseArgs &J, const tg::ParTable &T, int grid, size_t lds, hipStream_t stream) {
#if defined(TG_PROFILE)   // the diagnostic build instruments the default kernels only
    (void)team; (void)springs; (void)par; (void)d_prog; (void)A; (void)J; (void)T; (void)grid; (void)lds; (void)stream;
    return fail(TG_ERR_UNSUPPORTED, "the profiling build has no computed-torque kernel");
#else
    return dispatch_team(team, [&](auto team_tag) {
        constexpr int TEAM = decltype(team_tag)::value;
        auto kernel = par ? (springs ? &k_dyn_inverse<TEAM, true, true> : &k_dyn_inverse<TEAM, false, true>)
                          : (springs ? &k_dyn_inverse<TEAM, true, false> : &k_dyn_inverse<TEAM, false, false>);
        return launch_kernel(kernel, grid, lds, stream, d_prog, A, J, T);
    });
#endif
}
}  // namespace tg_detail
