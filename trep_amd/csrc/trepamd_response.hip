// trepamd_response.hip -- k_response: the static-response kernel (mvi_response.hpp, MODE_RESPONSE; tg_batch_static_response).
//
// Launch geometry of the generic kernels (trepamd.hip): one 64-thread workgroup holds 64 / TEAM teams, one pose per team; the team's
// LDS slice is the rollout slice plus the kernel's scratch (ResponseArgs::lds_per_team).  Generic only, with a parameter-table
// twin (PAR): the rest pose's stiffness depends on masses and gravity, so a set table is honoured; inertias and damping play no part.
// A translation unit of its own so that it compiles beside trepamd.hip.
#include <hip/hip_runtime.h>

#include "launch_generic.hpp"
#include "mvi_response.hpp"

namespace {

template <int TEAM, bool SPRINGS, bool PAR>
__global__ __launch_bounds__(64, 1) void k_response(const tg::DevProg *__restrict__ Pg, const tg::RunArgs A, const tg::ResponseArgs J, const tg::ParTable T) {
    double *lds = tg_lds_base();
    tg::CProg &P = *(tg::CProg *)Pg;
    const int team = threadIdx.x / TEAM, lane = threadIdx.x % TEAM;
    const int traj = tg::tg_remap_trajectory(A, (int)blockIdx.x * (64 / TEAM) + team);
    tg::run_response<TEAM, SPRINGS, PAR>(P, A, J, T, lds + (size_t)team * J.lds_per_team, lane, traj);
}

}  // namespace

namespace tg_detail {
int launch_response(int team, bool springs, bool par, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::ResponseArgs &J, const tg::ParTable &T, int grid, size_t lds, hipStream_t stream) {
#if defined(TG_PROFILE)   // the diagnostic build instruments the default kernels only
    (void)team; (void)springs; (void)par; (void)d_prog; (void)A; (void)J; (void)T; (void)grid; (void)lds; (void)stream;
    return fail(TG_ERR_UNSUPPORTED, "the profiling build has no static-response kernel");
#else
    return dispatch_team(team, [&](auto team_tag) {
        constexpr int TEAM = decltype(team_tag)::value;
        auto kernel = par ? (springs ? &k_response<TEAM, true, true> : &k_response<TEAM, false, true>)
                          : (springs ? &k_response<TEAM, true, false> : &k_response<TEAM, false, false>);
        return launch_kernel(kernel, grid, lds, stream, d_prog, A, J, T);
    });
#endif
}
}  // namespace tg_detail
