// trepamd_modes.hip -- k_modes: the normal-modes kernel (mvi_modes.hpp, MODE_MODES; tg_batch_normal_modes).
//
// Launch geometry of the generic kernels (trepamd.hip): one 64-thread workgroup holds 64 / TEAM teams, one pose per team; the team's
// LDS slice is the rollout slice plus the kernel's scratch (ModesArgs::lds_per_team).  Generic only, with a parameter-table
// twin (PAR): frequencies depend on masses, inertias and gravity, so a set table is honoured; damping plays no part.  A translation unit
// of its own so that it compiles beside trepamd.hip.
#include <hip/hip_runtime.h>

#include "launch_generic.hpp"
#include "mvi_modes.hpp"

namespace {

template <int TEAM, bool SPRINGS, bool PAR>
__global__ __launch_bounds__(64, 1) void k_modes(const tg::DevProg *__restrict__ Pg, const tg::RunArgs A, const tg::ModesArgs J, const tg::ParTable T) {
    double *lds = tg_lds_base();
    tg::CProg &P = *(tg::CProg *)Pg;
    const int team = threadIdx.x / TEAM, lane = threadIdx.x % TEAM;
    const int traj = tg::tg_remap_trajectory(A, (int)blockIdx.x * (64 / TEAM) + team);
    tg::run_modes<TEAM, SPRINGS, PAR>(P, A, J, T, lds + (size_t)team * J.lds_per_team, lane, traj);
}

}  // namespace

namespace tg_detail {
int launch_modes(int team, bool springs, bool par, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::ModesArgs &J, const tg::ParTable &T, int grid, size_t lds, hipStream_t stream) {
#if defined(TG_PROFILE)   // the diagnostic build instruments the default kernels only
    (void)team; (void)springs; (void)par; (void)d_prog; (void)A; (void)J; (void)T; (void)grid; (void)lds; (void)stream;
    return fail(TG_ERR_UNSUPPORTED, "the profiling build has no normal-modes kernel");
#else
    return dispatch_team(team, [&](auto team_tag) {
        constexpr int TEAM = decltype(team_tag)::value;
        auto kernel = par ? (springs ? &k_modes<TEAM, true, true> : &k_modes<TEAM, false, true>)
                          : (springs ? &k_modes<TEAM, true, false> : &k_modes<TEAM, false, false>);
        return launch_kernel(kernel, grid, lds, stream, d_prog, A, J, T);
    });
#endif
}
}  // namespace tg_detail
