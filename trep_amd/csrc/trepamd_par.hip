// trepamd_par.hip -- the generic kernels with per-trajectory masses / inertias, gravity and damping (tg_batch_set_parameters).
//
// k_run_par is k_run (trepamd.hip) with one more argument: the parameter table (mvi_core.hpp, ParTable).  The trajectory's row takes
// the place of the schedule's body inertias, gravity and damping (run_trajectory<..., PAR = true>); everything else -- launch
// geometry, LDS slice, launch bounds -- is its twin's.  A translation unit of its own so that it compiles beside trepamd.hip.
#include <hip/hip_runtime.h>

#include "launch_generic.hpp"

namespace {

template <int TEAM, int MODE, bool SPRINGS>
__global__ __launch_bounds__(64, (MODE == tg::MODE_DERIV1 || MODE == tg::MODE_DERIV2Z || MODE == tg::MODE_DYN_DERIV1) ? 1 : 2) void k_run_par(const tg::DevProg *__restrict__ Pg, const tg::RunArgs A, const tg::ParTable T) {
    double *lds = tg_lds_base();
    tg::CProg &P = *(tg::CProg *)Pg;
    const int team = threadIdx.x / TEAM, lane = threadIdx.x % TEAM;
    const int block = MODE == tg::MODE_ROLLOUT ? tg_xcd_block((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
    const int traj = tg::tg_remap_trajectory(A, block * (64 / TEAM) + team);
    const int stride = MODE == tg::MODE_DERIV2Z ? P.e_lds_per_team : (MODE == tg::MODE_DERIV1 ? P.a_lds_per_team : (MODE == tg::MODE_DYN_DERIV1 ? P.g_lds_per_team : P.lds_per_team));
    tg::run_trajectory<TEAM, MODE, SPRINGS, tg::CProg, tg::CArgs, -1, true>(P, A, lds + (size_t)team * stride, lane, traj, 0, 1, T);
}

template <int TEAM, int MODE>
int launch_one(bool springs, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::ParTable &T, int grid, size_t lds, hipStream_t stream) {
    return tg_detail::launch_kernel(springs ? &k_run_par<TEAM, MODE, true> : &k_run_par<TEAM, MODE, false>, grid, lds, stream, d_prog, A, T);
}

template <int TEAM>
int launch_team(bool springs, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::ParTable &T, int grid, size_t lds, hipStream_t stream) {
    switch (A.mode) {
    case tg::MODE_ROLLOUT: return launch_one<TEAM, tg::MODE_ROLLOUT>(springs, d_prog, A, T, grid, lds, stream);
    case tg::MODE_CALC_P2: return launch_one<TEAM, tg::MODE_CALC_P2>(springs, d_prog, A, T, grid, lds, stream);
    case tg::MODE_CALC_F: return launch_one<TEAM, tg::MODE_CALC_F>(springs, d_prog, A, T, grid, lds, stream);
    case tg::MODE_DERIV1: return launch_one<TEAM, tg::MODE_DERIV1>(springs, d_prog, A, T, grid, lds, stream);
    case tg::MODE_DERIV2Z: return launch_one<TEAM, tg::MODE_DERIV2Z>(springs, d_prog, A, T, grid, lds, stream);
    case tg::MODE_DYNAMICS: return launch_one<TEAM, tg::MODE_DYNAMICS>(springs, d_prog, A, T, grid, lds, stream);
    case tg::MODE_DYN_DERIV1: return launch_one<TEAM, tg::MODE_DYN_DERIV1>(springs, d_prog, A, T, grid, lds, stream);
    case tg::MODE_ENERGY: return launch_one<TEAM, tg::MODE_ENERGY>(springs, d_prog, A, T, grid, lds, stream);
    case tg::MODE_LAGRANGIAN: return launch_one<TEAM, tg::MODE_LAGRANGIAN>(springs, d_prog, A, T, grid, lds, stream);
    default: return tg_detail::fail(TG_ERR_INVALID, "unknown kernel mode");
    }
}

}  // namespace

namespace tg_detail {
int launch_par(int team, bool springs, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::ParTable &T, int grid, size_t lds, hipStream_t stream) {
#if defined(TG_PROFILE)   // the diagnostic build instruments the default kernels only
    (void)team; (void)springs; (void)d_prog; (void)A; (void)T; (void)grid; (void)lds; (void)stream;
    return fail(TG_ERR_UNSUPPORTED, "the profiling build has no per-trajectory parameter kernels");
#else
    return dispatch_team(team, [&](auto team_tag) { return launch_team<decltype(team_tag)::value>(springs, d_prog, A, T, grid, lds, stream); });
#endif
}
}  // namespace tg_detail
