// trepamd_inverse.hip -- k_inverse: the inverse-dynamics kernel (mvi_inverse.hpp, MODE_INVERSE; tg_batch_inverse_dynamics).
//
// Launch geometry of the generic kernels (trepamd.hip): one 64-thread workgroup holds 64 / TEAM teams; here a team is one step of one
// trajectory, team index b * n_steps + k, and its LDS slice is the rollout slice plus the solve's scratch
// (InverseArgs::lds_per_team).  Generic only, with a parameter-table twin (PAR): momenta and residuals depend on masses, gravity and
// damping, so a set table is honoured, trajectory b using row b / group.  A translation unit of its own so that it compiles beside
// trepamd.hip.
#include <hip/hip_runtime.h>

#include "launch_generic.hpp"
#include "mvi_inverse.hpp"

namespace {

// SOLVE: 0 the augmented image, 1 lsq_solve.hpp's least squares (LSQ), 2 bvls_solve.hpp's bounded least squares (BND)
template <int TEAM, bool SPRINGS, bool PAR, int SOLVE>
__global__ __launch_bounds__(64, 1) void k_inverse(const tg::DevProg *__restrict__ Pg, const tg::RunArgs A, const tg::InverseArgs J, const tg::ParTable T) {
    double *lds = tg_lds_base();
    tg::CProg &P = *(tg::CProg *)Pg;
    const int team = threadIdx.x / TEAM, lane = threadIdx.x % TEAM;
    const long long index = (long long)blockIdx.x * (64 / TEAM) + team;
    tg::run_inverse<TEAM, SPRINGS, PAR, SOLVE == 1, SOLVE == 2>(P, A, J, T, lds + (size_t)team * J.lds_per_team, lane, index);
}

}  // namespace

namespace tg_detail {
int launch_inverse(int team, bool springs, bool par, int solve, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::InverseArgs &J, const tg::ParTable &T, int grid, size_t lds, hipStream_t stream) {
#if defined(TG_PROFILE)   // the diagnostic build instruments the default kernels only
    (void)team; (void)springs; (void)par; (void)solve; (void)d_prog; (void)A; (void)J; (void)T; (void)grid; (void)lds; (void)stream;
    return fail(TG_ERR_UNSUPPORTED, "the profiling build has no inverse-dynamics kernel");
#else
    return dispatch_team(team, [&](auto team_tag) {
        constexpr int TEAM = decltype(team_tag)::value;
        auto pick = [&](auto solve_tag) {      // 1: tg_batch_inverse_dynamics_lsq, 2: tg_batch_inverse_dynamics_bounded
            constexpr int SOLVE = decltype(solve_tag)::value;
            return par ? (springs ? &k_inverse<TEAM, true, true, SOLVE> : &k_inverse<TEAM, false, true, SOLVE>)
                       : (springs ? &k_inverse<TEAM, true, false, SOLVE> : &k_inverse<TEAM, false, false, SOLVE>);
        };
        return launch_kernel(solve == 2 ? pick(tg::IntTag<2>()) : (solve == 1 ? pick(tg::IntTag<1>()) : pick(tg::IntTag<0>())), grid, lds, stream, d_prog, A, J, T);
    });
#endif
}
}  // namespace tg_detail
