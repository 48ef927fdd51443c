// trepamd_dyn_inverse.hip -- k_dyn_inverse: the computed-torque kernel (mvi_dyn_inverse.hpp, MODE_DYN_INVERSE; tg_batch_dynamics_inverse).
//
// Launch geometry of the generic kernels (trepamd.hip): one 64-thread workgroup holds 64 / TEAM teams; here a team is one state of one
// trajectory, team index b * n_states + s, and its LDS slice is the rollout slice plus the solve's scratch
// (DynInverseArgs::lds_per_team).  Generic only, with a parameter-table twin (PAR): the residual depends on masses, gravity and
// damping, so a set table is honoured, trajectory b using row b / group.  A translation unit of its own so that it compiles beside
// trepamd.hip.
// LSQ: the instantiations whose solve is the rank-revealing least squares of lsq_solve.hpp (tg_batch_dynamics_inverse_lsq), and
// k_lsq_debug, that solver alone on caller-supplied problems, one team each (tg_batch_debug_lsq_solve).
#include <hip/hip_runtime.h>

#include "launch_generic.hpp"
#include "mvi_dyn_inverse.hpp"

namespace {

// SOLVE: 0 the augmented image, 1 lsq_solve.hpp's least squares (LSQ), 2 bvls_solve.hpp's bounded least squares (BND)
template <int TEAM, bool SPRINGS, bool PAR, int SOLVE>
__global__ __launch_bounds__(64, 1) void k_dyn_inverse(const tg::DevProg *__restrict__ Pg, const tg::RunArgs A, const tg::DynInverseArgs J, const tg::ParTable T) {
    double *lds = tg_lds_base();
    tg::CProg &P = *(tg::CProg *)Pg;
    const int team = threadIdx.x / TEAM, lane = threadIdx.x % TEAM;
    const long long index = (long long)blockIdx.x * (64 / TEAM) + team;
    tg::run_dyn_inverse<TEAM, SPRINGS, PAR, SOLVE == 1, SOLVE == 2>(P, A, J, T, lds + (size_t)team * J.lds_per_team, lane, index);
}

// problem p = blockIdx.x * (blockDim.x / TEAM) + team of `count`: A [rows][cols] and c [rows] into the team's block W [rows][cols + 1],
// the solve, z [cols], rank and status out.  per_team: doubles of LDS per team (the block and the solver's scratch).  The workgroup
// holds 64 / TEAM teams, or as many as the LDS takes (blockDim.x a multiple of TEAM, at most 64)
template <int TEAM>
__global__ __launch_bounds__(64, 1) void k_lsq_debug(int count, int rows, int cols, int per_team, const double *__restrict__ Ag,
                                                     const double *__restrict__ cg, double rcond, double *__restrict__ zg, int *__restrict__ rank,
                                                     int *__restrict__ status) {
    double *lds = tg_lds_base();
    const int team = threadIdx.x / TEAM, lane = threadIdx.x % TEAM;
    const long long p = (long long)blockIdx.x * (blockDim.x / TEAM) + team;
    const bool on = p < count;
    const int ld = cols + 1;
    double *W = lds + (size_t)team * per_team, *scr = W + (size_t)rows * ld;
    if (on) {
        const double *a = Ag + (size_t)p * rows * cols, *c = cg + (size_t)p * rows;
        for (int e = lane; e < rows * cols; e += TEAM) W[(e / cols) * ld + e % cols] = a[e];
        for (int i = lane; i < rows; i += TEAM) W[i * ld + cols] = c[i];
    }
    TG_SYNC();
    bool ok = true;
    const int r = tg::lsq_solve<TEAM>(on, W, rows, cols, ld, rcond, (int *)scr, scr + cols, scr + 2 * cols, scr + 3 * cols, lane, ok);
    if (on) {
        for (int j = lane; j < cols; j += TEAM) zg[(size_t)p * cols + j] = ok ? scr[2 * cols + j] : 0.0;
        if (lane == 0) { rank[p] = ok ? r : 0; status[p] = ok ? TG_OK : TG_SINGULAR; }
    }
}

// The bounded solver alone: problem p as in k_lsq_debug, with its box lo, hi [cols]; the block stays pristine, the solver's scratch
// lies behind it.  z [cols], active [cols], solves, rank and status out (a problem without an answer reports zeros).
template <int TEAM>
__global__ __launch_bounds__(64, 1) void k_bvls_debug(int count, int rows, int cols, int per_team, const double *__restrict__ Ag,
                                                      const double *__restrict__ cg, const double *__restrict__ log, const double *__restrict__ hig,
                                                      double rcond, int max_solves, double *__restrict__ zg, int *__restrict__ active,
                                                      int *__restrict__ solves, int *__restrict__ rank, int *__restrict__ status) {
    double *lds = tg_lds_base();
    const int team = threadIdx.x / TEAM, lane = threadIdx.x % TEAM;
    const long long p = (long long)blockIdx.x * (blockDim.x / TEAM) + team;
    const bool on = p < count;
    const int ld = cols + 1;
    double *W = lds + (size_t)team * per_team, *scr = W + (size_t)rows * ld;
    const tg::BvlsScratch X = tg::bvls_scratch(scr, rows, cols);
    if (on) {
        const double *a = Ag + (size_t)p * rows * cols, *c = cg + (size_t)p * rows;
        for (int e = lane; e < rows * cols; e += TEAM) W[(e / cols) * ld + e % cols] = a[e];
        for (int i = lane; i < rows; i += TEAM) W[i * ld + cols] = c[i];
        for (int j = lane; j < cols; j += TEAM) { X.lo[j] = log[(size_t)p * cols + j]; X.hi[j] = hig[(size_t)p * cols + j]; }
    }
    TG_SYNC();
    int n_solves = 0, st = TG_OK;
    bool finite = true;
    const int r = tg::bvls_solve<TEAM, true>(on, W, rows, cols, ld, rcond, max_solves, scr, lane, n_solves, st, finite);
    if (on) {
        const bool answer = st != TG_SINGULAR;
        for (int j = lane; j < cols; j += TEAM) { zg[(size_t)p * cols + j] = answer ? X.z[j] : 0.0; active[(size_t)p * cols + j] = answer ? X.bnd[j] : 0; }
        if (lane == 0) { solves[p] = n_solves; rank[p] = finite ? r : 0; status[p] = st; }
    }
}

}  // namespace

namespace tg_detail {
int launch_dyn_inverse(int team, bool springs, bool par, int solve, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::DynInverseArgs &J, const tg::ParTable &T, int grid, size_t lds, hipStream_t stream) {
#if defined(TG_PROFILE)   // the diagnostic build instruments the default kernels only
    (void)team; (void)springs; (void)par; (void)solve; (void)d_prog; (void)A; (void)J; (void)T; (void)grid; (void)lds; (void)stream;
    return fail(TG_ERR_UNSUPPORTED, "the profiling build has no computed-torque kernel");
#else
    return dispatch_team(team, [&](auto team_tag) {
        constexpr int TEAM = decltype(team_tag)::value;
        auto pick = [&](auto solve_tag) {      // 1: tg_batch_dynamics_inverse_lsq, 2: tg_batch_dynamics_inverse_bounded
            constexpr int SOLVE = decltype(solve_tag)::value;
            return par ? (springs ? &k_dyn_inverse<TEAM, true, true, SOLVE> : &k_dyn_inverse<TEAM, false, true, SOLVE>)
                       : (springs ? &k_dyn_inverse<TEAM, true, false, SOLVE> : &k_dyn_inverse<TEAM, false, false, SOLVE>);
        };
        return launch_kernel(solve == 2 ? pick(tg::IntTag<2>()) : (solve == 1 ? pick(tg::IntTag<1>()) : pick(tg::IntTag<0>())), grid, lds, stream, d_prog, A, J, T);
    });
#endif
}

// the solver alone: `count` problems of one shape, one team of `team` lanes each, per_block teams to a workgroup
int launch_lsq_debug(int team, int per_block, int count, int rows, int cols, int per_team, const double *A, const double *c, double rcond, double *z,
                     int *rank, int *status, size_t lds, hipStream_t stream) {
    return dispatch_team(team, [&](auto team_tag) {
        constexpr int TEAM = decltype(team_tag)::value;
        auto kernel = &k_lsq_debug<TEAM>;
        if (lds > 64 * 1024) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return fail(TG_ERR_HIP, std::string("hipFuncSetAttribute failed: ") + hipGetErrorString(e));
        }
        hipLaunchKernelGGL(kernel, dim3((count + per_block - 1) / per_block), dim3(per_block * TEAM), lds, stream, count, rows, cols, per_team, A, c,
                           rcond, z, rank, status);
        return (int)TG_SUCCESS;
    });
}

// the bounded solver alone, as launch_lsq_debug
int launch_bvls_debug(int team, int per_block, int count, int rows, int cols, int per_team, const double *A, const double *c, const double *lo,
                      const double *hi, double rcond, int max_solves, double *z, int *active, int *solves, int *rank, int *status, size_t lds,
                      hipStream_t stream) {
    return dispatch_team(team, [&](auto team_tag) {
        constexpr int TEAM = decltype(team_tag)::value;
        auto kernel = &k_bvls_debug<TEAM>;
        if (lds > 64 * 1024) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return fail(TG_ERR_HIP, std::string("hipFuncSetAttribute failed: ") + hipGetErrorString(e));
        }
        hipLaunchKernelGGL(kernel, dim3((count + per_block - 1) / per_block), dim3(per_block * TEAM), lds, stream, count, rows, cols, per_team, A, c,
                           lo, hi, rcond, max_solves, z, active, solves, rank, status);
        return (int)TG_SUCCESS;
    });
}
}  // namespace tg_detail
