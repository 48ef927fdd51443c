// trepamd_tape.hip -- k_tape: the tape-measure kernel (mvi_tape.hpp, MODE_TAPE; tg_batch_tape_measures).
//
// Launch geometry of the generic kernels (trepamd.hip): one 64-thread workgroup holds 64 / TEAM teams; here a team is one state of
// one trajectory, team index b * n_states + m, and its LDS slice is the rollout slice plus one pass of staged segments
// (TapeArgs::lds_per_team).  One kernel per team size: lengths depend on nothing a SPRINGS or parameter twin would change.
// A translation unit of its own so that it compiles beside trepamd.hip.
#include <hip/hip_runtime.h>

#include "launch_generic.hpp"
#include "mvi_tape.hpp"

namespace {

template <int TEAM>
__global__ __launch_bounds__(64, 2) void k_tape(const tg::DevProg *__restrict__ Pg, const tg::RunArgs A, const tg::TapeArgs J) {
    double *lds = tg_lds_base();
    tg::CProg &P = *(tg::CProg *)Pg;
    const int team = threadIdx.x / TEAM, lane = threadIdx.x % TEAM;
    const long long index = (long long)blockIdx.x * (64 / TEAM) + team;
    tg::run_tape<TEAM>(P, A, J, lds + (size_t)team * J.lds_per_team, lane, index);
}

}  // namespace

namespace tg_detail {
int launch_tape(int team, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::TapeArgs &J, int grid, size_t lds, hipStream_t stream) {
#if defined(TG_PROFILE)   // the diagnostic build instruments the default kernels only
    (void)team; (void)d_prog; (void)A; (void)J; (void)grid; (void)lds; (void)stream;
    return fail(TG_ERR_UNSUPPORTED, "the profiling build has no tape-measure kernel");
#else
    return dispatch_team(team, [&](auto team_tag) {
        constexpr int TEAM = decltype(team_tag)::value;
        return launch_kernel(&k_tape<TEAM>, grid, lds, stream, d_prog, A, J);
    });
#endif
}
}  // namespace tg_detail
