// trepamd.hip -- libtrepamd.so: gfx950 kernels + the C ABI of include/trep_amd.h.
//
// Launch geometry: one 64-thread workgroup (exactly one CDNA4 wavefront) holds 64/TEAM teams, one
// trajectory per team; the grid is ceil(batch / teams-per-block) workgroups, i.e. >> 256 CUs for
// the benchmark batches.  Single-wave workgroups make every __syncthreads() a wave-local
// s_waitcnt (no cross-wave barrier) and let the LDS slice of a trajectory be private to its wave.
// Trajectories are independent, so there is no inter-workgroup communication at all.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device_buffer.hpp"
#include "launch_generic.hpp"
#include "mvi_project.hpp"
#include "mvi_equilibrium.hpp"
#include "mvi_modes.hpp"
#include "mvi_response.hpp"
#include "mvi_inverse.hpp"
#include "mvi_frames.hpp"
#include "mvi_tape.hpp"
#include "mvi_dyn_inverse.hpp"
#include "schedule.hpp"
#include <dlfcn.h>

namespace tg_detail {
// the generic per-trajectory-parameter kernels (trepamd_par.hip: their own object, compiled beside this one)
int launch_par(int team, bool springs, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::ParTable &T, int grid, size_t lds, hipStream_t stream);
// the constraint-projection kernel (trepamd_project.hip, likewise)
int launch_project(int team, bool springs, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::ProjectArgs &J, int grid, size_t lds, hipStream_t stream);
// the equilibrium-search kernel and its parameter-table twin (trepamd_equilibrium.hip, likewise)
int launch_equilibrium(int team, bool springs, bool par, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::EquilibriumArgs &J, const tg::ParTable &T, int grid, size_t lds, hipStream_t stream);
// the normal-modes kernel and its parameter-table twin (trepamd_modes.hip, likewise)
int launch_modes(int team, bool springs, bool par, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::ModesArgs &J, const tg::ParTable &T, int grid, size_t lds, hipStream_t stream);
// the static-response kernel and its parameter-table twin (trepamd_response.hip, likewise)
int launch_response(int team, bool springs, bool par, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::ResponseArgs &J, const tg::ParTable &T, int grid, size_t lds, hipStream_t stream);
// the inverse-dynamics kernel and its parameter-table twin (trepamd_inverse.hip, likewise)
int launch_inverse(int team, bool springs, bool par, int solve, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::InverseArgs &J, const tg::ParTable &T, int grid, size_t lds, hipStream_t stream);
// the frame-kinematics kernel (trepamd_frames.hip, likewise)
int launch_frames(int team, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::FrameArgs &J, int grid, size_t lds, hipStream_t stream);
// the tape-measure kernel (trepamd_tape.hip, likewise)
int launch_tape(int team, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::TapeArgs &J, int grid, size_t lds, hipStream_t stream);
// the computed-torque kernel and its parameter-table twin (trepamd_dyn_inverse.hip, likewise)
int launch_dyn_inverse(int team, bool springs, bool par, int solve, const tg::DevProg *d_prog, const tg::RunArgs &A, const tg::DynInverseArgs &J, const tg::ParTable &T, int grid, size_t lds, hipStream_t stream);
int launch_bvls_debug(int team, int per_block, int count, int rows, int cols, int per_team, const double *A, const double *c, const double *lo,
                      const double *hi, double rcond, int max_solves, double *z, int *active, int *solves, int *rank, int *status, size_t lds,
                      hipStream_t stream);
int launch_lsq_debug(int team, int per_block, int count, int rows, int cols, int per_team, const double *A, const double *c, double rcond, double *z,
                     int *rank, int *status, size_t lds, hipStream_t stream);
}

namespace {

thread_local std::string g_error;

int fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(TG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// The derivative modes keep 60-80 KB of LDS per trajectory, i.e. at most two wavefronts per CU: they may use the whole
// register file of a SIMD (no spills, deeper unrolling); the rollout modes run two wavefronts per SIMD.
template <int TEAM, int MODE, bool SPRINGS>
__global__ __launch_bounds__(64, (MODE == tg::MODE_DERIV1 || MODE == tg::MODE_DERIV2Z || MODE == tg::MODE_DYN_DERIV1) ? 1 : 2) void k_run(const tg::DevProg *__restrict__ Pg, const tg::RunArgs A) {
    double *lds = tg_lds_base();
    // The schedule sits in device memory and is read through a CONSTANT-address-space reference (mvi_core.hpp, CProg):
    // every field access is a scalar load that a phase issues when it needs it, instead of ~150 kernel-argument values
    // that the compiler would hoist, keep alive for the whole rollout and spill into VGPR lanes.
    tg::CProg &P = *(tg::CProg *)Pg;
    const int team = threadIdx.x / TEAM, lane = threadIdx.x % TEAM;
    const int block = MODE == tg::MODE_ROLLOUT ? tg_xcd_block((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
    const int traj = tg::tg_remap_trajectory(A, block * (64 / TEAM) + team);
    const int stride = MODE == tg::MODE_DERIV2Z ? P.e_lds_per_team : (MODE == tg::MODE_DERIV1 ? P.a_lds_per_team : (MODE == tg::MODE_DYN_DERIV1 ? P.g_lds_per_team : P.lds_per_team));
    tg::run_trajectory<TEAM, MODE, SPRINGS>(P, A, lds + (size_t)team * stride, lane, traj);
}

// Forward-mode kernels of the continuous dynamics (mvi_core.hpp, run_forward; dual.hpp): one wavefront per trajectory, the trajectory's
// LDS slice in units of Real.  Not a hot path (the reference's calc_dynamics_deriv2 is O(nq^4) per state): full-wave teams only.
template <int MODE, bool SPRINGS, class Real>
__global__ __launch_bounds__(64, 1) void k_forward(const tg::DevProg *__restrict__ Pg, const tg::RunArgs A) {
    Real *lds = (Real *)tg_lds_base();
    tg::CProg &P = *(tg::CProg *)Pg;
    tg::run_forward<64, MODE, SPRINGS>(P, A, lds, (int)threadIdx.x, (int)blockIdx.x);
}

}  // namespace

struct tg_system {
    tg::HostProgram H;
    int team = 64;
    bool has_gravity = false, has_damping = false;   // the system has a Gravity potential / a Damping force (parameter blocks it accepts)
};

struct tg_batch {
    tg_system *sys = nullptr;
    int batch = 0, device = 0;
    tg::DevProg P{};           // device-pointer view
    tg::DeviceBuffer<tg::DevProg> d_prog;   // the same view in device memory: what the kernels read (constant address space)
    // optional system-specialised rollout kernel (tg_batch_load_specialized): launcher exported by a generated library
    void *spec_lib = nullptr;
    int (*spec_launch)(int, const tg::RunArgs *, tg::RunArgs *, int, size_t, void *) = nullptr;
    // ... and its per-trajectory-parameter kernels (tg_spec_launch_par; null for a library without them)
    int (*spec_launch_par)(int, const tg::RunArgs *, tg::RunArgs *, int, size_t, void *, const double *, int, int) = nullptr;
    int spec_par_modes = 0;
    // per-trajectory parameter table (tg_batch_set_parameters): par_rows rows of par_stride doubles (tg::ParTable layout) on the device;
    // par_rows == 0: none set, the default kernels run
    tg::DeviceBuffer<double> par_dev;
    int par_rows = 0, par_group = 1, par_stride = 0;
    // launches so far, [parameter kernel?][specialised?]: bit m of modes = a mode-m launch went through a kernel of that kind
    // (tg_batch_info reports the default kernels, tg_batch_par_info the parameter kernels)
    struct Launched { unsigned int modes = 0; long long n = 0; void add(int mode) { modes |= 1u << mode; n++; } } launched[2][2];
    // argument blocks of the specialised kernels: ARG_SLOTS device-side blocks fed from a pinned host ring (a truly asynchronous
    // hipMemcpyAsync; a slot is reused only after the launch that read it has finished: arg_done[i])
    static constexpr int ARG_SLOTS = 4;
    tg::DeviceBuffer<tg::RunArgs> d_args;   // [ARG_SLOTS] device
    tg::PinnedBuffer<tg::RunArgs> h_args;   // [ARG_SLOTS] pinned host
    tg::Event arg_done[ARG_SLOTS];
    bool arg_used[ARG_SLOTS] = {false, false, false, false};
    int arg_next = 0;
    // small batches (the B = 1 drop-in path): tg_batch_step stages its inputs through ONE pinned block, and a pack kernel + ONE
    // copy bring (q2, p2, lambda1, iterations, status) back into a pinned host mirror that later tg_batch_get / tg_batch_status
    // calls answer from, until anything else touches the batch (launch(), tg_batch_set, restore ...)
    tg::PinnedBuffer<double> io_host;
    double *io_dev = nullptr;          // the same block as the device sees it
    size_t io_in = 0, io_out = 0;      // doubles in the input / output part
    bool mirror_valid = false;
    int spec_modes = 0, spec_waves = 1, spec_fb_n = 0, spec_tr_n = 0, spec_pose_carry = 0;
    std::string spec_path;
    tg::DeviceBuffer<int> d_ints;
    tg::DeviceBuffer<double> d_dbls;
    tg::DeviceBuffer<double> q1, q2, p1, p2, lam, u1;
    tg::DeviceBuffer<double> stage_u, stage_k, stage_qh, stage_lh, f_out;
    tg::DeviceBuffer<int> iters, status, fallbacks;
    tg::DeviceBuffer<double> z_dev, hz_dev, zl_dev;
    tg::DeviceBuffer<double> dyn;     // staging of the host-facing continuous-dynamics call: q, dq, u, ddq_k, ddq, lambda
    tg::DeviceBuffer<double> dyn_d1;  // ... and of its eight first-derivative arrays
    tg::DeviceBuffer<double> energy;  // [batch][2] output of tg_batch_energy
    tg::DeviceBuffer<double> lag;     // outputs of tg_batch_lagrangian
    tg::DeviceBuffer<int> dyn_ints;   // its status / iteration words (the integrator's own stay untouched)
    tg::DeviceBuffer<double> pose;    // staging of the host-facing pose solvers (stream-ordered, one call at a time): q0 in, q, mu out, and
                                      // the projection's dq0 in, dq out or the equilibrium search's V out
    tg::DeviceBuffer<int> pose_ints;  // their free mask [nq], iteration [batch] and status [batch] words
    tg::DeviceBuffer<double> modes_stage;   // staging of the host-facing normal-modes call: q, mu in; omega2, modes, mu, residual out
    tg::DeviceBuffer<int> modes_ints;       // its free mask [nq] (both entry points), then count, rank, sweeps, status [batch] each
    std::vector<int32_t> modes_mask;        // the mask as the host built it (kinematic configs cleared)
    tg::DeviceBuffer<double> response_stage;   // staging of the host-facing static-response call: q, mu in; dq, dmu, C, R, mu, residual, defect out
    tg::DeviceBuffer<int> response_ints;       // its free mask [nq] and drive list [n_drive] (both entry points), then rank, status [batch] each
    std::vector<int32_t> response_mask;        // mask [nq] and drive list as the host checked them
    // frame table of tg_batch_frame_kinematics (mvi_frames.hpp, FrameArgs::tab / ::off) for the selection frames_sel: rebuilt only
    // when a call's selection differs from it, reallocated only when it grows
    std::vector<int32_t> frames_sel;
    std::vector<int> frames_tab_host;
    std::vector<double> frames_off_host;
    tg::DeviceBuffer<int> frames_tab;
    tg::DeviceBuffer<double> frames_off;
    // table of tg_batch_tape_measures (mvi_tape.hpp, tape_table) for the selection (tape_start, tape_sel), cached likewise
    std::vector<int32_t> tape_start, tape_sel;
    tg::TapeTable tape_host;
    tg::DeviceBuffer<int> tape_words;
    tg::DeviceBuffer<double> tape_off;
    tg::DeviceBuffer<int> seeds;      // [2][batch] direction variables of the forward-mode calls
    tg::DeviceBuffer<double> d1[12];
    bool have_d1 = false;
    tg::DeviceBuffer<long long> prof; // diagnostic build only (TG_PROFILE)
    tg::DeviceBuffer<double> snap;    // snapshot of (q1,q2,p1,p2,lam,u1)
    double snap_t1 = 0.0, snap_t2 = 0.0;
    long long total_iters = 0;
    double t1 = 0.0, t2 = 0.0, tolerance = 1.0e-10;
    int predictor = 0;
    tg::DeviceBuffer<double> dt_dev;  // optional non-uniform time base (tg_batch_set_step_sizes)
    std::vector<double> dt_host;
    int dt_by_trajectory = 0;
    int exact_pivot = 0;       // 1: Newton systems solved with the reference's exact pivot rule (gj_rows_exact)
    hipStream_t stream = nullptr;
    bool own_stream = true;
    static constexpr size_t TIMING_CAP = 4096;
    bool timing = false;       // HIP-event timing of the launches: off until tg_batch_timing is called once
    double folded_ms = 0.0;    // launches recycled past TIMING_CAP
    long long folded_n = 0;
    std::vector<std::pair<tg::Event, tg::Event>> events;
    std::vector<tg::Event> pool;
};

namespace {

int widths(const tg_batch *b, int field) {
    const tg::DevProg &P = b->P;
    switch (field) {
    case TG_F_Q1: case TG_F_Q2: return P.nq;
    case TG_F_P1: case TG_F_P2: return P.nd;
    case TG_F_U1: return P.nu;
    case TG_F_LAMBDA1: return P.nc;
    default: break;
    }
    if (field >= TG_F_Q2_DQ1 && field <= TG_F_L1_DK2) {
        const int k = field - TG_F_Q2_DQ1, var = k % 4, out = k / 4;
        const int rows = var == 0 ? P.nq : (var == 1 ? P.nd : (var == 2 ? P.nu : P.nk));
        return rows * (out == 2 ? P.nc : P.nd);
    }
    return -1;
}
double *field_ptr(tg_batch *b, int field) {
    switch (field) {
    case TG_F_Q1: return b->q1.get();
    case TG_F_Q2: return b->q2.get();
    case TG_F_P1: return b->p1.get();
    case TG_F_P2: return b->p2.get();
    case TG_F_U1: return b->u1.get();
    case TG_F_LAMBDA1: return b->lam.get();
    default: break;
    }
    if (field >= TG_F_Q2_DQ1 && field <= TG_F_L1_DK2) return b->d1[field - TG_F_Q2_DQ1].get();
    return nullptr;
}

int pick_team(const tg::HostProgram &H) {
    if (const char *env = std::getenv("TREPAMD_TEAM")) {
        int t = std::atoi(env);
        if (t == 1 || t == 4 || t == 16 || t == 64) return t;
    }
    const tg::DevProg &P = H.p;
    int width = std::max(P.n_items, (P.nf * (P.nf + 1)) / 4);
    int team = width > 32 ? 64 : (width > 8 ? 16 : (width > 2 ? 4 : 1));
    // the block's LDS (all teams) must fit the 64 KiB a workgroup may use without opting in
    while (team < 64 && (size_t)(64 / team) * P.lds_per_team * sizeof(double) > 64 * 1024) team *= 4;
    return team;
}

template <typename T>
void append(std::vector<T> &pool, const std::vector<T> &v, size_t &off) {
    off = pool.size();
    pool.insert(pool.end(), v.begin(), v.end());
    while (pool.size() % 2) pool.push_back(T());
}

bool launch_springs(const tg::DevProg &P) { return P.has_cs || P.n_springs || P.has_plane || P.n_wrenches; }
bool launch_springs(const tg_batch *b) { return launch_springs(b->P); }
// doubles of LDS that one team of a mode-`mode` kernel keeps (the slice k_run strides its teams by)
int lds_per_team(const tg::DevProg &P, int mode) {
    return mode == tg::MODE_DERIV2Z ? P.e_lds_per_team : (mode == tg::MODE_DERIV1 ? P.a_lds_per_team : (mode == tg::MODE_DYN_DERIV1 ? P.g_lds_per_team : P.lds_per_team));
}

// systems with spring potentials run their own instantiation of every kernel (mvi_core.hpp, Core<TEAM, SPRINGS>)
template <int TEAM, int MODE>
int launch_one(tg_batch *b, const tg::RunArgs &A, int grid, size_t lds) {
#if defined(TG_PROFILE)   // the diagnostic build only instruments the plain kernels of full-wave teams (fewer instantiations)
    if (TEAM != 64 || launch_springs(b))
        return fail(TG_ERR_UNSUPPORTED, "the profiling build covers full-wave teams without spring / plane / wrench features");
    return tg_detail::launch_kernel(&k_run<64, MODE, false>, grid, lds, b->stream, b->d_prog.get(), A);
#else
    return tg_detail::launch_kernel(launch_springs(b) ? &k_run<TEAM, MODE, true> : &k_run<TEAM, MODE, false>, grid, lds, b->stream, b->d_prog.get(), A);
#endif
}

template <int TEAM>
int launch_team(tg_batch *b, const tg::RunArgs &A, int grid, size_t lds) {
    switch (A.mode) {
    case tg::MODE_ROLLOUT: return launch_one<TEAM, tg::MODE_ROLLOUT>(b, A, grid, lds);
    case tg::MODE_CALC_P2: return launch_one<TEAM, tg::MODE_CALC_P2>(b, A, grid, lds);
    case tg::MODE_CALC_F: return launch_one<TEAM, tg::MODE_CALC_F>(b, A, grid, lds);
    case tg::MODE_DERIV1: return launch_one<TEAM, tg::MODE_DERIV1>(b, A, grid, lds);
    case tg::MODE_DERIV2Z: return launch_one<TEAM, tg::MODE_DERIV2Z>(b, A, grid, lds);
#if !defined(TG_PROFILE)   // the continuous-dynamics modes are not instrumented (and not instantiated) in the diagnostic build
    case tg::MODE_DYNAMICS: return launch_one<TEAM, tg::MODE_DYNAMICS>(b, A, grid, lds);
    case tg::MODE_DYN_DERIV1: return launch_one<TEAM, tg::MODE_DYN_DERIV1>(b, A, grid, lds);
    case tg::MODE_ENERGY: return launch_one<TEAM, tg::MODE_ENERGY>(b, A, grid, lds);
    case tg::MODE_LAGRANGIAN: return launch_one<TEAM, tg::MODE_LAGRANGIAN>(b, A, grid, lds);
#endif
    default: return fail(TG_ERR_INVALID, "unknown kernel mode");
    }
}

// HIP-event timing is opt-in (the first tg_batch_timing call switches it on): a plain MidpointVI.step() loop creates
// no events.  When on, at most TIMING_CAP launches are kept; older pairs are recycled (their time is folded into
// the running totals), and every error path hands the pair back to the pool.  timing_begin before a launch, timing_end(rc) behind it.
struct LaunchTiming { tg::Event e0, e1; };
int timing_begin(tg_batch *b, LaunchTiming &t) {
    if (!b->timing) return TG_SUCCESS;
    tg::Event &e0 = t.e0, &e1 = t.e1;
    auto recycle = [&] { b->pool.push_back(std::move(e0)); b->pool.push_back(std::move(e1)); };
    if (b->events.size() >= tg_batch::TIMING_CAP) {
        float ms = 0.f;
        e0 = std::move(b->events.front().first); e1 = std::move(b->events.front().second);
        if (hipEventSynchronize(e1.get()) == hipSuccess && hipEventElapsedTime(&ms, e0.get(), e1.get()) == hipSuccess) { b->folded_ms += ms; b->folded_n++; }
        b->events.erase(b->events.begin());
    } else if (b->pool.size() >= 2) { e0 = std::move(b->pool.back()); b->pool.pop_back(); e1 = std::move(b->pool.back()); b->pool.pop_back(); }
    else {
        HIP_TRY(e0.create());
        if (e1.create() != hipSuccess) { b->pool.push_back(std::move(e0)); return fail(TG_ERR_HIP, "hipEventCreate failed"); }
    }
    if (hipEventRecord(e0.get(), b->stream) != hipSuccess) { recycle(); return fail(TG_ERR_HIP, "hipEventRecord failed"); }
    return TG_SUCCESS;
}
int timing_end(tg_batch *b, LaunchTiming &t, int rc) {
    if (!b->timing) return rc;
    if (rc != TG_SUCCESS || hipEventRecord(t.e1.get(), b->stream) != hipSuccess) {
        b->pool.push_back(std::move(t.e0)); b->pool.push_back(std::move(t.e1));
        return rc != TG_SUCCESS ? rc : fail(TG_ERR_HIP, "hipEventRecord failed");
    }
    b->events.emplace_back(std::move(t.e0), std::move(t.e1));
    return rc;
}

int launch(tg_batch *b, tg::RunArgs &A) {
    b->mirror_valid = false;
    const int team = b->sys->team, per_block = 64 / team;
    const int grid = ((A.remap_len > 0 ? A.remap_count : A.batch) + per_block - 1) / per_block;
    const size_t lds = (size_t)per_block * lds_per_team(b->P, A.mode) * sizeof(double);
    if (lds > 160 * 1024) return fail(TG_ERR_UNSUPPORTED, "system too large for the LDS-resident kernel");
    LaunchTiming timed;
    if (int trc = timing_begin(b, timed)) return trc;
    int rc;
    // a parameter table selects the PAR kernels: the library's specialised one of the mode if it has it, else the generic one
    const bool par = b->par_rows > 0;
    if (par ? (b->spec_launch_par && ((b->spec_par_modes >> A.mode) & 1)) : (b->spec_launch && ((b->spec_modes >> A.mode) & 1))) {
        const int i = b->arg_next;
        b->arg_next = (i + 1) % tg_batch::ARG_SLOTS;
        rc = TG_SUCCESS;
        if (b->arg_used[i] && hipEventSynchronize(b->arg_done[i].get()) != hipSuccess) rc = fail(TG_ERR_HIP, "hipEventSynchronize failed");
        if (rc == TG_SUCCESS) {
            tg::RunArgs *h = b->h_args.get() + i, *d = b->d_args.get() + i;
            *h = A;
            const int lrc = par ? b->spec_launch_par(A.mode, h, d, grid, lds, (void *)b->stream, b->par_dev.get(), b->par_group, b->par_stride)
                                : b->spec_launch(A.mode, h, d, grid, lds, (void *)b->stream);
            rc = lrc == 0 ? TG_SUCCESS : fail(TG_ERR_HIP, "specialised kernel launch failed");
            b->arg_used[i] = hipEventRecord(b->arg_done[i].get(), b->stream) == hipSuccess;
            if (!b->arg_used[i]) hipStreamSynchronize(b->stream);
            b->launched[par][1].add(A.mode);
        }
    } else {
        b->launched[par][0].add(A.mode);
        rc = par ? tg_detail::launch_par(team, launch_springs(b), b->d_prog.get(), A, tg::ParTable{b->par_dev.get(), b->par_group, b->par_stride}, grid, lds, b->stream)
                 : tg_detail::dispatch_team(team, [&](auto team_tag) { return launch_team<decltype(team_tag)::value>(b, A, grid, lds); });
    }
    if (rc == TG_SUCCESS && hipGetLastError() != hipSuccess) rc = fail(TG_ERR_HIP, "kernel launch failed");
    return timing_end(b, timed, rc);
}

#if !defined(TG_PROFILE)
template <int MODE, class Real>
int launch_forward_mode(tg_batch *b, const tg::RunArgs &A) {
    const size_t lds = (size_t)std::max(b->P.lds_per_team, lds_per_team(b->P, MODE)) * sizeof(Real);
    if (lds > 160 * 1024) return fail(TG_ERR_UNSUPPORTED, "system too large for the LDS-resident forward-mode kernel");
    b->launched[0][0].add(MODE);      // no forward-mode kernel is ever specialised (tg_batch_info)
    int rc = tg_detail::launch_kernel(launch_springs(b) ? &k_forward<MODE, true, Real> : &k_forward<MODE, false, Real>, A.batch, lds, b->stream, b->d_prog.get(), A);
    if (rc == TG_SUCCESS && hipGetLastError() != hipSuccess) rc = fail(TG_ERR_HIP, "kernel launch failed");
    return rc;
}
#endif
// A continuous-dynamics mode on dual numbers: A.seed1 (and A.seed2 for order 2) name the direction variable(s) of every trajectory.
int launch_forward(tg_batch *b, const tg::RunArgs &A, int order) {
#if defined(TG_PROFILE)
    (void)b; (void)A; (void)order;
    return fail(TG_ERR_UNSUPPORTED, "the profiling build has no forward-mode kernels");
#else
    typedef tgdual::Dual<double> D1;
    typedef tgdual::Dual<D1> D2;
    if (b->par_rows) return fail(TG_ERR_UNSUPPORTED, "forward-mode kernels take the system's own parameters: clear the parameter table first");
    b->mirror_valid = false;
    if (A.mode == tg::MODE_DYN_DERIV1 && order == 1) return launch_forward_mode<tg::MODE_DYN_DERIV1, D1>(b, A);
    if (A.mode == tg::MODE_LAGRANGIAN && order == 1) return launch_forward_mode<tg::MODE_LAGRANGIAN, D1>(b, A);
    if (A.mode == tg::MODE_LAGRANGIAN && order == 2) return launch_forward_mode<tg::MODE_LAGRANGIAN, D2>(b, A);
    return fail(TG_ERR_INVALID, "forward mode: first derivatives of the dynamics (order 1) or the Lagrangian (order 1, 2)");
#endif
}
// the direction variables of a forward-mode call, checked and copied to the device; null seed2: first order
int stage_seeds(tg_batch *b, const int32_t *seed1_host, const int32_t *seed2_host) {
    const size_t B = (size_t)b->batch;
    const int nvar = 2 * b->P.nq + b->P.nk + b->P.nu;
    for (size_t i = 0; i < B; i++) {
        if (seed1_host[i] < -1 || seed1_host[i] >= nvar) return fail(TG_ERR_INVALID, "direction variable out of range (q | dq | ddq_k | u)");
        if (seed2_host && (seed2_host[i] < -1 || seed2_host[i] >= nvar)) return fail(TG_ERR_INVALID, "direction variable out of range (q | dq | ddq_k | u)");
    }
    HIP_TRY(b->seeds.ensure(2 * B));
    HIP_TRY(hipMemcpyAsync(b->seeds.get(), seed1_host, B * sizeof(int), hipMemcpyHostToDevice, b->stream));
    if (seed2_host) HIP_TRY(hipMemcpyAsync(b->seeds.get() + B, seed2_host, B * sizeof(int), hipMemcpyHostToDevice, b->stream));
    return TG_SUCCESS;
}

// Host-facing derivative outputs: the twelve first-derivative arrays and the contraction buffers.  Allocated on
// first use so that batches that only roll out, or that write A/B and HZ into caller-provided device buffers,
// do not reserve 80+ kB per trajectory.
int ensure_deriv_buffers(tg_batch *b, bool first, bool second) {
    const tg::DevProg &P = b->P;
    const size_t B = (size_t)b->batch;
    bool ok = true;
    if (first) for (int k = 0; k < 12 && ok; k++) ok = b->d1[k].ensure(B * widths(b, TG_F_Q2_DQ1 + k), true) == hipSuccess;
    if (second && ok) ok = b->z_dev.ensure(B * P.nX, true) == hipSuccess && b->zl_dev.ensure(B * P.nc, true) == hipSuccess &&
                           b->hz_dev.ensure(B * (size_t)P.d_nrhs * P.d_nrhs, true) == hipSuccess;
    return ok ? TG_SUCCESS : fail(TG_ERR_HIP, "device allocation failed");
}

tg::RunArgs base_args(tg_batch *b, int mode) {
    tg::RunArgs A{};
    A.batch = b->batch; A.mode = mode; A.max_iterations = 200;
    A.t1 = b->t1; A.t2 = b->t2; A.tolerance = b->tolerance; A.predictor = b->predictor; A.exact_pivot = b->exact_pivot;
    A.dt_steps = b->dt_host.empty() ? nullptr : b->dt_dev.get();
    A.dt_period = (b->dt_by_trajectory && !b->dt_host.empty()) ? (int)b->dt_host.size() : 0;
    A.q1 = b->q1.get(); A.q2 = b->q2.get(); A.p1 = b->p1.get(); A.p2 = b->p2.get(); A.lam = b->lam.get(); A.u1 = b->u1.get();
    A.iters = b->iters.get(); A.status = b->status.get(); A.f_out = b->f_out.get(); A.fallbacks = b->fallbacks.get();
    A.prof_out = b->prof.get();
    for (int i = 0; i < 12; i++) A.d1[i] = b->d1[i].get();
    A.z = b->z_dev.get(); A.hz = b->hz_dev.get();
    A.group_size = 1;
    return A;
}

// the one-step rollout of tg_batch_step / tg_batch_set_from_trajectories: inputs and hints (null: none) in the given device buffers
tg::RunArgs step_args(tg_batch *b, double dt, int max_iterations, const double *U, const double *K, const double *q2_hint, const double *lam_hint) {
    tg::RunArgs A = base_args(b, tg::MODE_ROLLOUT);
    A.n_steps = 1; A.dt = dt; A.max_iterations = max_iterations;
    if (!A.dt_period) A.dt_steps = nullptr;      // a by-step list belongs to the rollouts: one step takes the caller's size
    A.U = U; A.K = K; A.q2_hint = q2_hint; A.lam_hint = lam_hint;
    return A;
}

// Staging block of the host-facing continuous-dynamics calls, b->dyn: (q, dq, u, ddq_k) in, (ddq, lambda) out, [batch][width] each.
// Allocated on first use with the calls' status / iteration words; uploads the inputs the call has (null: none).
struct DynStage { double *q, *dq, *u, *ddk, *ddq, *lam; };
int stage_dynamics(tg_batch *b, const double *q_host, const double *dq_host, const double *u_host, const double *ddqk_host, DynStage &s) {
    const tg::DevProg &P = b->P;
    const size_t B = (size_t)b->batch, nq = P.nq, nd = P.nd, nk = P.nk, nu = P.nu, nc = P.nc;
    HIP_TRY(b->dyn.ensure(B * (2 * nq + nu + nk + nd + nc)));
    HIP_TRY(b->dyn_ints.ensure(2 * B));
    s.q = b->dyn.get(); s.dq = s.q + B * nq; s.u = s.dq + B * nq; s.ddk = s.u + B * nu; s.ddq = s.ddk + B * nk; s.lam = s.ddq + B * nd;
    HIP_TRY(hipMemcpyAsync(s.q, q_host, B * nq * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(s.dq, dq_host, B * nq * sizeof(double), hipMemcpyHostToDevice, b->stream));
    if (nu && u_host) HIP_TRY(hipMemcpyAsync(s.u, u_host, B * nu * sizeof(double), hipMemcpyHostToDevice, b->stream));
    if (nk && ddqk_host) HIP_TRY(hipMemcpyAsync(s.ddk, ddqk_host, B * nk * sizeof(double), hipMemcpyHostToDevice, b->stream));
    return TG_SUCCESS;
}

// the system's own values in the layout of a parameter row (tg::ParTable): inertia [n_bodies][4] | gravity [3] | damping [nd]
void base_parameter_row(const tg::HostProgram &H, double *row) {
    const int nb = H.p.n_bodies;
    std::copy(H.b_inertia.begin(), H.b_inertia.end(), row);
    for (int k = 0; k < 3; k++) row[4 * nb + k] = H.p.grav[k];
    for (int i = 0; i < H.p.nd; i++) row[4 * nb + 3 + i] = H.damp.empty() ? 0.0 : H.damp[i];
}

// DSystem.set(X[s][k], U[s][k], k, xk_hint = X[s][k+1]) for trajectory t = s*horizon + k (dsystem.py:229-251):
// state (q2,p2) <- X[s][k] (the step kernel shifts it into slot 1), lambda <- 0, inputs and hint staged.
__global__ void k_set_from_trajectories(const tg::DevProg P, int seeds, int horizon, const double *X, const double *U,
                                        double *q1, double *q2, double *p1, double *p2, double *lam, double *su,
                                        double *sk, double *sqh) {
    const size_t t = blockIdx.x;
    const size_t s = t / horizon, k = t % horizon;
    const double *x0 = X + (s * (horizon + 1) + k) * P.nX, *x1 = x0 + P.nX, *u = U + (s * horizon + k) * (size_t)(P.nu + P.nk);
    for (int i = threadIdx.x; i < P.nq; i += blockDim.x) { q1[t * P.nq + i] = x0[i]; q2[t * P.nq + i] = x0[i]; }
    for (int i = threadIdx.x; i < P.nd; i += blockDim.x) {
        p1[t * P.nd + i] = x0[P.nq + i]; p2[t * P.nd + i] = x0[P.nq + i];
        sqh[t * P.nd + i] = x1[i];
    }
    for (int i = threadIdx.x; i < P.nc; i += blockDim.x) lam[t * P.nc + i] = 0.0;
    for (int i = threadIdx.x; i < P.nu; i += blockDim.x) su[t * P.nu + i] = u[i];
    for (int i = threadIdx.x; i < P.nk; i += blockDim.x) sk[t * P.nk + i] = u[P.nu + i];
}

// initialize_from_state(t, Q, p) with (Q, p) taken from the head of a DSystem state vector X = [Q; p; v]
__global__ void k_init_from_X(const tg::DevProg P, const double *X, size_t stride, double *q1, double *q2, double *p1,
                              double *p2, double *lam) {
    const size_t t = blockIdx.x;
    const double *x = X + t * stride;
    for (int i = threadIdx.x; i < P.nq; i += blockDim.x) { q1[t * P.nq + i] = x[i]; q2[t * P.nq + i] = x[i]; }
    for (int i = threadIdx.x; i < P.nd; i += blockDim.x) { p1[t * P.nd + i] = x[P.nq + i]; p2[t * P.nd + i] = x[P.nq + i]; }
    for (int i = threadIdx.x; i < P.nc; i += blockDim.x) lam[t * P.nc + i] = 0.0;
}


// Test hook: the Newton-system solver of the rollout kernels (gj_rows) on a caller-supplied matrix, with its pivot order.
__global__ void k_debug_solve(int n, int ld, int exact, const double *A_in, double *x_out, int *piv_out, int *status_out) {
#if defined(__HIP_DEVICE_COMPILE__)   // gj_rows exists in the device pass only
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    int *trace = (int *)(lds + n * ld);
    for (int e = lane; e < n * (n + 1); e += 64) lds[(e / (n + 1)) * ld + e % (n + 1)] = A_in[e];
    if (lane < 32) trace[lane] = -1;
    __syncthreads();
    bool ok = true;
    if (exact == 1) switch ((n + 3) >> 2) {
    case 1: ok = tg::gj_rows_exact<64, 4, true>(true, lds, n, ld, lane, trace); break;
    case 2: ok = tg::gj_rows_exact<64, 8, true>(true, lds, n, ld, lane, trace); break;
    case 3: ok = tg::gj_rows_exact<64, 12, true>(true, lds, n, ld, lane, trace); break;
    case 4: ok = tg::gj_rows_exact<64, 16, true>(true, lds, n, ld, lane, trace); break;
    case 5: ok = tg::gj_rows_exact<64, 20, true>(true, lds, n, ld, lane, trace); break;
    case 6: ok = tg::gj_rows_exact<64, 24, true>(true, lds, n, ld, lane, trace); break;
    case 7: ok = tg::gj_rows_exact<64, 28, true>(true, lds, n, ld, lane, trace); break;
    default: ok = tg::gj_rows_exact<64, 32, true>(true, lds, n, ld, lane, trace); break;
    }
    else if (exact == 2) {     // the full-wave panel solver (default pivot rule), 16 < n < 32; scratch behind the trace words
        double *scr = lds + n * ld + 16;
        switch ((n + 3) >> 2) {
        case 5: ok = tg::gj_panel<20, true>(true, lds, n, ld, lane, scr, trace); break;
        case 6: ok = tg::gj_panel<24, true>(true, lds, n, ld, lane, scr, trace); break;
        case 7: ok = tg::gj_panel<28, true>(true, lds, n, ld, lane, scr, trace); break;
        default: ok = tg::gj_panel<32, true>(true, lds, n, ld, lane, scr, trace); break;
        }
    }
    else switch ((n + 3) >> 2) {
    case 1: ok = tg::gj_rows<64, 4, true>(true, lds, n, ld, lane, trace); break;
    case 2: ok = tg::gj_rows<64, 8, true>(true, lds, n, ld, lane, trace); break;
    case 3: ok = tg::gj_rows<64, 12, true>(true, lds, n, ld, lane, trace); break;
    case 4: ok = tg::gj_rows<64, 16, true>(true, lds, n, ld, lane, trace); break;
    case 5: ok = tg::gj_rows<64, 20, true>(true, lds, n, ld, lane, trace); break;
    case 6: ok = tg::gj_rows<64, 24, true>(true, lds, n, ld, lane, trace); break;
    case 7: ok = tg::gj_rows<64, 28, true>(true, lds, n, ld, lane, trace); break;
    default: ok = tg::gj_rows<64, 32, true>(true, lds, n, ld, lane, trace); break;
    }
    __syncthreads();
    if (lane < n) { x_out[lane] = lds[lane * ld + n]; piv_out[lane] = trace[lane]; }
    if (lane == 0) *status_out = ok ? TG_OK : TG_SINGULAR;
#endif
}

}  // namespace

namespace tg_detail {
int fail(int code, const std::string &msg) { return ::fail(code, msg); }
}

extern "C" {

const char *tg_version(void) { return "trep_amd 0.1 (gfx950)"; }
const char *tg_last_error(void) { return g_error.c_str(); }

int tg_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

/* out[0..3] = compute units, LDS bytes a workgroup may use (opt-in maximum), wavefront size, 0 */
int tg_device_info(int32_t device, int32_t out[4]) {
    if (!out) return fail(TG_ERR_INVALID, "null argument");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    out[0] = prop.multiProcessorCount; out[1] = (int32_t)prop.sharedMemPerBlockOptin; out[2] = prop.warpSize; out[3] = 0;
    return TG_SUCCESS;
}

tg_system *tg_system_create(const tg_system_desc *desc) {
    if (!desc) { fail(TG_ERR_INVALID, "null descriptor"); return nullptr; }
    try {
        tg_system *s = new tg_system();
        s->H = tg::build_program(desc);
        s->team = pick_team(s->H);
        s->has_gravity = desc->n_gravity > 0; s->has_damping = desc->n_damping > 0;
        return s;
    } catch (const std::exception &e) {
        fail(TG_ERR_INVALID, e.what());
        return nullptr;
    }
}
void tg_system_destroy(tg_system *sys) { delete sys; }

int tg_system_sizes(const tg_system *sys, int32_t out[6]) {
    if (!sys) return fail(TG_ERR_INVALID, "null system");
    const tg::DevProg &P = sys->H.p;
    out[0] = P.nq; out[1] = P.nd; out[2] = P.nk; out[3] = P.nu; out[4] = P.nc; out[5] = P.nX;
    return TG_SUCCESS;
}

/* Introspection used by bench.py / DESIGN.md: team size, LDS bytes per trajectory, schedule sizes. */
int tg_system_info(const tg_system *sys, int32_t out[8]) {
    if (!sys) return fail(TG_ERR_INVALID, "null system");
    const tg::DevProg &P = sys->H.p;
    out[0] = sys->team; out[1] = (int32_t)(P.lds_per_team * sizeof(double)); out[2] = P.n_joints; out[3] = P.n_levels;
    out[4] = P.n_bodies; out[5] = P.n_items; out[6] = P.n_pairs; out[7] = P.n_dh;
    return TG_SUCCESS;
}

tg_batch *tg_batch_create(tg_system *sys, int32_t batch, int32_t device) {
    if (!sys || batch <= 0) { fail(TG_ERR_INVALID, "bad arguments"); return nullptr; }
    int ndev = tg_device_count();
    if (ndev <= 0) { fail(TG_ERR_HIP, "no HIP device visible: libtrepamd has no CPU path"); return nullptr; }
    if (device < 0 || device >= ndev) { fail(TG_ERR_INVALID, "device index out of range"); return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { fail(TG_ERR_HIP, "hipSetDevice failed"); return nullptr; }
    tg_batch *b = new tg_batch();
    b->sys = sys; b->batch = batch; b->device = device;
    const tg::HostProgram &H = sys->H;
    b->P = H.p;
    // all index / constant tables live in two device buffers; bind() points the DevProg into them
    const std::vector<int> &ints = H.ipool;
    const std::vector<double> &dbls = H.dpool;
    bool ok = b->d_ints.ensure(ints.size()) == hipSuccess && b->d_dbls.ensure(dbls.size()) == hipSuccess &&
              hipMemcpy(b->d_ints.get(), ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(b->d_dbls.get(), dbls.data(), dbls.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    tg::DevProg &P = b->P;
    H.bind(P, b->d_ints.get(), b->d_dbls.get());
    if (ok) ok = b->d_prog.ensure(1) == hipSuccess && hipMemcpy(b->d_prog.get(), &P, sizeof(tg::DevProg), hipMemcpyHostToDevice) == hipSuccess;
    auto zeroed = [&](auto &buf, size_t n) { ok = ok && buf.ensure(n, true) == hipSuccess; };
    const size_t B = (size_t)batch;
    zeroed(b->q1, B * P.nq); zeroed(b->q2, B * P.nq); zeroed(b->p1, B * P.nd); zeroed(b->p2, B * P.nd);
    zeroed(b->lam, B * P.nc); zeroed(b->u1, B * P.nu); zeroed(b->f_out, B * P.nf);
    zeroed(b->stage_u, B * P.nu); zeroed(b->stage_k, B * P.nk); zeroed(b->stage_qh, B * P.nd); zeroed(b->stage_lh, B * P.nc);
    // derivative outputs (d1[12], z, hz) are allocated on first use: ensure_deriv_buffers()
    zeroed(b->snap, B * (2 * (size_t)P.nq + 2 * (size_t)P.nd + P.nc + P.nu));
    zeroed(b->iters, B); zeroed(b->status, B); zeroed(b->fallbacks, B);
#if defined(TG_PROFILE)
    zeroed(b->prof, 16);
#endif
    if (ok) ok = hipStreamCreate(&b->stream) == hipSuccess;
    if (!ok) { fail(TG_ERR_HIP, "device allocation failed"); tg_batch_destroy(b); return nullptr; }
    return b;
}

void tg_batch_destroy(tg_batch *b) {
    if (!b) return;
    hipSetDevice(b->device);
    if (b->stream) hipStreamSynchronize(b->stream);
    if (b->stream && b->own_stream) hipStreamDestroy(b->stream);
    if (b->spec_lib) dlclose(b->spec_lib);
    delete b;      // every buffer and event of the batch frees itself
}

int tg_batch_set_tolerance(tg_batch *b, double tolerance) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    b->tolerance = tolerance;
    return TG_SUCCESS;
}
int tg_batch_set_times(tg_batch *b, double t1, double t2) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    b->t1 = t1; b->t2 = t2;
    return TG_SUCCESS;
}
int tg_batch_get_times(const tg_batch *b, double *t1, double *t2) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    *t1 = b->t1; *t2 = b->t2;
    return TG_SUCCESS;
}
int tg_batch_field_width(const tg_batch *b, int32_t field) { return b ? widths(b, field) : -1; }

int tg_batch_set(tg_batch *b, int32_t field, const double *host) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    int w = widths(b, field);
    double *dst = field_ptr(b, field);
    if (w < 0 || !dst) return fail(TG_ERR_INVALID, "unknown or read-only field");
    if (w == 0) return TG_SUCCESS;
    b->mirror_valid = false;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipMemcpyAsync(dst, host, (size_t)b->batch * w * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return TG_SUCCESS;
}
int tg_batch_get(tg_batch *b, int32_t field, double *host) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    int w = widths(b, field);
    double *src = field_ptr(b, field);
    if (w < 0 || !src) return fail(TG_ERR_INVALID, "unknown field");
    if (w == 0) return TG_SUCCESS;
    if (b->mirror_valid && (field == TG_F_Q2 || field == TG_F_P2 || field == TG_F_LAMBDA1)) {   // answered from the last step's mirror
        const tg::DevProg &P = b->P;
        const size_t B = (size_t)b->batch;
        const double *m = b->io_host.get() + b->io_in + (field == TG_F_Q2 ? 0 : (field == TG_F_P2 ? B * P.nq : B * (P.nq + P.nd)));
        std::memcpy(host, m, B * w * sizeof(double));
        return TG_SUCCESS;
    }
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipMemcpyAsync(host, src, (size_t)b->batch * w * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return TG_SUCCESS;
}

int tg_batch_calc_p2(tg_batch *b) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    if (b->t2 == b->t1) return fail(TG_ERR_STATE, "calc_p2 needs t2 != t1");
    HIP_TRY(hipSetDevice(b->device));
    tg::RunArgs A = base_args(b, tg::MODE_CALC_P2);
    if (int rc = launch(b, A)) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    return TG_SUCCESS;
}

int tg_batch_calc_f(tg_batch *b, double *f_host) {
    if (!b || !f_host) return fail(TG_ERR_INVALID, "null argument");
    if (b->t2 == b->t1) return fail(TG_ERR_STATE, "calc_f needs t2 != t1");
    HIP_TRY(hipSetDevice(b->device));
    tg::RunArgs A = base_args(b, tg::MODE_CALC_F);
    if (int rc = launch(b, A)) return rc;
    HIP_TRY(hipMemcpyAsync(f_host, b->f_out.get(), (size_t)b->batch * b->P.nf * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return TG_SUCCESS;
}

/* Per trajectory: how many Newton systems of the last rollout / step launch the structured solve (bbd.hpp) handed to the pivoting
 * solver because a pivot guard failed.  Zero for kernels without a structured solve.  Results are correct either way; a batch that
 * reports fallbacks on most systems (very small time steps, very heavy bodies) runs slower than with the pivoting solver alone. */
int tg_batch_solver_fallbacks(tg_batch *b, int32_t *fallbacks_out) {
    if (!b || !fallbacks_out) return fail(TG_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipMemcpyAsync(fallbacks_out, b->fallbacks.get(), (size_t)b->batch * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return TG_SUCCESS;
}

int tg_batch_status(tg_batch *b, int32_t *iterations_out, int32_t *status_out) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    if (b->mirror_valid) {
        const tg::DevProg &P = b->P;
        const size_t B = (size_t)b->batch;
        const int32_t *m = reinterpret_cast<const int32_t *>(b->io_host.get() + b->io_in + B * (P.nq + P.nd + P.nc));
        if (iterations_out) std::memcpy(iterations_out, m, B * sizeof(int32_t));
        if (status_out) std::memcpy(status_out, m + B, B * sizeof(int32_t));
        return TG_SUCCESS;
    }
    HIP_TRY(hipSetDevice(b->device));
    if (iterations_out) HIP_TRY(hipMemcpyAsync(iterations_out, b->iters.get(), (size_t)b->batch * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    if (status_out) HIP_TRY(hipMemcpyAsync(status_out, b->status.get(), (size_t)b->batch * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return TG_SUCCESS;
}

int tg_batch_step(tg_batch *b, double t2_new, const double *u1_host, const double *k2_host, const double *q2_hint_host,
                  const double *lambda_hint_host, int32_t max_iterations, int32_t *iterations_out, int32_t *status_out) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    const tg::DevProg &P = b->P;
    if ((P.nu && !u1_host) || (P.nk && !k2_host)) return fail(TG_ERR_INVALID, "u1 / k2 required");
    if (t2_new == b->t2) return fail(TG_ERR_STATE, "step needs t2_new != t2");
    HIP_TRY(hipSetDevice(b->device));
    const size_t B = (size_t)b->batch;
    const bool want_lh = lambda_hint_host && P.nc;
    // Small batches: the call is host-latency bound (a MidpointVI.step() loop; tools/step_latency.py).  Inputs and results live in one
    // pinned, device-visible host block: the kernel reads (u1, k2, hints) from it at the head of the step and writes (q2, p2, lambda1,
    // iterations, status) into it beside the device state -- one launch on the stream, no copy engine, no packing kernel.
    const size_t n_in = B * ((size_t)P.nu + P.nk + P.nd + P.nc), n_out = B * ((size_t)P.nq + P.nd + P.nc) + B;   // 2 B ints = B doubles
    // (gated on the trajectory count: the path was measured at B = 1 .. 64 only; larger batches take the copy engine below)
    const bool pinned = B <= 64 && (n_in + n_out) * sizeof(double) <= (1u << 20);
    double *du, *dk, *dq, *dl;       // where the kernel reads (u1, k2, hints)
    if (pinned) {
        if (!b->io_host) {
            if (b->io_host.ensure(n_in + n_out, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
                hipHostGetDevicePointer(reinterpret_cast<void **>(&b->io_dev), b->io_host.get(), 0) != hipSuccess) { b->io_host.reset(); return fail(TG_ERR_HIP, "allocation of the step staging block failed"); }
            b->io_in = n_in; b->io_out = n_out;
        }
        double *hu = b->io_host.get(), *hk = hu + B * P.nu, *hq = hk + B * P.nk, *hl = hq + B * P.nd;
        du = b->io_dev; dk = du + B * P.nu; dq = dk + B * P.nk; dl = dq + B * P.nd;
        if (P.nu) std::memcpy(hu, u1_host, B * P.nu * sizeof(double));
        if (P.nk) std::memcpy(hk, k2_host, B * P.nk * sizeof(double));
        if (q2_hint_host) std::memcpy(hq, q2_hint_host, B * P.nd * sizeof(double));
        if (want_lh) std::memcpy(hl, lambda_hint_host, B * P.nc * sizeof(double));
    } else {
        du = b->stage_u.get(); dk = b->stage_k.get(); dq = b->stage_qh.get(); dl = b->stage_lh.get();
        if (P.nu) HIP_TRY(hipMemcpyAsync(du, u1_host, B * P.nu * sizeof(double), hipMemcpyHostToDevice, b->stream));
        if (P.nk) HIP_TRY(hipMemcpyAsync(dk, k2_host, B * P.nk * sizeof(double), hipMemcpyHostToDevice, b->stream));
        if (q2_hint_host) HIP_TRY(hipMemcpyAsync(dq, q2_hint_host, B * P.nd * sizeof(double), hipMemcpyHostToDevice, b->stream));
        if (want_lh) HIP_TRY(hipMemcpyAsync(dl, lambda_hint_host, B * P.nc * sizeof(double), hipMemcpyHostToDevice, b->stream));
    }
    tg::RunArgs A = step_args(b, t2_new - b->t2, max_iterations, du, dk, q2_hint_host ? dq : nullptr, want_lh ? dl : nullptr);
    if (pinned) A.mirror = b->io_dev + n_in;
    if (int rc = launch(b, A)) return rc;
    b->t1 = b->t2; b->t2 = t2_new;
    if (pinned) { HIP_TRY(hipStreamSynchronize(b->stream)); b->mirror_valid = true; }
    return tg_batch_status(b, iterations_out, status_out);
}

int tg_batch_set_step_sizes(tg_batch *b, int32_t count, const double *dt_host, int32_t by_trajectory) {
    if (!b || count < 0 || (count > 0 && !dt_host)) return fail(TG_ERR_INVALID, "bad arguments");
    // validate first: a refused list leaves the batch's current one in place
    for (int i = 0; i < count; i++) {
        if (dt_host[i] == 0.0) return fail(TG_ERR_INVALID, "zero step size");
        if (!std::isfinite(dt_host[i])) return fail(TG_ERR_INVALID, "step size is not finite");
    }
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));          // a launch in flight may still read the old list
    tg::DeviceBuffer<double> fresh;
    if (count > 0) HIP_TRY(fresh.ensure((size_t)count));
    if (count > 0 && hipMemcpy(fresh.get(), dt_host, sizeof(double) * (size_t)count, hipMemcpyHostToDevice) != hipSuccess)
        return fail(TG_ERR_HIP, "copy of the step-size list failed");
    b->dt_dev = std::move(fresh);
    if (count > 0) b->dt_host.assign(dt_host, dt_host + count); else b->dt_host.clear();
    b->dt_by_trajectory = (count > 0 && by_trajectory) ? 1 : 0;
    return TG_SUCCESS;
}

// What the three rollouts share: the step-size-list refusals, the launch and the new times.  A: base_args plus the caller's buffers.
static int run_rollout(tg_batch *b, tg::RunArgs &A, int n_steps, double dt, int max_iterations) {
    const bool by_step = !b->dt_host.empty() && !b->dt_by_trajectory;
    // a by-trajectory list (set only with a list) belongs to one-step batches: every step of a longer rollout would take the
    // trajectory's size while the times advance by the scalar
    if (n_steps > 1 && b->dt_by_trajectory) return fail(TG_ERR_INVALID, "a by-trajectory step-size list takes one-step launches only");
    if (by_step && (size_t)n_steps > b->dt_host.size()) return fail(TG_ERR_INVALID, "rollout longer than the step-size list");
    if (!A.Kproj && ((b->P.nu && !A.U) || (b->P.nk && !A.K))) return fail(TG_ERR_INVALID, "U / K device buffers required");   // open loop
    HIP_TRY(hipSetDevice(b->device));
    A.n_steps = n_steps; A.dt = dt; A.max_iterations = max_iterations;
    if (int rc = launch(b, A)) return rc;
    // t1, t2 after n_steps steps from t2 with the uniform step dt or the batch's step-size list
    if (by_step) {
        double t = b->t2;
        for (int k = 0; k < n_steps; k++) { b->t1 = t; t += b->dt_host[k]; }
        b->t2 = t;
    } else {
        b->t1 = b->t2 + (n_steps - 1) * dt;
        b->t2 = b->t2 + n_steps * dt;
    }
    return TG_SUCCESS;
}

int tg_batch_rollout(tg_batch *b, int32_t n_steps, double dt, const double *U_dev, const double *K_dev, double *X_dev,
                     int32_t max_iterations) {
    if (!b || n_steps <= 0 || dt == 0.0) return fail(TG_ERR_INVALID, "bad arguments");
    tg::RunArgs A = base_args(b, tg::MODE_ROLLOUT);
    A.U = U_dev; A.K = K_dev; A.X = X_dev;
    return run_rollout(b, A, n_steps, dt, max_iterations);
}

int tg_batch_rollout_closed_loop(tg_batch *b, int32_t n_steps, double dt, const double *Kproj_dev, int32_t group_size,
                                 const double *bX_dev, const double *bU_dev, double *X_dev, double *U_dev,
                                 int32_t max_iterations) {
    if (!b || n_steps <= 0 || dt == 0.0 || !Kproj_dev || !bX_dev || !bU_dev || group_size <= 0)
        return fail(TG_ERR_INVALID, "bad arguments");
    tg::RunArgs A = base_args(b, tg::MODE_ROLLOUT);
    A.Kproj = Kproj_dev; A.bX = bX_dev; A.bU = bU_dev; A.Uout = U_dev; A.group_size = group_size; A.X = X_dev;
    return run_rollout(b, A, n_steps, dt, max_iterations);
}

int tg_batch_rollout_closed_loop_subset(tg_batch *b, int32_t n_trajectories, int32_t n_steps, double dt, const double *Kproj_dev,
                                        int32_t group_size, const int32_t *group_select_dev, const double *bX_dev,
                                        const double *bU_dev, double *X_dev, double *U_dev, int32_t max_iterations) {
    if (!b || n_steps <= 0 || dt == 0.0 || !Kproj_dev || !bX_dev || !bU_dev || group_size <= 0 || n_trajectories <= 0 ||
        n_trajectories > b->batch)
        return fail(TG_ERR_INVALID, "bad arguments");
    tg::RunArgs A = base_args(b, tg::MODE_ROLLOUT);
    A.batch = n_trajectories;
    A.Kproj = Kproj_dev; A.bX = bX_dev; A.bU = bU_dev; A.Uout = U_dev; A.group_size = group_size; A.X = X_dev;
    A.group_map = group_select_dev;
    return run_rollout(b, A, n_steps, dt, max_iterations);
}

int tg_batch_rollout_stats(tg_batch *b, int64_t *total_iterations, int32_t *n_failed) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    std::vector<int> it(b->batch), st(b->batch);
    int rc = tg_batch_status(b, it.data(), st.data());
    if (rc) return rc;
    int64_t tot = 0; int nf = 0;
    for (int i = 0; i < b->batch; i++) { tot += it[i]; nf += (st[i] != TG_OK); }
    if (total_iterations) *total_iterations = tot;
    if (n_failed) *n_failed = nf;
    return TG_SUCCESS;
}

static int snapshot_copy(tg_batch *b, bool save) {
    const tg::DevProg &P = b->P;
    const size_t B = (size_t)b->batch;
    double *fields[6] = {b->q1.get(), b->q2.get(), b->p1.get(), b->p2.get(), b->lam.get(), b->u1.get()};
    const size_t w[6] = {(size_t)P.nq, (size_t)P.nq, (size_t)P.nd, (size_t)P.nd, (size_t)P.nc, (size_t)P.nu};
    size_t off = 0;
    for (int i = 0; i < 6; i++) {
        if (w[i]) {
            double *dst = save ? b->snap.get() + off : fields[i];
            const double *src = save ? fields[i] : b->snap.get() + off;
            HIP_TRY(hipMemcpyAsync(dst, src, B * w[i] * sizeof(double), hipMemcpyDeviceToDevice, b->stream));
        }
        off += B * w[i];
    }
    return TG_SUCCESS;
}

int tg_batch_snapshot(tg_batch *b) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    HIP_TRY(hipSetDevice(b->device));
    b->snap_t1 = b->t1; b->snap_t2 = b->t2;
    return snapshot_copy(b, true);
}

int tg_batch_restore(tg_batch *b) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    HIP_TRY(hipSetDevice(b->device));
    b->mirror_valid = false;
    b->t1 = b->snap_t1; b->t2 = b->snap_t2;
    return snapshot_copy(b, false);
}

/* Diagnostic build (make prof): per-phase cycle counters of trajectory 0 of the last launch. */
int tg_batch_profile(tg_batch *b, int64_t out[16]) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    if (!b->prof) return fail(TG_ERR_UNSUPPORTED, "library was not built with TG_PROFILE");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(out, b->prof.get(), 16 * sizeof(long long), hipMemcpyDeviceToHost));
    return TG_SUCCESS;
}

int tg_batch_deriv1(tg_batch *b) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    if (b->t2 == b->t1) return fail(TG_ERR_STATE, "Integrator has not solved the next time step yet.");
    HIP_TRY(hipSetDevice(b->device));
    if (int rc = ensure_deriv_buffers(b, true, false)) return rc;
    tg::RunArgs A = base_args(b, tg::MODE_DERIV1);
    if (int rc = launch(b, A)) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->have_d1 = true;
    return TG_SUCCESS;
}

int tg_batch_deriv2_contract(tg_batch *b, const double *z_host, double *hz_host) {
    if (!b || !z_host || !hz_host) return fail(TG_ERR_INVALID, "null argument");
    return tg_batch_deriv2_contract_lambda(b, z_host, nullptr, hz_host);
}

int tg_batch_deriv2_contract_lambda(tg_batch *b, const double *z_host, const double *zlambda_host, double *hz_host) {
    if (!b || !hz_host || (!z_host && !zlambda_host)) return fail(TG_ERR_INVALID, "null argument");
    if (b->P.n_true_springs) return fail(TG_ERR_UNSUPPORTED, "V_dqdqdq() is undefined for LinearSpring (as in the reference): no second derivatives");
    if (b->t2 == b->t1) return fail(TG_ERR_STATE, "Integrator has not solved the next time step yet.");
    HIP_TRY(hipSetDevice(b->device));
    const size_t B = (size_t)b->batch, R = (size_t)b->P.d_nrhs;
    if (int rc0 = ensure_deriv_buffers(b, false, true)) return rc0;
    if (z_host) HIP_TRY(hipMemcpyAsync(b->z_dev.get(), z_host, B * b->P.nX * sizeof(double), hipMemcpyHostToDevice, b->stream));
    else HIP_TRY(hipMemsetAsync(b->z_dev.get(), 0, B * b->P.nX * sizeof(double), b->stream));
    if (zlambda_host && b->P.nc) HIP_TRY(hipMemcpyAsync(b->zl_dev.get(), zlambda_host, B * b->P.nc * sizeof(double), hipMemcpyHostToDevice, b->stream));
    tg::RunArgs A = base_args(b, tg::MODE_DERIV2Z);
    A.zl = (zlambda_host && b->P.nc) ? b->zl_dev.get() : nullptr;
    if (int rc = launch(b, A)) return rc;
    HIP_TRY(hipMemcpyAsync(hz_host, b->hz_dev.get(), B * R * R * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return TG_SUCCESS;
}

int tg_batch_dynamics_device(tg_batch *b, const double *q_dev, const double *dq_dev, const double *u_dev, const double *ddqk_dev,
                             double *ddq_dev, double *lambda_dev, int32_t *status_dev) {
    if (!b || !q_dev || !dq_dev || !ddq_dev) return fail(TG_ERR_INVALID, "null argument");
    const tg::DevProg &P = b->P;
    if ((P.nu && !u_dev) || (P.nk && !ddqk_dev) || (P.nc && !lambda_dev)) return fail(TG_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(b->dyn_ints.ensure(2 * (size_t)b->batch));
    tg::RunArgs A = base_args(b, tg::MODE_DYNAMICS);
    // the state is an argument of this call: nothing of the integrator (q1, q2, p, lambda1, status) is touched
    A.q1 = A.q2 = const_cast<double *>(q_dev);
    A.u1 = const_cast<double *>(u_dev ? u_dev : b->u1.get());
    A.dq_in = dq_dev; A.ddqk_in = ddqk_dev; A.ddq_out = ddq_dev; A.lam_out = lambda_dev;
    A.iters = b->dyn_ints.get(); A.status = status_dev ? status_dev : b->dyn_ints.get() + b->batch;
    return launch(b, A);
}

static int lagrangian_host(tg_batch *b, const double *q_host, const double *dq_host, const int32_t *seed1_host, const int32_t *seed2_host, double *first_host, double *second_host) {
    if (!b || !q_host || !dq_host || !first_host || !second_host) return fail(TG_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(b->device));
    const size_t B = (size_t)b->batch, nq = b->P.nq, out_total = B * nq * (2 + 3 * nq);
    DynStage s;
    if (int rc = stage_dynamics(b, q_host, dq_host, nullptr, nullptr, s)) return rc;
    HIP_TRY(b->lag.ensure(out_total));
    double *o1 = b->lag.get(), *o2 = o1 + 2 * B * nq;
    HIP_TRY(hipMemsetAsync(o1, 0, out_total * sizeof(double), b->stream));     // the kernel accumulates
    tg::RunArgs A = base_args(b, tg::MODE_LAGRANGIAN);
    A.q1 = A.q2 = s.q; A.dq_in = s.dq; A.lag1_out = o1; A.lag2_out = o2;
    A.iters = b->dyn_ints.get(); A.status = b->dyn_ints.get() + b->batch;
    if (seed1_host) {
        if (int rc = stage_seeds(b, seed1_host, seed2_host)) return rc;
        A.seed1 = b->seeds.get(); A.seed2 = seed2_host ? b->seeds.get() + B : nullptr;
        if (int rc = launch_forward(b, A, seed2_host ? 2 : 1)) return rc;
    } else if (int rc = launch(b, A)) return rc;
    HIP_TRY(hipMemcpyAsync(first_host, o1, 2 * B * nq * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipMemcpyAsync(second_host, o2, 3 * B * nq * nq * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return TG_SUCCESS;
}

int tg_batch_lagrangian(tg_batch *b, const double *q_host, const double *dq_host, double *first_host, double *second_host) {
    return lagrangian_host(b, q_host, dq_host, nullptr, nullptr, first_host, second_host);
}
int tg_batch_lagrangian_forward(tg_batch *b, const double *q_host, const double *dq_host, const int32_t *seed1_host, const int32_t *seed2_host,
                                double *first_host, double *second_host) {
    if (!seed1_host) return fail(TG_ERR_INVALID, "null argument");
    return lagrangian_host(b, q_host, dq_host, seed1_host, seed2_host, first_host, second_host);
}

int tg_batch_set_predictor(tg_batch *b, int32_t mode) {
    if (!b || mode < 0 || mode > 1) return fail(TG_ERR_INVALID, "predictor mode must be 0 or 1");
    b->predictor = mode;
    return TG_SUCCESS;
}

int tg_batch_energy(tg_batch *b, const double *q_host, const double *dq_host, double *energy_host) {
    if (!b || !q_host || !dq_host || !energy_host) return fail(TG_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(b->device));
    const size_t B = (size_t)b->batch;
    DynStage s;
    if (int rc = stage_dynamics(b, q_host, dq_host, nullptr, nullptr, s)) return rc;
    HIP_TRY(b->energy.ensure(2 * B));
    tg::RunArgs A = base_args(b, tg::MODE_ENERGY);
    A.q1 = A.q2 = s.q; A.dq_in = s.dq; A.energy_out = b->energy.get();
    A.iters = b->dyn_ints.get(); A.status = b->dyn_ints.get() + b->batch;
    if (int rc = launch(b, A)) return rc;
    HIP_TRY(hipMemcpyAsync(energy_host, b->energy.get(), 2 * B * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return TG_SUCCESS;
}

static int dyn_deriv1_device(tg_batch *b, const double *q_dev, const double *dq_dev, const double *u_dev, const double *ddqk_dev, const int *seed_dev,
                             double *const out_dev[8], int32_t *status_dev) {
    if (!b || !q_dev || !dq_dev || !out_dev) return fail(TG_ERR_INVALID, "null argument");
    const tg::DevProg &P = b->P;
    if ((P.nu && !u_dev) || (P.nk && !ddqk_dev)) return fail(TG_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(b->dyn_ints.ensure(2 * (size_t)b->batch));
    tg::RunArgs A = base_args(b, tg::MODE_DYN_DERIV1);
    A.q1 = A.q2 = const_cast<double *>(q_dev);
    A.u1 = const_cast<double *>(u_dev ? u_dev : b->u1.get());
    A.dq_in = dq_dev; A.ddqk_in = ddqk_dev; A.ddq_out = nullptr; A.lam_out = nullptr;
    for (int g = 0; g < 8; g++) A.g1[g] = out_dev[g];
    A.iters = b->dyn_ints.get(); A.status = status_dev ? status_dev : b->dyn_ints.get() + b->batch;
    if (seed_dev) { A.seed1 = seed_dev; return launch_forward(b, A, 1); }
    return launch(b, A);
}
int tg_batch_dynamics_deriv1_device(tg_batch *b, const double *q_dev, const double *dq_dev, const double *u_dev, const double *ddqk_dev,
                                    double *const out_dev[8], int32_t *status_dev) {
    return dyn_deriv1_device(b, q_dev, dq_dev, u_dev, ddqk_dev, nullptr, out_dev, status_dev);
}

static int dyn_deriv1_host(tg_batch *b, const double *q_host, const double *dq_host, const double *u_host, const double *ddqk_host, const int32_t *seed_host,
                           double *f_dq, double *f_ddq, double *f_dddk, double *f_du,
                           double *lambda_dq, double *lambda_ddq, double *lambda_dddk, double *lambda_du, int32_t *status_host) {
    if (!b || !q_host || !dq_host) return fail(TG_ERR_INVALID, "null argument");
    const tg::DevProg &P = b->P;
    if ((P.nu && !u_host) || (P.nk && !ddqk_host)) return fail(TG_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(b->device));
    const size_t B = (size_t)b->batch, nq = P.nq, nd = P.nd, nk = P.nk, nu = P.nu, nc = P.nc;
    DynStage s;
    if (int rc = stage_dynamics(b, q_host, dq_host, u_host, ddqk_host, s)) return rc;
    const size_t rows[4] = {nq, nq, nk, nu};
    double *host[8] = {f_dq, f_ddq, f_dddk, f_du, lambda_dq, lambda_ddq, lambda_dddk, lambda_du};
    size_t cnt[8], out_total = 0;
    for (int g = 0; g < 8; g++) out_total += cnt[g] = B * rows[g & 3] * (g < 4 ? nd : nc);
    HIP_TRY(b->dyn_d1.ensure(out_total));
    double *dev[8], *next = b->dyn_d1.get();
    for (int g = 0; g < 8; g++) { dev[g] = (host[g] && cnt[g]) ? next : nullptr; next += cnt[g]; }
    if (seed_host) { if (int rc = stage_seeds(b, seed_host, nullptr)) return rc; }
    if (int rc = dyn_deriv1_device(b, s.q, s.dq, nu ? s.u : nullptr, nk ? s.ddk : nullptr, seed_host ? b->seeds.get() : nullptr, dev, nullptr)) return rc;
    for (int g = 0; g < 8; g++)
        if (dev[g]) HIP_TRY(hipMemcpyAsync(host[g], dev[g], cnt[g] * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (status_host) HIP_TRY(hipMemcpyAsync(status_host, b->dyn_ints.get() + B, B * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return TG_SUCCESS;
}
int tg_batch_dynamics_deriv1(tg_batch *b, const double *q_host, const double *dq_host, const double *u_host, const double *ddqk_host,
                             double *f_dq, double *f_ddq, double *f_dddk, double *f_du,
                             double *lambda_dq, double *lambda_ddq, double *lambda_dddk, double *lambda_du, int32_t *status_host) {
    return dyn_deriv1_host(b, q_host, dq_host, u_host, ddqk_host, nullptr, f_dq, f_ddq, f_dddk, f_du, lambda_dq, lambda_ddq, lambda_dddk, lambda_du, status_host);
}
int tg_batch_dynamics_deriv1_forward(tg_batch *b, const double *q_host, const double *dq_host, const double *u_host, const double *ddqk_host,
                                     const int32_t *seed_host, double *f_dq, double *f_ddq, double *f_dddk, double *f_du,
                                     double *lambda_dq, double *lambda_ddq, double *lambda_dddk, double *lambda_du, int32_t *status_host) {
    if (!seed_host) return fail(TG_ERR_INVALID, "null argument");
    return dyn_deriv1_host(b, q_host, dq_host, u_host, ddqk_host, seed_host, f_dq, f_ddq, f_dddk, f_du, lambda_dq, lambda_ddq, lambda_dddk, lambda_du, status_host);
}

int tg_batch_dynamics(tg_batch *b, const double *q_host, const double *dq_host, const double *u_host, const double *ddqk_host,
                      double *ddq_host, double *lambda_host, int32_t *status_host) {
    if (!b || !q_host || !dq_host || !ddq_host) return fail(TG_ERR_INVALID, "null argument");
    const tg::DevProg &P = b->P;
    if ((P.nu && !u_host) || (P.nk && !ddqk_host) || (P.nc && !lambda_host)) return fail(TG_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(b->device));
    const size_t B = (size_t)b->batch, nd = P.nd, nc = P.nc;
    DynStage s;
    if (int rc = stage_dynamics(b, q_host, dq_host, u_host, ddqk_host, s)) return rc;
    if (int rc = tg_batch_dynamics_device(b, s.q, s.dq, P.nu ? s.u : nullptr, P.nk ? s.ddk : nullptr, s.ddq, s.lam, nullptr)) return rc;
    HIP_TRY(hipMemcpyAsync(ddq_host, s.ddq, B * nd * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (nc) HIP_TRY(hipMemcpyAsync(lambda_host, s.lam, B * nc * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (status_host) HIP_TRY(hipMemcpyAsync(status_host, b->dyn_ints.get() + B, B * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return TG_SUCCESS;
}

// ---- the pose solvers: constraint projection (mvi_project.hpp) and equilibrium search (mvi_equilibrium.hpp) on the frame of mvi_pose.hpp

// out[0..3] of a tg_system_*_lds call for a kernel that keeps per_team doubles of LDS per team
static int pose_lds(const tg_system *sys, int per_team, const char *too_large, int32_t out[4]) {
    const long long bytes = (long long)(64 / sys->team) * per_team * (long long)sizeof(double);
    out[0] = sys->team; out[1] = per_team; out[2] = (int32_t)std::min<long long>(bytes, 0x7fffffff); out[3] = 0;
    if (bytes > 160 * 1024) return fail(TG_ERR_UNSUPPORTED, too_large);
    return TG_SUCCESS;
}

// what every entry point of a pose solver checks first
static int pose_check(const tg_batch *b, const double *q, const double *q_out, double tolerance, int32_t max_iterations) {
    if (!b || !q || !q_out) return fail(TG_ERR_INVALID, "null argument");
    if (!(tolerance > 0.0)) return fail(TG_ERR_INVALID, "tolerance must be positive");
    if (max_iterations < 0) return fail(TG_ERR_INVALID, "max_iterations must not be negative");
    return TG_SUCCESS;
}

// The launch of a pose solver behind its checks: the mode's arguments and the grid.  The pose is an argument of the call: nothing of the
// integrator (q1, q2, p, lambda1, status) is read or written, and a loaded specialised library has no say.  Iteration and status
// words nobody asked for go to the batch's own.
static int pose_prepare(tg_batch *b, int mode, double tolerance, int32_t max_iterations, int32_t *iterations_out_dev, int32_t *status_out_dev,
                        tg::RunArgs &A, int &grid) {
    HIP_TRY(hipSetDevice(b->device));
    const size_t B = (size_t)b->batch;
    HIP_TRY(b->pose_ints.ensure(b->P.nq + 2 * B));
    A = base_args(b, mode);
    A.q1 = A.q2 = A.p1 = A.p2 = A.lam = A.u1 = nullptr;
    A.tolerance = tolerance; A.max_iterations = max_iterations;
    A.iters = iterations_out_dev ? iterations_out_dev : b->pose_ints.get() + b->P.nq;
    A.status = status_out_dev ? status_out_dev : b->pose_ints.get() + b->P.nq + B;
    const int per_block = 64 / b->sys->team;
    grid = (b->batch + per_block - 1) / per_block;
    return TG_SUCCESS;
}

// Staging of the host-facing pose solvers: q0 and the mask in; q, mu, the iteration and status words out.  `extra` is the call's
// own: the projection's dq0 and dq, the search's V.
struct PoseStage {
    double *q0, *q, *mu, *extra;
    int *mask, *iters, *status;
};
static int pose_stage_in(tg_batch *b, const double *q_host, const int32_t *free_host, PoseStage &s) {
    HIP_TRY(hipSetDevice(b->device));
    const size_t B = (size_t)b->batch, nq = b->P.nq, nc = b->P.nc;
    HIP_TRY(b->pose.ensure(B * (2 * nq + nc + std::max<size_t>(2 * nq, 2))));      // (whichever call needs more)
    HIP_TRY(b->pose_ints.ensure(nq + 2 * B));
    s.q0 = b->pose.get(); s.q = s.q0 + B * nq; s.mu = s.q + B * nq; s.extra = s.mu + B * nc;
    s.mask = b->pose_ints.get(); s.iters = s.mask + nq; s.status = s.iters + B;
    HIP_TRY(hipMemcpyAsync(s.q0, q_host, B * nq * sizeof(double), hipMemcpyHostToDevice, b->stream));
    if (free_host && nq) HIP_TRY(hipMemcpyAsync(s.mask, free_host, nq * sizeof(int), hipMemcpyHostToDevice, b->stream));
    return TG_SUCCESS;
}
static int pose_stage_out(tg_batch *b, const PoseStage &s, double *q_out, double *mu_out, int32_t *iterations_out, int32_t *status_out) {
    const size_t B = (size_t)b->batch, nq = b->P.nq, nc = b->P.nc;
    HIP_TRY(hipMemcpyAsync(q_out, s.q, B * nq * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (mu_out && nc) HIP_TRY(hipMemcpyAsync(mu_out, s.mu, B * nc * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (iterations_out) HIP_TRY(hipMemcpyAsync(iterations_out, s.iters, B * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    if (status_out) HIP_TRY(hipMemcpyAsync(status_out, s.status, B * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return TG_SUCCESS;
}

/* Team size, doubles of LDS per team and bytes of LDS per workgroup of the projection kernel for this system (out[0..2]; out[3] 0):
 * the rollout slice plus the KKT image, q0, the solver's row scales and the free configs' places (mvi_project.hpp).
 * TG_ERR_UNSUPPORTED, with out filled, above the 160 KiB a workgroup can have. */
int tg_system_projection_lds(const tg_system *sys, int32_t out[4]) {
    if (!sys || !out) return fail(TG_ERR_INVALID, "null argument");
    tg::ProjectArgs J{};
    tg::project_layout(sys->H.p.lds_per_team, sys->H.p.nq, sys->H.p.nc, J);
    return pose_lds(sys, J.lds_per_team, "system too large for the LDS-resident projection kernel", out);
}

int tg_batch_project_constraints_device(tg_batch *b, const double *q_dev, const double *dq_dev, const int32_t *free_dev, double tolerance,
                                        int32_t max_iterations, double *q_out_dev, double *dq_out_dev, double *mu_out_dev,
                                        int32_t *iterations_out_dev, int32_t *status_out_dev) {
    if (int rc = pose_check(b, q_dev, q_out_dev, tolerance, max_iterations)) return rc;
    if (dq_out_dev && !dq_dev) return fail(TG_ERR_INVALID, "dq_out without dq");
    if (dq_dev && !dq_out_dev) return fail(TG_ERR_INVALID, "dq without dq_out");
    int32_t geo[4];
    if (int rc = tg_system_projection_lds(b->sys, geo)) return rc;
    // no parameter table has a say either (constraints do not depend on inertia, gravity or damping)
    tg::RunArgs A;
    int grid;
    if (int rc = pose_prepare(b, tg::MODE_PROJECT, tolerance, max_iterations, iterations_out_dev, status_out_dev, A, grid)) return rc;
    tg::ProjectArgs J{};
    tg::project_layout(b->P.lds_per_team, b->P.nq, b->P.nc, J);
    J.free_mask = free_dev; J.q0 = q_dev; J.dq0 = dq_dev; J.q = q_out_dev; J.dq = dq_out_dev; J.mu = mu_out_dev;
    b->launched[0][0].add(tg::MODE_PROJECT);
    int rc = tg_detail::launch_project(b->sys->team, launch_springs(b), b->d_prog.get(), A, J, grid, (size_t)geo[2], b->stream);
    if (rc == TG_SUCCESS && hipGetLastError() != hipSuccess) rc = fail(TG_ERR_HIP, "kernel launch failed");
    return rc;
}

int tg_batch_project_constraints(tg_batch *b, const double *q_host, const double *dq_host, const int32_t *free_host, double tolerance,
                                 int32_t max_iterations, double *q_out, double *dq_out, double *mu_out, int32_t *iterations_out, int32_t *status_out) {
    if (int rc = pose_check(b, q_host, q_out, tolerance, max_iterations)) return rc;
    if (dq_out && !dq_host) return fail(TG_ERR_INVALID, "dq_out without dq");
    int32_t geo[4];
    if (int rc = tg_system_projection_lds(b->sys, geo)) return rc;
    PoseStage s;
    if (int rc = pose_stage_in(b, q_host, free_host, s)) return rc;
    const size_t rates = (size_t)b->batch * b->P.nq;
    double *dq0 = s.extra, *dq = dq0 + rates;
    if (dq_host) HIP_TRY(hipMemcpyAsync(dq0, dq_host, rates * sizeof(double), hipMemcpyHostToDevice, b->stream));
    if (int rc = tg_batch_project_constraints_device(b, s.q0, dq_host ? dq0 : nullptr, free_host ? s.mask : nullptr, tolerance, max_iterations,
                                                     s.q, dq_host ? dq : nullptr, s.mu, s.iters, s.status)) return rc;
    if (dq_out) HIP_TRY(hipMemcpyAsync(dq_out, dq, rates * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    return pose_stage_out(b, s, q_out, mu_out, iterations_out, status_out);
}

/* Team size, doubles of LDS per team and bytes of LDS per workgroup of the equilibrium kernel for this system (out[0..2]; out[3] 0):
 * the rollout slice plus the KKT image, W, the Cholesky work area, q0, the kept pose and multipliers, V_q, g, V, the solver's row
 * scales and the free configs' places (mvi_equilibrium.hpp).  TG_ERR_UNSUPPORTED, with out filled, above the 160 KiB a workgroup can
 * have, and for a system with a NonlinearConfigSpring (no potential to minimise). */
int tg_system_equilibrium_lds(const tg_system *sys, int32_t out[4]) {
    if (!sys || !out) return fail(TG_ERR_INVALID, "null argument");
    tg::EquilibriumArgs J{};
    tg::equilibrium_layout(sys->H.p.lds_per_team, sys->H.p.nq, sys->H.p.nc, J);
    const int rc = pose_lds(sys, J.lds_per_team, "system too large for the LDS-resident equilibrium kernel", out);
    if (sys->H.p.n_ncs > 0) return fail(TG_ERR_UNSUPPORTED, "a NonlinearConfigSpring has a force but no potential energy (as in the reference): nothing to minimise");
    return rc;
}

int tg_batch_minimize_potential_device(tg_batch *b, const double *q_dev, const int32_t *free_dev, double tolerance, int32_t max_iterations,
                                       double *q_out_dev, double *mu_out_dev, double *v_out_dev, int32_t *iterations_out_dev,
                                       int32_t *status_out_dev) {
    if (int rc = pose_check(b, q_dev, q_out_dev, tolerance, max_iterations)) return rc;
    int32_t geo[4];
    if (int rc = tg_system_equilibrium_lds(b->sys, geo)) return rc;
    // a parameter table has a say (masses and gravity move an equilibrium; damping plays no part)
    tg::RunArgs A;
    int grid;
    if (int rc = pose_prepare(b, tg::MODE_EQUILIBRIUM, tolerance, max_iterations, iterations_out_dev, status_out_dev, A, grid)) return rc;
    tg::EquilibriumArgs J{};
    tg::equilibrium_layout(b->P.lds_per_team, b->P.nq, b->P.nc, J);
    J.free_mask = free_dev; J.q0 = q_dev; J.q = q_out_dev; J.mu = mu_out_dev; J.v = v_out_dev;
    const bool par = b->par_rows > 0;
    int rc = tg_detail::launch_equilibrium(b->sys->team, launch_springs(b), par, b->d_prog.get(), A, J,
                                           tg::ParTable{par ? b->par_dev.get() : nullptr, par ? b->par_group : 1, par ? b->par_stride : 0}, grid,
                                           (size_t)geo[2], b->stream);
    if (rc == TG_SUCCESS && hipGetLastError() != hipSuccess) rc = fail(TG_ERR_HIP, "kernel launch failed");
    if (rc == TG_SUCCESS) b->launched[par][0].add(tg::MODE_EQUILIBRIUM);      // a refused launch (the profiling build) is not counted
    return rc;
}

int tg_batch_minimize_potential(tg_batch *b, const double *q_host, const int32_t *free_host, double tolerance, int32_t max_iterations,
                                double *q_out, double *mu_out, double *v_out, int32_t *iterations_out, int32_t *status_out) {
    if (int rc = pose_check(b, q_host, q_out, tolerance, max_iterations)) return rc;
    int32_t geo[4];
    if (int rc = tg_system_equilibrium_lds(b->sys, geo)) return rc;
    PoseStage s;
    if (int rc = pose_stage_in(b, q_host, free_host, s)) return rc;
    if (int rc = tg_batch_minimize_potential_device(b, s.q0, free_host ? s.mask : nullptr, tolerance, max_iterations, s.q, s.mu, s.extra, s.iters, s.status)) return rc;
    if (v_out) HIP_TRY(hipMemcpyAsync(v_out, s.extra, (size_t)b->batch * 2 * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    return pose_stage_out(b, s, q_out, mu_out, iterations_out, status_out);
}

// ---- batched normal modes (mvi_modes.hpp): one team per pose, one launch

/* Team size, doubles of LDS per team and bytes of LDS per workgroup of the normal-modes kernel for this system (out[0..2]; out[3] 0):
 * the rollout slice plus the image, K, M, four [nq][nq | 1] images, q0, V_q, g, V, the least-squares and Jacobi scratch, the
 * eigenvalues and their places, the row scales and the free configs' places (mvi_modes.hpp: modes_layout).  TG_ERR_UNSUPPORTED, with out
 * filled, above the 160 KiB a workgroup can have, for a system with a NonlinearConfigSpring and in the profiling build. */
int tg_system_normal_modes_lds(const tg_system *sys, int32_t out[4]) {
    if (!sys || !out) return fail(TG_ERR_INVALID, "null argument");
    tg::ModesArgs J{};
    tg::modes_layout(sys->H.p.lds_per_team, sys->H.p.nq, sys->H.p.nc, J);
    const int rc = pose_lds(sys, J.lds_per_team, "system too large for the LDS-resident normal-modes kernel", out);
    if (sys->H.p.n_ncs > 0) return fail(TG_ERR_UNSUPPORTED, "a NonlinearConfigSpring has a force but no potential energy (as in the reference): no stiffness to take modes of");
#if defined(TG_PROFILE)
    if (rc == TG_SUCCESS) return fail(TG_ERR_UNSUPPORTED, "the profiling build has no normal-modes kernel");
#endif
    return rc;
}

// what both entry points check before a device is touched; the mask the kernel gets (kinematic configs cleared) and n_free
static int modes_check(tg_batch *b, const double *q, const int32_t *free_host, double rcond, int32_t max_sweeps, const double *omega2, const double *modes,
                       int32_t geo[4], int &n_free) {
    if (!b || !q || !omega2 || !modes) return fail(TG_ERR_INVALID, "null argument");
    if (!(rcond >= 0.0)) return fail(TG_ERR_INVALID, "rcond must not be negative");
    if (max_sweeps < 1) return fail(TG_ERR_INVALID, "max_sweeps must be at least 1");
    const int nq = b->sys->H.p.nq, nd = b->sys->H.p.nd;
    if (free_host) for (int k = nd; k < nq; k++) if (free_host[k]) return fail(TG_ERR_INVALID, "a kinematic config cannot be free: its motion is prescribed");
    if (int rc = tg_system_normal_modes_lds(b->sys, geo)) return rc;
    b->modes_mask.assign((size_t)nq, 0);
    n_free = 0;
    for (int k = 0; k < nd; k++) if (!free_host || free_host[k]) { b->modes_mask[k] = 1; n_free++; }
    return TG_SUCCESS;
}

static int modes_launch(tg_batch *b, const int32_t geo[4], int n_free, const double *q_dev, const double *mu_dev, double rcond, int32_t max_sweeps,
                        double *omega2, double *modes, int32_t *count, int32_t *rank, double *mu_out, double *residual, int32_t *sweeps, int32_t *status) {
    tg::RunArgs A;
    int grid;
    if (int rc = pose_prepare(b, tg::MODE_MODES, 1.0, max_sweeps, sweeps, status, A, grid)) return rc;
    const size_t nq = b->P.nq;
    HIP_TRY(b->modes_ints.ensure(nq + 4 * (size_t)b->batch));
    if (nq) HIP_TRY(hipMemcpyAsync(b->modes_ints.get(), b->modes_mask.data(), nq * sizeof(int), hipMemcpyHostToDevice, b->stream));
    tg::ModesArgs J{};
    tg::modes_layout(b->P.lds_per_team, b->P.nq, b->P.nc, J);
    J.free_mask = b->modes_ints.get(); J.q0 = q_dev; J.mu_in = mu_dev; J.q = nullptr; J.mu = mu_out; J.omega2 = omega2; J.modes = modes;
    J.residual = residual; J.count = count; J.rank = rank; J.rcond = rcond; J.n_free = n_free; J.max_sweeps = max_sweeps;
    const bool par = b->par_rows > 0;
    int rc = tg_detail::launch_modes(b->sys->team, launch_springs(b), par, b->d_prog.get(), A, J,
                                     tg::ParTable{par ? b->par_dev.get() : nullptr, par ? b->par_group : 1, par ? b->par_stride : 0}, grid,
                                     (size_t)geo[2], b->stream);
    if (rc == TG_SUCCESS && hipGetLastError() != hipSuccess) rc = fail(TG_ERR_HIP, "kernel launch failed");
    if (rc == TG_SUCCESS) b->launched[par][0].add(tg::MODE_MODES);
    return rc;
}

int tg_batch_normal_modes_device(tg_batch *b, const double *q_dev, const double *mu_dev, const int32_t *free_host, double rcond, int32_t max_sweeps,
                                 double *omega2_out_dev, double *modes_out_dev, int32_t *count_out_dev, int32_t *rank_out_dev, double *mu_out_dev,
                                 double *residual_out_dev, int32_t *sweeps_out_dev, int32_t *status_out_dev) {
    int32_t geo[4];
    int n_free;
    if (int rc = modes_check(b, q_dev, free_host, rcond, max_sweeps, omega2_out_dev, modes_out_dev, geo, n_free)) return rc;
    return modes_launch(b, geo, n_free, q_dev, mu_dev, rcond, max_sweeps, omega2_out_dev, modes_out_dev, count_out_dev, rank_out_dev, mu_out_dev,
                        residual_out_dev, sweeps_out_dev, status_out_dev);
}

int tg_batch_normal_modes(tg_batch *b, const double *q_host, const double *mu_host, const int32_t *free_host, double rcond, int32_t max_sweeps,
                          double *omega2_out, double *modes_out, int32_t *count_out, int32_t *rank_out, double *mu_out, double *residual_out,
                          int32_t *sweeps_out, int32_t *status_out) {
    int32_t geo[4];
    int n_free;
    if (int rc = modes_check(b, q_host, free_host, rcond, max_sweeps, omega2_out, modes_out, geo, n_free)) return rc;
    HIP_TRY(hipSetDevice(b->device));
    const size_t B = (size_t)b->batch, nq = b->P.nq, nc = b->P.nc, nF = (size_t)n_free;
    HIP_TRY(b->modes_stage.ensure(B * (nq + 2 * nc + nF + nF * nq + 1)));
    HIP_TRY(b->modes_ints.ensure(nq + 4 * B));
    double *q = b->modes_stage.get(), *mu_in = q + B * nq, *o2 = mu_in + B * nc, *md = o2 + B * nF, *mu = md + B * nF * nq, *res = mu + B * nc;
    int *count = b->modes_ints.get() + nq, *rank = count + B, *sweeps = rank + B, *status = sweeps + B;
    HIP_TRY(hipMemcpyAsync(q, q_host, B * nq * sizeof(double), hipMemcpyHostToDevice, b->stream));
    if (mu_host && nc) HIP_TRY(hipMemcpyAsync(mu_in, mu_host, B * nc * sizeof(double), hipMemcpyHostToDevice, b->stream));
    if (int rc = modes_launch(b, geo, n_free, q, mu_host && nc ? mu_in : nullptr, rcond, max_sweeps, o2, md, count, rank, mu, res, sweeps, status)) return rc;
    if (nF) HIP_TRY(hipMemcpyAsync(omega2_out, o2, B * nF * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (nF && nq) HIP_TRY(hipMemcpyAsync(modes_out, md, B * nF * nq * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (mu_out && nc) HIP_TRY(hipMemcpyAsync(mu_out, mu, B * nc * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (residual_out) HIP_TRY(hipMemcpyAsync(residual_out, res, B * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (count_out) HIP_TRY(hipMemcpyAsync(count_out, count, B * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    if (rank_out) HIP_TRY(hipMemcpyAsync(rank_out, rank, B * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    if (sweeps_out) HIP_TRY(hipMemcpyAsync(sweeps_out, sweeps, B * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    if (status_out) HIP_TRY(hipMemcpyAsync(status_out, status, B * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return TG_SUCCESS;
}

// ---- batched static response (mvi_response.hpp): one team per pose, one launch

/* Team size, doubles of LDS per team and bytes of LDS per workgroup of the static-response kernel for this system and these sizes
 * of a launch (out[0..2]; out[3] 0): the rollout slice plus the image, W, the pseudo-inverse, K_r, a work area and the two column
 * blocks X and G [n_free][n_drive (+ n_free with the compliance)], q0, V_q, V, the least-squares scratch, the free configs' list, the
 * identity index, the row scales and the free configs' places (mvi_response.hpp: response_layout).  TG_ERR_UNSUPPORTED, with out filled,
 * above the 160 KiB a workgroup can have, for a system with a NonlinearConfigSpring and in the profiling build. */
int tg_system_static_response_lds(const tg_system *sys, int32_t n_free, int32_t n_drive, int32_t with_compliance, int32_t out[4]) {
    if (!sys || !out) return fail(TG_ERR_INVALID, "null argument");
    const int nq = sys->H.p.nq;
    if (n_free < 0 || n_drive < 0 || n_free > nq || n_drive > nq - n_free) return fail(TG_ERR_INVALID, "n_free configs free and n_drive of the others driven: more than the system has");
    tg::ResponseArgs J{};
    tg::response_layout(sys->H.p.lds_per_team, nq, sys->H.p.nc, n_free, n_drive, with_compliance != 0, J);
    const int rc = pose_lds(sys, J.lds_per_team, "system too large for the LDS-resident static-response kernel", out);
    if (sys->H.p.n_ncs > 0) return fail(TG_ERR_UNSUPPORTED, "a NonlinearConfigSpring has a force but no potential energy (as in the reference): no stiffness to respond with");
#if defined(TG_PROFILE)
    if (rc == TG_SUCCESS) return fail(TG_ERR_UNSUPPORTED, "the profiling build has no static-response kernel");
#endif
    return rc;
}

// what both entry points check before a device is touched; the mask and the drive list the kernel gets, and n_free
static int response_check(tg_batch *b, const double *q, const int32_t *free_host, int32_t n_drive, const int32_t *drive_host, int32_t with_compliance,
                          double rcond, const double *dq, const double *dmu, const double *compliance, const double *reaction, int32_t geo[4], int &n_free) {
    if (!b || !q) return fail(TG_ERR_INVALID, "null argument");
    if (!(rcond >= 0.0)) return fail(TG_ERR_INVALID, "rcond must not be negative");
    if (n_drive < 0 || (n_drive > 0 && (!drive_host || !dq || !dmu))) return fail(TG_ERR_INVALID, "n_drive configs driven: drive, dq and dmu are needed");
    if (with_compliance && (!compliance || !reaction)) return fail(TG_ERR_INVALID, "null argument");
    if (n_drive == 0 && !with_compliance) return fail(TG_ERR_INVALID, "nothing to compute: no config driven and no compliance asked");
    const int nq = b->sys->H.p.nq;
    b->response_mask.assign((size_t)nq, 0);
    n_free = 0;
    for (int k = 0; k < nq; k++) if (!free_host || free_host[k]) { b->response_mask[k] = 1; n_free++; }
    for (int j = 0; j < n_drive; j++) {
        const int k = drive_host[j];
        if (k < 0 || k >= nq) return fail(TG_ERR_INVALID, "a driven config is out of range");
        if (b->response_mask[k]) return fail(TG_ERR_INVALID, "a driven config is free: only a held config can be driven");
        for (int i = 0; i < j; i++) if (drive_host[i] == k) return fail(TG_ERR_INVALID, "a config is driven twice");
    }
    if (int rc = tg_system_static_response_lds(b->sys, n_free, n_drive, with_compliance, geo)) return rc;
    b->response_mask.insert(b->response_mask.end(), drive_host, drive_host + n_drive);
    return TG_SUCCESS;
}

static int response_launch(tg_batch *b, const int32_t geo[4], int n_free, int n_drive, bool loads, const double *q_dev, const double *mu_dev, double rcond,
                           double *dq, double *dmu, double *compliance, double *reaction, int32_t *rank, double *mu_out, double *residual, double *defect,
                           int32_t *status) {
    tg::RunArgs A;
    int grid;
    if (int rc = pose_prepare(b, tg::MODE_RESPONSE, 1.0, 0, nullptr, status, A, grid)) return rc;
    const size_t nq = b->P.nq, words = nq + (size_t)n_drive;
    HIP_TRY(b->response_ints.ensure(words + 2 * (size_t)b->batch));
    if (words) HIP_TRY(hipMemcpyAsync(b->response_ints.get(), b->response_mask.data(), words * sizeof(int), hipMemcpyHostToDevice, b->stream));
    tg::ResponseArgs J{};
    tg::response_layout(b->P.lds_per_team, b->P.nq, b->P.nc, n_free, n_drive, loads, J);
    J.free_mask = b->response_ints.get(); J.drive = b->response_ints.get() + nq; J.q0 = q_dev; J.mu_in = mu_dev; J.q = nullptr; J.mu = mu_out;
    J.dq = dq; J.dmu = dmu; J.compliance = compliance; J.reaction = reaction; J.residual = residual; J.defect = defect; J.rank = rank;
    J.rcond = rcond; J.n_free = n_free; J.n_drive = n_drive; J.loads = loads ? 1 : 0;
    const bool par = b->par_rows > 0;
    int rc = tg_detail::launch_response(b->sys->team, launch_springs(b), par, b->d_prog.get(), A, J,
                                        tg::ParTable{par ? b->par_dev.get() : nullptr, par ? b->par_group : 1, par ? b->par_stride : 0}, grid,
                                        (size_t)geo[2], b->stream);
    if (rc == TG_SUCCESS && hipGetLastError() != hipSuccess) rc = fail(TG_ERR_HIP, "kernel launch failed");
    if (rc == TG_SUCCESS) b->launched[par][0].add(tg::MODE_RESPONSE);
    return rc;
}

int tg_batch_static_response_device(tg_batch *b, const double *q_dev, const double *mu_dev, const int32_t *free_host, int32_t n_drive,
                                    const int32_t *drive_host, int32_t with_compliance, double rcond, double *dq_out_dev, double *dmu_out_dev,
                                    double *compliance_out_dev, double *reaction_out_dev, int32_t *rank_out_dev, double *mu_out_dev,
                                    double *residual_out_dev, double *defect_out_dev, int32_t *status_out_dev) {
    int32_t geo[4];
    int n_free;
    if (int rc = response_check(b, q_dev, free_host, n_drive, drive_host, with_compliance, rcond, dq_out_dev, dmu_out_dev, compliance_out_dev,
                                reaction_out_dev, geo, n_free)) return rc;
    return response_launch(b, geo, n_free, n_drive, with_compliance != 0, q_dev, mu_dev, rcond, dq_out_dev, dmu_out_dev, compliance_out_dev,
                           reaction_out_dev, rank_out_dev, mu_out_dev, residual_out_dev, defect_out_dev, status_out_dev);
}

int tg_batch_static_response(tg_batch *b, const double *q_host, const double *mu_host, const int32_t *free_host, int32_t n_drive,
                             const int32_t *drive_host, int32_t with_compliance, double rcond, double *dq_out, double *dmu_out, double *compliance_out,
                             double *reaction_out, int32_t *rank_out, double *mu_out, double *residual_out, double *defect_out, int32_t *status_out) {
    int32_t geo[4];
    int n_free;
    if (int rc = response_check(b, q_host, free_host, n_drive, drive_host, with_compliance, rcond, dq_out, dmu_out, compliance_out, reaction_out, geo,
                                n_free)) return rc;
    HIP_TRY(hipSetDevice(b->device));
    const size_t B = (size_t)b->batch, nq = b->P.nq, nc = b->P.nc, nD = (size_t)n_drive, words = nq + nD;
    const size_t load = with_compliance ? nq * (nq + nc) : 0;
    HIP_TRY(b->response_stage.ensure(B * (nq + 2 * nc + nD * (nq + nc) + load + 2)));
    HIP_TRY(b->response_ints.ensure(words + 2 * B));
    double *q = b->response_stage.get(), *mu_in = q + B * nq, *dq = mu_in + B * nc, *dmu = dq + B * nD * nq, *cm = dmu + B * nD * nc;
    double *re = cm + (with_compliance ? B * nq * nq : 0), *mu = cm + B * load, *res = mu + B * nc, *def = res + B;
    int *rank = b->response_ints.get() + words, *status = rank + B;
    HIP_TRY(hipMemcpyAsync(q, q_host, B * nq * sizeof(double), hipMemcpyHostToDevice, b->stream));
    if (mu_host && nc) HIP_TRY(hipMemcpyAsync(mu_in, mu_host, B * nc * sizeof(double), hipMemcpyHostToDevice, b->stream));
    if (int rc = response_launch(b, geo, n_free, n_drive, with_compliance != 0, q, mu_host && nc ? mu_in : nullptr, rcond, dq, dmu, cm, re, rank, mu, res,
                                 def, status)) return rc;
    if (nD && nq) HIP_TRY(hipMemcpyAsync(dq_out, dq, B * nD * nq * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (nD && nc) HIP_TRY(hipMemcpyAsync(dmu_out, dmu, B * nD * nc * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (with_compliance && nq) HIP_TRY(hipMemcpyAsync(compliance_out, cm, B * nq * nq * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (with_compliance && nq && nc) HIP_TRY(hipMemcpyAsync(reaction_out, re, B * nq * nc * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (mu_out && nc) HIP_TRY(hipMemcpyAsync(mu_out, mu, B * nc * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (residual_out) HIP_TRY(hipMemcpyAsync(residual_out, res, B * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (defect_out) HIP_TRY(hipMemcpyAsync(defect_out, def, B * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (rank_out) HIP_TRY(hipMemcpyAsync(rank_out, rank, B * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    if (status_out) HIP_TRY(hipMemcpyAsync(status_out, status, B * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return TG_SUCCESS;
}

// ---- batched inverse dynamics (mvi_inverse.hpp): one team per (trajectory, step), one launch

/* Team size, doubles of LDS per team and bytes of LDS per workgroup of the inverse-dynamics kernel for this system (out[0..2];
 * out[3] 0): the rollout slice plus the image [m][m + 1], m = nd + nu + nc, p_k [nd] and the solver's row scales [m]
 * (mvi_inverse.hpp).  TG_ERR_UNSUPPORTED, with out filled, above the 160 KiB a workgroup can have, and in the profiling build. */
int tg_system_inverse_dynamics_lds(const tg_system *sys, int32_t out[4]) {
    if (!sys || !out) return fail(TG_ERR_INVALID, "null argument");
    tg::InverseArgs J{};
    tg::inverse_layout(sys->H.p.lds_per_team, sys->H.p.nd, sys->H.p.nu, sys->H.p.nc, J);
    const int rc = pose_lds(sys, J.lds_per_team, "system too large for the LDS-resident inverse-dynamics kernel", out);
#if defined(TG_PROFILE)
    if (rc == TG_SUCCESS) return fail(TG_ERR_UNSUPPORTED, "the profiling build has no inverse-dynamics kernel");
#endif
    return rc;
}

/* The same for the kernel whose solve is the rank-revealing least squares (tg_batch_inverse_dynamics_lsq): the stacked block
 * [nd + n][n + 1], n = nu + nc, in place of the image and the solver's 4 n doubles in place of the row scales (inverse_lsq_layout). */
int tg_system_inverse_dynamics_lsq_lds(const tg_system *sys, int32_t out[4]) {
    if (!sys || !out) return fail(TG_ERR_INVALID, "null argument");
    tg::InverseArgs J{};
    tg::inverse_lsq_layout(sys->H.p.lds_per_team, sys->H.p.nd, sys->H.p.nu, sys->H.p.nc, J);
    const int rc = pose_lds(sys, J.lds_per_team, "system too large for the LDS-resident inverse-dynamics kernel", out);
#if defined(TG_PROFILE)
    if (rc == TG_SUCCESS) return fail(TG_ERR_UNSUPPORTED, "the profiling build has no inverse-dynamics kernel");
#endif
    return rc;
}

/* ... and for the kernel whose solve is the bounded least squares (tg_batch_inverse_dynamics_bounded): the pristine stacked block, and
 * in place of the 4 n doubles the solver's scratch, (nd + n)(n + 1) + 9 n doubles (inverse_bounded_layout). */
int tg_system_inverse_dynamics_bounded_lds(const tg_system *sys, int32_t out[4]) {
    if (!sys || !out) return fail(TG_ERR_INVALID, "null argument");
    tg::InverseArgs J{};
    tg::inverse_bounded_layout(sys->H.p.lds_per_team, sys->H.p.nd, sys->H.p.nu, sys->H.p.nc, J);
    const int rc = pose_lds(sys, J.lds_per_team, "system too large for the LDS-resident inverse-dynamics kernel", out);
#if defined(TG_PROFILE)
    if (rc == TG_SUCCESS) return fail(TG_ERR_UNSUPPORTED, "the profiling build has no inverse-dynamics kernel");
#endif
    return rc;
}

// the box of the _bounded entry points and their two additional outputs; lo, hi: host arrays in the host variants (checked entry by
// entry), device arrays in the _device variants (their contents are the caller's word)
struct BoundedArgs {
    const double *lo, *hi;
    int32_t bound_rows;
    int32_t *active, *solves;
};

// what the _bounded entry points refuse on top of the _lsq siblings' refusals (after those: b is not null); host: lo, hi can be read
static int bounded_check(const tg_batch *b, double ridge, const BoundedArgs &box, bool host) {
    const int n = b->P.nu + b->P.nc;
    if (n > b->P.nd && ridge == 0.0)
        return fail(TG_ERR_INVALID, "more unknowns (nu + nc) than dynamic configs: the bounded problem is not strictly convex without a ridge");
    if (box.bound_rows != 1 && box.bound_rows != b->batch) return fail(TG_ERR_INVALID, "bound_rows must be 1 or the batch size");
    if (n > 0 && (!box.lo || !box.hi)) return fail(TG_ERR_INVALID, "null lo or hi");
    if (host) for (size_t i = 0; i < (size_t)box.bound_rows * n; i++) {
        if (std::isnan(box.lo[i]) || std::isnan(box.hi[i])) return fail(TG_ERR_INVALID, "a bound is not a number");
        if (box.lo[i] > box.hi[i]) return fail(TG_ERR_INVALID, "a lower bound above its upper bound");
        if (box.lo[i] == INFINITY || box.hi[i] == -INFINITY) return fail(TG_ERR_INVALID, "a bound that no finite value meets");
    }
    return TG_SUCCESS;
}

// what the least-squares entry points refuse on top of their siblings' refusals
static int rcond_check(double rcond) {
    if (!(rcond >= 0.0) || !(rcond < 1.0)) return fail(TG_ERR_INVALID, "rcond must be finite, not negative and below 1");
    return TG_SUCCESS;
}

// what both entry points refuse, decided on the host before anything is staged or launched (lsq: n > nd needs no ridge)
static int inverse_check(const tg_batch *b, int32_t n_steps, double dt, const double *Q, double ridge, bool lsq = false) {
    if (!b || !Q) return fail(TG_ERR_INVALID, "null argument");
    if (!(ridge >= 0.0) || !std::isfinite(ridge)) return fail(TG_ERR_INVALID, "ridge must be finite and not negative");
    if (n_steps < 1) return fail(TG_ERR_INVALID, "n_steps must be at least 1");
    if (b->dt_by_trajectory) return fail(TG_ERR_INVALID, "a by-trajectory step-size list takes one-step launches only");
    if (!b->dt_host.empty() && (size_t)n_steps > b->dt_host.size()) return fail(TG_ERR_INVALID, "path longer than the step-size list");
    if (b->dt_host.empty() && (dt == 0.0 || !std::isfinite(dt))) return fail(TG_ERR_INVALID, "step size must be finite and not zero");
    if (!lsq && b->P.nu + b->P.nc > b->P.nd && ridge == 0.0)
        return fail(TG_ERR_INVALID, "more unknowns (nu + nc) than dynamic configs: the least-squares image is singular without a ridge");
    return TG_SUCCESS;
}

// both device entry points: lsq selects the least-squares kernel, its layout, rcond and the rank words
static int inverse_device(tg_batch *b, int32_t n_steps, double dt, const double *Q_dev, uint64_t q_row_stride_doubles, const double *p0_dev,
                          double ridge, bool lsq, double rcond, double *U_dev, double *LAM_dev, double *P_dev, double *RHO_dev, double *H_dev,
                          int32_t *rank_dev, int32_t *status_dev, const BoundedArgs *box = nullptr, bool box_checked = false) {
    if (lsq) if (int rc = rcond_check(rcond)) return rc;
    if (int rc = inverse_check(b, n_steps, dt, Q_dev, ridge, lsq)) return rc;
    if (q_row_stride_doubles < (uint64_t)b->P.nq) return fail(TG_ERR_INVALID, "row stride of Q shorter than a configuration");
    if (box && !box_checked) if (int rc = bounded_check(b, ridge, *box, false)) return rc;
    int32_t geo[4];
    if (int rc = box ? tg_system_inverse_dynamics_bounded_lds(b->sys, geo)
                     : (lsq ? tg_system_inverse_dynamics_lsq_lds(b->sys, geo) : tg_system_inverse_dynamics_lds(b->sys, geo))) return rc;
    const long long teams = (long long)b->batch * n_steps, per_block = 64 / b->sys->team;
    if ((teams + per_block - 1) / per_block > 0x7fffffffLL) return fail(TG_ERR_INVALID, "too many steps for one launch");
    HIP_TRY(hipSetDevice(b->device));
    // the path is an argument of the call: nothing of the integrator (q1, q2, p, lambda1, status, times) is read or written, and a
    // loaded specialised library has no say; a parameter table has (masses, gravity and damping move momenta and residuals)
    tg::RunArgs A = base_args(b, tg::MODE_INVERSE);
    A.q1 = A.q2 = A.p1 = A.p2 = A.lam = A.u1 = nullptr;
    A.iters = A.status = nullptr;
    A.n_steps = n_steps; A.dt = dt;
    tg::InverseArgs J{};
    if (box) tg::inverse_bounded_layout(b->P.lds_per_team, b->P.nd, b->P.nu, b->P.nc, J);
    else if (lsq) tg::inverse_lsq_layout(b->P.lds_per_team, b->P.nd, b->P.nu, b->P.nc, J);
    else tg::inverse_layout(b->P.lds_per_team, b->P.nd, b->P.nu, b->P.nc, J);
    if (box) {
        J.lo = box->lo; J.hi = box->hi; J.bound_rows = box->bound_rows; J.active = box->active; J.solves = box->solves;
        J.max_solves = tg::bvls_max_solves(b->P.nu + b->P.nc);
    }
    J.rcond = rcond; J.rank = rank_dev;
    J.Q = Q_dev; J.p0 = p0_dev; J.dt_steps = b->dt_host.empty() ? nullptr : b->dt_dev.get();
    J.U = U_dev; J.LAM = LAM_dev; J.P = P_dev; J.RHO = RHO_dev; J.H = H_dev; J.status = status_dev;
    J.dt = dt; J.ridge = ridge; J.q_stride = (size_t)q_row_stride_doubles; J.n_steps = n_steps;
    const bool par = b->par_rows > 0;
    int rc = tg_detail::launch_inverse(b->sys->team, launch_springs(b), par, box ? 2 : (lsq ? 1 : 0), b->d_prog.get(), A, J,
                                       tg::ParTable{par ? b->par_dev.get() : nullptr, par ? b->par_group : 1, par ? b->par_stride : 0},
                                       (int)((teams + per_block - 1) / per_block), (size_t)geo[2], b->stream);
    if (rc == TG_SUCCESS && hipGetLastError() != hipSuccess) rc = fail(TG_ERR_HIP, "kernel launch failed");
    if (rc == TG_SUCCESS) b->launched[par][0].add(tg::MODE_INVERSE);      // a refused launch (the profiling build) is not counted
    return rc;
}

int tg_batch_inverse_dynamics_device(tg_batch *b, int32_t n_steps, double dt, const double *Q_dev, uint64_t q_row_stride_doubles,
                                     const double *p0_dev, double ridge, double *U_dev, double *LAM_dev, double *P_dev, double *RHO_dev,
                                     double *H_dev, int32_t *status_dev) {
    return inverse_device(b, n_steps, dt, Q_dev, q_row_stride_doubles, p0_dev, ridge, false, 0.0, U_dev, LAM_dev, P_dev, RHO_dev, H_dev, nullptr, status_dev);
}

int tg_batch_inverse_dynamics_lsq_device(tg_batch *b, int32_t n_steps, double dt, const double *Q_dev, uint64_t q_row_stride_doubles,
                                         const double *p0_dev, double ridge, double rcond, double *U_dev, double *LAM_dev, double *P_dev,
                                         double *RHO_dev, double *H_dev, int32_t *rank_dev, int32_t *status_dev) {
    return inverse_device(b, n_steps, dt, Q_dev, q_row_stride_doubles, p0_dev, ridge, true, rcond, U_dev, LAM_dev, P_dev, RHO_dev, H_dev, rank_dev, status_dev);
}

// both host entry points
static int inverse_host(tg_batch *b, int32_t n_steps, double dt, const double *Q_host, const double *p0_host, double ridge, bool lsq, double rcond,
                        double *U, double *LAM, double *P, double *RHO, double *H, int32_t *rank, int32_t *status, const BoundedArgs *box = nullptr) {
    if (lsq) if (int rc = rcond_check(rcond)) return rc;
    if (int rc = inverse_check(b, n_steps, dt, Q_host, ridge, lsq)) return rc;
    if (box) if (int rc = bounded_check(b, ridge, *box, true)) return rc;
    int32_t geo[4];
    if (int rc = box ? tg_system_inverse_dynamics_bounded_lds(b->sys, geo)
                     : (lsq ? tg_system_inverse_dynamics_lsq_lds(b->sys, geo) : tg_system_inverse_dynamics_lds(b->sys, geo))) return rc;
    HIP_TRY(hipSetDevice(b->device));
    // staging of this call alone (its size follows n_steps): Q, p0 in; U, LAM, P, RHO, H and the status words out
    const size_t B = (size_t)b->batch, N = (size_t)n_steps, nq = b->P.nq, nd = b->P.nd, nu = b->P.nu, nc = b->P.nc;
    const size_t n_q = B * (N + 1) * nq, n_p0 = B * nd, n_u = B * N * nu, n_l = B * N * nc, n_p = B * (N + 1) * nd, n_r = B * N * nd;
    tg::DeviceBuffer<double> stage;
    tg::DeviceBuffer<int> words;
    // (the box and its outputs behind them: lo and hi [bound_rows][n]; solves, then active [B][N][n])
    const size_t n_box = box ? (size_t)box->bound_rows * (nu + nc) : 0, n_act = box ? B * N * (nu + nc) : 0;
    HIP_TRY(stage.ensure(n_q + n_p0 + n_u + n_l + n_p + n_r + n_l + 2 * n_box));
    HIP_TRY(words.ensure(2 * B * N + (box ? B * N + n_act : 0)));      // (status, then rank)
    double *q = stage.get(), *p0 = q + n_q, *u = p0 + n_p0, *lam = u + n_u, *p = lam + n_l, *rho = p + n_p, *h = rho + n_r, *lo = h + n_l, *hi = lo + n_box;
    HIP_TRY(hipMemcpyAsync(q, Q_host, n_q * sizeof(double), hipMemcpyHostToDevice, b->stream));
    if (p0_host && n_p0) HIP_TRY(hipMemcpyAsync(p0, p0_host, n_p0 * sizeof(double), hipMemcpyHostToDevice, b->stream));
    BoundedArgs dev{};
    if (box) {
        dev = BoundedArgs{lo, hi, box->bound_rows, box->active ? words.get() + 3 * B * N : nullptr, box->solves ? words.get() + 2 * B * N : nullptr};
        if (n_box) HIP_TRY(hipMemcpyAsync(lo, box->lo, n_box * sizeof(double), hipMemcpyHostToDevice, b->stream));
        if (n_box) HIP_TRY(hipMemcpyAsync(hi, box->hi, n_box * sizeof(double), hipMemcpyHostToDevice, b->stream));
    }
    int rc = inverse_device(b, n_steps, dt, q, nq, p0_host ? p0 : nullptr, ridge, lsq, rcond, u, lam, p, rho, h, lsq ? words.get() + B * N : nullptr, words.get(),
                            box ? &dev : nullptr, true);
    auto back = [&](void *dst, const void *src, size_t bytes) {
        if (rc == TG_SUCCESS && dst && bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, b->stream) != hipSuccess)
            rc = fail(TG_ERR_HIP, "copy of the results failed");
    };
    back(U, u, n_u * sizeof(double)); back(LAM, lam, n_l * sizeof(double)); back(P, p, n_p * sizeof(double));
    back(RHO, rho, n_r * sizeof(double)); back(H, h, n_l * sizeof(double)); back(status, words.get(), B * N * sizeof(int));
    if (lsq) back(rank, words.get() + B * N, B * N * sizeof(int));
    if (box) { back(box->solves, words.get() + 2 * B * N, B * N * sizeof(int)); back(box->active, words.get() + 3 * B * N, n_act * sizeof(int)); }
    if (hipStreamSynchronize(b->stream) != hipSuccess && rc == TG_SUCCESS) rc = fail(TG_ERR_HIP, "hipStreamSynchronize failed");      // (before the staging is freed)
    return rc;
}

int tg_batch_inverse_dynamics(tg_batch *b, int32_t n_steps, double dt, const double *Q_host, const double *p0_host, double ridge,
                              double *U, double *LAM, double *P, double *RHO, double *H, int32_t *status) {
    return inverse_host(b, n_steps, dt, Q_host, p0_host, ridge, false, 0.0, U, LAM, P, RHO, H, nullptr, status);
}

int tg_batch_inverse_dynamics_lsq(tg_batch *b, int32_t n_steps, double dt, const double *Q_host, const double *p0_host, double ridge, double rcond,
                                  double *U, double *LAM, double *P, double *RHO, double *H, int32_t *rank, int32_t *status) {
    return inverse_host(b, n_steps, dt, Q_host, p0_host, ridge, true, rcond, U, LAM, P, RHO, H, rank, status);
}

int tg_batch_inverse_dynamics_bounded(tg_batch *b, int32_t n_steps, double dt, const double *Q_host, const double *p0_host, double ridge, double rcond,
                                      const double *lo_host, const double *hi_host, int32_t bound_rows, double *U, double *LAM, double *P, double *RHO,
                                      double *H, int32_t *active, int32_t *solves, int32_t *rank, int32_t *status) {
    const BoundedArgs box{lo_host, hi_host, bound_rows, active, solves};
    return inverse_host(b, n_steps, dt, Q_host, p0_host, ridge, true, rcond, U, LAM, P, RHO, H, rank, status, &box);
}

int tg_batch_inverse_dynamics_bounded_device(tg_batch *b, int32_t n_steps, double dt, const double *Q_dev, uint64_t q_row_stride_doubles,
                                             const double *p0_dev, double ridge, double rcond, const double *lo_dev, const double *hi_dev,
                                             int32_t bound_rows, double *U_dev, double *LAM_dev, double *P_dev, double *RHO_dev, double *H_dev,
                                             int32_t *active_dev, int32_t *solves_dev, int32_t *rank_dev, int32_t *status_dev) {
    const BoundedArgs box{lo_dev, hi_dev, bound_rows, active_dev, solves_dev};
    return inverse_device(b, n_steps, dt, Q_dev, q_row_stride_doubles, p0_dev, ridge, true, rcond, U_dev, LAM_dev, P_dev, RHO_dev, H_dev, rank_dev,
                          status_dev, &box);
}

// ---- batched frame kinematics (mvi_frames.hpp): one team per state, one launch

/* Team size, doubles of LDS per team and bytes of LDS per workgroup of the frame-kinematics kernel for this system (out[0..2];
 * out[3] 0): the rollout slice plus one pass of staged frames, kFramePass poses [12] and world twists [6], whatever the selection
 * (mvi_frames.hpp).  TG_ERR_UNSUPPORTED, with out filled, above the 160 KiB a workgroup can have, and in the profiling build. */
int tg_system_frame_kinematics_lds(const tg_system *sys, int32_t out[4]) {
    if (!sys || !out) return fail(TG_ERR_INVALID, "null argument");
    tg::FrameArgs J{};
    tg::frames_layout(sys->H.p.lds_per_team, J);
    const int rc = pose_lds(sys, J.lds_per_team, "system too large for the LDS-resident frame-kinematics kernel", out);
#if defined(TG_PROFILE)
    if (rc == TG_SUCCESS) return fail(TG_ERR_UNSUPPORTED, "the profiling build has no frame-kinematics kernel");
#endif
    return rc;
}

// what both entry points refuse, decided on the host before a device is touched: first what the arguments alone show, then what
// needs the system (the strides are nq for the host variant)
static int frames_check(const tg_batch *b, int32_t n_states, const double *Q, const double *dQ, uint64_t q_stride, uint64_t dq_stride,
                        int32_t n_frames, const int32_t *frames, const double *G, const double *VB, const double *JP, const double *JB) {
    if (n_states < 1) return fail(TG_ERR_INVALID, "n_states must be at least 1");
    if (!Q) return fail(TG_ERR_INVALID, "null Q");
    if (n_frames < 1 || !frames) return fail(TG_ERR_INVALID, "no frames selected");
    if (VB && !dQ) return fail(TG_ERR_INVALID, "VB without dQ");
    if (!G && !VB && !JP && !JB) return fail(TG_ERR_INVALID, "no output asked for");
    if (!b || !b->sys) return fail(TG_ERR_INVALID, "null argument");
    const int32_t nfr = (int32_t)b->sys->H.frame_anchor.size();
    for (int32_t s = 0; s < n_frames; s++)
        if (frames[s] < 0 || frames[s] >= nfr) return fail(TG_ERR_INVALID, "frame index outside the system");
    if (q_stride < (uint64_t)b->sys->H.p.nq) return fail(TG_ERR_INVALID, "row stride of Q shorter than a configuration");
    if (dQ && dq_stride < (uint64_t)b->sys->H.p.nq) return fail(TG_ERR_INVALID, "row stride of dQ shorter than a configuration");
    return TG_SUCCESS;
}

int tg_batch_frame_kinematics_device(tg_batch *b, int32_t n_states, const double *Q_dev, uint64_t q_row_stride_doubles, const double *dQ_dev,
                                     uint64_t dq_row_stride_doubles, int32_t n_frames, const int32_t *frames_host, double *G_dev,
                                     double *VB_dev, double *JP_dev, double *JB_dev) {
    if (int rc = frames_check(b, n_states, Q_dev, dQ_dev, q_row_stride_doubles, dq_row_stride_doubles, n_frames, frames_host, G_dev, VB_dev, JP_dev, JB_dev)) return rc;
    int32_t geo[4];
    if (int rc = tg_system_frame_kinematics_lds(b->sys, geo)) return rc;
    const long long teams = (long long)b->batch * n_states, per_block = 64 / b->sys->team;
    if ((teams + per_block - 1) / per_block > 0x7fffffffLL) return fail(TG_ERR_INVALID, "too many states for one launch");
    HIP_TRY(hipSetDevice(b->device));
    // the cached table serves while the selection stays; a new selection waits for the launches that read the old one (once), then
    // overwrites it, on a larger buffer only if it grew
    if (!b->frames_tab || b->frames_sel.size() != (size_t)n_frames || !std::equal(b->frames_sel.begin(), b->frames_sel.end(), frames_host)) {
        HIP_TRY(hipStreamSynchronize(b->stream));
        b->frames_sel.clear();
        tg::frames_table(b->sys->H, n_frames, frames_host, b->frames_tab_host, b->frames_off_host);
        if (b->frames_tab_host.size() > b->frames_tab.count() || b->frames_off_host.size() > b->frames_off.count()) {
            b->frames_tab.reset(); b->frames_off.reset();
            HIP_TRY(b->frames_tab.ensure(b->frames_tab_host.size()));
            HIP_TRY(b->frames_off.ensure(b->frames_off_host.size()));
        }
        HIP_TRY(hipMemcpyAsync(b->frames_tab.get(), b->frames_tab_host.data(), b->frames_tab_host.size() * sizeof(int), hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipMemcpyAsync(b->frames_off.get(), b->frames_off_host.data(), b->frames_off_host.size() * sizeof(double), hipMemcpyHostToDevice, b->stream));
        b->frames_sel.assign(frames_host, frames_host + n_frames);
    }
    // the states are arguments of the call: nothing of the integrator (q1, q2, p, lambda1, status, times) is read or written, and
    // neither a loaded specialised library nor a parameter table has a say (poses and twists know no masses or forces)
    tg::RunArgs A = base_args(b, tg::MODE_FRAMES);
    A.q1 = A.q2 = A.p1 = A.p2 = A.lam = A.u1 = nullptr;
    A.iters = A.status = nullptr;
    A.n_steps = n_states;
    tg::FrameArgs J{};
    tg::frames_layout(b->P.lds_per_team, J);
    J.Q = Q_dev; J.dQ = dQ_dev; J.G = G_dev; J.VB = VB_dev; J.JP = JP_dev; J.JB = JB_dev;
    J.tab = b->frames_tab.get(); J.off = b->frames_off.get();
    J.q_stride = (size_t)q_row_stride_doubles; J.dq_stride = (size_t)dq_row_stride_doubles;
    J.n_states = n_states; J.n_frames = n_frames;
    LaunchTiming timed;
    if (int rc = timing_begin(b, timed)) return rc;
    int rc = tg_detail::launch_frames(b->sys->team, b->d_prog.get(), A, J, (int)((teams + per_block - 1) / per_block), (size_t)geo[2], b->stream);
    if (rc == TG_SUCCESS && hipGetLastError() != hipSuccess) rc = fail(TG_ERR_HIP, "kernel launch failed");
    if (rc == TG_SUCCESS) b->launched[0][0].add(tg::MODE_FRAMES);      // a refused launch (the profiling build) is not counted
    return timing_end(b, timed, rc);
}

int tg_batch_frame_kinematics(tg_batch *b, int32_t n_states, const double *Q_host, const double *dQ_host, int32_t n_frames,
                              const int32_t *frames_host, double *G, double *VB, double *JP, double *JB) {
    const uint64_t nq_ = b && b->sys ? (uint64_t)b->sys->H.p.nq : 0;
    if (int rc = frames_check(b, n_states, Q_host, dQ_host, nq_, nq_, n_frames, frames_host, G, VB, JP, JB)) return rc;
    int32_t geo[4];
    if (int rc = tg_system_frame_kinematics_lds(b->sys, geo)) return rc;
    HIP_TRY(hipSetDevice(b->device));
    // staging of this call alone (its size follows n_states and the selection): Q, dQ in; the outputs asked for out
    const size_t rows = (size_t)b->batch * n_states, nq = b->P.nq, F = (size_t)n_frames;
    const size_t n_q = rows * nq, n_dq = dQ_host ? n_q : 0, n_g = G ? rows * F * 12 : 0, n_vb = VB ? rows * F * 6 : 0;
    const size_t n_jp = JP ? rows * F * nq * 3 : 0, n_jb = JB ? rows * F * nq * 6 : 0;
    tg::DeviceBuffer<double> stage;
    HIP_TRY(stage.ensure(n_q + n_dq + n_g + n_vb + n_jp + n_jb));
    double *q = stage.get(), *dq = q + n_q, *g = dq + n_dq, *vb = g + n_g, *jp = vb + n_vb, *jb = jp + n_jp;
    HIP_TRY(hipMemcpyAsync(q, Q_host, n_q * sizeof(double), hipMemcpyHostToDevice, b->stream));
    if (n_dq) HIP_TRY(hipMemcpyAsync(dq, dQ_host, n_dq * sizeof(double), hipMemcpyHostToDevice, b->stream));
    int rc = tg_batch_frame_kinematics_device(b, n_states, q, nq, dQ_host ? dq : nullptr, nq, n_frames, frames_host, G ? g : nullptr,
                                              VB ? vb : nullptr, JP ? jp : nullptr, JB ? jb : nullptr);
    auto back = [&](void *dst, const void *src, size_t bytes) {
        if (rc == TG_SUCCESS && dst && bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, b->stream) != hipSuccess)
            rc = fail(TG_ERR_HIP, "copy of the results failed");
    };
    back(G, g, n_g * sizeof(double)); back(VB, vb, n_vb * sizeof(double)); back(JP, jp, n_jp * sizeof(double)); back(JB, jb, n_jb * sizeof(double));
    if (hipStreamSynchronize(b->stream) != hipSuccess && rc == TG_SUCCESS) rc = fail(TG_ERR_HIP, "hipStreamSynchronize failed");      // (before the staging is freed)
    return rc;
}

// ---- batched tape measures (mvi_tape.hpp): one team per state, one launch

/* Team size, doubles of LDS per team and bytes of LDS per workgroup of the tape-measure kernel for this system and a selection whose
 * longest measure has longest_measure_segments segments (out[0..2]; out[3] 0): the rollout slice plus kTapeStage doubles for each of
 * max(kTapePass, longest_measure_segments) staged segments (mvi_tape.hpp).  TG_ERR_UNSUPPORTED, with out filled, above the 160 KiB a
 * workgroup can have, and in the profiling build. */
int tg_system_tape_measures_lds(const tg_system *sys, int32_t longest_measure_segments, int32_t out[4]) {
    if (!sys || !out) return fail(TG_ERR_INVALID, "null argument");
    if (longest_measure_segments < 1) return fail(TG_ERR_INVALID, "a measure has at least one segment");
    tg::TapeArgs J{};
    tg::tape_layout(sys->H.p.lds_per_team, (int)std::min<int32_t>(longest_measure_segments, 1 << 24), J);
    const int rc = pose_lds(sys, J.lds_per_team, "system or measure too large for the LDS-resident tape-measure kernel", out);
#if defined(TG_PROFILE)
    if (rc == TG_SUCCESS) return fail(TG_ERR_UNSUPPORTED, "the profiling build has no tape-measure kernel");
#endif
    return rc;
}

// what both entry points refuse, decided on the host before a device is touched: first what the arguments alone show, then what
// needs the system (the strides are nq for the host variant); longest: the segments of the longest measure
static int tape_check(const tg_batch *b, int32_t n_states, const double *Q, const double *dQ, uint64_t q_stride, uint64_t dq_stride,
                      int32_t n_measures, const int32_t *start, const int32_t *frames, const double *L, const double *V, const double *LQ,
                      const double *VQ, const double *LQQ, int32_t &longest) {
    if (n_states < 1) return fail(TG_ERR_INVALID, "n_states must be at least 1");
    if (!Q) return fail(TG_ERR_INVALID, "null Q");
    if (n_measures < 1 || !start || !frames) return fail(TG_ERR_INVALID, "no measures selected");
    longest = 0;
    for (int32_t t = 0; t < n_measures; t++) {
        if (start[t] < 0 || (int64_t)start[t + 1] - start[t] < 2) return fail(TG_ERR_INVALID, "a measure needs at least two frames");
        longest = std::max(longest, start[t + 1] - start[t] - 1);
        for (int32_t i = start[t]; i + 1 < start[t + 1]; i++)
            if (frames[i] == frames[i + 1]) return fail(TG_ERR_INVALID, "two equal consecutive frames in a measure");
    }
    if ((V || VQ) && !dQ) return fail(TG_ERR_INVALID, "V or VQ without dQ");
    if (!L && !V && !LQ && !VQ && !LQQ) return fail(TG_ERR_INVALID, "no output asked for");
    if (!b || !b->sys) return fail(TG_ERR_INVALID, "null argument");
    const int32_t nfr = (int32_t)b->sys->H.frame_anchor.size();
    for (int32_t i = start[0]; i < start[n_measures]; i++)
        if (frames[i] < 0 || frames[i] >= nfr) return fail(TG_ERR_INVALID, "frame index outside the system");
    if (q_stride < (uint64_t)b->sys->H.p.nq) return fail(TG_ERR_INVALID, "row stride of Q shorter than a configuration");
    if (dQ && dq_stride < (uint64_t)b->sys->H.p.nq) return fail(TG_ERR_INVALID, "row stride of dQ shorter than a configuration");
    return TG_SUCCESS;
}

int tg_batch_tape_measures_device(tg_batch *b, int32_t n_states, const double *Q_dev, uint64_t q_row_stride_doubles, const double *dQ_dev,
                                  uint64_t dq_row_stride_doubles, int32_t n_measures, const int32_t *measure_start_host,
                                  const int32_t *frames_host, double *L_dev, double *V_dev, double *LQ_dev, double *VQ_dev, double *LQQ_dev) {
    int32_t longest = 0;
    if (int rc = tape_check(b, n_states, Q_dev, dQ_dev, q_row_stride_doubles, dq_row_stride_doubles, n_measures, measure_start_host, frames_host,
                            L_dev, V_dev, LQ_dev, VQ_dev, LQQ_dev, longest)) return rc;
    int32_t geo[4];
    if (int rc = tg_system_tape_measures_lds(b->sys, longest, geo)) return rc;
    const long long teams = (long long)b->batch * n_states, per_block = 64 / b->sys->team;
    if ((teams + per_block - 1) / per_block > 0x7fffffffLL) return fail(TG_ERR_INVALID, "too many states for one launch");
    HIP_TRY(hipSetDevice(b->device));
    // the cached table serves while the selection stays; a new selection waits for the launches that read the old one (once), then
    // overwrites it, on a larger buffer only if it grew
    const int32_t *f0 = frames_host + measure_start_host[0];
    const size_t n_fr = (size_t)(measure_start_host[n_measures] - measure_start_host[0]);
    bool same = b->tape_words && b->tape_start.size() == (size_t)n_measures + 1 && b->tape_sel.size() == n_fr && std::equal(b->tape_sel.begin(), b->tape_sel.end(), f0);
    for (int32_t t = 0; same && t <= n_measures; t++) same = b->tape_start[t] == measure_start_host[t] - measure_start_host[0];
    if (!same) {
        HIP_TRY(hipStreamSynchronize(b->stream));
        b->tape_start.clear(); b->tape_sel.clear();
        tg::tape_table(b->sys->H, n_measures, measure_start_host, frames_host, b->tape_host);
        if (b->tape_host.words.size() > b->tape_words.count() || b->tape_host.off.size() > b->tape_off.count()) {
            b->tape_words.reset(); b->tape_off.reset();
            HIP_TRY(b->tape_words.ensure(b->tape_host.words.size()));
            HIP_TRY(b->tape_off.ensure(b->tape_host.off.size()));
        }
        HIP_TRY(hipMemcpyAsync(b->tape_words.get(), b->tape_host.words.data(), b->tape_host.words.size() * sizeof(int), hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipMemcpyAsync(b->tape_off.get(), b->tape_host.off.data(), b->tape_host.off.size() * sizeof(double), hipMemcpyHostToDevice, b->stream));
        b->tape_sel.assign(f0, f0 + n_fr);
        for (int32_t t = 0; t <= n_measures; t++) b->tape_start.push_back(measure_start_host[t] - measure_start_host[0]);
    }
    // the states are arguments of the call: nothing of the integrator (q1, q2, p, lambda1, status, times) is read or written, and
    // neither a loaded specialised library nor a parameter table has a say (lengths know no masses or forces)
    tg::RunArgs A = base_args(b, tg::MODE_TAPE);
    A.q1 = A.q2 = A.p1 = A.p2 = A.lam = A.u1 = nullptr;
    A.iters = A.status = nullptr;
    A.n_steps = n_states;
    tg::TapeArgs J{};
    tg::tape_layout(b->P.lds_per_team, longest, J);
    J.Q = Q_dev; J.dQ = dQ_dev; J.L = L_dev; J.V = V_dev; J.LQ = LQ_dev; J.VQ = VQ_dev; J.LQQ = LQQ_dev;
    const int *words = b->tape_words.get();
    J.ftab = words; J.off = b->tape_off.get();
    J.seg = words + b->tape_host.o_seg; J.mstart = words + b->tape_host.o_mstart; J.cuts = words + b->tape_host.o_cuts;
    J.q_stride = (size_t)q_row_stride_doubles; J.dq_stride = (size_t)dq_row_stride_doubles;
    J.n_states = n_states; J.n_measures = n_measures; J.n_pass = b->tape_host.n_pass;
    LaunchTiming timed;
    if (int rc = timing_begin(b, timed)) return rc;
    int rc = tg_detail::launch_tape(b->sys->team, b->d_prog.get(), A, J, (int)((teams + per_block - 1) / per_block), (size_t)geo[2], b->stream);
    if (rc == TG_SUCCESS && hipGetLastError() != hipSuccess) rc = fail(TG_ERR_HIP, "kernel launch failed");
    if (rc == TG_SUCCESS) b->launched[0][0].add(tg::MODE_TAPE);      // a refused launch (the profiling build) is not counted
    return timing_end(b, timed, rc);
}

int tg_batch_tape_measures(tg_batch *b, int32_t n_states, const double *Q_host, const double *dQ_host, int32_t n_measures,
                           const int32_t *measure_start_host, const int32_t *frames_host, double *L, double *V, double *LQ, double *VQ, double *LQQ) {
    const uint64_t nq_ = b && b->sys ? (uint64_t)b->sys->H.p.nq : 0;
    int32_t longest = 0;
    if (int rc = tape_check(b, n_states, Q_host, dQ_host, nq_, nq_, n_measures, measure_start_host, frames_host, L, V, LQ, VQ, LQQ, longest)) return rc;
    int32_t geo[4];
    if (int rc = tg_system_tape_measures_lds(b->sys, longest, geo)) return rc;
    HIP_TRY(hipSetDevice(b->device));
    // staging of this call alone (its size follows n_states and the selection): Q, dQ in; the outputs asked for out
    const size_t rows = (size_t)b->batch * n_states, nq = b->P.nq, T = (size_t)n_measures;
    const size_t n_q = rows * nq, n_dq = dQ_host ? n_q : 0, n_l = L ? rows * T : 0, n_v = V ? rows * T : 0;
    const size_t n_lq = LQ ? rows * T * nq : 0, n_vq = VQ ? rows * T * nq : 0, n_lqq = LQQ ? rows * T * nq * nq : 0;
    tg::DeviceBuffer<double> stage;
    HIP_TRY(stage.ensure(n_q + n_dq + n_l + n_v + n_lq + n_vq + n_lqq));
    double *q = stage.get(), *dq = q + n_q, *l = dq + n_dq, *v = l + n_l, *lq = v + n_v, *vq = lq + n_lq, *lqq = vq + n_vq;
    HIP_TRY(hipMemcpyAsync(q, Q_host, n_q * sizeof(double), hipMemcpyHostToDevice, b->stream));
    if (n_dq) HIP_TRY(hipMemcpyAsync(dq, dQ_host, n_dq * sizeof(double), hipMemcpyHostToDevice, b->stream));
    int rc = tg_batch_tape_measures_device(b, n_states, q, nq, dQ_host ? dq : nullptr, nq, n_measures, measure_start_host, frames_host,
                                           L ? l : nullptr, V ? v : nullptr, LQ ? lq : nullptr, VQ ? vq : nullptr, LQQ ? lqq : nullptr);
    auto back = [&](void *dst, const void *src, size_t bytes) {
        if (rc == TG_SUCCESS && dst && bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, b->stream) != hipSuccess)
            rc = fail(TG_ERR_HIP, "copy of the results failed");
    };
    back(L, l, n_l * sizeof(double)); back(V, v, n_v * sizeof(double)); back(LQ, lq, n_lq * sizeof(double));
    back(VQ, vq, n_vq * sizeof(double)); back(LQQ, lqq, n_lqq * sizeof(double));
    if (hipStreamSynchronize(b->stream) != hipSuccess && rc == TG_SUCCESS) rc = fail(TG_ERR_HIP, "hipStreamSynchronize failed");      // (before the staging is freed)
    return rc;
}

// ---- batched computed torque (mvi_dyn_inverse.hpp): one team per state, one launch

/* Team size, doubles of LDS per team and bytes of LDS per workgroup of the computed-torque kernel for this system (out[0..2];
 * out[3] 0): the rollout slice plus the image [m][m + 1], m = nd + nu + nc, the given accelerations [nq] and the solver's row scales
 * [m] (mvi_dyn_inverse.hpp).  TG_ERR_UNSUPPORTED, with out filled, above the 160 KiB a workgroup can have, and in the profiling build. */
int tg_system_dynamics_inverse_lds(const tg_system *sys, int32_t out[4]) {
    if (!sys || !out) return fail(TG_ERR_INVALID, "null argument");
    tg::DynInverseArgs J{};
    tg::dyn_inverse_layout(sys->H.p.lds_per_team, sys->H.p.nq, sys->H.p.nd, sys->H.p.nu, sys->H.p.nc, J);
    const int rc = pose_lds(sys, J.lds_per_team, "system too large for the LDS-resident computed-torque kernel", out);
#if defined(TG_PROFILE)
    if (rc == TG_SUCCESS) return fail(TG_ERR_UNSUPPORTED, "the profiling build has no computed-torque kernel");
#endif
    return rc;
}

/* The same for the kernel whose solve is the rank-revealing least squares (tg_batch_dynamics_inverse_lsq): the stacked block
 * [nd + n][n + 1], n = nu + nc, in place of the image and the solver's 4 n doubles in place of the row scales (dyn_inverse_lsq_layout). */
int tg_system_dynamics_inverse_lsq_lds(const tg_system *sys, int32_t out[4]) {
    if (!sys || !out) return fail(TG_ERR_INVALID, "null argument");
    tg::DynInverseArgs J{};
    tg::dyn_inverse_lsq_layout(sys->H.p.lds_per_team, sys->H.p.nq, sys->H.p.nd, sys->H.p.nu, sys->H.p.nc, J);
    const int rc = pose_lds(sys, J.lds_per_team, "system too large for the LDS-resident computed-torque kernel", out);
#if defined(TG_PROFILE)
    if (rc == TG_SUCCESS) return fail(TG_ERR_UNSUPPORTED, "the profiling build has no computed-torque kernel");
#endif
    return rc;
}

/* ... and for the kernel whose solve is the bounded least squares (tg_batch_dynamics_inverse_bounded): the pristine stacked block, and
 * in place of the 4 n doubles the solver's scratch, (nd + n)(n + 1) + 9 n doubles (dyn_inverse_bounded_layout). */
int tg_system_dynamics_inverse_bounded_lds(const tg_system *sys, int32_t out[4]) {
    if (!sys || !out) return fail(TG_ERR_INVALID, "null argument");
    tg::DynInverseArgs J{};
    tg::dyn_inverse_bounded_layout(sys->H.p.lds_per_team, sys->H.p.nq, sys->H.p.nd, sys->H.p.nu, sys->H.p.nc, J);
    const int rc = pose_lds(sys, J.lds_per_team, "system too large for the LDS-resident computed-torque kernel", out);
#if defined(TG_PROFILE)
    if (rc == TG_SUCCESS) return fail(TG_ERR_UNSUPPORTED, "the profiling build has no computed-torque kernel");
#endif
    return rc;
}

// what both entry points refuse, decided on the host before a device is touched: first what the arguments alone show, then what
// needs the system (the strides are nq for the host variant; lsq: n > nd needs no ridge)
static int dyn_inverse_check(const tg_batch *b, int32_t n_states, const double *Q, const double *dQ, const double *ddQ, uint64_t q_stride,
                             uint64_t dq_stride, uint64_t ddq_stride, double ridge, bool lsq = false) {
    if (!(ridge >= 0.0) || !std::isfinite(ridge)) return fail(TG_ERR_INVALID, "ridge must be finite and not negative");
    if (n_states < 1) return fail(TG_ERR_INVALID, "n_states must be at least 1");
    if (!Q) return fail(TG_ERR_INVALID, "null Q");
    if (!dQ) return fail(TG_ERR_INVALID, "null dQ");
    if (!ddQ) return fail(TG_ERR_INVALID, "null ddQ");
    if (!b || !b->sys) return fail(TG_ERR_INVALID, "null argument");
    const uint64_t nq = (uint64_t)b->sys->H.p.nq;
    if (q_stride < nq) return fail(TG_ERR_INVALID, "row stride of Q shorter than a configuration");
    if (dq_stride < nq) return fail(TG_ERR_INVALID, "row stride of dQ shorter than a configuration");
    if (ddq_stride < nq) return fail(TG_ERR_INVALID, "row stride of ddQ shorter than a configuration");
    if (!lsq && b->P.nu + b->P.nc > b->P.nd && ridge == 0.0)
        return fail(TG_ERR_INVALID, "more unknowns (nu + nc) than dynamic configs: the least-squares image is singular without a ridge");
    return TG_SUCCESS;
}

// both device entry points: lsq selects the least-squares kernel, its layout, rcond and the rank words
static int dyn_inverse_device(tg_batch *b, int32_t n_states, const double *Q_dev, uint64_t q_row_stride_doubles, const double *dQ_dev,
                              uint64_t dq_row_stride_doubles, const double *ddQ_dev, uint64_t ddq_row_stride_doubles, double ridge, bool lsq,
                              double rcond, double *U_dev, double *LAM_dev, double *RHO_dev, double *TAU_dev, double *ACC_dev, int32_t *rank_dev,
                              int32_t *status_dev, const BoundedArgs *box = nullptr, bool box_checked = false) {
    if (lsq) if (int rc = rcond_check(rcond)) return rc;
    if (int rc = dyn_inverse_check(b, n_states, Q_dev, dQ_dev, ddQ_dev, q_row_stride_doubles, dq_row_stride_doubles, ddq_row_stride_doubles, ridge, lsq)) return rc;
    if (box && !box_checked) if (int rc = bounded_check(b, ridge, *box, false)) return rc;
    int32_t geo[4];
    if (int rc = box ? tg_system_dynamics_inverse_bounded_lds(b->sys, geo)
                     : (lsq ? tg_system_dynamics_inverse_lsq_lds(b->sys, geo) : tg_system_dynamics_inverse_lds(b->sys, geo))) return rc;
    const long long teams = (long long)b->batch * n_states, per_block = 64 / b->sys->team;
    if ((teams + per_block - 1) / per_block > 0x7fffffffLL) return fail(TG_ERR_INVALID, "too many states for one launch");
    HIP_TRY(hipSetDevice(b->device));
    // the states are arguments of the call: nothing of the integrator (q1, q2, p, lambda1, status, times) is read or written, and a
    // loaded specialised library has no say; a parameter table has (masses, gravity and damping move the residual)
    tg::RunArgs A = base_args(b, tg::MODE_DYN_INVERSE);
    A.q1 = A.q2 = A.p1 = A.p2 = A.lam = A.u1 = nullptr;
    A.iters = A.status = nullptr;
    A.n_steps = n_states;
    tg::DynInverseArgs J{};
    if (box) tg::dyn_inverse_bounded_layout(b->P.lds_per_team, b->P.nq, b->P.nd, b->P.nu, b->P.nc, J);
    else if (lsq) tg::dyn_inverse_lsq_layout(b->P.lds_per_team, b->P.nq, b->P.nd, b->P.nu, b->P.nc, J);
    else tg::dyn_inverse_layout(b->P.lds_per_team, b->P.nq, b->P.nd, b->P.nu, b->P.nc, J);
    if (box) {
        J.lo = box->lo; J.hi = box->hi; J.bound_rows = box->bound_rows; J.active = box->active; J.solves = box->solves;
        J.max_solves = tg::bvls_max_solves(b->P.nu + b->P.nc);
    }
    J.rcond = rcond; J.rank = rank_dev;
    J.Q = Q_dev; J.dQ = dQ_dev; J.ddQ = ddQ_dev;
    J.U = U_dev; J.LAM = LAM_dev; J.RHO = RHO_dev; J.TAU = TAU_dev; J.ACC = ACC_dev; J.status = status_dev;
    J.ridge = ridge; J.n_states = n_states;
    J.q_stride = (size_t)q_row_stride_doubles; J.dq_stride = (size_t)dq_row_stride_doubles; J.ddq_stride = (size_t)ddq_row_stride_doubles;
    const bool par = b->par_rows > 0;
    LaunchTiming timed;
    if (int rc = timing_begin(b, timed)) return rc;
    int rc = tg_detail::launch_dyn_inverse(b->sys->team, launch_springs(b), par, box ? 2 : (lsq ? 1 : 0), b->d_prog.get(), A, J,
                                           tg::ParTable{par ? b->par_dev.get() : nullptr, par ? b->par_group : 1, par ? b->par_stride : 0},
                                           (int)((teams + per_block - 1) / per_block), (size_t)geo[2], b->stream);
    if (rc == TG_SUCCESS && hipGetLastError() != hipSuccess) rc = fail(TG_ERR_HIP, "kernel launch failed");
    if (rc == TG_SUCCESS) b->launched[par][0].add(tg::MODE_DYN_INVERSE);      // a refused launch (the profiling build) is not counted
    return timing_end(b, timed, rc);
}

int tg_batch_dynamics_inverse_device(tg_batch *b, int32_t n_states, const double *Q_dev, uint64_t q_row_stride_doubles, const double *dQ_dev,
                                     uint64_t dq_row_stride_doubles, const double *ddQ_dev, uint64_t ddq_row_stride_doubles, double ridge,
                                     double *U_dev, double *LAM_dev, double *RHO_dev, double *TAU_dev, double *ACC_dev, int32_t *status_dev) {
    return dyn_inverse_device(b, n_states, Q_dev, q_row_stride_doubles, dQ_dev, dq_row_stride_doubles, ddQ_dev, ddq_row_stride_doubles, ridge, false,
                              0.0, U_dev, LAM_dev, RHO_dev, TAU_dev, ACC_dev, nullptr, status_dev);
}

int tg_batch_dynamics_inverse_lsq_device(tg_batch *b, int32_t n_states, const double *Q_dev, uint64_t q_row_stride_doubles, const double *dQ_dev,
                                         uint64_t dq_row_stride_doubles, const double *ddQ_dev, uint64_t ddq_row_stride_doubles, double ridge,
                                         double rcond, double *U_dev, double *LAM_dev, double *RHO_dev, double *TAU_dev, double *ACC_dev,
                                         int32_t *rank_dev, int32_t *status_dev) {
    return dyn_inverse_device(b, n_states, Q_dev, q_row_stride_doubles, dQ_dev, dq_row_stride_doubles, ddQ_dev, ddq_row_stride_doubles, ridge, true,
                              rcond, U_dev, LAM_dev, RHO_dev, TAU_dev, ACC_dev, rank_dev, status_dev);
}

// both host entry points
static int dyn_inverse_host(tg_batch *b, int32_t n_states, const double *Q_host, const double *dQ_host, const double *ddQ_host, double ridge,
                            bool lsq, double rcond, double *U, double *LAM, double *RHO, double *TAU, double *ACC, int32_t *rank, int32_t *status,
                            const BoundedArgs *box = nullptr) {
    if (lsq) if (int rc = rcond_check(rcond)) return rc;
    const uint64_t nq_ = b && b->sys ? (uint64_t)b->sys->H.p.nq : 0;
    if (int rc = dyn_inverse_check(b, n_states, Q_host, dQ_host, ddQ_host, nq_, nq_, nq_, ridge, lsq)) return rc;
    if (box) if (int rc = bounded_check(b, ridge, *box, true)) return rc;
    int32_t geo[4];
    if (int rc = box ? tg_system_dynamics_inverse_bounded_lds(b->sys, geo)
                     : (lsq ? tg_system_dynamics_inverse_lsq_lds(b->sys, geo) : tg_system_dynamics_inverse_lds(b->sys, geo))) return rc;
    HIP_TRY(hipSetDevice(b->device));
    // staging of this call alone (its size follows n_states): Q, dQ, ddQ in; the outputs asked for and the status words out
    const size_t rows = (size_t)b->batch * n_states, nq = b->P.nq, nd = b->P.nd, nu = b->P.nu, nc = b->P.nc;
    const size_t n_q = rows * nq, n_u = U ? rows * nu : 0, n_l = LAM ? rows * nc : 0, n_r = RHO ? rows * nd : 0, n_t = TAU ? rows * nd : 0;
    const size_t n_a = ACC ? rows * nc : 0;
    tg::DeviceBuffer<double> stage;
    tg::DeviceBuffer<int> words;
    // (the box and its outputs behind them: lo and hi [bound_rows][n]; solves, then active [rows][n])
    const size_t n_box = box ? (size_t)box->bound_rows * (nu + nc) : 0, n_act = box ? rows * (nu + nc) : 0;
    HIP_TRY(stage.ensure(3 * n_q + n_u + n_l + n_r + n_t + n_a + 2 * n_box));
    if (status || rank || box) HIP_TRY(words.ensure(2 * rows + (box ? rows + n_act : 0)));      // (status, then rank)
    double *q = stage.get(), *dq = q + n_q, *ddq = dq + n_q, *u = ddq + n_q, *lam = u + n_u, *rho = lam + n_l, *tau = rho + n_r, *acc = tau + n_t;
    double *lo = acc + n_a, *hi = lo + n_box;
    BoundedArgs dev{};
    if (box) {
        dev = BoundedArgs{lo, hi, box->bound_rows, box->active ? words.get() + 3 * rows : nullptr, box->solves ? words.get() + 2 * rows : nullptr};
        if (n_box) HIP_TRY(hipMemcpyAsync(lo, box->lo, n_box * sizeof(double), hipMemcpyHostToDevice, b->stream));
        if (n_box) HIP_TRY(hipMemcpyAsync(hi, box->hi, n_box * sizeof(double), hipMemcpyHostToDevice, b->stream));
    }
    HIP_TRY(hipMemcpyAsync(q, Q_host, n_q * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(dq, dQ_host, n_q * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(ddq, ddQ_host, n_q * sizeof(double), hipMemcpyHostToDevice, b->stream));
    int rc = dyn_inverse_device(b, n_states, q, nq, dq, nq, ddq, nq, ridge, lsq, rcond, n_u ? u : nullptr, n_l ? lam : nullptr, n_r ? rho : nullptr,
                                n_t ? tau : nullptr, n_a ? acc : nullptr, rank ? words.get() + rows : nullptr, status ? words.get() : nullptr,
                                box ? &dev : nullptr, true);
    auto back = [&](void *dst, const void *src, size_t bytes) {
        if (rc == TG_SUCCESS && dst && bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, b->stream) != hipSuccess)
            rc = fail(TG_ERR_HIP, "copy of the results failed");
    };
    back(U, u, n_u * sizeof(double)); back(LAM, lam, n_l * sizeof(double)); back(RHO, rho, n_r * sizeof(double));
    back(TAU, tau, n_t * sizeof(double)); back(ACC, acc, n_a * sizeof(double)); back(status, words.get(), rows * sizeof(int));
    if (rank) back(rank, words.get() + rows, rows * sizeof(int));
    if (box) { back(box->solves, words.get() + 2 * rows, rows * sizeof(int)); back(box->active, words.get() + 3 * rows, n_act * sizeof(int)); }
    if (hipStreamSynchronize(b->stream) != hipSuccess && rc == TG_SUCCESS) rc = fail(TG_ERR_HIP, "hipStreamSynchronize failed");      // (before the staging is freed)
    return rc;
}

int tg_batch_dynamics_inverse(tg_batch *b, int32_t n_states, const double *Q_host, const double *dQ_host, const double *ddQ_host, double ridge,
                              double *U, double *LAM, double *RHO, double *TAU, double *ACC, int32_t *status) {
    return dyn_inverse_host(b, n_states, Q_host, dQ_host, ddQ_host, ridge, false, 0.0, U, LAM, RHO, TAU, ACC, nullptr, status);
}

int tg_batch_dynamics_inverse_lsq(tg_batch *b, int32_t n_states, const double *Q_host, const double *dQ_host, const double *ddQ_host, double ridge,
                                  double rcond, double *U, double *LAM, double *RHO, double *TAU, double *ACC, int32_t *rank, int32_t *status) {
    return dyn_inverse_host(b, n_states, Q_host, dQ_host, ddQ_host, ridge, true, rcond, U, LAM, RHO, TAU, ACC, rank, status);
}

int tg_batch_dynamics_inverse_bounded(tg_batch *b, int32_t n_states, const double *Q_host, const double *dQ_host, const double *ddQ_host, double ridge,
                                      double rcond, const double *lo_host, const double *hi_host, int32_t bound_rows, double *U, double *LAM,
                                      double *RHO, double *TAU, double *ACC, int32_t *active, int32_t *solves, int32_t *rank, int32_t *status) {
    const BoundedArgs box{lo_host, hi_host, bound_rows, active, solves};
    return dyn_inverse_host(b, n_states, Q_host, dQ_host, ddQ_host, ridge, true, rcond, U, LAM, RHO, TAU, ACC, rank, status, &box);
}

int tg_batch_dynamics_inverse_bounded_device(tg_batch *b, int32_t n_states, const double *Q_dev, uint64_t q_row_stride_doubles, const double *dQ_dev,
                                             uint64_t dq_row_stride_doubles, const double *ddQ_dev, uint64_t ddq_row_stride_doubles, double ridge,
                                             double rcond, const double *lo_dev, const double *hi_dev, int32_t bound_rows, double *U_dev,
                                             double *LAM_dev, double *RHO_dev, double *TAU_dev, double *ACC_dev, int32_t *active_dev,
                                             int32_t *solves_dev, int32_t *rank_dev, int32_t *status_dev) {
    const BoundedArgs box{lo_dev, hi_dev, bound_rows, active_dev, solves_dev};
    return dyn_inverse_device(b, n_states, Q_dev, q_row_stride_doubles, dQ_dev, dq_row_stride_doubles, ddQ_dev, ddq_row_stride_doubles, ridge, true,
                              rcond, U_dev, LAM_dev, RHO_dev, TAU_dev, ACC_dev, rank_dev, status_dev, &box);
}

/* Test hook (tests/test_gpu_bounded.py): the bounded least-squares solver of the _bounded kernels (bvls_solve.hpp) alone, as
 * tg_batch_debug_lsq_solve runs lsq_solve.hpp: `count` problems of one shape with a box each, lo and hi [count][cols] (host), one team of
 * `team` lanes on each, in one launch.  max_solves: the cap on the solves of a problem (0: the kernels' 3 cols + 3); a problem that
 * needs more reports TG_NOT_CONVERGED with its last feasible iterate.  z and active [count][cols]; solves, rank (the first solve's),
 * status [count]; TG_SINGULAR (first solve of rank < cols, or something not finite -- rank 0 then) comes with z = 0, active = 0.  Only
 * here do teams that need different numbers of solves share a wavefront. */
int tg_batch_debug_bvls_solve(tg_batch *b, int32_t team, int32_t count, int32_t rows, int32_t cols, const double *A_host, const double *c_host,
                              const double *lo_host, const double *hi_host, double rcond, int32_t max_solves, double *z_host, int32_t *active_host,
                              int32_t *solves_host, int32_t *rank_host, int32_t *status_host) {
    if (!b || !A_host || !c_host || !lo_host || !hi_host || !z_host || !active_host || !solves_host || !rank_host || !status_host)
        return fail(TG_ERR_INVALID, "null argument");
    if (team != 1 && team != 4 && team != 16 && team != 64) return fail(TG_ERR_INVALID, "team must be 1, 4, 16 or 64");
    if (count < 1 || rows < 1 || cols < 1 || rows > 1024 || cols > 1024) return fail(TG_ERR_INVALID, "count, rows and cols must be positive (rows, cols at most 1024)");
    if (max_solves < 0 || max_solves > 3 * cols + 3) return fail(TG_ERR_INVALID, "max_solves must lie in 0 .. 3 cols + 3");
    if (int rc = rcond_check(rcond)) return rc;
    for (size_t i = 0; i < (size_t)count * cols; i++) {
        if (std::isnan(lo_host[i]) || std::isnan(hi_host[i])) return fail(TG_ERR_INVALID, "a bound is not a number");
        if (lo_host[i] > hi_host[i]) return fail(TG_ERR_INVALID, "a lower bound above its upper bound");
        if (lo_host[i] == INFINITY || hi_host[i] == -INFINITY) return fail(TG_ERR_INVALID, "a bound that no finite value meets");
    }
    const int per_team = (rows * (cols + 1) + tg::bvls_scratch_doubles(rows, cols) + 1) & ~1;
    const int per_block = (int)std::min<size_t>(64 / team, (160 * 1024) / (per_team * sizeof(double)));
    if (per_block < 1) return fail(TG_ERR_UNSUPPORTED, "problem too large for the LDS of a workgroup");
    const size_t lds = (size_t)per_block * per_team * sizeof(double);
    HIP_TRY(hipSetDevice(b->device));
    const size_t cA = (size_t)count * rows * cols, cc = (size_t)count * rows, cz = (size_t)count * cols;
    tg::DeviceBuffer<double> buf;
    tg::DeviceBuffer<int> words;
    HIP_TRY(buf.ensure(cA + cc + 3 * cz));
    HIP_TRY(words.ensure(3 * (size_t)count + cz));
    double *dA = buf.get(), *dc = dA + cA, *dlo = dc + cc, *dhi = dlo + cz, *dz = dhi + cz;
    int *dsolves = words.get(), *drank = dsolves + count, *dstatus = drank + count, *dactive = dstatus + count;
    HIP_TRY(hipMemcpyAsync(dA, A_host, cA * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(dc, c_host, cc * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(dlo, lo_host, cz * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(dhi, hi_host, cz * sizeof(double), hipMemcpyHostToDevice, b->stream));
    int rc = tg_detail::launch_bvls_debug(team, per_block, count, rows, cols, per_team, dA, dc, dlo, dhi, rcond, max_solves ? max_solves : tg::bvls_max_solves(cols),
                                          dz, dactive, dsolves, drank, dstatus, lds, b->stream);
    if (rc == TG_SUCCESS && hipGetLastError() != hipSuccess) rc = fail(TG_ERR_HIP, "kernel launch failed");
    auto back = [&](void *dst, const void *src, size_t bytes) {
        if (rc == TG_SUCCESS && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, b->stream) != hipSuccess) rc = fail(TG_ERR_HIP, "copy of the results failed");
    };
    back(z_host, dz, cz * sizeof(double)); back(active_host, dactive, cz * sizeof(int)); back(solves_host, dsolves, count * sizeof(int));
    back(rank_host, drank, count * sizeof(int)); back(status_host, dstatus, count * sizeof(int));
    if (hipStreamSynchronize(b->stream) != hipSuccess && rc == TG_SUCCESS) rc = fail(TG_ERR_HIP, "hipStreamSynchronize failed");      // (before the staging is freed)
    return rc;
}

/* Test hook (tests/test_gpu_min_norm.py): the rank-revealing least-squares solver of the _lsq kernels (lsq_solve.hpp) alone, on `count`
 * caller-supplied problems of one shape, A [count][rows][cols] and c [count][rows] (host), one team of `team` lanes (1, 4, 16 or 64,
 * whatever the batch's own team size) on each, in one launch: z [count][cols], rank [count], status [count] (TG_OK, or TG_SINGULAR with
 * z = 0 and rank 0 for an answer that is not finite).  Only here do teams of different rank share a wavefront. */
int tg_batch_debug_lsq_solve(tg_batch *b, int32_t team, int32_t count, int32_t rows, int32_t cols, const double *A_host, const double *c_host,
                             double rcond, double *z_host, int32_t *rank_host, int32_t *status_host) {
    if (!b || !A_host || !c_host || !z_host || !rank_host || !status_host) return fail(TG_ERR_INVALID, "null argument");
    if (team != 1 && team != 4 && team != 16 && team != 64) return fail(TG_ERR_INVALID, "team must be 1, 4, 16 or 64");
    if (count < 1 || rows < 1 || cols < 1 || rows > 1024 || cols > 1024) return fail(TG_ERR_INVALID, "count, rows and cols must be positive (rows, cols at most 1024)");
    if (int rc = rcond_check(rcond)) return rc;
    const int per_team = (rows * (cols + 1) + tg::lsq_scratch_doubles(cols) + 1) & ~1;
    // 64 / team teams to a workgroup as in the kernels, or as many as its 160 KiB of LDS take
    const int per_block = (int)std::min<size_t>(64 / team, (160 * 1024) / (per_team * sizeof(double)));
    if (per_block < 1) return fail(TG_ERR_UNSUPPORTED, "problem too large for the LDS of a workgroup");
    const size_t lds = (size_t)per_block * per_team * sizeof(double);
    HIP_TRY(hipSetDevice(b->device));
    const size_t cA = (size_t)count * rows * cols, cc = (size_t)count * rows, cz = (size_t)count * cols;
    tg::DeviceBuffer<double> buf;
    tg::DeviceBuffer<int> words;
    HIP_TRY(buf.ensure(cA + cc + cz));
    HIP_TRY(words.ensure(2 * (size_t)count));
    double *dA = buf.get(), *dc = dA + cA, *dz = dc + cc;
    HIP_TRY(hipMemcpyAsync(dA, A_host, cA * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(dc, c_host, cc * sizeof(double), hipMemcpyHostToDevice, b->stream));
    int rc = tg_detail::launch_lsq_debug(team, per_block, count, rows, cols, per_team, dA, dc, rcond, dz, words.get(), words.get() + count, lds, b->stream);
    if (rc == TG_SUCCESS && hipGetLastError() != hipSuccess) rc = fail(TG_ERR_HIP, "kernel launch failed");
    auto back = [&](void *dst, const void *src, size_t bytes) {
        if (rc == TG_SUCCESS && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, b->stream) != hipSuccess) rc = fail(TG_ERR_HIP, "copy of the results failed");
    };
    back(z_host, dz, cz * sizeof(double)); back(rank_host, words.get(), count * sizeof(int)); back(status_host, words.get() + count, count * sizeof(int));
    if (hipStreamSynchronize(b->stream) != hipSuccess && rc == TG_SUCCESS) rc = fail(TG_ERR_HIP, "hipStreamSynchronize failed");      // (before the staging is freed)
    return rc;
}

// z and hz in device memory; horizon > 0: only steps k_begin .. k_end - 1 of every seed of a seeds x horizon batch
static int deriv2_contract_device(tg_batch *b, const double *z_dev, double *hz_dev, int horizon, int k_begin, int k_end) {
    if (b->P.n_true_springs) return fail(TG_ERR_UNSUPPORTED, "V_dqdqdq() is undefined for LinearSpring (as in the reference): no second derivatives");
    if (b->t2 == b->t1) return fail(TG_ERR_STATE, "Integrator has not solved the next time step yet.");
    HIP_TRY(hipSetDevice(b->device));
    tg::RunArgs A = base_args(b, tg::MODE_DERIV2Z);
    A.z = z_dev; A.hz = hz_dev;
    if (horizon > 0) { A.remap_len = k_end - k_begin; A.remap_stride = horizon; A.remap_off = k_begin; A.remap_count = (b->batch / horizon) * (k_end - k_begin); }
    return launch(b, A);
}

int tg_batch_deriv2_contract_device(tg_batch *b, const double *z_dev, double *hz_dev) {
    if (!b || !z_dev || !hz_dev) return fail(TG_ERR_INVALID, "null argument");
    return deriv2_contract_device(b, z_dev, hz_dev, 0, 0, 0);
}

int tg_batch_deriv2_contract_device_range(tg_batch *b, const double *z_dev, double *hz_dev, int32_t horizon, int32_t k_begin, int32_t k_end) {
    if (!b || !z_dev || !hz_dev) return fail(TG_ERR_INVALID, "null argument");
    if (horizon <= 0 || b->batch % horizon != 0 || k_begin < 0 || k_end > horizon || k_begin >= k_end) return fail(TG_ERR_INVALID, "bad step range");
    return deriv2_contract_device(b, z_dev, hz_dev, horizon, k_begin, k_end);
}

int tg_batch_set_from_trajectories(tg_batch *b, int32_t seeds, int32_t horizon, double t0, double dt, const double *X_dev,
                                   const double *U_dev, int32_t max_iterations) {
    if (!b || !X_dev || !U_dev || seeds <= 0 || horizon <= 0 || dt == 0.0) return fail(TG_ERR_INVALID, "bad arguments");
    if ((int64_t)seeds * horizon != b->batch) return fail(TG_ERR_INVALID, "batch size must be seeds * horizon");
    HIP_TRY(hipSetDevice(b->device));
    const tg::DevProg &P = b->P;
    b->mirror_valid = false;
    hipLaunchKernelGGL(k_set_from_trajectories, dim3(b->batch), dim3(64), 0, b->stream, P, seeds, horizon, X_dev, U_dev,
                       b->q1.get(), b->q2.get(), b->p1.get(), b->p2.get(), b->lam.get(), b->stage_u.get(), b->stage_k.get(), b->stage_qh.get());
    HIP_TRY(hipGetLastError());
    b->t1 = t0; b->t2 = t0;
    tg::RunArgs A = step_args(b, dt, max_iterations, b->stage_u.get(), b->stage_k.get(), b->stage_qh.get(), nullptr);
    if (int rc = launch(b, A)) return rc;
    b->t1 = t0; b->t2 = t0 + dt;
    return TG_SUCCESS;
}

int tg_batch_initialize_from_state_device(tg_batch *b, double t, const double *X_dev, uint64_t row_stride_doubles) {
    if (!b || !X_dev || row_stride_doubles < (uint64_t)(b->P.nq + b->P.nd)) return fail(TG_ERR_INVALID, "bad arguments");
    HIP_TRY(hipSetDevice(b->device));
    b->mirror_valid = false;
    hipLaunchKernelGGL(k_init_from_X, dim3(b->batch), dim3(64), 0, b->stream, b->P, X_dev, (size_t)row_stride_doubles, b->q1.get(), b->q2.get(),
                       b->p1.get(), b->p2.get(), b->lam.get());
    HIP_TRY(hipGetLastError());
    b->t1 = t; b->t2 = t;
    return TG_SUCCESS;
}

int tg_batch_linearize(tg_batch *b, double *A_dev, double *B_dev) {
    if (!b || !A_dev || !B_dev) return fail(TG_ERR_INVALID, "null argument");
    if (b->t2 == b->t1) return fail(TG_ERR_STATE, "Integrator has not solved the next time step yet.");
    HIP_TRY(hipSetDevice(b->device));
    tg::RunArgs A = base_args(b, tg::MODE_DERIV1);
    A.A_out = A_dev; A.B_out = B_dev;
    return launch(b, A);
}

void *tg_device_alloc(int32_t device, uint64_t bytes) {
    void *p = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipMalloc(&p, bytes ? bytes : 8) != hipSuccess) { fail(TG_ERR_HIP, "hipMalloc failed"); return nullptr; }
    return p;
}
int tg_device_free(int32_t device, void *ptr) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipFree(ptr));
    return TG_SUCCESS;
}
int tg_memcpy_h2d(int32_t device, void *dst_dev, const void *src_host, uint64_t bytes) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpy(dst_dev, src_host, bytes, hipMemcpyHostToDevice));
    return TG_SUCCESS;
}
int tg_memcpy_d2h(int32_t device, void *dst_host, const void *src_dev, uint64_t bytes) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpy(dst_host, src_dev, bytes, hipMemcpyDeviceToHost));
    return TG_SUCCESS;
}

int tg_batch_synchronize(tg_batch *b) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return TG_SUCCESS;
}

int tg_batch_set_stream(tg_batch *b, void *hip_stream) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (b->own_stream && b->stream) HIP_TRY(hipStreamDestroy(b->stream));
    if (hip_stream) { b->stream = (hipStream_t)hip_stream; b->own_stream = false; }
    else { HIP_TRY(hipStreamCreate(&b->stream)); b->own_stream = true; }
    return TG_SUCCESS;
}

/* Test hook (tests/test_gpu_parity.py): solves the n x n system [A | b] (row-major [n][n+1], n <= 32) with the register
 * Gauss-Jordan of the rollout kernels and reports which original row was the pivot of each column: the reference's
 * LU_decomp (math-code.c:337-432, implicit scaling, strict `>` scan) must pick the same rows, ties included. */
int tg_debug_solve(int32_t device, int32_t n, int32_t exact, const double *A_aug_host, double *x_host, int32_t *pivot_rows_host, int32_t *status_host) {
    if (n <= 0 || n > 32 || !A_aug_host || !x_host || !pivot_rows_host || !status_host) return fail(TG_ERR_INVALID, "bad arguments");
    if (exact == 2 && (n <= 16 || n >= 32)) return fail(TG_ERR_INVALID, "the panel solver takes 16 < n < 32");
    HIP_TRY(hipSetDevice(device));
    tg::DeviceBuffer<double> dA, dx;
    tg::DeviceBuffer<int> dp, ds;
    const int ld = (n + 1) | 1;
    HIP_TRY(dA.ensure((size_t)n * (n + 1))); HIP_TRY(dx.ensure(n)); HIP_TRY(dp.ensure(n)); HIP_TRY(ds.ensure(1));
    HIP_TRY(hipMemcpy(dA.get(), A_aug_host, sizeof(double) * n * (n + 1), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_debug_solve, dim3(1), dim3(64), sizeof(double) * (n * ld + 16 + 192), 0, n, ld, (int)exact, dA.get(), dx.get(), dp.get(), ds.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(x_host, dx.get(), sizeof(double) * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pivot_rows_host, dp.get(), sizeof(int) * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(status_host, ds.get(), sizeof(int), hipMemcpyDeviceToHost));
    return TG_SUCCESS;
}

int tg_batch_set_pivot_rule(tg_batch *b, int32_t exact) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    b->exact_pivot = exact ? 1 : 0;
    return TG_SUCCESS;
}

}  // extern "C"
namespace {
std::string spec_header_text(const tg_system *sys) {
    std::string out;
    char line[160];
    std::snprintf(line, sizeof(line), "#define SPEC_TEAM %d\n#define SPEC_SPRINGS %s\n", sys->team,
                  launch_springs(sys->H.p) ? "true" : "false");
    out += line;
    tg::emit_spec_header(sys->H, out);
    return out;
}
uint64_t fnv1a64(const std::string &t) {
    uint64_t h = 1469598103934665603ull;
    for (unsigned char c : t) { h ^= c; h *= 1099511628211ull; }
    return h;
}
}  // namespace
extern "C" {

/* Text of the specialisation header of a system (schedule.hpp, emit_spec_header); returns the length needed (incl. the terminator). */
int64_t tg_system_spec_header(const tg_system *sys, char *buf, uint64_t capacity) {
    if (!sys) { fail(TG_ERR_INVALID, "null system"); return -1; }
    const std::string out = spec_header_text(sys);
    if (buf && capacity) {
        const size_t n = std::min((size_t)capacity - 1, out.size());
        std::memcpy(buf, out.data(), n);
        buf[n] = 0;
    }
    return (int64_t)out.size() + 1;
}

/* FNV-1a (64 bit) of that text: what a specialised library carries as tg_spec_key() (-DTG_SPEC_KEY=...) and what
 * tg_batch_load_specialized compares, so a library built for another system -- or another parameter set of the same
 * topology -- is refused even when every size agrees. */
uint64_t tg_system_spec_key(const tg_system *sys) {
    if (!sys) { fail(TG_ERR_INVALID, "null system"); return 0; }
    return fnv1a64(spec_header_text(sys));
}

/* Rollouts of this batch use the kernel of a library built by trep_amd/specialize.py for exactly this system. */
int tg_batch_load_specialized(tg_batch *b, const char *library_path) {
    if (!b || !library_path) return fail(TG_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(b->device));
    std::unique_ptr<void, int (*)(void *)> lib(dlopen(library_path, RTLD_NOW | RTLD_LOCAL), dlclose);     // closed again by every refusal
    void *h = lib.get();
    const char *why = h ? nullptr : dlerror();      // (one call: dlerror() clears the message it returns)
    if (!h) return fail(TG_ERR_INVALID, std::string("cannot load ") + library_path + ": " + (why ? why : "?"));
    auto launch_fn = reinterpret_cast<int (*)(int, const tg::RunArgs *, tg::RunArgs *, int, size_t, void *)>(dlsym(h, "tg_spec_launch"));
    auto sizes_fn = reinterpret_cast<const int *(*)(void)>(dlsym(h, "tg_spec_sizes"));
    auto modes_fn = reinterpret_cast<int (*)(void)>(dlsym(h, "tg_spec_modes"));
    auto key_fn = reinterpret_cast<uint64_t (*)(void)>(dlsym(h, "tg_spec_key"));
    if (!launch_fn || !sizes_fn || !modes_fn || !key_fn) return fail(TG_ERR_INVALID, "not a specialised trep_amd kernel library");
    const tg::DevProg &P = b->P;
    const int want[8] = {(int)sizeof(tg::DevProg), (int)sizeof(tg::RunArgs), P.nq, P.nd, P.nc, P.n_items, P.n_pairs, P.lds_per_team};
    const int *got = sizes_fn();
    for (int i = 0; i < 8; i++) if (got[i] != want[i]) return fail(TG_ERR_INVALID, "specialised kernel was built for a different system or library version");
    if (key_fn() != tg_system_spec_key(b->sys)) return fail(TG_ERR_INVALID, "specialised kernel was built from a different schedule (header hash mismatch)");
    if (!b->d_args) {      // built in locals and moved in when complete: a refused call leaves the batch as it was
        tg::DeviceBuffer<tg::RunArgs> d_args;
        tg::PinnedBuffer<tg::RunArgs> h_args;
        tg::Event done[tg_batch::ARG_SLOTS];
        bool ok = d_args.ensure(tg_batch::ARG_SLOTS) == hipSuccess && h_args.ensure(tg_batch::ARG_SLOTS, hipHostMallocDefault) == hipSuccess;
        for (int i = 0; i < tg_batch::ARG_SLOTS && ok; i++) ok = done[i].create(hipEventDisableTiming) == hipSuccess;
        if (!ok) return fail(TG_ERR_HIP, "allocation of the argument blocks failed");
        b->d_args = std::move(d_args); b->h_args = std::move(h_args);
        for (int i = 0; i < tg_batch::ARG_SLOTS; i++) b->arg_done[i] = std::move(done[i]);
    }
    if (b->spec_lib) { hipStreamSynchronize(b->stream); dlclose(b->spec_lib); }
    b->spec_lib = lib.release(); b->spec_launch = launch_fn; b->spec_modes = modes_fn(); b->spec_path = library_path;
    auto waves_fn = reinterpret_cast<int (*)(void)>(dlsym(h, "tg_spec_waves"));
    b->spec_waves = waves_fn ? waves_fn() : 1;
    auto fb_fn = reinterpret_cast<int (*)(void)>(dlsym(h, "tg_spec_fb_n"));
    b->spec_fb_n = fb_fn ? fb_fn() : 0;
    auto tr_fn = reinterpret_cast<int (*)(void)>(dlsym(h, "tg_spec_tr_n"));
    b->spec_tr_n = tr_fn ? tr_fn() : 0;
    auto pc_fn = reinterpret_cast<int (*)(void)>(dlsym(h, "tg_spec_pose_carry"));
    b->spec_pose_carry = pc_fn ? pc_fn() : 0;
    auto par_fn = reinterpret_cast<int (*)(int, const tg::RunArgs *, tg::RunArgs *, int, size_t, void *, const double *, int, int)>(dlsym(h, "tg_spec_launch_par"));
    auto par_modes_fn = reinterpret_cast<int (*)(void)>(dlsym(h, "tg_spec_par_modes"));
    b->spec_launch_par = par_modes_fn ? par_fn : nullptr;
    b->spec_par_modes = (par_fn && par_modes_fn) ? par_modes_fn() : 0;
    return TG_SUCCESS;
}

/* The structured-solve plan of a system (bbd.hpp; host only): out[0..7] = plan found, groups, largest own block, largest border
 * list, trailing size, nf, nd, 0; pattern (optional, [nf * nf]) the structural non-zeros of the Newton matrix the plan was derived
 * from (symmetrised; all zero if the system is outside the plan's range); tab (optional, [128]) the packed plan tables. */
int tg_system_newton_plan(const tg_system *sys, int32_t out[8], uint8_t *pattern, int32_t *tab) {
    if (!sys || !out) return fail(TG_ERR_INVALID, "null argument");
    const tg::DevProg &P = sys->H.p;
    out[0] = P.bbd_ok; out[1] = P.bbd_g; out[2] = P.bbd_ng; out[3] = P.bbd_nb; out[4] = P.bbd_t; out[5] = P.nf; out[6] = P.nd; out[7] = 0;
    if (pattern) {
        std::memset(pattern, 0, (size_t)P.nf * P.nf);
        if (sys->H.newton_pattern.size() == (size_t)P.nf * P.nf) std::memcpy(pattern, sys->H.newton_pattern.data(), sys->H.newton_pattern.size());
    }
    if (tab) for (int i = 0; i < 128; i++) tab[i] = i < (int)sys->H.bbd_tab.size() ? sys->H.bbd_tab[i] : 0;
    return TG_SUCCESS;
}

/* Test hook (tests/test_gpu_parity.py): the Newton-system solve of the batch's SPECIALISED rollout kernel on caller-supplied
 * systems [n_mats][nf][nf + 1] (nf = the system's unknowns): the structured solve along the system's plan if it has one (bbd.hpp),
 * the pivoting solver when a pivot guard fails or skip_structured is set.  path[m]: 1 structured, 2 pivoting, -1 singular. */
int tg_batch_debug_newton_solve(tg_batch *b, int32_t n_mats, int32_t skip_structured, const double *A_aug_host, double *x_host, int32_t *path_host) {
    if (!b || n_mats <= 0 || !A_aug_host || !x_host || !path_host) return fail(TG_ERR_INVALID, "bad arguments");
    if (!b->spec_lib) return fail(TG_ERR_INVALID, "no specialised kernel library loaded");
    auto fn = reinterpret_cast<int (*)(const double *, double *, int *, int, int)>(dlsym(b->spec_lib, "tg_spec_debug_solve"));
    if (!fn) return fail(TG_ERR_INVALID, "the specialised library has no solve hook");
    const int nf = b->P.nf;
    HIP_TRY(hipSetDevice(b->device));
    tg::DeviceBuffer<double> dA, dx;
    tg::DeviceBuffer<int> dp;
    const size_t cA = (size_t)n_mats * nf * (nf + 1), cx = (size_t)n_mats * nf, cp = (size_t)n_mats;
    auto failed = [](const char *what) { (void)hipGetLastError(); return fail(TG_ERR_HIP, what); };
    if (dA.ensure(cA) != hipSuccess || dx.ensure(cx) != hipSuccess || dp.ensure(cp) != hipSuccess) return failed("solve hook: device allocation failed");
    if (hipMemcpy(dA.get(), A_aug_host, cA * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return failed("solve hook: upload failed");
    const int rc = fn(dA.get(), dx.get(), dp.get(), n_mats, skip_structured);
    if (hipDeviceSynchronize() != hipSuccess || rc != 0) return failed("solve hook launch failed");
    if (hipMemcpy(x_host, dx.get(), cx * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(path_host, dp.get(), cp * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return failed("solve hook: download failed");
    return TG_SUCCESS;
}

/* Which kernels this batch runs: out[0] bit m = mode m (tg::MODE_*) has a specialised kernel loaded; out[1] / out[2] bit m = a
 * mode-m launch has gone through a specialised / a generic kernel since the batch was created; out[3] / out[4] the number of
 * such launches; out[5] pivot rule; out[6] team size; out[7] bits 0-7 wavefronts per trajectory of the loaded library's derivative kernels,
 * bits 8-15 the joints of the translational prefix its rollout kernel has closed forms for, as the library itself reports them
 * (tg_spec_fb_n; 0: none, compiled out, or no library), bits 16-23 the joints of translation runs whose world poses its rollout
 * kernel stores directly (tg_spec_tr_n; likewise), bit 24 its rollout kernel carries the q2 poses into a step's first evaluation behind the
 * step edge, bits 25-28 the joints without a q2 twin that needs (tg_spec_pose_carry; likewise). */
int tg_batch_info(const tg_batch *b, int32_t out[8]) {
    if (!b || !out) return fail(TG_ERR_INVALID, "null argument");
    out[0] = b->spec_launch ? b->spec_modes : 0;
    for (int spec = 0; spec < 2; spec++) { out[2 - spec] = (int32_t)b->launched[0][spec].modes; out[4 - spec] = (int32_t)std::min<long long>(b->launched[0][spec].n, 0x7fffffff); }
    out[5] = b->exact_pivot; out[6] = b->sys->team; out[7] = b->spec_launch ? b->spec_waves : 1;
    if (b->spec_launch) out[7] |= (b->spec_fb_n << 8) | ((b->spec_tr_n & 0xFF) << 16) | ((b->spec_pose_carry & 0x1F) << 24);
    return TG_SUCCESS;
}

/* The parameter kernels of this batch (tg_batch_set_parameters): out[0] bit m = mode m has a specialised parameter kernel loaded;
 * out[1] / out[2] bit m = a mode-m launch has gone through a specialised / a generic parameter kernel; out[3] / out[4] the number of
 * such launches; out[5] rows of the current table (0: none set); out[6] its group; out[7] 0. */
int tg_batch_par_info(const tg_batch *b, int32_t out[8]) {
    if (!b || !out) return fail(TG_ERR_INVALID, "null argument");
    out[0] = b->spec_launch_par ? b->spec_par_modes : 0;
    for (int spec = 0; spec < 2; spec++) { out[2 - spec] = (int32_t)b->launched[1][spec].modes; out[4 - spec] = (int32_t)std::min<long long>(b->launched[1][spec].n, 0x7fffffff); }
    out[5] = b->par_rows; out[6] = b->par_rows ? b->par_group : 0; out[7] = 0;
    return TG_SUCCESS;
}

/* Base values of the per-trajectory parameters (tg_batch_set_parameters): sizes_out = n_bodies, nd, has_gravity, has_damping;
 * inertia [n_bodies][4] (mass, Ixx, Iyy, Izz of every massive frame in System.masses order: reference frame.py set_mass), gravity [3]
 * (the sum over the Gravity potentials: potentials/gravity.py), damping [nd] (the summed coefficient of every dynamic config:
 * forces/damping.py).  Null outputs are skipped. */
int tg_system_parameters(const tg_system *sys, int32_t sizes_out[4], double *inertia, double *gravity, double *damping) {
    if (!sys) return fail(TG_ERR_INVALID, "null system");
    const tg::HostProgram &H = sys->H;
    if (sizes_out) { sizes_out[0] = H.p.n_bodies; sizes_out[1] = H.p.nd; sizes_out[2] = sys->has_gravity; sizes_out[3] = sys->has_damping; }
    const int nb = H.p.n_bodies, nd = H.p.nd;
    std::vector<double> row(4 * (size_t)nb + 3 + nd);
    base_parameter_row(H, row.data());
    if (inertia) std::copy_n(row.begin(), 4 * nb, inertia);
    if (gravity) std::copy_n(row.begin() + 4 * nb, 3, gravity);
    if (damping) std::copy_n(row.begin() + 4 * nb + 3, nd, damping);
    return TG_SUCCESS;
}

/* Per-trajectory parameters: `rows` rows of inertia [n_bodies][4], gravity [3] and damping [nd] (host arrays, row-major; null: the
 * system's own values in every row); trajectory t uses row t / group (t after any subset remapping).  rows * group == batch, or rows
 * == 1 for the whole batch.  Refused (TG_ERR_INVALID, nothing changed) for bad shapes, non-finite values, or a gravity / damping block
 * of a system without a Gravity potential / Damping force.  The reference's own parameter writes are Frame.set_mass (frame.py),
 * Gravity.gravity (potentials/gravity.py) and Damping.set_damping_coefficient (forces/damping.py): a row acts as a system rebuilt with
 * them; the structure (which frames are massive) never changes.  Ordered on the batch's stream: launches already enqueued keep the
 * table they were launched with, later ones see the new one. */
int tg_batch_set_parameters(tg_batch *b, int32_t rows, int32_t group, const double *inertia_host, const double *gravity_host,
                            const double *damping_host) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    if (rows <= 0 || group <= 0) return fail(TG_ERR_INVALID, "rows and group must be positive");
    if (rows != 1 && (int64_t)rows * group != b->batch) return fail(TG_ERR_INVALID, "rows * group must equal the batch size (or rows == 1)");
    if (gravity_host && !b->sys->has_gravity) return fail(TG_ERR_INVALID, "the system has no Gravity potential: no gravity block");
    if (damping_host && !b->sys->has_damping) return fail(TG_ERR_INVALID, "the system has no Damping force: no damping block");
    const tg::HostProgram &H = b->sys->H;
    const int nb = H.p.n_bodies, nd = H.p.nd, stride = 4 * nb + 3 + nd;
    std::vector<double> tab((size_t)rows * stride);
    for (int r = 0; r < rows; r++) {
        double *row = tab.data() + (size_t)r * stride;
        base_parameter_row(H, row);
        if (inertia_host) std::copy_n(inertia_host + (size_t)r * 4 * nb, 4 * nb, row);
        if (gravity_host) std::copy_n(gravity_host + 3 * (size_t)r, 3, row + 4 * nb);
        if (damping_host) std::copy_n(damping_host + (size_t)r * nd, nd, row + 4 * nb + 3);
    }
    for (double v : tab) if (!std::isfinite(v)) return fail(TG_ERR_INVALID, "parameter values must be finite");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));          // a launch in flight keeps reading the old table until it has finished
    if (tab.size() > b->par_dev.count()) {
        if (b->par_dev) { b->par_dev.reset(); b->par_rows = 0; }
        HIP_TRY(b->par_dev.ensure(tab.size()));
    }
    HIP_TRY(hipMemcpyAsync(b->par_dev.get(), tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->par_rows = rows; b->par_group = rows == 1 ? b->batch : group; b->par_stride = stride;
    b->mirror_valid = false;
    return TG_SUCCESS;
}

/* Back to the system's own parameters: the default kernels run again. */
int tg_batch_clear_parameters(tg_batch *b) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    b->par_rows = 0;
    b->mirror_valid = false;
    return TG_SUCCESS;
}

/* The HIP stream the batch launches on (hipStream_t as void *): for ordering foreign work after it (tg_comm_wait_stream). */
void *tg_batch_stream(tg_batch *b) { return b ? (void *)b->stream : nullptr; }

int tg_batch_timing(tg_batch *b, int32_t reset, int32_t *n_launches, double *total_ms) {
    if (!b) return fail(TG_ERR_INVALID, "null batch");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->timing = true;
    double ms = b->folded_ms;
    for (auto &e : b->events) {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, e.first.get(), e.second.get()));
        ms += t;
    }
    if (n_launches) *n_launches = (int32_t)(b->events.size() + b->folded_n);
    if (total_ms) *total_ms = ms;
    if (reset) {
        for (auto &e : b->events) { b->pool.push_back(std::move(e.first)); b->pool.push_back(std::move(e.second)); }
        b->events.clear();
        b->folded_ms = 0.0; b->folded_n = 0;
    }
    return TG_SUCCESS;
}

}  // extern "C"
