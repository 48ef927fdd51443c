/*
 * trep_amd.h -- C ABI of libtrepamd.so, the MI355X (gfx950) batched MidpointVI engine.
 *
 * This is the drop-in boundary for the MidpointVI hot path of MurpheyLab/trep.
 * It replaces what the reference reaches through the CPython type
 * `_trep._MidpointVI` (reference trep/_trep/midpointvi.c:2756-2921: _solve_DEL,
 * calc_p2, _calc_f, _calc_deriv1, _calc_deriv2 and the numpy work arrays they
 * mutate) and through the exported C-API slot `MidpointVI_solve_DEL`
 * (trep/_trep/c_api.h:88,586-590,693; trep/_trep/trep.h:781-783), for a BATCH of
 * independent trajectories of one mechanical system.
 *
 * Plain C, plain pointers and sizes; no Python, numpy or torch types.  All
 * floating point is IEEE fp64.  Host arrays are caller-owned and row-major
 * [batch][n]; device buffers are owned by the library.  Handles are not
 * thread-safe; one HIP stream per batch.
 */
#ifndef TREP_AMD_H
#define TREP_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Frame transform kinds (reference trep/_trep/trep.h:160-167 TREP_WORLD..TREP_CONST_SE3). */
enum { TG_WORLD = 0, TG_TX = 1, TG_TY = 2, TG_TZ = 3, TG_RX = 4, TG_RY = 5, TG_RZ = 6, TG_CONST_SE3 = 7 };
/* Constraint kinds (reference constraints/distance.c, constraints/point.c). */
enum { TG_CONSTRAINT_DISTANCE = 0, TG_CONSTRAINT_POINT = 1, TG_CONSTRAINT_PLANE = 2 };

/*
 * Flattened mechanical system: the integer topology tables the reference keeps in
 * Frame_s / Config_s / System_s (trep/_trep/trep.h:105-273, 541-633), as computed by
 * System._structure_changed (trep/system.py:672-771) and Frame._structure_changed
 * (trep/frame.py:658-691), plus the parameters of the supported potential / force /
 * constraint types.  All index arrays are int32; "none" is -1.
 */
typedef struct tg_system_desc {
    int32_t n_frames, n_configs, n_dyn, n_kin, n_inputs, n_constraints, n_masses;
    int32_t n_gravity, n_damping, n_config_forces;
    /* frames in System.frames order (depth-first, parent before child) */
    const int32_t *frame_transform;   /* [n_frames]  TG_WORLD..TG_CONST_SE3 */
    const int32_t *frame_parent;      /* [n_frames]  -1 for the world frame */
    const int32_t *frame_config;      /* [n_frames]  driving config index, -1 if fixed */
    const double  *frame_value;       /* [n_frames]  constant parameter of a fixed TX..RZ frame */
    const double  *frame_lg;          /* [n_frames*12] row-major 3x4 constant transform (CONST_SE3) */
    const double  *frame_inertia;     /* [n_frames*4] mass, Ixx, Iyy, Izz */
    const int32_t *frame_cache_size;  /* [n_frames]  number of configs on the path world->frame */
    const int32_t *frame_cache_index; /* [n_frames*(n_configs+1)] path configs, padded with -1 */
    /* configs: the n_dyn dynamic ones first, then the n_kin kinematic ones */
    const int32_t *config_kinematic;  /* [n_configs] 0/1 */
    const int32_t *config_k_index;    /* [n_configs] index among kinematic configs, -1 if dynamic */
    const int32_t *config_gen;        /* [n_configs] position in every dependent frame's path; n_configs if none */
    const int32_t *config_masses_off; /* [n_configs+1] CSR offsets into config_masses */
    const int32_t *config_masses;     /* frame indices of the massive frames depending on each config */
    const int32_t *masses;            /* [n_masses] frame indices with non-zero inertia */
    /* potentials / forces */
    const double  *gravity;           /* [n_gravity*3] */
    const double  *damping;           /* [n_damping*n_dyn] */
    const int32_t *config_force_config; /* [n_config_forces] config index */
    const int32_t *config_force_input;  /* [n_config_forces] input index */
    /* holonomic constraints */
    const int32_t *constraint_type;      /* [n_constraints] */
    const int32_t *constraint_frame1;    /* [n_constraints] */
    const int32_t *constraint_frame2;    /* [n_constraints] */
    const int32_t *constraint_config;    /* [n_constraints] distance: kinematic length config or -1 */
    const int32_t *constraint_component; /* [n_constraints] point: 0,1,2 */
    const double  *constraint_distance;  /* [n_constraints] distance: constant length if no config */
    const double  *constraint_tolerance; /* [n_constraints] */
    /* potentials on single configs: V = 1/2 k (q - q0)^2 (potentials/configspring.c:15-45) */
    int32_t n_config_springs;
    const int32_t *config_spring_config; /* [n_config_springs] config index */
    const double  *config_spring_k;      /* [n_config_springs] */
    const double  *config_spring_q0;     /* [n_config_springs] */
    /* springs between the origins of two frames: V = 1/2 k (|p1 - p2| - x0)^2 (potentials/linearspring.c:16-78).
     * Like the reference, which defines V, V_dq and V_dqdq only, systems with such springs have no second
     * derivatives of the step map (tg_batch_deriv2_* return TG_ERR_UNSUPPORTED). */
    int32_t n_linear_springs;
    const int32_t *linear_spring_frame1; /* [n_linear_springs] */
    const int32_t *linear_spring_frame2; /* [n_linear_springs] */
    const double  *linear_spring_k;      /* [n_linear_springs] */
    const double  *linear_spring_x0;     /* [n_linear_springs] */
    /* TG_CONSTRAINT_PLANE: h = (R(frame1) n) . (p(frame1) - p(frame2)), frame1 = plane frame, frame2 = point frame
     * (constraints/plane.c:13-26) */
    const double  *constraint_normal;    /* [n_constraints*3] plane normal n in plane-frame coordinates (others: zeros) */
    /* forces/hybridwrench.c: a wrench applied at the origin of a frame, force and torque both given by their world-frame
     * components; each of the six components (fx, fy, fz, tx, ty, tz) is an input or a constant. */
    int32_t n_hybrid_wrenches;
    const int32_t *hybrid_wrench_frame;  /* [n_hybrid_wrenches] */
    const int32_t *hybrid_wrench_input;  /* [n_hybrid_wrenches*6] input index of each component, or -1 for a constant */
    const double  *hybrid_wrench_const;  /* [n_hybrid_wrenches*6] the constant components */
    const int32_t *hybrid_wrench_kind;   /* [n_hybrid_wrenches] 0: HybridWrench; 1: SpatialWrench (forces/spatialwrench.c: all six
                                          * coefficients from g_dq g^-1, the joint's spatial twist); 2: BodyWrench
                                          * (forces/bodywrench.c: from g^-1 g_dq, the body twist) */
    /* forces/lineardamper.c: f = -c (d/dt |p1 - p2|) d|p1 - p2|/dq between the origins of two frames. */
    int32_t n_linear_dampers;
    const int32_t *linear_damper_frame1; /* [n_linear_dampers] */
    const int32_t *linear_damper_frame2; /* [n_linear_dampers] */
    const double  *linear_damper_c;      /* [n_linear_dampers] */
    /* potentials/nonlinear_config_spring.c:24-61: dV/dq = -y(m q + b) on one config, y a piecewise-quintic Spline
     * (trep/spline.py:6-259, evaluation _trep/spline.c:8-57).  Spring i uses the table rows first[i] .. first[i+1]-1, one row per
     * polynomial piece in x order: (left knot, a, b, c, d, e, f), y = a t^5 + b t^4 + c t^3 + d t^2 + e t + f with t = x - left knot;
     * the first / last piece also serve x below / above the knots. */
    int32_t n_nonlinear_springs;
    const int32_t *nonlinear_spring_config; /* [n_nonlinear_springs] config index */
    const double  *nonlinear_spring_m;      /* [n_nonlinear_springs] */
    const double  *nonlinear_spring_b;      /* [n_nonlinear_springs] */
    const int32_t *nonlinear_spring_first;  /* [n_nonlinear_springs + 1] CSR offsets into the rows of nonlinear_spring_pieces */
    const double  *nonlinear_spring_pieces; /* [rows * 7] */
} tg_system_desc;

/* Per-trajectory status written by every solve (reference: ConvergenceError / ValueError("singular")
 * raised from MidpointVI_solve_DEL, midpointvi.c:715-718, math-code.c:393-398). */
enum { TG_OK = 0, TG_NOT_CONVERGED = 1, TG_SINGULAR = 2 };

/* Library-level error codes returned by the functions below (0 = success). */
enum { TG_SUCCESS = 0, TG_ERR_INVALID = -1, TG_ERR_HIP = -2, TG_ERR_UNSUPPORTED = -3, TG_ERR_STATE = -4 };

/* Batch state fields for tg_batch_set / tg_batch_get (row-major [batch][width]). */
enum {
    TG_F_Q1 = 0,      /* width nq */
    TG_F_Q2 = 1,      /* width nq */
    TG_F_P1 = 2,      /* width nd */
    TG_F_P2 = 3,      /* width nd */
    TG_F_U1 = 4,      /* width nu */
    TG_F_LAMBDA1 = 5, /* width nc */
    /* first derivatives (valid after tg_batch_deriv1); [deriv var][output] like the reference
     * (trep.h:425-437): */
    TG_F_Q2_DQ1 = 10, /* nq x nd */
    TG_F_Q2_DP1 = 11, /* nd x nd */
    TG_F_Q2_DU1 = 12, /* nu x nd */
    TG_F_Q2_DK2 = 13, /* nk x nd */
    TG_F_P2_DQ1 = 14, TG_F_P2_DP1 = 15, TG_F_P2_DU1 = 16, TG_F_P2_DK2 = 17,
    TG_F_L1_DQ1 = 18, /* nq x nc */
    TG_F_L1_DP1 = 19, TG_F_L1_DU1 = 20, TG_F_L1_DK2 = 21
};

typedef struct tg_system tg_system;
typedef struct tg_batch tg_batch;

const char *tg_version(void);
const char *tg_last_error(void);
/* Number of visible HIP devices (<=0: none; the library then refuses to create batches). */
int tg_device_count(void);
/* out[0..3] = compute units, LDS bytes a workgroup may use (opt-in maximum), wavefront size, 0 */
int tg_device_info(int32_t device, int32_t out[4]);

/* Compile the flattened system into the device schedule.  The descriptor is copied. */
tg_system *tg_system_create(const tg_system_desc *desc);
void tg_system_destroy(tg_system *sys);
/* sizes: out[0..5] = nq, nd, nk, nu, nc, nX(=nq+nd+nk) */
int tg_system_sizes(const tg_system *sys, int32_t out[6]);

/* Introspection: out[0..7] = team size (lanes per trajectory), LDS bytes per trajectory, joints,
 * levels, bodies, (body,config) items, (item,item) pairs, constraint-Jacobian items. */
int tg_system_info(const tg_system *sys, int32_t out[8]);

/* A batch of `batch` independent trajectories of `sys` resident on HIP device `device`. */
tg_batch *tg_batch_create(tg_system *sys, int32_t batch, int32_t device);
void tg_batch_destroy(tg_batch *b);
/* Newton tolerance on |DEL| (reference MidpointVI.tolerance, default 1e-10). */
int tg_batch_set_tolerance(tg_batch *b, double tolerance);
/* Integrator times, shared by the whole batch (reference MidpointVI.t1/.t2). */
int tg_batch_set_times(tg_batch *b, double t1, double t2);
int tg_batch_get_times(const tg_batch *b, double *t1, double *t2);
/* Copy a state field host->device / device->host. */
int tg_batch_set(tg_batch *b, int32_t field, const double *host);
int tg_batch_get(tg_batch *b, int32_t field, double *host);
int tg_batch_field_width(const tg_batch *b, int32_t field);

/* p2 = D2 L_d(q1, q2) at the current (q1,q2,t1,t2): reference MidpointVI.calc_p2
 * (midpointvi.c:491-504 via :2691-2700). */
int tg_batch_calc_p2(tg_batch *b);
/* DEL residual f (width nd+nc) at the current state: reference MidpointVI.calc_f
 * (midpointvi.c:567-575). */
int tg_batch_calc_f(tg_batch *b, double *f_host);

/*
 * One MidpointVI.step for every trajectory (reference trep/midpointvi.py:174-201 +
 * MidpointVI_solve_DEL, midpointvi.c:691-747): q1<-q2, p1<-p2, t1<-t2, t2<-t2_new,
 * u1<-u1_host, q2[nd:]<-k2_host, optional q2 / lambda1 hints, Newton solve, p2.
 * u1_host [batch][nu], k2_host [batch][nk] (NULL allowed when the width is 0);
 * q2_hint_host [batch][nd] or NULL; lambda_hint_host [batch][nc] or NULL.
 * iterations_out / status_out: [batch] or NULL.  Returns TG_SUCCESS even when some
 * trajectories fail: inspect status_out.
 */
int tg_batch_step(tg_batch *b, double t2_new, const double *u1_host, const double *k2_host,
                  const double *q2_hint_host, const double *lambda_hint_host,
                  int32_t max_iterations, int32_t *iterations_out, int32_t *status_out);

/*
 * Device-resident rollout: n_steps consecutive steps of size dt in ONE kernel launch,
 * starting from the batch's current (t2, q2, p2, lambda1).  U_dev [batch][n_steps][nu]
 * and K_dev [batch][n_steps][nk] are DEVICE pointers (NULL when the width is 0);
 * X_dev, if not NULL, is a DEVICE buffer [batch][n_steps+1][nX] receiving the DSystem-style
 * state X_k = [q2 ; p2 ; v2] (reference trep/discopt/dsystem.py:11-63) for k = 0..n_steps.
 * iterations are accumulated per trajectory (tg_batch_rollout_stats).  Asynchronous on the
 * batch's stream; tg_batch_synchronize waits.
 */
int tg_batch_rollout(tg_batch *b, int32_t n_steps, double dt, const double *U_dev,
                     const double *K_dev, double *X_dev, int32_t max_iterations);
/*
 * Closed-loop rollout (the projection operator of trep.discopt: DSystem.project, dsystem.py:426-451, and
 * DOptimizer.armijo_simulate, doptimizer.py:405-428): the inputs are computed in the kernel,
 *   U_k = bU_k - Kproj_k (X_k - bX_k),   X_k = [q2; p2; v2],   U_k = [u1; k2],
 * Kproj_dev [groups][n_steps][nU][nX] with one gain schedule per `group_size` consecutive trajectories
 * (e.g. all Armijo candidates of one seed), bX_dev [batch][n_steps+1][nX], bU_dev [batch][n_steps][nU].
 * X_dev [batch][n_steps+1][nX] and U_dev [batch][n_steps][nU] (either may be NULL) receive the projected
 * trajectory.  Starts from the batch's current (t2, q2, p2, lambda1) like tg_batch_rollout.
 */
int tg_batch_rollout_closed_loop(tg_batch *b, int32_t n_steps, double dt, const double *Kproj_dev, int32_t group_size,
                                 const double *bX_dev, const double *bU_dev, double *X_dev, double *U_dev,
                                 int32_t max_iterations);
int tg_batch_rollout_stats(tg_batch *b, int64_t *total_iterations, int32_t *n_failed);
int tg_batch_status(tg_batch *b, int32_t *iterations_out, int32_t *status_out);
/* Per trajectory, for the last rollout / step launch: how many of its Newton systems (reference: one LU_decomp per Newton iteration,
 * midpointvi.c:720-733) the structured solve of a specialised kernel handed to the pivoting solver because a pivot guard failed.
 * Results are the same either way; a batch that reports fallbacks for most systems (time steps <= 1e-3, very heavy bodies) would run
 * faster with tg_batch_set_pivot_rule(b, 1) or without a specialised kernel.  Zeros from kernels without a structured solve. */
int tg_batch_solver_fallbacks(tg_batch *b, int32_t *fallbacks_out);

/* Device-side snapshot / restore of the whole integrator state (q1,q2,p1,p2,lambda1,u1,t1,t2):
 * asynchronous device-to-device copies on the batch's stream.  Lets a caller replay rollouts from
 * the same state (line-search candidates, benchmarks) without touching the host. */
int tg_batch_snapshot(tg_batch *b);
int tg_batch_restore(tg_batch *b);

/* First derivatives of the last solved step (reference MidpointVI_calc_deriv1,
 * midpointvi.c:1100-1120); results are read with tg_batch_get(TG_F_Q2_DQ1 ...). */
int tg_batch_deriv1(tg_batch *b);

/*
 * Second derivatives of the last solved step, contracted with z over the output index
 * (reference MidpointVI_calc_deriv2, midpointvi.c:2516-2545, as consumed by DSystem.fdxdx / fdxdu /
 * fdudu, trep/discopt/dsystem.py:320-386):
 *   hz[b][A][B] = sum_o z[b][o] * q2_dAdB[A][B][o] + z[b][nq+o] * p2_dAdB[A][B][o]
 * with the derivative variables ordered A,B in (q1[nq], p1[nd], u1[nu], k2[nk]); R = nq+nd+nu+nk.
 * z_host [batch][nX] (only the Qd and p parts are read, like the reference), hz_host [batch][R][R].
 * The full [A][B][out] tensors are never materialised.
 */
int tg_batch_deriv2_contract(tg_batch *b, const double *z_host, double *hz_host);
/* Same with an additional weight vector on the multiplier outputs (either vector may be NULL = zeros):
 *   hz[b][A][B] += sum_c zlambda[b][c] * l1_dAdB[A][B][c]      (the reference's _l1_dAdB tensors, trep.h:439-473;
 * in the implicit-function solve this is a seed on the constraint rows of the adjoint vector). */
int tg_batch_deriv2_contract_lambda(tg_batch *b, const double *z_host, const double *zlambda_host, double *hz_host);

/* Device memory helpers so a host language without a HIP binding can stage inputs. */
void *tg_device_alloc(int32_t device, uint64_t bytes);
int tg_device_free(int32_t device, void *ptr);
int tg_memcpy_h2d(int32_t device, void *dst_dev, const void *src_host, uint64_t bytes);
int tg_memcpy_d2h(int32_t device, void *dst_host, const void *src_dev, uint64_t bytes);

int tg_batch_synchronize(tg_batch *b);
/* Use an externally created hipStream_t (e.g. torch's current stream); NULL = own stream. */
int tg_batch_set_stream(tg_batch *b, void *hip_stream);
/* Non-uniform time base.  The reference's DSystem takes an arbitrary time vector (trep/discopt/dsystem.py:229-274: every
 * set / step uses t[k+1] - t[k]).  A list of `count` step sizes on the batch replaces the scalar dt of the entry points
 * below it: by_trajectory = 0: step k of a rollout / closed-loop rollout uses dt[k] (n_steps <= count); by_trajectory = 1:
 * trajectory t of a one-step batch (tg_batch_step, tg_batch_set_from_trajectories and the derivative kernels that follow:
 * batch = seeds x horizon) uses dt[t % count].  count = 0 removes the list.
 *   - A refused call (TG_ERR_INVALID: a zero or non-finite entry) changes nothing: the list set before stays in use.
 *   - A by-step list belongs to the rollouts.  The one-step entry points (tg_batch_step, tg_batch_set_from_trajectories) step by
 *     what the caller passes (t2_new - t2, dt) unless the list is by trajectory.
 *   - While a by-trajectory list is set, EVERY kernel mode takes the trajectory's size for t2 - t1: the derivative kernels, calc_f, and
 *     calc_p2 (tg_batch_calc_p2 of an initialisation from two configurations included: set the list after it).
 *   - A by-trajectory list belongs to one-step launches.  A rollout or closed-loop rollout of more than one step is refused with
 *     TG_ERR_INVALID while one is set, before anything is launched. */
int tg_batch_set_step_sizes(tg_batch *b, int32_t count, const double *dt_host, int32_t by_trajectory);

/* Pivot rule of the Newton-system solve (replaces LU_decomp + LU_solve_vec, math-code.c:337-461, as used by
 * MidpointVI_solve_DEL, midpointvi.c:720-733).  Both settings are Gauss-Jordan with implicit row scaling and partial
 * pivoting over the rows not used yet, singular if the scaled pivot is <= 1e-20:
 *   exact = 0 (default): candidates are ranked in single precision (one 32-bit wave max per step); candidates within
 *       2^-17 relative of each other are taken in row order.  Fast; the solution agrees with the reference's to rounding.
 *   exact = 1: the reference's rule bit for bit -- fp64 comparison, ties to the first row of its (swapped) row order,
 *       exact singular test -- i.e. the same pivot ROW for every column, also where candidates differ by one ulp
 *       (every row's largest entry scales to 1 +- 1 ulp, so that happens in most puppet solves).  About 9 % slower.
 * Full-wave teams with 17..31 unknowns (the puppet: 28) run the default rule as gj_panel -- panels of four columns eliminated one
 * row per lane, the trailing matrix kept in the accumulator layout of v_mfma_f64_16x16x4_f64 and updated on the matrix cores --
 * which ranks the candidates exactly as above and differs in rounding only (block update instead of four rank-1 updates).
 * tg_debug_solve (test hook) solves [A | b] (row-major [n][n+1], n <= 32) with either rule (exact = 0 / 1; exact = 2: the default
 * rule through gj_panel, 16 < n < 32) and reports which original row served as pivot of each column; status TG_OK or TG_SINGULAR. */
int tg_batch_set_pivot_rule(tg_batch *b, int32_t exact);
int tg_debug_solve(int32_t device, int32_t n, int32_t exact, const double *A_aug_host, double *x_host, int32_t *pivot_rows_host, int32_t *status_host);
/* Structured Newton solve (csrc/bbd.hpp; system-specialised rollout kernels, default pivot rule).  The reference factors the dense
 * matrix with a pivot search per column (midpointvi.c:720-733 -> math-code.c:337-461).  For a tree mechanism the matrix
 * [[Df11, -Dh1^T], [Dh2, 0]] is bordered block diagonal -- the limbs couple only through the trunk's configs and the constraints --
 * and Df11 = -M/dt + O(dt) needs no pivot search: the schedule compiler derives the blocks from the matrix's structural pattern,
 * the kernel eliminates the blocks side by side on 16-lane DPP rows, then the dense border system (configs first, constraints
 * last), and back-substitutes.  Every pivot is guarded (|pivot| > 2^-20 of its row's largest entry); a failed guard hands the
 * untouched matrix to the pivoting solver above, so singular systems are reported exactly as before.
 * tg_batch_debug_newton_solve (test hook) runs that solve -- as compiled into the batch's loaded specialised library -- on
 * n_mats caller-supplied systems [nf][nf + 1]; path[m] = 1 structured, 2 pivoting solver (guard failed, no plan, or
 * skip_structured != 0), -1 singular. */
/* tg_system_newton_plan (host only): out[0..7] = plan found, groups, largest own block, largest border list, trailing size, nf, nd, 0;
 * pattern (optional, [nf * nf]): structural non-zeros of the Newton matrix (symmetrised); tab (optional, [128]): packed plan tables. */
int tg_system_newton_plan(const tg_system *sys, int32_t out[8], uint8_t *pattern, int32_t *tab);
int tg_batch_debug_newton_solve(tg_batch *b, int32_t n_mats, int32_t skip_structured, const double *A_aug_host, double *x_host, int32_t *path_host);

/* System-specialised rollout kernel.  The reference interprets the frame tree at run time; the generic kernels here
 * interpret a flat schedule.  For long rollouts of one system the schedule can instead be compiled into the kernel:
 * tg_system_spec_header returns a generated C++ header (every size, count and LDS offset a constant, the index tables
 * constant arrays); trep_amd/specialize.py compiles csrc/spec_kernel.hip against it with hipcc and
 * tg_batch_load_specialized makes the rollouts of a batch use that kernel (same template source as the generic
 * kernel: identical Newton iteration counts, states equal up to the compiler's FMA contraction choices, <= 1e-12
 * relative).  Returns the text length incl. terminator (or -1).
 * tg_system_spec_key is the 64-bit FNV-1a hash of that text; a specialised library exports the key of the header it
 * was compiled against (tg_spec_key) and tg_batch_load_specialized refuses a library whose key or sizes differ.
 * tg_batch_info: out[0] bit m = kernel mode m has a specialised kernel loaded; out[1] / out[2] bit m = a mode-m launch
 * went through a specialised / generic kernel since the batch was created; out[3] / out[4] = number of such launches;
 * out[5] pivot rule; out[6] team size; out[7] bits 0-7 wavefronts per trajectory in the loaded library's derivative kernels (1, or 2
 * with helper waves), bits 8-15 fb_n: the joints of the floating base's translational prefix whose terms the loaded rollout kernel
 * takes in closed form, as that library reports it (0: none, compiled out, or no specialised library), bits 16-23
 * tr_n: the joints of translation runs whose world poses the loaded rollout kernel stores directly instead of sweeping them, as that
 * library reports it (0 likewise), bit 24: the loaded rollout kernel takes the poses of a step's first evaluation behind
 * the step edge from the q2 poses of the converged evaluation before it, bits 25-28 the joints without a q2 twin whose q2 pose it keeps
 * for that (carried poses; 0 likewise).  (Modes: 0 rollout/step, 1 calc_p2, 2 calc_f, 3 deriv1, 4 deriv2z, 5.. dynamics.) */
int64_t tg_system_spec_header(const tg_system *sys, char *buf, uint64_t capacity);
uint64_t tg_system_spec_key(const tg_system *sys);
int tg_batch_load_specialized(tg_batch *b, const char *library_path);
int tg_batch_info(const tg_batch *b, int32_t out[8]);
/* The HIP stream (hipStream_t) the batch launches on, for ordering foreign work after it (tg_comm_wait_stream). */
void *tg_batch_stream(tg_batch *b);

/* HIP-event timing of the kernels launched on the batch's stream since the last reset (opt-in: the first call switches
 * the per-launch events on and returns zeros; launches before it are not timed):
 * number of launches and the sum of their durations in milliseconds. */
int tg_batch_timing(tg_batch *b, int32_t reset, int32_t *n_launches, double *total_ms);

/* Per-trajectory parameters: one batch, many parameter sets, without rebuilding the schedule or the specialised kernels.
 * The reference changes them one system at a time with Frame.set_mass (trep/frame.py), the Gravity.gravity setter
 * (trep/potentials/gravity.py) and Damping.set_damping_coefficient (trep/forces/damping.py); a row of the table acts as a
 * system rebuilt with its values.  Blocks of a row:
 *   inertia [n_bodies][4]  (mass, Ixx, Iyy, Izz) of every massive frame, in System.masses order
 *   gravity [3]            the gravity vector (sum over the system's Gravity potentials)      -- systems with a Gravity only
 *   damping [nd]           total damping coefficient of every dynamic config                  -- systems with a Damping only
 * tg_system_parameters: sizes_out = n_bodies, nd, has_gravity, has_damping, and the system's own values (null outputs skipped).
 * tg_batch_set_parameters: `rows` rows per block (null block: the system's values in every row); trajectory t -- its batch
 * index after any subset remapping -- uses row t / group; rows * group == batch, or rows == 1 for the whole batch.  Values must
 * be finite (a zero mass is allowed); a massless frame stays massless.  TG_ERR_INVALID, with the table unchanged, for bad
 * shapes, non-finite values or a block the system does not have.  The upload is ordered on the batch's stream: launches already
 * enqueued keep their table.  While a table is set every mode runs a parameter kernel (the loaded specialised library's if it
 * has one for the mode -- rollout, deriv1, deriv2z -- else the generic one); the forward-mode entry points (*_forward) return
 * TG_ERR_UNSUPPORTED.  tg_batch_clear_parameters returns to the default kernels.
 * tg_batch_par_info: out[0] bit m = mode m has a specialised parameter kernel loaded; out[1] / out[2] bit m = a mode-m launch went
 * through a specialised / generic parameter kernel; out[3] / out[4] the number of such launches (tg_batch_info counts only the
 * default kernels); out[5] rows of the current table (0: none); out[6] its group; out[7] 0. */
int tg_system_parameters(const tg_system *sys, int32_t sizes_out[4], double *inertia, double *gravity, double *damping);
int tg_batch_set_parameters(tg_batch *b, int32_t rows, int32_t group, const double *inertia_host, const double *gravity_host,
                            const double *damping_host);
int tg_batch_clear_parameters(tg_batch *b);
int tg_batch_par_info(const tg_batch *b, int32_t out[8]);

/* ------------------------------------------------------------------------------------------------------
 * Device-side discopt primitives: the direct caller of the MidpointVI path.
 * Everything below takes DEVICE pointers (tg_device_alloc) and is asynchronous; tg_device_synchronize or any
 * tg_memcpy_* waits.  "Seeds" are independent optimisation problems of the same system and horizon N:
 *   X [S][N+1][nX], U [S][N][nU], A [S][N][nX][nX], B [S][N][nX][nU], K [S][N][nU][nX] ...
 * `select_dev` (optional, int32 [n_problems]) restricts a call to a subset of the seeds.
 * ------------------------------------------------------------------------------------------------------ */

/* ---- continuous dynamics -------------------------------------------------------------
 * Replaces calc_dynamics (system.c:749-893) behind System.f() / System.lambda_() (system.py:951-959, 1018-1024),
 * for every trajectory of the batch at once: accelerations of the dynamic configs and constraint forces at the state
 * (q [B][nq], dq [B][nq], u [B][nu], ddq of the kinematic configs [B][nk]).  Outputs ddq [B][nd], lambda [B][nc],
 * status [B] (TG_OK or TG_SINGULAR; may be NULL).  Arrays of zero width may be NULL.  The integrator state of the
 * batch (q1, q2, p, lambda1, caches) is not touched.  The _device variant takes device pointers, launches on the
 * batch's stream and does not synchronise. */
int tg_batch_dynamics(tg_batch *b, const double *q_host, const double *dq_host, const double *u_host,
                      const double *ddqk_host, double *ddq_host, double *lambda_host, int32_t *status_host);
int tg_batch_dynamics_device(tg_batch *b, const double *q_dev, const double *dq_dev, const double *u_dev,
                             const double *ddqk_dev, double *ddq_dev, double *lambda_dev, int32_t *status_dev);
/* First derivatives of the same map: calc_dynamics_deriv1 (system.c:912-1299) behind System.f_dq(), f_ddq(), f_dddk(),
 * f_du(), lambda_dq(), lambda_ddq(), lambda_dddk(), lambda_du() (system.py:961-980, 1026-1044).  Arrays are laid out
 * like the reference's internal ones, derivative variable first: f_dq, f_ddq [B][nq][nd]; f_dddk [B][nk][nd];
 * f_du [B][nu][nd]; lambda_* the same with nc outputs.  Any output may be NULL (not wanted).  The _device variant takes
 * the eight device pointers in that order. */
int tg_batch_dynamics_deriv1(tg_batch *b, const double *q_host, const double *dq_host, const double *u_host,
                             const double *ddqk_host, double *f_dq, double *f_ddq, double *f_dddk, double *f_du,
                             double *lambda_dq, double *lambda_ddq, double *lambda_dddk, double *lambda_du,
                             int32_t *status_host);
int tg_batch_dynamics_deriv1_device(tg_batch *b, const double *q_dev, const double *dq_dev, const double *u_dev,
                                    const double *ddqk_dev, double *const out_dev[8], int32_t *status_dev);
/* First and second derivatives of the Lagrangian of every state of the batch, for every config / pair of configs
 * (System_L_dq, L_ddq, L_dqdq, L_ddqdq, L_ddqddq, system.c:129-489 behind System.L_dq() ... System.L_ddqddq(),
 * system.py:852-925).  first [B][2][nq] = (L_dq, L_ddq); second [B][3][nq][nq] = (L_dqdq, L_ddqdq with the velocity
 * config as the row and the configuration config as the column, L_ddqddq). */
int tg_batch_lagrangian(tg_batch *b, const double *q_host, const double *dq_host, double *first_host, double *second_host);
/* Forward-mode (dual-number) runs of the two calls above: every elementary operation of the analytic kernel carries its exact
 * derivative along one input variable per trajectory (csrc/dual.hpp) -- no step size, no truncation error.  seed [B]: the
 * variable, numbered q [nq] | dq [nq] | ddq_k [nk] | u [nu] (-1: none, the outputs are then zero).  The outputs have the layout
 * of the plain call and hold the DERIVATIVE of each entry along that variable:
 *   tg_batch_dynamics_deriv1_forward -- the second derivatives of the continuous dynamics: replaces calc_dynamics_deriv2
 *     (system.c:1301-2029; M_dqdq, D_dqdq ... lambda_dudu, f_dudu) behind System.f_dqdq() ... lambda_dudu() (system.py:982-1078):
 *     d f_dq / d q_j = f_dqdq[., j], d f_ddq / d q_j = f_ddqdq[., j], d f_ddq / d dq_j = f_ddqddq[., j], ... one variable per trajectory;
 *   tg_batch_lagrangian_forward -- the third derivatives of the Lagrangian (one seed: System_L_dqdqdq, L_ddqdqdq, L_ddqddqdq,
 *     system.c:204-268, 336-393, 491-530) and the fourth (seed2 not NULL: L_ddqdqdqdq, L_ddqddqdqdq, system.c:395-457, 532-622),
 *     behind System.L_dqdqdq() ... L_ddqddqdqdq() (system.py:869-949).
 * One wavefront per trajectory whatever the system's team size; TG_ERR_UNSUPPORTED if the dual-number slice exceeds the LDS. */
int tg_batch_dynamics_deriv1_forward(tg_batch *b, const double *q_host, const double *dq_host, const double *u_host,
                                     const double *ddqk_host, const int32_t *seed_host, double *f_dq, double *f_ddq,
                                     double *f_dddk, double *f_du, double *lambda_dq, double *lambda_ddq,
                                     double *lambda_dddk, double *lambda_du, int32_t *status_host);
int tg_batch_lagrangian_forward(tg_batch *b, const double *q_host, const double *dq_host, const int32_t *seed1_host,
                                const int32_t *seed2_host, double *first_host, double *second_host);

/* Initial guess of the Newton iteration in the device-resident rollouts.  0 (default): the reference's, q2 <- the previous
 * q2 (midpointvi.py:188-197) -- iteration counts then match the reference's.  1: constant-velocity extrapolation
 * q2 + (q2 - q1) dt_k / dt_{k-1} (the last displacement, scaled by the step ratio on a non-uniform time base); same root
 * to within the solver tolerance, about one Newton iteration fewer per step.  An opt-in that departs from the reference's
 * iteration-by-iteration behaviour; the headline benchmark uses 0. */
int tg_batch_set_predictor(tg_batch *b, int32_t mode);

/* Kinetic and potential energy of every state of the batch: energy[b] = {T, V} with T = sum over the massive frames of
 * 1/2 <v_b, I v_b> and V the sum of the potentials, so that System.L() = T - V and System.total_energy() = T + V
 * (System_L / System_total_energy, system.c:78-127).  q, dq [B][nq]; energy [B][2]. */
int tg_batch_energy(tg_batch *b, const double *q_host, const double *dq_host, double *energy_host);

/* ---- batched constraint projection ---------------------------------------------------------------------------------
 * System.satisfy_constraints (reference trep/system.py:158-214) for every trajectory of the batch at once, in one launch:
 * per trajectory, minimise 1/2 |q - q0|^2 over the FREE configs subject to h(q) = 0, the other configs held at their input
 * values.  free [nq]: non-zero = free, the same set for the whole batch (NULL: every config; the reference's keep_kinematic
 * is the dynamic configs, its constant_q_list everything outside the list).  Newton on the KKT conditions with the constraint
 * curvature: from q = q0, mu = 0, with D = Dh(q)[:, F] and g = (q - q0)_F + D' mu, each step solves
 *   [[I + sum_c mu_c h_c,qq (F x F), D'], [D, 0]] (dq_F, dmu) = -(g, h).
 * A trajectory is converged when max |h| <= tolerance and max |g| <= tolerance at the current iterate, tested before stepping.
 * status [B]: TG_OK converged; TG_NOT_CONVERGED max_iterations steps were taken, q is the last iterate; TG_SINGULAR the solver
 * rejected the KKT matrix, q is the iterate before that solve.  With an empty free set or nc == 0 nothing is solved: TG_OK if the
 * input passes the test (always for nc == 0), else TG_SINGULAR, q unchanged.  No damping or globalisation: a perturbation too
 * large for plain Newton reports a status.  iterations [B]: steps taken.  q, dq [B][nq]; mu [B][nc] the multipliers.
 * Velocity part (dq not NULL; dq_out then required): for converged trajectories dq_out = dq with dq_F -= D' nu,
 * D D' nu = Dh(q) dq at the converged pose -- the nearest rates tangent to the constraints, Dh(q) dq_out = 0, the fixed rates
 * kept; dq is returned unchanged for the others (and a rejected velocity solve also reports TG_SINGULAR).
 * mu_out, iterations_out, status_out may be NULL.  Outputs may alias inputs.  Generic kernel of its own (mode 9 in
 * tg_batch_info) whatever library or parameter table the batch has: constraints do not depend on inertia, gravity or damping.
 * The integrator state of the batch (q1, q2, p, lambda1, status, iterations) is not touched.  TG_ERR_INVALID for tolerance <= 0,
 * max_iterations < 0, a null q or q_out, or dq_out without dq; TG_ERR_UNSUPPORTED if the workgroup's LDS -- per team the rollout
 * slice plus (n + 1) n + n + nq + nq / 2 doubles, n = nq + nc -- exceeds 160 KiB (tg_system_projection_lds: out = team size,
 * doubles per team, bytes per workgroup, 0; the same refusal, computed without a device).
 * The _device variant takes device pointers, launches on the batch's stream and does not synchronise. */
int tg_system_projection_lds(const tg_system *sys, int32_t out[4]);
int tg_batch_project_constraints(tg_batch *b, const double *q_host, const double *dq_host, const int32_t *free_host,
                                 double tolerance, int32_t max_iterations, double *q_out, double *dq_out, double *mu_out,
                                 int32_t *iterations_out, int32_t *status_out);
int tg_batch_project_constraints_device(tg_batch *b, const double *q_dev, const double *dq_dev, const int32_t *free_dev,
                                        double tolerance, int32_t max_iterations, double *q_out_dev, double *dq_out_dev,
                                        double *mu_out_dev, int32_t *iterations_out_dev, int32_t *status_out_dev);

/* ---- batched equilibrium search -----------------------------------------------------------------------------------
 * System.minimize_potential_energy (reference trep/system.py:215-272) for every pose of the batch at once, in one launch: per
 * pose, minimise V(q) over the FREE configs subject to h(q) = 0, the other configs held at their input values bit for bit.
 * free [nq] as in tg_batch_project_constraints (NULL: every config).  A safeguarded Newton iteration on the KKT conditions
 * (tests/equilibrium_reference.py is its specification).  At (q, mu): D = Dh(q)[:, F], g = V_q[F] + D' mu,
 * W = V_qq[F, F] + sum_c mu_c h_c,qq[F, F].  From q = q0 with the least-squares multipliers of the start
 * ([[I, D'], [D, 0]] (d, mu) = (-V_q[F], 0); zero where that matrix is rejected), tau = 0, rho = 0.  A pose is converged when
 * max |h| <= tolerance and max |g| <= tolerance (a NaN fails the test).  Otherwise a trial, each of which counts toward
 * max_iterations and is rejected if it fails any of: (1) W + tau I + sigma D'D has an unpivoted Cholesky factor, with
 * sigma = 1e8 wmax / max diag(D'D), wmax = max |diag W|; (2) [[W + tau I, D'], [D, 0]] (d, dmu) = -(g, h) is solved and the
 * step is finite; (3) at the trial point (q_F + d, mu + dmu), with rho+ = max(rho, 2 |mu + dmu|inf) and phi = V + rho+ |h|_1 on
 * both sides, phi_trial <= phi + 64 eps max(1, |phi|) -- or, while tau <= 1e-3 wmax, the KKT residual max(|h|inf, |g|inf) of the
 * trial point is at most half the current one.  Accepted: tau /= 4, and 0 once under 1e-6 wmax.  Rejected:
 * tau = max(4 tau, 1e-3 wmax); tau > 1e9 wmax ends the search.
 * status [B]: TG_OK converged (a minimum: (1) held at every accepted step); TG_NOT_CONVERGED max_iterations trials were made, q is
 * the last accepted iterate; TG_SINGULAR tau ran out, or nothing is free and the input does not pass the test.  A system without
 * constraints is a normal case.  iterations [B]: trials made.  q [B][nq]; mu [B][nc]; v_out [B][2]: V at the start and at the
 * returned pose.  mu_out, v_out, iterations_out, status_out may be NULL.  q_out may alias q.
 * Generic kernel of its own (mode 10 in tg_batch_info) whatever library the batch has; with a parameter table
 * (tg_batch_set_parameters) its parameter twin runs (mode 10 in tg_batch_par_info) and every pose uses its row's masses, inertias
 * and gravity -- damping plays no part.  The integrator state of the batch (q1, q2, p, lambda1, status, iterations) is not touched.
 * TG_ERR_INVALID for tolerance <= 0, max_iterations < 0, a null q or q_out; TG_ERR_UNSUPPORTED for a system with a
 * NonlinearConfigSpring (its V() is 0 in the reference while its force is not: there is no potential to minimise), for the
 * profiling build, and if the workgroup's LDS -- per team the rollout slice plus (n + 1) n + 2 nq^2 + 2 n + 3 nq + 2 + nq / 2
 * doubles, n = nq + nc -- exceeds 160 KiB (tg_system_equilibrium_lds: out = team size, doubles per team, bytes per workgroup, 0;
 * the same refusals, computed without a device).
 * The _device variant takes device pointers, launches on the batch's stream and does not synchronise. */
int tg_system_equilibrium_lds(const tg_system *sys, int32_t out[4]);
int tg_batch_minimize_potential(tg_batch *b, const double *q_host, const int32_t *free_host, double tolerance,
                                int32_t max_iterations, double *q_out, double *mu_out, double *v_out, int32_t *iterations_out,
                                int32_t *status_out);
int tg_batch_minimize_potential_device(tg_batch *b, const double *q_dev, const int32_t *free_dev, double tolerance,
                                       int32_t max_iterations, double *q_out_dev, double *mu_out_dev, double *v_out_dev,
                                       int32_t *iterations_out_dev, int32_t *status_out_dev);

/* ---- batched normal modes ------------------------------------------------------------------------------------------
 * The small-oscillation eigenproblem K phi = omega^2 M phi on the tangent space of the constraints, for every pose of the batch in
 * one launch (tests/normal_modes_reference.py is the specification).  free [nq] (HOST memory in both variants: it is the launch's,
 * nq words, and is checked before a device is touched), NULL: every dynamic config; a kinematic config is never free.  n_free = the
 * number of free configs.  Per pose, over the free configs F:
 *   1. at rest (dq = 0): V_q, V_qq[F, F], h, D = Dh[:, F], M = L_ddqddq[F, F]; a parameter table is honoured as in the equilibrium
 *      search (its twin is mode 15 in tg_batch_par_info, the default kernel mode 15 in tg_batch_info);
 *   2. mu [B][nc] as supplied (mu_in, for example what tg_batch_minimize_potential returned), or (NULL) the minimum-norm minimiser
 *      of |V_q[F] + D' mu| by column-pivoted QR under rcond; residual = |V_q[F] + D' mu|inf says how far the pose is from rest;
 *   3. K = V_qq[F, F] + sum_c mu_c h_c,qq[F, F];
 *   4. column-pivoted Householder QR of D' with the identity carried along; r = the rank under rcond, Z = the last nm = n_free - r
 *      columns of Q (the identity without constraints);
 *   5. M_r = Z'MZ and K_r = Z'KZ, symmetrised; unpivoted Cholesky M_r = LL', a pivot that is not > 0 ends the pose with TG_SINGULAR;
 *      C = L^-1 K_r L^-T, symmetrised;
 *   6. cyclic Jacobi on C in the round-robin ordering (csrc/sym_eig.hpp), sweeps until max |off-diagonal| <= eps max |entry| (tested
 *      at the start of a sweep), max_sweeps at the most: a pose that uses them all is TG_NOT_CONVERGED, its current answer written;
 *   7. omega2 [B][n_free] ascending (equal values in column order), modes [B][n_free][nq] = (Z L^-T Y)' with zeros at the held
 *      configs, M-orthonormal and tangent to the constraints, the component of largest magnitude of every shape positive (of equal
 *      magnitudes the lowest config index decides); rows beyond count = nm are zero.
 * count, rank, sweeps, status [B]; mu_out [B][nc]; residual [B].  A pose that is TG_SINGULAR (also: a q, multipliers or C that are
 * not finite) has every numeric output zero.  mu_in, mu_out, residual_out, count_out, rank_out, sweeps_out, status_out may be NULL.
 * The integrator state of the batch is not touched.  TG_ERR_INVALID for a null q, omega2 or modes, rcond < 0 (or not a number),
 * max_sweeps < 1, a mask that frees a kinematic config; TG_ERR_UNSUPPORTED for a system with a NonlinearConfigSpring (a force without
 * a potential, as in the equilibrium search), for the profiling build, and if the workgroup's LDS exceeds 160 KiB
 * (tg_system_normal_modes_lds: out = team size, doubles per team, bytes per workgroup, 0; computed without a device).  All of these
 * are refused before a device is touched.
 * The _device variant takes device pointers (except free), launches on the batch's stream and does not synchronise. */
int tg_system_normal_modes_lds(const tg_system *sys, int32_t out[4]);
int tg_batch_normal_modes(tg_batch *b, const double *q_host, const double *mu_host, const int32_t *free_host, double rcond,
                          int32_t max_sweeps, double *omega2_out, double *modes_out, int32_t *count_out, int32_t *rank_out,
                          double *mu_out, double *residual_out, int32_t *sweeps_out, int32_t *status_out);
int tg_batch_normal_modes_device(tg_batch *b, const double *q_dev, const double *mu_dev, const int32_t *free_host, double rcond,
                                 int32_t max_sweeps, double *omega2_out_dev, double *modes_out_dev, int32_t *count_out_dev,
                                 int32_t *rank_out_dev, double *mu_out_dev, double *residual_out_dev, int32_t *sweeps_out_dev,
                                 int32_t *status_out_dev);

/* ---- batched static response ----------------------------------------------------------------------------------------
 * How a rest pose and its constraint forces answer a moved held config and a load, for every pose of the batch in one launch
 * (tests/static_response_reference.py is the specification).  free [nq] (HOST memory in both variants, as the drive list is: they
 * are the launch's and are checked before a device is touched), NULL: every config; F the free configs, n_free of them, H the held
 * ones.  drive [n_drive]: the driven configs, distinct and all held; E selects them.  Per pose, at rest (dq = 0) at the input pose,
 * under the pose's parameter row if a table is set (its twin is mode 16 in tg_batch_par_info, the default kernel mode 16 in
 * tg_batch_info):
 *   1. V_q, V_qq over all configs, h, Dh, D_F = Dh[:, F], D_H = Dh[:, H];
 *   2. mu [B][nc] as supplied (mu_in, for example what tg_batch_minimize_potential returned), or (NULL) the minimum-norm minimiser
 *      of |V_q[F] + D_F' mu| by column-pivoted QR under rcond; residual = |V_q[F] + D_F' mu|inf says how far the pose is from rest;
 *   3. W = V_qq + sum_c mu_c h_c,qq over all config pairs; the blocks W_FF and W_FH are used;
 *   4. column-pivoted Householder QR of D_F' with the identity carried along; r = the rank under rcond, Z = the last n_free - r
 *      columns of Q (the identity without constraints); the pseudo-inverses below are those of the rank-r part, through the same
 *      factorisation (a second, unpivoted stage where r < nc), minimum norm;
 *   5. K_r = Z' W_FF Z, symmetrised; unpivoted Cholesky, a pivot that is not > 0 ends the pose with TG_SINGULAR (the pose is not a
 *      strict minimum on the tangent space of the constraints);
 *   6. the drive response: X_p = -D_F^+ D_H E, X = X_p + Z K_r^-1 Z' (-W_FH E - W_FF X_p), dmu = -(D_F')^+ (W_FF X + W_FH E);
 *      defect = |D_F X + D_H E|inf, non-zero only where the constraints cannot follow the drive;
 *   7. with_compliance: C = Z K_r^-1 Z' and R = (D_F')^+ (I - W_FF C): a generalized force f on the free configs' equations
 *      V_q[F] + D_F' mu = f moves the pose by C f and the multipliers by R f.
 * dq [B][n_drive][nq]: row j = the pose's derivative along driven config j (X[:, j] at F, 1 at its own place, 0 at the other held
 * configs); dmu [B][n_drive][nc]; compliance [B][nq][nq] = C with zero rows and columns at H; reaction [B][nq][nc] = R' with zero
 * rows at H; rank, status [B]; mu_out [B][nc]; residual, defect [B].  A pose that is TG_SINGULAR (also: a q, multipliers or result
 * that are not finite) has every numeric output zero; nothing else is reported per pose.  mu_in, rank_out, mu_out, residual_out,
 * defect_out, status_out may be NULL; dq and dmu only with n_drive == 0, compliance and reaction only without with_compliance.
 * The integrator state of the batch is not touched.  TG_ERR_INVALID for a null q, rcond < 0 (or not a number), a drive entry that
 * is free, out of range or repeated, and for n_drive == 0 without with_compliance (nothing to compute); TG_ERR_UNSUPPORTED for a
 * system with a NonlinearConfigSpring (a force without a potential, as in the equilibrium search), for the profiling build, and if
 * the workgroup's LDS exceeds 160 KiB (tg_system_static_response_lds for these sizes of a launch: out = team size, doubles per
 * team, bytes per workgroup, 0; computed without a device).  All of these are refused before a device is touched.
 * The _device variant takes device pointers (except free and drive), launches on the batch's stream and does not synchronise. */
int tg_system_static_response_lds(const tg_system *sys, int32_t n_free, int32_t n_drive, int32_t with_compliance, int32_t out[4]);
int tg_batch_static_response(tg_batch *b, const double *q_host, const double *mu_host, const int32_t *free_host, int32_t n_drive,
                             const int32_t *drive_host, int32_t with_compliance, double rcond, double *dq_out, double *dmu_out,
                             double *compliance_out, double *reaction_out, int32_t *rank_out, double *mu_out, double *residual_out,
                             double *defect_out, int32_t *status_out);
int tg_batch_static_response_device(tg_batch *b, const double *q_dev, const double *mu_dev, const int32_t *free_host, int32_t n_drive,
                                    const int32_t *drive_host, int32_t with_compliance, double rcond, double *dq_out_dev,
                                    double *dmu_out_dev, double *compliance_out_dev, double *reaction_out_dev, int32_t *rank_out_dev,
                                    double *mu_out_dev, double *residual_out_dev, double *defect_out_dev, int32_t *status_out_dev);

/* ---- batched inverse dynamics --------------------------------------------------------------------------------------
 * Given configuration paths Q [B][N + 1][nq] (kinematic configs included; B = the batch size, N = n_steps >= 1), the inputs u_k and
 * constraint forces lambda_k that make the discrete Euler-Lagrange equations hold on every step, and the impulse rho_k that no
 * input can supply.  Every (b, k), k = 0 .. N - 1, is an independent linear problem, one team each, all in one launch
 * (tests/inverse_dynamics_reference.py is the specification):
 *   p_k = p0[b] for k = 0, else D2L_d(Q_{k-1}, Q_k; dt_{k-1}) (tg_batch_calc_p2's formula: it depends on neither u nor lambda);
 *   r0 = p_k + D1L_d(Q_k, Q_{k+1}) + fm2(Q_k, Q_{k+1}, u = 0) on the dynamic configs (tg_batch_calc_f with u1 = lambda1 = 0) and
 *   h = h(Q_{k+1});  A~ = [F_du | -Dh(Q_k)[:, :nd]'], nd x n, n = nu + nc, F_du at the midpoint (the residual is affine in (u, lambda):
 *   r = r0 + A~ z~ with the impulses z~ = (dt_k u, lambda));
 *   minimise |rho|^2 + ridge |z~|^2, rho = r0 + A~ z~, through the augmented system [[I, A~], [A~', -ridge I]] (-rho, z~) = (-r0, 0)
 *   of size nd + n (Gauss-Jordan with implicit-scaled partial pivoting; not the normal equations).
 * Step sizes: the scalar dt, or the batch's by-step list (tg_batch_set_step_sizes) as tg_batch_rollout reads it: dt_k = list[k].
 * Outputs, each may be NULL: U [B][N][nu] = z~_u / dt_k; LAM [B][N][nc]; RHO [B][N][nd], zero on a feasible path; H [B][N][nc] =
 * h(Q_{k+1}); P [B][N + 1][nd] with P[b][k + 1] = D2L_d(Q_k, Q_{k+1}; dt_k) and P[b][0] = p_0; status [B][N]: TG_OK, or TG_SINGULAR
 * when the solver rejects the image or its answer is not finite -- U, LAM and RHO of that step are then zero, P and H still written.
 * p0 == NULL: step 0 is not solved; P[b][0] = -r0 evaluated at p = 0, the momentum that makes step 0 force-free, and U, LAM, RHO of
 * step 0 are zero with TG_OK: initialize_from_state(t_0, Q_0, P_0) followed by a rollout with U then retraces Q.  n == 0: nothing
 * to solve, rho = r0.
 * A rank-deficient A~ with n <= nd and ridge == 0 is NOT detected (the pivot guard is 1e-20; the puppet driven by forces on its
 * string ends has sigma_min ~ 2e-19): such systems need ridge > 0, and the answer is then the ridge solution, not the minimum-norm one.
 * Generic kernel of its own (mode 11 in tg_batch_info) whatever library the batch has; with a parameter table
 * (tg_batch_set_parameters) its parameter twin runs (mode 11 in tg_batch_par_info) and trajectory b uses row b / group for masses,
 * inertias, gravity and damping.  The integrator state of the batch (q1, q2, p, lambda1, status, iterations, times) is not touched.
 * TG_ERR_INVALID for ridge < 0 or not finite, n_steps < 1, a null Q, a by-trajectory step-size list, a by-step list shorter than
 * n_steps, a zero or non-finite dt without a list, n > nd with ridge == 0 (the image is structurally singular), and (_device) a
 * row stride under nq; TG_ERR_UNSUPPORTED for the profiling build and if the workgroup's LDS -- per team the rollout slice plus
 * (m + 1) m + nd + m doubles, m = nd + n -- exceeds 160 KiB (tg_system_inverse_dynamics_lds: out = team size, doubles per team,
 * bytes per workgroup, 0; the same refusals, computed without a device).
 * The _device variant takes device pointers, launches on the batch's stream and does not synchronise; row (b, k) of Q is read at
 * Q_dev + (b (N + 1) + k) q_row_stride_doubles, so q_row_stride_doubles = nX reads Q straight from a rollout's X [B][N + 1][nX]. */
int tg_system_inverse_dynamics_lds(const tg_system *sys, int32_t out[4]);
int tg_batch_inverse_dynamics(tg_batch *b, int32_t n_steps, double dt, const double *Q_host, const double *p0_host, double ridge,
                              double *U, double *LAM, double *P, double *RHO, double *H, int32_t *status);
int tg_batch_inverse_dynamics_device(tg_batch *b, int32_t n_steps, double dt, const double *Q_dev, uint64_t q_row_stride_doubles,
                                     const double *p0_dev, double ridge, double *U_dev, double *LAM_dev, double *P_dev,
                                     double *RHO_dev, double *H_dev, int32_t *status_dev);

/* The same question answered by rank-revealing least squares (csrc/lsq_solve.hpp; tests/min_norm_reference.py is the
 * specification): column-pivoted Householder QR of the stacked block W = [A~; sqrt(ridge) I] (W = A~ at ridge == 0) with a
 * minimum-norm completion, in place of the augmented image.  z~ = (dt_k u, lambda) is argmin |r0 + A~ z~|^2 + ridge |z~|^2 and, where
 * A~ loses rank, the minimiser of least |z~| -- numpy.linalg.lstsq(W, c, rcond)'s answer --, so it does not depend on a ridge, and
 * n > nd is accepted at ridge == 0.  rcond after ridge: a pivot column norm <= rcond * the first pivot's ends the factorisation;
 * rank [B][N] before status (nullable): the number of pivots accepted, 0 for a step that is not solved (n == 0, step 0 without p0) or
 * whose status is TG_SINGULAR.  With ridge > 0 the rank test runs on the STACKED block, whose singular values are
 * sqrt(sigma^2 + ridge): it then reports n unless rcond^2 sigma_1^2 exceeds the ridge.  TG_SINGULAR only for an answer that is not
 * finite -- z~, rho, or an A~ or r0 with an entry that is not finite (a configuration that is not a number) -- with U, LAM, RHO zero
 * and rank 0; a zero A~ is rank 0 with z~ = 0 and TG_OK.  rho = r0 + A~ z~ is formed from r0 and A~ themselves.  Column norms are
 * plain sums of squares: entries of A~ of scale 1e-160 and below count as zero, 1e154 and above overflow into TG_SINGULAR.
 * Everything else -- outputs, strides, the parameter twin, mode 11 in tg_batch_info -- is the sibling's.  TG_ERR_INVALID, before
 * a device is touched, for rcond negative, >= 1 or not finite and for everything the sibling refuses EXCEPT n > nd with
 * ridge == 0; the LDS refusal is tg_system_inverse_dynamics_lsq_lds's: per team the rollout slice plus (nd + n)(n + 1) + nd + 4 n
 * doubles, never more than 4 n above the sibling's. */
int tg_system_inverse_dynamics_lsq_lds(const tg_system *sys, int32_t out[4]);
int tg_batch_inverse_dynamics_lsq(tg_batch *b, int32_t n_steps, double dt, const double *Q_host, const double *p0_host, double ridge,
                                  double rcond, double *U, double *LAM, double *P, double *RHO, double *H, int32_t *rank, int32_t *status);
int tg_batch_inverse_dynamics_lsq_device(tg_batch *b, int32_t n_steps, double dt, const double *Q_dev, uint64_t q_row_stride_doubles,
                                         const double *p0_dev, double ridge, double rcond, double *U_dev, double *LAM_dev, double *P_dev,
                                         double *RHO_dev, double *H_dev, int32_t *rank_dev, int32_t *status_dev);

/* ---- batched frame kinematics ------------------------------------------------------------------------------------------
 * Where the frames are: for configurations Q [B][n_states][nq] (B = the batch size; kinematic configs included) and rates dQ of the
 * same shape, the world pose, the body velocity and the two Jacobians of every selected frame of every state, one team per state,
 * all in one launch (tests/frame_kinematics_reference.py is the specification; reference frame.py: g(), p(), vb(), p_dq(), vb_ddq()).
 * frames_host [n_frames]: indices into the descriptor's frame list (System.frames, 0 = the world), a host array in both variants;
 * repeats and any order are allowed.  With g_F = (R_F | p_F) the world pose of frame F, K the frame config k drives, a_k the world
 * direction of K's joint axis (column x / y / z of R_K) and o_k = p_K:
 *   G  [B][n_states][F][12]     rows 0..2 of Frame.g(), row-major 3 x 4 (Frame.p() is its fourth column);
 *   JP [B][n_states][F][nq][3]  Frame.p_dq(k)[:3]: a_k x (p_F - o_k) for a rotary k on F's path, a_k for a prismatic one, 0 off it;
 *   JB [B][n_states][F][nq][6]  Frame.vb_ddq(k) as (v, omega), v = M[0:3, 3], omega = (M[2][1], M[0][2], M[1][0]) of the 4 x 4 matrix
 *                               the accessor returns: (R_F' JP_k, R_F' a_k), omega = 0 for a prismatic k, 0 off the path;
 *   VB [B][n_states][F][6]      Frame.vb() likewise, sum_k JB_k dq_k; it needs dQ.
 * Any output may be NULL; every entry of a requested output is written, zeros included.  A state's answer does not depend on B,
 * n_states or its neighbours in the launch.
 * Kinematics do not depend on masses, gravity, damping, a loaded specialised library or the time base: one generic kernel (mode 12
 * in tg_batch_info) whatever the batch has set.  The integrator state of the batch (q1, q2, p, lambda1, status, iterations, times)
 * is not touched.
 * TG_ERR_INVALID, decided before a device is touched, for n_states < 1, a null Q, n_frames < 1 or a null frame list, a frame index
 * outside the system, VB without dQ, all four outputs null, and (_device) a row stride under nq; TG_ERR_UNSUPPORTED for the
 * profiling build and if the workgroup's LDS -- per team the rollout slice plus 144 doubles (eight staged frames: pose [12] and
 * world twist [6]; it does not grow with n_frames) -- exceeds 160 KiB (tg_system_frame_kinematics_lds: out = team size, doubles per
 * team, bytes per workgroup, 0; the same refusal, computed without a device).
 * The _device variant takes device pointers, launches on the batch's stream and does not synchronise; row (b, m) is read at
 * Q_dev + (b n_states + m) q_row_stride_doubles (dQ_dev likewise), so q_row_stride_doubles = nX reads the configurations straight
 * from a rollout's X [B][n_states][nX].  The frame table of a selection lives in a buffer of the batch: a call with the selection
 * of the call before allocates nothing; another selection waits for the stream once and rebuilds it. */
int tg_system_frame_kinematics_lds(const tg_system *sys, int32_t out[4]);
int tg_batch_frame_kinematics(tg_batch *b, int32_t n_states, const double *Q_host, const double *dQ_host,
                              int32_t n_frames, const int32_t *frames_host,
                              double *G, double *VB, double *JP, double *JB);
int tg_batch_frame_kinematics_device(tg_batch *b, int32_t n_states, const double *Q_dev, uint64_t q_row_stride_doubles,
                                     const double *dQ_dev, uint64_t dq_row_stride_doubles,
                                     int32_t n_frames, const int32_t *frames_host,
                                     double *G_dev, double *VB_dev, double *JP_dev, double *JB_dev);

/* ---- batched tape measures ---------------------------------------------------------------------------------------------
 * Lengths of broken lines through frame origins (reference tapemeasure.py; the host class trep_amd.TapeMeasure is the
 * specification): for configurations Q [B][n_states][nq] (kinematic configs included) and rates dQ of the same shape, the length,
 * its rate and their config derivatives of every selected measure of every state, one team per state, all in one launch.
 * Measure t is the frames frames_host[measure_start_host[t] .. measure_start_host[t + 1]) (indices into System.frames, host arrays
 * in both variants): at least two, consecutive ones different, repeats allowed.  Its segments join consecutive frames.  For a
 * segment from a to b: d = p_b - p_a, l = |d|; only the configs on exactly one of the two paths move it (a common ancestor moves
 * both ends rigidly); for those d_k = JP_b[k] - JP_a[k] (JP of tg_batch_frame_kinematics), d_jk = P_b[j,k] - P_a[j,k] with
 * P_F[j,k] = a_j x JP_F[k] for j, k on F's path, j rotary and the one nearer the world (or j == k), else 0, and
 *   l_k = d . d_k / l,   l_jk = (d_j . d_k + d . d_jk - l_j l_k) / l,   v = d . (sum_k d_k dq_k) / l,   v_k = sum_j l_jk dq_j.
 * Outputs, sums over the segments of a measure (segments ascending, configs ascending within a sum):
 *   L   [B][n_states][T]          TapeMeasure.length();
 *   V   [B][n_states][T]          velocity(); it needs dQ;
 *   LQ  [B][n_states][T][nq]      length_dq(k) = velocity_ddq(k);
 *   VQ  [B][n_states][T][nq]      velocity_dq(k); it needs dQ;
 *   LQQ [B][n_states][T][nq][nq]  length_dqdq(j, k) = velocity_ddqdq(j, k).
 * Any output may be NULL; every entry of a requested output is written, and a derivative entry that no segment's exclusive configs
 * reach is an exact 0.0.  A segment of zero length divides by zero, as on the host: that measure's outputs are then not finite, and
 * there is no status array.  Third derivatives stay on the host.  A state's answer does not depend on B, n_states or its neighbours.
 * One generic kernel (mode 13 in tg_batch_info) whatever masses, parameters, a specialised library or the time base the batch has
 * set; the integrator state of the batch is not touched.
 * TG_ERR_INVALID, decided before a device is touched, for n_states < 1, a null Q, n_measures < 1 or null tables, a measure with
 * fewer than two frames, two equal consecutive frames in a measure, a frame index outside the system, V or VQ without dQ, all five
 * outputs null, and (_device) a row stride under nq; TG_ERR_UNSUPPORTED for the profiling build and if the workgroup's LDS -- per
 * team the rollout slice plus 14 doubles for each of max(16, segments of the longest measure) staged segments -- exceeds 160 KiB
 * (tg_system_tape_measures_lds: out = team size, doubles per team, bytes per workgroup, 0; the same refusal without a device).
 * The _device variant takes device pointers, launches on the batch's stream and does not synchronise; row strides as for
 * tg_batch_frame_kinematics_device (nX reads a rollout's X in place).  The table of a selection lives in buffers of the batch: a
 * call with the selection of the call before allocates nothing; another selection waits for the stream once and rebuilds it. */
int tg_system_tape_measures_lds(const tg_system *sys, int32_t longest_measure_segments, int32_t out[4]);
int tg_batch_tape_measures(tg_batch *b, int32_t n_states, const double *Q_host, const double *dQ_host,
                           int32_t n_measures, const int32_t *measure_start_host, const int32_t *frames_host,
                           double *L, double *V, double *LQ, double *VQ, double *LQQ);
int tg_batch_tape_measures_device(tg_batch *b, int32_t n_states, const double *Q_dev, uint64_t q_row_stride_doubles,
                                  const double *dQ_dev, uint64_t dq_row_stride_doubles,
                                  int32_t n_measures, const int32_t *measure_start_host, const int32_t *frames_host,
                                  double *L_dev, double *V_dev, double *LQ_dev, double *VQ_dev, double *LQQ_dev);

/* ---- batched computed torque ---------------------------------------------------------------------------------------------
 * The continuous inverse of tg_batch_dynamics: for states Q, dQ, ddQ [B][n_states][nq] each (B = the batch size; kinematic configs
 * included -- the kinematic part of ddQ is what tg_batch_dynamics calls ddqk) the inputs u and constraint forces lambda that produce
 * those accelerations, the generalized force the motion needs in total and the part of it no input can supply.  One team per state,
 * all in one launch (tests/dynamics_inverse_reference.py is the specification).  With Ad = Dh(q)[:, :nd], Ak = Dh(q)[:, nd:], M the
 * dynamic block of L_ddqddq, the continuous equations M ddq_d - Ad' lambda = D0(q, dq, ddq_k) + F_du u:
 *   r0 = D0 - M ddq_d, summed per (body, joint) item as tg_batch_dynamics sums its bias but with the accelerations of every config
 *   (no M is formed, nothing is factored, M may be singular);
 *   A = [F_du | +Ad'], nd x n, n = nu + nc, F_du at (q, dq); the multiplier columns carry a plus, unlike tg_batch_inverse_dynamics;
 *   minimise |rho|^2 + ridge |z|^2, rho = r0 + A z, z = (u, lambda), through the augmented system
 *   [[I, A], [A', -ridge I]] (-rho, z) = (-r0, 0) of size nd + n (Gauss-Jordan with implicit-scaled partial pivoting).  The unknowns
 *   are forces: no step size takes part, and the batch's time base has no say.
 * Outputs, each may be NULL: U [B][n_states][nu]; LAM [..][nc]; RHO [..][nd], zero where inputs and constraints can supply the
 * motion; TAU [..][nd] = -r0 = F_du u + Ad' lambda - rho, the recursive-Newton-Euler answer (with one ConfigForce per config: the joint
 * torques); ACC [..][nc] = Ad ddq_d + Ak ddq_k + sum_ij h_dqdq(i, j) dq_i dq_j, zero for accelerations consistent with the
 * constraints (those tg_batch_dynamics returns); status [B][n_states]: TG_OK, or TG_SINGULAR when the solver rejects the image or
 * its answer is not finite -- U, LAM and RHO of that state are then zero, TAU and ACC still written.  n == 0: nothing to solve,
 * rho = r0.  A state's answer does not depend on B, n_states or its neighbours in the launch.
 * A rank-deficient A with n <= nd and ridge == 0 is NOT detected (the pivot guard is 1e-20): such systems need ridge > 0, and the
 * answer is then the ridge solution, not the minimum-norm one.
 * Generic kernel of its own (mode 14 in tg_batch_info) whatever library the batch has; with a parameter table
 * (tg_batch_set_parameters) its parameter twin runs (mode 14 in tg_batch_par_info) and trajectory b uses row b / group for masses,
 * inertias, gravity and damping.  The integrator state of the batch (q1, q2, p, lambda1, status, iterations, times) is not touched.
 * TG_ERR_INVALID, decided before a device is touched, for ridge < 0 or not finite, n_states < 1, a null Q, dQ or ddQ, n > nd with
 * ridge == 0 (the image is structurally singular), and (_device) a row stride under nq; TG_ERR_UNSUPPORTED for the profiling build
 * and if the workgroup's LDS -- per team the rollout slice plus (m + 1) m + nq + m doubles, m = nd + n -- exceeds 160 KiB
 * (tg_system_dynamics_inverse_lds: out = team size, doubles per team, bytes per workgroup, 0; the same refusal without a device).
 * The _device variant takes device pointers, launches on the batch's stream and does not synchronise; row (b, s) of Q is read at
 * Q_dev + (b n_states + s) q_row_stride_doubles, dQ_dev and ddQ_dev likewise with their own strides (nX reads Q from a rollout's X). */
int tg_system_dynamics_inverse_lds(const tg_system *sys, int32_t out[4]);
int tg_batch_dynamics_inverse(tg_batch *b, int32_t n_states, const double *Q_host, const double *dQ_host, const double *ddQ_host,
                              double ridge, double *U, double *LAM, double *RHO, double *TAU, double *ACC, int32_t *status);
int tg_batch_dynamics_inverse_device(tg_batch *b, int32_t n_states, const double *Q_dev, uint64_t q_row_stride_doubles,
                                     const double *dQ_dev, uint64_t dq_row_stride_doubles,
                                     const double *ddQ_dev, uint64_t ddq_row_stride_doubles, double ridge,
                                     double *U_dev, double *LAM_dev, double *RHO_dev, double *TAU_dev, double *ACC_dev,
                                     int32_t *status_dev);

/* Computed torque by rank-revealing least squares: as tg_batch_inverse_dynamics_lsq is to tg_batch_inverse_dynamics.  z = (u, lambda)
 * is numpy.linalg.lstsq(W, c, rcond)'s answer on W = [A; sqrt(ridge) I], c = (-r0; 0) -- of minimum norm where A loses rank, whatever
 * the ridge --, n > nd is accepted at ridge == 0, rcond follows ridge and rank [B][n_states] (nullable) precedes status; with
 * ridge > 0 the rank test runs on the stacked block.  n == 0: rank = 0, rho = r0, nothing is solved.  TG_SINGULAR only for an answer
 * that is not finite (z, rho, or a state that is not a number: U, LAM, RHO zero and rank 0, as the sibling answers); the range of
 * the column norms is tg_batch_inverse_dynamics_lsq's.  TG_ERR_INVALID, before a device is touched, for rcond negative, >= 1 or not finite and for everything the
 * sibling refuses except n > nd with ridge == 0; the LDS refusal is tg_system_dynamics_inverse_lsq_lds's: per team the rollout slice
 * plus (nd + n)(n + 1) + nq + 4 n doubles.
 * tg_batch_debug_lsq_solve (test hook) runs the solver alone on `count` caller-supplied problems of one shape, A [count][rows][cols]
 * and c [count][rows] on the host, one team of `team` lanes (1, 4, 16 or 64) on each, in one launch: z [count][cols] = argmin
 * |c - A z| of minimum norm, rank and status [count].  Only here do teams of different rank share a wavefront. */
int tg_system_dynamics_inverse_lsq_lds(const tg_system *sys, int32_t out[4]);
int tg_batch_dynamics_inverse_lsq(tg_batch *b, int32_t n_states, const double *Q_host, const double *dQ_host, const double *ddQ_host,
                                  double ridge, double rcond, double *U, double *LAM, double *RHO, double *TAU, double *ACC,
                                  int32_t *rank, int32_t *status);
int tg_batch_dynamics_inverse_lsq_device(tg_batch *b, int32_t n_states, const double *Q_dev, uint64_t q_row_stride_doubles,
                                         const double *dQ_dev, uint64_t dq_row_stride_doubles,
                                         const double *ddQ_dev, uint64_t ddq_row_stride_doubles, double ridge, double rcond,
                                         double *U_dev, double *LAM_dev, double *RHO_dev, double *TAU_dev, double *ACC_dev,
                                         int32_t *rank_dev, int32_t *status_dev);
int tg_batch_debug_lsq_solve(tg_batch *b, int32_t team, int32_t count, int32_t rows, int32_t cols, const double *A_host,
                             const double *c_host, double rcond, double *z_host, int32_t *rank_host, int32_t *status_host);

/* ---- bounded inverse dynamics: strings that only pull, inputs within limits ------------------------------------------------
 * The box-constrained versions of tg_batch_dynamics_inverse_lsq and tg_batch_inverse_dynamics_lsq.  Per state or step
 *   minimise |r0 + A z|^2 + ridge |z|^2   subject to   lo <= z <= hi,   z = (u, lambda),
 * with r0, A, TAU, ACC, P, H evaluated exactly as by the _lsq siblings, solved exactly by an active-set method (Stark-Parker BVLS, the
 * method of scipy.optimize.lsq_linear(method="bvls")): a short sequence of rank-revealing least-squares solves on the free columns of
 * W = [A; sqrt(ridge) I], c = (-r0; 0) (csrc/bvls_solve.hpp; tests/bounded_reference.py is the specification).  The first solve has
 * every variable free: with all bounds infinite the results are the _lsq siblings' bit for bit, and a state whose unconstrained answer
 * lies in the box costs one solve.
 * Arguments: those of the _lsq sibling, and behind rcond
 *   lo, hi [bound_rows][nu + nc] in (u | lambda) order: host arrays in the host variants, device arrays in the _device variants;
 *   bound_rows is 1 (one box for the launch) or B (trajectory b uses row b); -INFINITY / +INFINITY mean no bound.  In
 *   tg_batch_inverse_dynamics_bounded the bounds on u are FORCES (the kernel scales them by the step's own dt_k, uniform or from
 *   tg_batch_set_step_sizes, to bounds on the impulses it solves for) and the bounds on lambda apply to lambda as returned;
 * and, ahead of rank,
 *   active [..][nu + nc] (int32, nullable): -1 at the lower bound, +1 at the upper, 0 free (scipy's active_mask); lo == hi reports -1;
 *   solves [..] (int32, nullable): the least-squares solves the state took (0 where nothing is solved).
 * rank is the FIRST solve's.  status: TG_OK (the KKT conditions hold); TG_SINGULAR when the first solve finds rank < n at rcond -- the
 * problem is then not strictly convex and its minimiser not unique: USE A RIDGE; U, LAM, RHO and active are zero, rank is reported --
 * and for anything not finite (rank 0 too, as the siblings); TG_NOT_CONVERGED when 3 n + 3 solves did not reach the KKT conditions (not
 * observed): U, LAM, RHO, active are then the last feasible iterate's.  n == 0: nothing is solved, rho = r0.
 * WHICH SIGN PULLS.  A Distance constraint is h = |p1 - p2| - d (reference Distance.h).  In the continuous equations the multipliers
 * enter as +Ad' lambda on the side of the applied forces: lambda > 0 pushes the two points apart, so a string (which can only pull
 * them together) has lambda <= 0 in tg_batch_dynamics_inverse*: lo = -inf, hi = 0.  In the discrete equations they enter as
 * -Dh' lambda: a string has lambda >= 0 in tg_batch_inverse_dynamics* (and in the integrator's lambda1): lo = 0, hi = +inf.
 * TG_ERR_INVALID, before a device is touched: everything the _lsq sibling refuses; n > nd at ridge == 0 (never strictly convex);
 * bound_rows other than 1 or B; a null lo or hi with n > 0; and, in the host variants, which can read the box, a bound that is not a
 * number, lo_j > hi_j, lo_j == +inf or hi_j == -inf.  The _device variants take the box's contents on trust (a box that breaks these
 * rules cannot hang the kernel -- its loop has a fixed cap -- but the answer is then not specified).
 * LDS per team: the _lsq sibling's, plus a second block (nd + n)(n + 1) and 5 n doubles (tg_system_*_bounded_lds: the 160 KiB refusal
 * without a device).  Generic kernels only, with parameter twins, counted under modes 14 and 11 of tg_batch_info like their siblings.
 * tg_batch_debug_bvls_solve (test hook) runs the solver alone as tg_batch_debug_lsq_solve does, with lo, hi [count][cols] and a cap
 * max_solves in 0 .. 3 cols + 3 (0: 3 cols + 3) on the solves of a problem. */
int tg_system_dynamics_inverse_bounded_lds(const tg_system *sys, int32_t out[4]);
int tg_batch_dynamics_inverse_bounded(tg_batch *b, int32_t n_states, const double *Q_host, const double *dQ_host, const double *ddQ_host,
                                      double ridge, double rcond, const double *lo_host, const double *hi_host, int32_t bound_rows,
                                      double *U, double *LAM, double *RHO, double *TAU, double *ACC,
                                      int32_t *active, int32_t *solves, int32_t *rank, int32_t *status);
int tg_batch_dynamics_inverse_bounded_device(tg_batch *b, int32_t n_states, const double *Q_dev, uint64_t q_row_stride_doubles,
                                             const double *dQ_dev, uint64_t dq_row_stride_doubles,
                                             const double *ddQ_dev, uint64_t ddq_row_stride_doubles, double ridge, double rcond,
                                             const double *lo_dev, const double *hi_dev, int32_t bound_rows,
                                             double *U_dev, double *LAM_dev, double *RHO_dev, double *TAU_dev, double *ACC_dev,
                                             int32_t *active_dev, int32_t *solves_dev, int32_t *rank_dev, int32_t *status_dev);
int tg_system_inverse_dynamics_bounded_lds(const tg_system *sys, int32_t out[4]);
int tg_batch_inverse_dynamics_bounded(tg_batch *b, int32_t n_steps, double dt, const double *Q_host, const double *p0_host, double ridge,
                                      double rcond, const double *lo_host, const double *hi_host, int32_t bound_rows,
                                      double *U, double *LAM, double *P, double *RHO, double *H,
                                      int32_t *active, int32_t *solves, int32_t *rank, int32_t *status);
int tg_batch_inverse_dynamics_bounded_device(tg_batch *b, int32_t n_steps, double dt, const double *Q_dev, uint64_t q_row_stride_doubles,
                                             const double *p0_dev, double ridge, double rcond,
                                             const double *lo_dev, const double *hi_dev, int32_t bound_rows,
                                             double *U_dev, double *LAM_dev, double *P_dev, double *RHO_dev, double *H_dev,
                                             int32_t *active_dev, int32_t *solves_dev, int32_t *rank_dev, int32_t *status_dev);
int tg_batch_debug_bvls_solve(tg_batch *b, int32_t team, int32_t count, int32_t rows, int32_t cols, const double *A_host,
                              const double *c_host, const double *lo_host, const double *hi_host, double rcond, int32_t max_solves,
                              double *z_host, int32_t *active_host, int32_t *solves_host, int32_t *rank_host, int32_t *status_host);

/* DSystem.set(X[s][k], U[s][k], k, xk_hint = X[s][k+1]) for every (s, k) at once (reference
 * trep/discopt/dsystem.py:229-251 as used by linearize_trajectory, :406-423, and calc_newton_model,
 * doptimizer.py:333-335): the batch must hold seeds*horizon trajectories, trajectory t = s*horizon + k;
 * lambda1 is reset to 0 and the dynamic part of X[s][k+1] is the Newton start, like the reference. */
int tg_batch_set_from_trajectories(tg_batch *b, int32_t seeds, int32_t horizon, double t0, double dt,
                                   const double *X_dev, const double *U_dev, int32_t max_iterations);
/* initialize_from_state(t, Q, p) (midpointvi.py:145-153) with trajectory b's (Q, p) read from the head of the
 * DSystem state vector X_dev[b*row_stride_doubles ...] = [Q; p; v]; lambda1 <- 0. */
int tg_batch_initialize_from_state_device(tg_batch *b, double t, const double *X_dev, uint64_t row_stride_doubles);
/* tg_batch_rollout_closed_loop for the first n_trajectories trajectories of the batch only, with an optional
 * indirection for the gain schedules: group g (= trajectory / group_size) uses Kproj_dev[group_select_dev[g]].
 * Used for the later rounds of a batched Armijo search, when only some seeds are still searching. */
int tg_batch_rollout_closed_loop_subset(tg_batch *b, int32_t n_trajectories, int32_t n_steps, double dt,
                                        const double *Kproj_dev, int32_t group_size, const int32_t *group_select_dev,
                                        const double *bX_dev, const double *bU_dev, double *X_dev, double *U_dev,
                                        int32_t max_iterations);
/* DSystem.fdx / fdu of every solved step (dsystem.py:284-317): A_dev [batch][nX][nX], B_dev [batch][nX][nU],
 * written directly by the first-derivative kernel (the twelve reference-layout arrays are not produced). */
int tg_batch_linearize(tg_batch *b, double *A_dev, double *B_dev);
/* tg_batch_deriv2_contract with device-resident z [batch][nX] and hz [batch][R][R]. */
int tg_batch_deriv2_contract_device(tg_batch *b, const double *z_dev, double *hz_dev);
/* ... for the trajectories s * horizon + k, k_begin <= k < k_end, of a batch of seeds * horizon trajectories only (same arrays, same layout) */
int tg_batch_deriv2_contract_device_range(tg_batch *b, const double *z_dev, double *hz_dev, int32_t horizon, int32_t k_begin, int32_t k_end);

/* Time-varying LQ problem (reference trep/discopt/dlqr.py:41-81; with q_dev = r_dev = NULL and no curvature it
 * is solve_tv_lqr, dlqr.py:9-38).  Weights: Q_k = Q_dev[s*Q_seed_stride + k*Q_step_stride + ...] (strides in
 * doubles, 0 = shared), terminal Qf, R_k likewise.  If hz_dev != NULL the z-contracted second derivative of the
 * dynamics HZ [S][N][hz_R][hz_R] (variables ordered x-part[hz_nx], u-part[nU]) is added on the fly:
 * Q_k += HZ[:hz_nx,:hz_nx], S_k = HZ[:hz_nx, hz_nx:], R_k += HZ[hz_nx:, hz_nx:]  (the Newton model of
 * doptimizer.py:319-345).  Outputs: K [S][N][nU][nX], C [S][N][nU] (affine only), P0 [S][nX][nX], b0 [S][nX],
 * status [S] (TG_OK / TG_SINGULAR).  Q_k and Qf must be symmetric (every P_k then is: the recursion symmetrises
 * it like the reference does). */
typedef struct tg_lq_problem {
    int32_t n_problems, horizon, nX, nU;
    const int32_t *select_dev;
    const double *A_dev, *B_dev;
    const double *Q_dev;  int64_t Q_seed_stride, Q_step_stride;
    const double *Qf_dev; int64_t Qf_seed_stride;
    const double *R_dev;  int64_t R_seed_stride, R_step_stride;
    const double *hz_dev; int32_t hz_R, hz_nx;
    const double *q_dev, *r_dev;          /* [S][N+1][nX], [S][N][nU] or both NULL */
    double *K_dev, *C_dev, *P0_dev, *b0_dev;
    int32_t *status_dev;
    double *b_next_dev;                   /* optional (with q, r): [S][N][nX], row k = b_{k+1}, the affine term entering step k.  With
                                           * the projection weights (Q = R = I) and the cost gradients as q, r this is the adjoint
                                           * z_{k+1} of the Newton model (doptimizer.py:340-343): tg_adjoint_sweep for free */
    int32_t ds_nd, ds_nk, ds_nu;          /* optional: A_k, B_k have the block structure of DSystem.fdx / fdu (dsystem.py:284-317) for a system with
                                           * ds_nd dynamic and ds_nk kinematic configs and ds_nu force inputs -- states [Qd | Qk | p | v], inputs
                                           * [u | rho]: A's Qk rows and v columns are zero and a v row holds one entry (its Qk column); B's Qk and v
                                           * rows hold one entry each (their rho column).  The sweep then skips those blocks in its matrix products
                                           * (about half of the matrix-core work at the puppet's sizes); they must hold exact zeros.  ds_nd = 0: dense.
                                           * Requires nX = 2 (ds_nd + ds_nk), nU = ds_nu + ds_nk. */
    int32_t k_begin, k_end;               /* optional: sweep only the steps k_end - 1 ... k_begin of the horizon (k_end = 0: all of it).  Every array
                                           * keeps its full-horizon layout.  With k_end < horizon the sweep starts from ... */
    const double *Pt_dev, *bt_dev;        /* ... (P, b) at step k_end: [S][nX][nX], [S][nX] -- the P0_dev / b0_dev an earlier launch over the steps
                                           * [k_end, ...) wrote (which, with k_begin > 0, are (P, b) at step k_begin).  A horizon swept in chunks
                                           * this way gives bit for bit the gains of one sweep: the pipelined Newton step of BatchDOptimizer runs the
                                           * projection sweep, the second derivatives and the Newton-model sweep chunk by chunk in three stream lanes */
} tg_lq_problem;
int tg_tv_lq(int32_t device, const tg_lq_problem *problem);
/* Which kernel tg_tv_lq would launch for this problem, decided on the host alone (no device is touched; the same environment
 * switches are read): out[0] kernel (0 = the VALU kernel k_tv_lq, 1 = the matrix-core kernel k_tv_lq_mfma, 2 = the DSystem-structured
 * kernel k_tv_lq_ds), out[1] size class (tile size TS of the VALU kernel: 2, 4, 5, 6; else NT = 16 x 16 tiles per dimension: 1, 2, 3,
 * 5, 6), out[2] NR (rows of the input solve in registers: 4, 8, 20, 32; 0 for the VALU kernel), out[3] threads per workgroup,
 * out[4] dynamic LDS bytes, out[5] 0.  Returns what tg_tv_lq would return before launching (TG_ERR_INVALID, TG_ERR_UNSUPPORTED;
 * `out` is then meaningless); tg_tv_lq launches what this reports.  The structured kernel loads A_k, B_k sixteen bytes at a
 * time, and it never computes the v columns of the gains: a structured problem whose A_dev or B_dev is not 16-byte aligned, or whose
 * curvature block reaches into the v rows (hz_nx > 2 ds_nd + ds_nk), takes the dense kernel.  An affine sweep that continues
 * from Pt_dev needs bt_dev, and Pt_dev is refused for a sweep that starts at the horizon's end (k_end = 0 or horizon), which
 * starts from Qf and q_N. */
int tg_tv_lq_plan(const tg_lq_problem *problem, int32_t out[6]);

/* Backward adjoint of the Newton model (doptimizer.py:319-345): Z[s][k] = z_{k+1}, the vector the second
 * derivatives of step k are contracted with; z_k = q_k - K_k' r_k + (A_k - B_k K_k)' z_{k+1}, z_N = q_N. */
int tg_adjoint_sweep(int32_t device, int32_t n_problems, int32_t horizon, int32_t nX, int32_t nU,
                     const int32_t *select_dev, const double *A_dev, const double *B_dev, const double *K_dev,
                     const double *q_dev, const double *r_dev, double *Z_dev);
/* Descent direction from the LQ solution (doptimizer.py:391-402): dU_k = -K_k dX_k - C_k,
 * dX_{k+1} = A_k dX_k + B_k dU_k, dX_0 = 0; dcost[s] = sum_k q_k.dX_k + r_k.dU_k (calc_dcost, :262-270). */
int tg_tangent_rollout(int32_t device, int32_t n_problems, int32_t horizon, int32_t nX, int32_t nU,
                       const int32_t *select_dev, const double *A_dev, const double *B_dev, const double *K_dev,
                       const double *C_dev, const double *q_dev, const double *r_dev, double *dX_dev, double *dU_dev,
                       double *dcost_dev);
/* Which kernel tg_tangent_rollout would launch (host only; the pointers are looked at for their alignment, never dereferenced):
 * out[0] kernel (0 = the LDS-staged k_tangent, 1 = k_tangent_rows with the rows in registers), out[1..3] the register class
 * CA, CB, CK (0 for k_tangent), out[4] 1 = pairs of columns per thread with 16-byte loads (even sizes and 16-byte aligned A, B,
 * K), out[5] threads per workgroup.  Returns TG_SUCCESS or what tg_tangent_rollout would refuse the sizes with. */
int tg_tangent_rollout_plan(int32_t nX, int32_t nU, const void *A_dev, const void *B_dev, const void *K_dev, int32_t out[6]);
/* DCost (trep/discopt/dcost.py:5-118): cost[t] = sum_k 1/2 (x-xd)'Q(x-xd) + 1/2 (u-ud)'R(u-ud) + terminal
 * with Qf, for n_trajectories trajectories of which `group` consecutive ones share the reference of one seed:
 * trajectory t is compared with Xd/Ud of seed select_dev[t/group] (or t/group if select_dev is NULL). */
int tg_quadratic_cost(int32_t device, int32_t n_trajectories, int32_t group, const int32_t *select_dev, int32_t horizon,
                      int32_t nX, int32_t nU, const double *X_dev, const double *U_dev, const double *Xd_dev, const double *Ud_dev,
                      const double *Q_dev, const double *R_dev, const double *Qf_dev, double *cost_dev);
/* Its gradients q [S][N+1][nX] (row N = terminal), r [S][N][nU] (dcost.py:62-84). */
int tg_quadratic_cost_gradients(int32_t device, int32_t n_problems, int32_t horizon, int32_t nX, int32_t nU,
                                const int32_t *select_dev, const double *X_dev, const double *U_dev,
                                const double *Xd_dev, const double *Ud_dev, const double *Q_dev, const double *R_dev,
                                const double *Qf_dev, double *q_dev, double *r_dev);
/* Armijo candidates (doptimizer.py:436-446): row c = i*n_lambdas + m of bX/bU is X[s_i] + lambda_m dX[s_i]. */
int tg_armijo_candidates(int32_t device, int32_t n_problems, int32_t n_lambdas, int32_t horizon, int32_t nX,
                         int32_t nU, const int32_t *select_dev, const double *lambdas_dev, const double *X_dev,
                         const double *U_dev, const double *dX_dev, const double *dU_dev, double *bX_dev,
                         double *bU_dev);
/* dst[dst_rows[i]] = src[src_rows[i]], rows of row_doubles doubles (NULL index = identity). */
int tg_copy_rows(int32_t device, int32_t n_rows, uint64_t row_doubles, const int32_t *dst_rows_dev,
                 const int32_t *src_rows_dev, const double *src_dev, double *dst_dev);
/* Stream lane of the calling thread for every discrete-optimisation launch above (tg_tv_lq ... tg_copy_rows): 0 = the
 * device's default stream (initial state), 1 / 2 = two ordinary streams per device.  Streams created without flags order
 * themselves against the default stream in both directions, so kernels launched on lanes 1 and 2 run side by side and
 * anything launched after returning to lane 0 waits for both -- BatchDOptimizer runs the projection-gain sweep and the
 * quasi-Newton LQ sweep of a step this way when the GPU has idle CUs (the reference runs them one after the other,
 * doptimizer.py:462-480; the results do not depend on it). */
int tg_dopt_use_stream(int32_t device, int32_t lane);
/* lanes 1 .. 4: the lane's HIP stream (hipStream_t as void *) -- e.g. for tg_batch_set_stream --, and "lane `waiter` continues after
 * everything enqueued so far in lane `signal`" (an event, no host synchronisation) */
void *tg_dopt_lane_stream(int32_t device, int32_t lane);
int tg_dopt_lane_wait(int32_t device, int32_t waiter, int32_t signal);
int tg_device_synchronize(int32_t device);

/* ---- multi-GPU: one process per GPU, batch sharded, one collective ----------------------
 * The reference has no counterpart (one trajectory per System object, one process).  The only exchange of the path
 * is an all-gather of per-trajectory results (terminal states, costs) after a rollout -- what the discopt line search
 * (trep/discopt/doptimizer.py:405-459) looks at -- plus scalar reductions for barriers / timings.  Implemented on
 * RCCL directly (librccl is dlopen'ed on first use; xGMI on the GPU box).  Rank 0 makes the 128-byte id with
 * tg_comm_unique_id and passes it to the other ranks out of band BEFORE they call tg_comm_create. */
#define TG_COMM_ID_BYTES 128
enum { TG_REDUCE_SUM = 0, TG_REDUCE_MAX = 1, TG_REDUCE_MIN = 2 };
typedef struct tg_comm tg_comm;
int tg_comm_unique_id(uint8_t id_out[TG_COMM_ID_BYTES]);
tg_comm *tg_comm_create(int32_t device, int32_t world, int32_t rank, const uint8_t id_in[TG_COMM_ID_BYTES]);
void tg_comm_destroy(tg_comm *comm);
int tg_comm_info(const tg_comm *comm, int32_t out[3]);   /* ranks and this rank as RCCL reports them (ncclCommCount / ncclCommUserRank), device */
/* recv_dev [world][bytes_per_rank] <- every rank's send_dev [bytes_per_rank]; asynchronous on the communicator's own
 * stream.  That stream is ordered after work on the device's NULL stream only: a buffer produced on another stream (a
 * tg_batch's: tg_batch_stream) must be handed over with tg_comm_wait_stream(comm, producer_stream) first -- it records an
 * event on the producer and makes the communicator's stream wait for it (no host synchronisation).
 * tg_comm_all_gather_after does both in one call.  tg_comm_stream_wait_comm is the other direction (a consumer stream waits for the collective). */
int tg_comm_all_gather(tg_comm *comm, const void *send_dev, void *recv_dev, uint64_t bytes_per_rank);
int tg_comm_wait_stream(tg_comm *comm, void *producer_hip_stream);
int tg_comm_all_gather_after(tg_comm *comm, void *producer_hip_stream, const void *send_dev, void *recv_dev, uint64_t bytes_per_rank);
int tg_comm_stream_wait_comm(tg_comm *comm, void *consumer_hip_stream);
int tg_comm_synchronize(tg_comm *comm);
/* In-place reduction of n host doubles over all ranks (blocking); tg_comm_barrier is a 1-element sum. */
int tg_comm_all_reduce_host(tg_comm *comm, double *values, int32_t n, int32_t op);
int tg_comm_barrier(tg_comm *comm);

#ifdef __cplusplus
}
#endif
#endif /* TREP_AMD_H */
