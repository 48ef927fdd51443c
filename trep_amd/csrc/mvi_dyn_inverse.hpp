// mvi_dyn_inverse.hpp -- MODE_DYN_INVERSE: batched computed torque, one team per state (tg_batch_dynamics_inverse).
//
// The continuous counterpart of mvi_inverse.hpp.  Given states (q, dq, ddq) [B][M] with the accelerations of ALL configs, find the
// inputs u and constraint forces lambda that produce them, the generalized force the motion needs in total, and the part of it no input
// can supply.  In the notation of Core::dynamics (Ad = Dh(q)[:, :nd], Ak = Dh(q)[:, nd:], M the dynamic block of L_ddqddq) the
// continuous equations are M ddq_d - Ad' lambda = D(q, dq, ddq_k, u), and every built-in force is affine in u: D = D0 + F_du u.
// Per team (b, s), tests/dynamics_inverse_reference.py being the specification:
//   r0 = D0 - M ddq_d: Core::dynamics' right-hand side with S_F = sum_k (W_k dq_k + J_k ddq_k) taken over EVERY config k, not only the
//   kinematic ones, evaluated at u = 0 -- no M is formed, nothing is factored;
//   TAU = -r0: what inputs and constraints have to supply together (the recursive-Newton-Euler answer);
//   A = [F_du | +Ad'], nd x n, n = nu + nc: the ConfigForce coefficients, the wrench Jacobians wD through wr_in and the Dh items.  The
//   multiplier columns carry a PLUS (TAU = F_du u + Ad' lambda; the discrete kernel has -Dh' there);
//   z = (u, lambda) minimises |rho|^2 + ridge |z|^2 with rho = r0 + A z, solved in the augmented form
//   [[I, A], [A', -ridge I]] (-rho, z) = (-r0, 0) by Core::gauss_jordan (not the normal equations: A'A squares the conditioning).  The
//   unknowns are forces, not impulses: no step size appears anywhere in this kernel;
//   ACC = Ad ddq_d + Ak ddq_k + sum_ij h_dq_i dq_j dq_i dq_j: how far the accelerations are from consistent with the constraints (zero for
//   accelerations that dynamics() returned), from the Dh items and the cpair4 table as Core::dynamics builds its constraint rows, over
//   all configs.
// Outputs: U, LAM, RHO, TAU, ACC, status TG_OK or TG_SINGULAR (the solver rejected the image or its answer is not finite: U, LAM, RHO of
// that state are zero, TAU and ACC still written).  With n == 0 nothing is solved: rho = r0.
// A rank-deficient A with n <= nd and ridge == 0 is NOT detected unless a scaled pivot falls to 1e-20 (gauss_jordan's guard): such
// systems need ridge > 0 -- or the LSQ instantiation (tg_batch_dynamics_inverse_lsq): the same evaluation, and in place of the image
// the stacked block [A; sqrt(ridge) I] with (-r0; 0) through the rank-revealing least squares of lsq_solve.hpp (inverse_lsq_stage in
// mvi_inverse_rows.hpp).  z is then the minimum-norm minimiser whatever the ridge, n > nd needs none, the rank of every state is
// returned (J.rank), rho = r0 + A z is formed from r0 and rows of A assembled a second time, and TG_SINGULAR means only an answer that
// is not finite.  LDS of a team there: the block [nd + n][n + 1] in place of the image and 4 n doubles in place of the row scales
// (dyn_inverse_lsq_layout).
//
// No team reads what another writes and every sum runs in an order the team's own lanes fix (LDS only, no global atomics): a state's
// result does not depend on B, M or the team's neighbours in the wavefront.
// LDS of a team: the rollout slice and behind it the image [m][m + 1], m = nd + n, the given accelerations [nq] (the slice's own
// place for them holds the kinematic ones alone) and the solver's row scales [m].
// Compiled by hipcc (trepamd_dyn_inverse.hip: k_dyn_inverse) and, with TEAM = 1, by g++ for the CPU tests (tests/emu_dyn_inverse).
#pragma once
#include <cfloat>

#include "mvi_inverse_rows.hpp"

namespace tg {

constexpr int MODE_DYN_INVERSE = 14;

// passed beside RunArgs (whose layout stays), as InverseArgs is; RunArgs supplies batch = B
struct DynInverseArgs {
    const double *Q, *dQ, *ddQ;  // states: row (b, s) at X + (b n_states + s) x_stride, [nq] each; ddQ = (ddq_d [nd] | ddq_k [nk])
    double *U, *LAM, *RHO, *TAU, *ACC;   // [batch][n_states][nu], [..][nc], [..][nd], [..][nd], [..][nc]; each may be null
    int *status;                 // [batch][n_states] or null
    double ridge;
    size_t q_stride, dq_stride, ddq_stride;      // doubles between consecutive rows (nq or more)
    int n_states;
    int o_kkt, o_ddq, o_scal;    // LDS offsets (doubles) behind the rollout slice
    int lds_per_team;            // doubles per team: what the kernel strides its teams by
    double rcond;                // the LSQ kernels alone: pivot norms <= rcond * the first one end the factorisation
    int *rank;                   // the LSQ kernels alone: [batch][n_states] or null
    // the BND kernels alone (which use rcond and rank too):
    const double *lo, *hi;       // the box [bound_rows][nu + nc] in (u | lambda) order, -inf / +inf: no bound
    int bound_rows;              // 1: one box for the launch; batch: one per trajectory
    int max_solves;              // the cap on the least-squares solves of a state (bvls_max_solves)
    int *active, *solves;        // [batch][n_states][nu + nc] (-1 at lo, +1 at hi, 0 free), [batch][n_states]; each may be null
};

// the scratch layout of one team (host; the same numbers for the device launch and the emulation)
inline void dyn_inverse_layout(int rollout_lds_per_team, int nq, int nd, int nu, int nc, DynInverseArgs &J) {
    const int m = nd + nu + nc;
    int off = (rollout_lds_per_team + 1) & ~1;
    J.o_kkt = off; off += m * (m + 1);
    J.o_ddq = off; off += nq;
    J.o_scal = off; off += m;
    J.lds_per_team = (off + 1) & ~1;
}

// ... and of the LSQ kernels: o_kkt the stacked block [nd + n][n + 1] (sized for a ridge), o_scal the solver's 4 n doubles (lsq_solve.hpp).
// Against the layout above that is m (n + 1) + 4 n for m (m + 1) + m, m = nd + n: never more than 4 n doubles larger.
inline void dyn_inverse_lsq_layout(int rollout_lds_per_team, int nq, int nd, int nu, int nc, DynInverseArgs &J) {
    const int n = nu + nc;
    int off = (rollout_lds_per_team + 1) & ~1;
    J.o_kkt = off; off += (nd + n) * (n + 1);
    J.o_ddq = off; off += nq;
    J.o_scal = off; off += lsq_scratch_doubles(n);
    J.lds_per_team = (off + 1) & ~1;
}

// ... and of the BND kernels: o_kkt the PRISTINE stacked block [nd + n][n + 1], o_scal the solver's scratch (bvls_solve.hpp: the
// working block of the same size, lo, hi, z, the gradient, the bound-state words, and lsq_solve's 4 n)
inline void dyn_inverse_bounded_layout(int rollout_lds_per_team, int nq, int nd, int nu, int nc, DynInverseArgs &J) {
    const int n = nu + nc;
    int off = (rollout_lds_per_team + 1) & ~1;
    J.o_kkt = off; off += (nd + n) * (n + 1);
    J.o_ddq = off; off += nq;
    J.o_scal = off; off += bvls_scratch_doubles(nd + n, n);
    J.lds_per_team = (off + 1) & ~1;
}

// team index i = b * n_states + s; i >= batch * n_states: an idle team, which still takes part in every TG_SYNC
// LSQ: the solve is lsq_solve.hpp's on [A; sqrt(ridge) I] (inverse_lsq_stage) in place of the augmented image, and J.rank is written
// BND: the solve is bvls_solve.hpp's on the same block with the box J.lo, J.hi (inverse_bounded_stage); J.rank, J.active and J.solves
// are written, and the status may be TG_NOT_CONVERGED (U, LAM, RHO then belong to the last feasible iterate)
template <int TEAM, bool SPRINGS, bool PAR, bool LSQ = false, bool BND = false, class PROG, class ARGS>
TG_HD void run_dyn_inverse(PROG &P, ARGS &A, const DynInverseArgs &J, const ParTable T, double *S, int lane, long long team_index) {
    const int nq = P.nq, nd = P.nd, nu = P.nu, nc = P.nc, nf = P.nf, M = J.n_states;
    const int n = nu + nc, m = nd + n, ld = m + 1;
    const bool live = team_index < (long long)A.batch * M;
    const size_t bs = (size_t)(live ? team_index : 0), b = bs / (size_t)M;
    Core<TEAM, SPRINGS, PROG, double, PAR> core(P, S, lane, 1.0);      // (the step size takes no part)
    if constexpr (PAR) core.par = T.rows + (b / (size_t)T.group) * (size_t)T.stride + 4 * P.n_bodies;
    else (void)T;
    core.init_sweep_schedule(false);
    double *K = S + J.o_kkt, *ddq = S + J.o_ddq, *scal = S + J.o_scal, *rhs = S + P.o_f;

    // ---- the state: q in q1 = q2, no inputs, no multipliers ------------------------------------------------------------------------
    if (live) {
        const double *q = J.Q + bs * J.q_stride, *dq = J.dQ + bs * J.dq_stride, *acc = J.ddQ + bs * J.ddq_stride;
        TG_FOR(i, nq) { S[P.o_q1 + i] = q[i]; S[P.o_q2 + i] = q[i]; S[P.o_dq + i] = dq[i]; ddq[i] = acc[i]; }
        TG_FOR(i, nd) S[P.o_p1 + i] = 0.0;
        TG_FOR(i, nc) S[P.o_lam + i] = 0.0;
        TG_FOR(i, nu) S[P.o_u + i] = 0.0;
        TG_FOR(i, P.n_dh) { S[P.o_Dh1 + i] = 0.0; S[P.o_Dh2 + i] = 0.0; }
        TG_FOR(i, nf) rhs[i] = 0.0;
    }
    TG_SYNC();

    // ---- r0 and ACC: Core::dynamics' evaluation with the accelerations of all configs ----------------------------------------------
    core.pose_sweep(live, 2);
    core.attach_points(live, true, true);
    core.spring_terms(live);
    core.wrench_terms(live);
    if (nc) {
        core.constraints(live, 2, false, S + P.o_Dh2, 0);
        if (live) {
            TG_FOR(e, P.n_dh) {
                const int c = P.dh_pack[8 * (size_t)e], k = P.dh_pack[8 * (size_t)e + 1];
                lds_add(&rhs[nd + c], S[P.o_Dh2 + e] * ddq[k]);
            }
            TG_FOR(pp, P.n_cpair) {
                const int *pw = P.cpair4 + 4 * (size_t)pp;
                const int c = pw[0], na = pw[1], nb = pw[2], ka = pw[3] & 0xFFFF, kb = pw[3] >> 16;
                const double h = core.con_d2(c, na, nb) * S[P.o_dq + ka] * S[P.o_dq + kb];
                lds_add(&rhs[nd + c], na != nb ? 2.0 * h : h);
            }
        }
        TG_SYNC();
    }
    core.jacobians(live);
    core.velocities(live);
    double *SF = S + P.o_G;      // S_F per body, in the (now dead) joint pose area
    if (live) TG_FOR(idx, 6 * P.n_bodies) {
        const int body = idx / 6, c6 = idx % 6;
        double acc = 0.0;
        for (int k = P.b_item_off[body]; k < P.b_item_off[body + 1]; k++) {
            const int cfg = P.it_pack[4 * (size_t)k + 3] & 0xFFFF;
            acc += S[P.o_W + 6 * k + c6] * S[P.o_dq + cfg] + S[P.o_J + 6 * k + c6] * ddq[cfg];
        }
        SF[idx] = acc;
    }
    TG_SYNC();
    if (live) {
        TG_FOR(it, P.n_items) {
            const int body = P.it_pack[4 * (size_t)it], cfg = P.it_pack[4 * (size_t)it + 3] & 0xFFFF;
            const double *I = S + P.o_I + 4 * body, *v = S + P.o_vB + 6 * body, *gam = S + P.o_gam + 3 * body;
            const double *Jt = S + P.o_J + 6 * it;
            double jv[6];
            bracket(Jt, v, jv);
            const double term = I[0] * (gam[0] * Jt[0] + gam[1] * Jt[1] + gam[2] * Jt[2]) - inner6(I, Jt, SF + 6 * body) - inner6(I, jv, v);
            if (cfg < nd) lds_add(&rhs[cfg], term);
        }
        TG_FOR(i, nd) {      // the forces at u = 0 (the constant components of the wrenches are in wF)
            double force = -core.damp_of(P, i) * S[P.o_dq + i];
            if (core.has_cs()) force -= core.cs_d1(i, S[P.o_q2 + i]);
            if (core.n_springs()) force -= S[P.o_sV + i];
            if (core.n_wrenches()) force += S[P.o_wF + i];
            if (core.has_damper()) force += S[P.o_sF + i];
            lds_add(&rhs[i], force);
        }
    }
    TG_SYNC();
    if (live) {
        if (J.TAU) TG_FOR(i, nd) J.TAU[bs * nd + i] = -rhs[i];
        if (J.ACC) TG_FOR(c, nc) J.ACC[bs * nc + c] = rhs[nd + c];
    }

    const bool solve = live && n > 0;
    if (live && !solve && J.RHO) TG_FOR(i, nd) J.RHO[bs * nd + i] = rhs[i];      // n == 0: rho = r0
    if constexpr (BND) {
        // ---- the pristine stacked block, the active-set loop around the rank-revealing solve, rho from r0 and the block's rows ------
        int r = 0, solves = 0, st = TG_OK;
        const size_t box = (J.bound_rows > 1 ? b : 0) * (size_t)n;
        if (n > 0) r = inverse_bounded_stage<TEAM>(core, P, S, lane, solve, rhs, S + P.o_Dh2, false, J.ridge, J.rcond, J.lo + box, J.hi + box, 1.0,
                                                   J.max_solves, K, scal, solves, st);
        const bool answer = solve && st != TG_SINGULAR;
        const BvlsScratch X = bvls_scratch(scal, nd + (J.ridge > 0.0 ? n : 0), n);
        if (live) {
            if (J.U) TG_FOR(i, nu) J.U[bs * nu + i] = answer ? X.z[i] : 0.0;
            if (J.LAM) TG_FOR(c, nc) J.LAM[bs * nc + c] = answer ? X.z[nu + c] : 0.0;
            if (solve && J.RHO) TG_FOR(i, nd) J.RHO[bs * nd + i] = answer ? K[i * (n + 1) + n] : 0.0;
            if (J.active) TG_FOR(j, n) J.active[bs * n + j] = answer ? X.bnd[j] : 0;
            if (lane == 0 && J.solves) J.solves[bs] = solves;
            if (lane == 0 && J.rank) J.rank[bs] = solve ? r : 0;
            if (lane == 0 && J.status) J.status[bs] = st;
        }
        return;
    }
    if constexpr (LSQ) {
        // ---- the stacked block [A; sqrt(ridge) I] with (-r0; 0), its rank-revealing solve, rho from r0 and A ----------------------------
        bool ok = true;
        int r = 0;
        if (n > 0) r = inverse_lsq_stage<TEAM>(core, P, S, lane, solve, rhs, S + P.o_Dh2, false, J.ridge, J.rcond, K, scal, ok);
        const bool answer = solve && ok;
        const double *z = scal + 2 * n;
        if (live) {
            if (J.U) TG_FOR(i, nu) J.U[bs * nu + i] = answer ? z[i] : 0.0;
            if (J.LAM) TG_FOR(c, nc) J.LAM[bs * nc + c] = answer ? z[nu + c] : 0.0;
            if (solve && J.RHO) TG_FOR(i, nd) J.RHO[bs * nd + i] = answer ? K[i * (n + 1) + n] : 0.0;
            if (lane == 0 && J.rank) J.rank[bs] = answer ? r : 0;
            if (lane == 0 && J.status) J.status[bs] = ok ? TG_OK : TG_SINGULAR;
        }
        return;
    }

    // ---- the image [[I, A], [A', -ridge I]] with the right-hand side (-r0, 0): every lane owns rows of [I, A], then the transpose ----
    if (solve) TG_FOR(i, m * ld) K[i] = 0.0;
    TG_SYNC();
    if (solve) TG_FOR(i, nd) {
        double *row = K + i * ld;
        row[i] = 1.0;
        inverse_row(core, P, S, i, row + nd, S + P.o_Dh2, false);
        row[m] = -rhs[i];
    }
    TG_SYNC();
    if (solve) {
        TG_FOR(e, n * nd) { const int j = e / nd, i = e % nd; K[(nd + j) * ld + i] = K[i * ld + nd + j]; }
        TG_FOR(j, n) K[(nd + j) * ld + nd + j] = -J.ridge;
    }
    TG_SYNC();

    // ---- the solve -----------------------------------------------------------------------------------------------------------------
    bool ok = true;
    if (n > 0) ok = core.gauss_jordan(solve, K, m, 1, ld, scal);      // (n is the launch's: every team of the wavefront takes the same way)
    if (solve && ok) for (int i = 0; i < m; i++) if (!(fabs(K[i * ld + m]) <= DBL_MAX)) ok = false;      // (every lane scans the same words: team-uniform)
    const bool answer = solve && ok;
    if (live) {
        if (J.U) TG_FOR(i, nu) J.U[bs * nu + i] = answer ? K[(nd + i) * ld + m] : 0.0;
        if (J.LAM) TG_FOR(c, nc) J.LAM[bs * nc + c] = answer ? K[(nd + nu + c) * ld + m] : 0.0;
        if (solve && J.RHO) TG_FOR(i, nd) J.RHO[bs * nd + i] = answer ? -K[i * ld + m] : 0.0;
        if (lane == 0 && J.status) J.status[bs] = ok ? TG_OK : TG_SINGULAR;
    }
}

}  // namespace tg
