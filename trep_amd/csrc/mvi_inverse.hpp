// mvi_inverse.hpp -- MODE_INVERSE: batched inverse dynamics, one team per (trajectory, step) (tg_batch_inverse_dynamics).
//
// Given configuration paths Q [B][N + 1][nq], find for every step k of every path the inputs u_k and constraint forces lambda_k that
// make the discrete Euler-Lagrange equations hold, and the impulse rho_k that no input can supply.  Two facts make the B x N steps
// independent linear problems:
//   (1) p_{k+1} = D2L_d(q_k, q_{k+1}) does not depend on u or lambda (midpointvi.c:491-504), so every p_k of a given path is known
//       without a sweep;
//   (2) the residual of a step is affine in (u, lambda): r(u, lambda) = r0 + dt F_du u - Dh(q_k)[:, :nd]' lambda, F_du at the midpoint
//       (every built-in force has f_dudu = 0).
// Per team (b, k), tests/inverse_dynamics_reference.py being the specification:
//   p_k = p0[b] (k = 0) or D2L_d(Q_{k-1}, Q_k; dt_{k-1}): a midpoint evaluation of pair k - 1 (calc_p2's formula);
//   r0 = p_k + D1L_d(Q_k, Q_{k+1}) + fm2(Q_k, Q_{k+1}, u = 0) on the dynamic configs and h = h(Q_{k+1}): calc_f with u1 = lambda1 = 0;
//   A~ = [F_du | -Dh(Q_k)[:, :nd]'], nd x n, n = nu + nc: the ConfigForce coefficients and the wrench Jacobians wD through wr_in (what
//   kkt_rest puts into the u1 columns of deriv1, without their dt);
//   the unknowns are impulses z~ = (dt_k u, lambda): minimise |rho|^2 + ridge |z~|^2 with rho = r0 + A~ z~, solved in the augmented
//   form [[I, A~], [A~', -ridge I]] (-rho, z~) = (-r0, 0) by Core::gauss_jordan (not the normal equations: A~'A~ squares the
//   conditioning).
// Outputs: U = z~_u / dt_k, LAM, RHO, H = h(Q_{k+1}), P[k + 1] = D2L_d(Q_k, Q_{k+1}; dt_k) from the same evaluation, P[0] = p_0,
// status TG_OK or TG_SINGULAR (the solver rejected the image or its answer is not finite: U, LAM, RHO of that step are zero, P and H
// still written).
// Without p0, step 0 is not solved: P[0] = -r0 evaluated at p = 0 -- the momentum that makes step 0 force-free -- and U, LAM, RHO of
// step 0 are zero, so that initialize_from_state(t_0, Q_0, P_0) followed by a rollout with U retraces Q.  With n == 0 nothing is
// solved either: rho = r0.
// A rank-deficient A~ with n <= nd and ridge == 0 is NOT detected unless a scaled pivot falls to 1e-20 (gauss_jordan's guard): such
// systems need ridge > 0 -- or the LSQ instantiation (tg_batch_inverse_dynamics_lsq): the same evaluation, and in place of the image
// the stacked block [A~; sqrt(ridge) I] with (-r0; 0) through the rank-revealing least squares of lsq_solve.hpp (inverse_lsq_stage in
// mvi_inverse_rows.hpp), the unknowns still the impulses z~ = (dt_k u, lambda) and the multiplier columns still -Dh'.  z~ is then the
// minimum-norm minimiser whatever the ridge, n > nd needs none, the rank of every step is returned (J.rank; 0 for a step that is not
// solved), rho = r0 + A~ z~ is formed from r0 and rows of A~ assembled a second time -- the solve therefore runs before h(Q_{k+1}) is
// evaluated --, and TG_SINGULAR means only an answer that is not finite.  LDS of a team there: the block [nd + n][n + 1] in place of
// the image and 4 n doubles in place of the row scales (inverse_lsq_layout).
//
// No team reads what another writes: a (b, k) result does not depend on B, N or the team's neighbours in the wavefront.
// LDS of a team: the rollout slice and behind it the image [m][m + 1], m = nd + n, p_k [nd] and the solver's row scales [m].
// Compiled by hipcc (trepamd_inverse.hip: k_inverse) and, with TEAM = 1, by g++ for the CPU tests (tests/emu_invdyn).
#pragma once
#include <cfloat>

#include "mvi_inverse_rows.hpp"

namespace tg {

constexpr int MODE_INVERSE = 11;

// passed beside RunArgs (whose layout stays), as ParTable is; RunArgs supplies batch = B
struct InverseArgs {
    const double *Q;             // configurations: row (b, k) at Q + (b (n_steps + 1) + k) q_stride, k = 0 .. n_steps
    const double *p0;            // [batch][nd] or null
    const double *dt_steps;      // [n_steps] step sizes, or null: dt
    double *U, *LAM, *P, *RHO, *H;   // [batch][n_steps][nu], [..][nc], [batch][n_steps + 1][nd], [batch][n_steps][nd], [..][nc]; each may be null
    int *status;                 // [batch][n_steps] or null
    double dt, ridge;
    size_t q_stride;             // doubles between consecutive rows of Q (nq, or nX to read a rollout's X)
    int n_steps;
    int o_kkt, o_pk, o_scal;     // LDS offsets (doubles) behind the rollout slice
    int lds_per_team;            // doubles per team: what the kernel strides its teams by
    double rcond;                // the LSQ kernels alone: pivot norms <= rcond * the first one end the factorisation
    int *rank;                   // the LSQ kernels alone: [batch][n_steps] or null
    // the BND kernels alone (which use rcond and rank too):
    const double *lo, *hi;       // the box [bound_rows][nu + nc] in (u | lambda) order, u as FORCES; -inf / +inf: no bound
    int bound_rows;              // 1: one box for the launch; batch: one per trajectory
    int max_solves;              // the cap on the least-squares solves of a step (bvls_max_solves)
    int *active, *solves;        // [batch][n_steps][nu + nc] (-1 at lo, +1 at hi, 0 free), [batch][n_steps]; each may be null
};

// the scratch layout of one team (host; the same numbers for the device launch and the emulation)
inline void inverse_layout(int rollout_lds_per_team, int nd, int nu, int nc, InverseArgs &J) {
    const int m = nd + nu + nc;
    int off = (rollout_lds_per_team + 1) & ~1;
    J.o_kkt = off; off += m * (m + 1);
    J.o_pk = off; off += nd;
    J.o_scal = off; off += m;
    J.lds_per_team = (off + 1) & ~1;
}

// ... and of the LSQ kernels: o_kkt the stacked block [nd + n][n + 1] (sized for a ridge), o_scal the solver's 4 n doubles (lsq_solve.hpp).
// Against the layout above that is m (n + 1) + 4 n for m (m + 1) + m, m = nd + n: never more than 4 n doubles larger.
inline void inverse_lsq_layout(int rollout_lds_per_team, int nd, int nu, int nc, InverseArgs &J) {
    const int n = nu + nc;
    int off = (rollout_lds_per_team + 1) & ~1;
    J.o_kkt = off; off += (nd + n) * (n + 1);
    J.o_pk = off; off += nd;
    J.o_scal = off; off += lsq_scratch_doubles(n);
    J.lds_per_team = (off + 1) & ~1;
}

// ... and of the BND kernels: o_kkt the PRISTINE stacked block [nd + n][n + 1], o_scal the solver's scratch (bvls_solve.hpp: the
// working block of the same size, lo, hi, z, the gradient, the bound-state words, and lsq_solve's 4 n)
inline void inverse_bounded_layout(int rollout_lds_per_team, int nd, int nu, int nc, InverseArgs &J) {
    const int n = nu + nc;
    int off = (rollout_lds_per_team + 1) & ~1;
    J.o_kkt = off; off += (nd + n) * (n + 1);
    J.o_pk = off; off += nd;
    J.o_scal = off; off += bvls_scratch_doubles(nd + n, n);
    J.lds_per_team = (off + 1) & ~1;
}

// team index i = b * n_steps + k; i >= batch * n_steps: an idle team, which still takes part in every TG_SYNC
// LSQ: the solve is lsq_solve.hpp's on [A~; sqrt(ridge) I] (inverse_lsq_stage) in place of the augmented image, run BEFORE the
// constraints of Q_{k+1} are evaluated (r0, o_wD and Dh(Q_k) are then still in place for rho), and J.rank is written
// BND: as LSQ, the solve being bvls_solve.hpp's with the box J.lo, J.hi (inverse_bounded_stage): the bounds on u are forces and are
// scaled by this step's dt_k to bounds on the impulses dt_k u; those on lambda apply to lambda as returned.  J.active and J.solves
// are written, and the status may be TG_NOT_CONVERGED (U, LAM, RHO then belong to the last feasible iterate)
template <int TEAM, bool SPRINGS, bool PAR, bool LSQ = false, bool BND = false, class PROG, class ARGS>
TG_HD void run_inverse(PROG &P, ARGS &A, const InverseArgs &J, const ParTable T, double *S, int lane, long long team_index) {
    const int nq = P.nq, nd = P.nd, nu = P.nu, nc = P.nc, N = J.n_steps;
    const int n = nu + nc, m = nd + n, ld = m + 1;
    const bool live = team_index < (long long)A.batch * N;
    const size_t b = (size_t)(live ? team_index / N : 0);
    const int k = (int)(live ? team_index % N : 0);
    const size_t bk = b * (size_t)N + k;
    const double dt_k = J.dt_steps ? J.dt_steps[k] : J.dt;
    const double dt_prev = k > 0 && J.dt_steps ? J.dt_steps[k - 1] : J.dt;
    Core<TEAM, SPRINGS, PROG, double, PAR> core(P, S, lane, dt_prev);
    if constexpr (PAR) core.par = T.rows + (b / (size_t)T.group) * (size_t)T.stride + 4 * P.n_bodies;
    else (void)T;
    core.init_sweep_schedule(false);
    double *K = S + J.o_kkt, *pk = S + J.o_pk, *scal = S + J.o_scal;
    const double *rows = J.Q + (b * (size_t)(N + 1) + k) * J.q_stride;     // Q_k; Q_{k-1} and Q_{k+1} one stride before and behind

    // the pair (Q_first, Q_first+1) with p1 = p, no inputs, no multipliers
    auto load_pair = [&](bool on, const double *q_first, const double *p) {
        if (on) {
            TG_FOR(i, nq) { S[P.o_q1 + i] = q_first[i]; S[P.o_q2 + i] = q_first[J.q_stride + i]; }
            TG_FOR(i, nd) S[P.o_p1 + i] = p ? p[i] : 0.0;
            TG_FOR(i, nc) S[P.o_lam + i] = 0.0;
            TG_FOR(i, nu) S[P.o_u + i] = 0.0;
            TG_FOR(i, P.n_dh) { S[P.o_Dh1 + i] = 0.0; S[P.o_Dh2 + i] = 0.0; }
        }
        TG_SYNC();
    };

    // ---- p_k: the momentum the path arrives with ------------------------------------------------------------------------------
    const bool arrives = live && k > 0;
    load_pair(arrives, rows - J.q_stride, nullptr);
    core.eval_midpoint(arrives);
    if (live) TG_FOR(i, nd) pk[i] = k > 0 ? 0.5 * dt_prev * S[P.o_Ldq + i] + S[P.o_Lddq + i] : (J.p0 ? J.p0[b * nd + i] : 0.0);
    TG_SYNC();

    // ---- r0, h, P_{k+1} of the pair (Q_k, Q_{k+1}) ----------------------------------------------------------------------------
    core.dt = dt_k; core.inv_dt = 1.0 / dt_k;
    load_pair(live, rows, pk);
    core.eval_constraints(live, 1, false, S + P.o_Dh1);
    core.eval_midpoint(live);
    const bool solve = live && n > 0 && (k > 0 || J.p0);
    // what both solves share behind the evaluation of the pair: P_{k+1} (and P_0), rho = r0 where nothing is solved, then h(Q_{k+1}),
    // which overwrites the poses and Dh2 -- the LSQ stage runs before it, the augmented image is assembled before it
    auto momenta_and_h = [&]() {
        if (live) {
            if (J.P) {
                double *Pb = J.P + b * (size_t)(N + 1) * nd;
                TG_FOR(i, nd) Pb[(size_t)(k + 1) * nd + i] = 0.5 * dt_k * S[P.o_Ldq + i] + S[P.o_Lddq + i];
                if (k == 0) TG_FOR(i, nd) Pb[i] = J.p0 ? pk[i] : -S[P.o_f + i];
            }
            if (!solve && J.RHO) TG_FOR(i, nd) J.RHO[bk * nd + i] = (k > 0 || J.p0) ? S[P.o_f + i] : 0.0;     // n == 0: rho = r0
        }
        TG_SYNC();
        core.eval_constraints(live, 2, true, S + P.o_Dh2);
        if (live && J.H) TG_FOR(c, nc) J.H[bk * nc + c] = S[P.o_f + nd + c];
    };
    if constexpr (BND) {
        // the pristine stacked block, the active-set loop around the rank-revealing solve, rho from r0 and the block's rows
        int r = 0, solves = 0, st = TG_OK;
        const size_t box = (J.bound_rows > 1 ? b : 0) * (size_t)n;
        if (n > 0) r = inverse_bounded_stage<TEAM>(core, P, S, lane, solve, S + P.o_f, S + P.o_Dh1, true, J.ridge, J.rcond, J.lo + box, J.hi + box,
                                                   dt_k, J.max_solves, K, scal, solves, st);
        const bool answer = solve && st != TG_SINGULAR;
        const BvlsScratch X = bvls_scratch(scal, nd + (J.ridge > 0.0 ? n : 0), n);
        if (live) {
            if (J.U) TG_FOR(i, nu) J.U[bk * nu + i] = answer ? X.z[i] / dt_k : 0.0;
            if (J.LAM) TG_FOR(c, nc) J.LAM[bk * nc + c] = answer ? X.z[nu + c] : 0.0;
            if (solve && J.RHO) TG_FOR(i, nd) J.RHO[bk * nd + i] = answer ? K[i * (n + 1) + n] : 0.0;
            if (J.active) TG_FOR(j, n) J.active[bk * n + j] = answer ? X.bnd[j] : 0;
            if (lane == 0 && J.solves) J.solves[bk] = solves;
            if (lane == 0 && J.rank) J.rank[bk] = solve ? r : 0;
            if (lane == 0 && J.status) J.status[bk] = st;
        }
        momenta_and_h();
        return;
    }
    if constexpr (LSQ) {
        // the stacked block [A~; sqrt(ridge) I] with (-r0; 0), its rank-revealing solve, rho from r0 and A~
        bool ok = true;
        int r = 0;
        if (n > 0) r = inverse_lsq_stage<TEAM>(core, P, S, lane, solve, S + P.o_f, S + P.o_Dh1, true, J.ridge, J.rcond, K, scal, ok);
        const bool answer = solve && ok;
        const double *z = scal + 2 * n;
        if (live) {
            if (J.U) TG_FOR(i, nu) J.U[bk * nu + i] = answer ? z[i] / dt_k : 0.0;
            if (J.LAM) TG_FOR(c, nc) J.LAM[bk * nc + c] = answer ? z[nu + c] : 0.0;
            if (solve && J.RHO) TG_FOR(i, nd) J.RHO[bk * nd + i] = answer ? K[i * (n + 1) + n] : 0.0;
            if (lane == 0 && J.rank) J.rank[bk] = answer ? r : 0;
            if (lane == 0 && J.status) J.status[bk] = ok ? TG_OK : TG_SINGULAR;
        }
        momenta_and_h();
        return;
    }
    // the image [[I, A~], [A~', -ridge I]] with the right-hand side (-r0, 0): every lane owns rows of [I, A~], then the transpose
    if (solve) TG_FOR(i, m * ld) K[i] = 0.0;
    TG_SYNC();
    if (solve) TG_FOR(i, nd) {
        double *row = K + i * ld;
        row[i] = 1.0;
        inverse_row(core, P, S, i, row + nd, S + P.o_Dh1, true);
        row[m] = -S[P.o_f + i];
    }
    TG_SYNC();
    if (solve) {
        TG_FOR(e, n * nd) { const int j = e / nd, i = e % nd; K[(nd + j) * ld + i] = K[i * ld + nd + j]; }
        TG_FOR(j, n) K[(nd + j) * ld + nd + j] = -J.ridge;
    }
    momenta_and_h();

    // ---- the solve ------------------------------------------------------------------------------------------------------------
    bool ok = true;
    if (n > 0) ok = core.gauss_jordan(solve, K, m, 1, ld, scal);      // (n is the launch's: every team of the wavefront takes the same way)
    if (solve && ok) for (int i = 0; i < m; i++) if (!(fabs(K[i * ld + m]) <= DBL_MAX)) ok = false;      // (every lane scans the same words: team-uniform)
    const bool answer = solve && ok;
    if (live) {
        if (J.U) TG_FOR(i, nu) J.U[bk * nu + i] = answer ? K[(nd + i) * ld + m] / dt_k : 0.0;
        if (J.LAM) TG_FOR(c, nc) J.LAM[bk * nc + c] = answer ? K[(nd + nu + c) * ld + m] : 0.0;
        if (solve && J.RHO) TG_FOR(i, nd) J.RHO[bk * nd + i] = answer ? -K[i * ld + m] : 0.0;
        if (lane == 0 && J.status) J.status[bk] = ok ? TG_OK : TG_SINGULAR;
    }
}

}  // namespace tg
