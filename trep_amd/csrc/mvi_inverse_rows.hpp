// mvi_inverse_rows.hpp -- what the two inverse questions (mvi_inverse.hpp, mvi_dyn_inverse.hpp) share: the rows of A, and the
// least-squares stage of their _lsq kernels (lsq_solve.hpp) and its box-constrained sibling of the _bounded kernels (bvls_solve.hpp).
#pragma once
#include "bvls_solve.hpp"
#include "lsq_solve.hpp"
#include "mvi_core.hpp"

namespace tg {

static_assert(BVLS_OK == TG_OK && BVLS_NOT_CONVERGED == TG_NOT_CONVERGED && BVLS_SINGULAR == TG_SINGULAR, "bvls_solve.hpp restates the status words");

// Row i (a dynamic config) of A = [F_du | +-Dh[:, :nd]'], nd x (nu + nc), added into dst [nu + nc] (zero before): the ConfigForce
// coefficients, the wrench Jacobians wD through wr_in (what kkt_rest puts into the u1 columns of deriv1, without their dt) and the
// items Dh of the constraints, with a minus for the discrete equations.  Reads the tables and o_wD / Dh of the team's slice alone.
template <class CORE, class PROG>
TG_HD void inverse_row(const CORE &core, const PROG &P, const double *S, int i, double *dst, const double *Dh, bool minus) {
    for (int f = 0; f < P.n_cf; f++) if (P.cf_cfg[f] == i) dst[P.cf_in[f]] += 1.0;
    if (core.n_wrenches()) {
        const int m0 = P.n_dh + core.n_sdh(), c0 = P.nc + core.n_springs();
        for (int w_ = 0; w_ < core.n_wdh(); w_++) {
            if (P.dh_cfg[m0 + w_] != i) continue;
            const int w = P.dh_c[m0 + w_] - c0;
            for (int s6 = 0; s6 < 6; s6++) { const int in = P.wr_in[6 * w + s6]; if (in >= 0) dst[in] += S[P.o_wD + 6 * w_ + s6]; }
        }
    }
    for (int c = 0; c < P.nc; c++) { const int e = P.dh_lookup[c * P.nq + i]; if (e >= 0) dst[P.nu + c] = minus ? -Dh[e] : Dh[e]; }
}

// The solve stage of the _lsq kernels: z = argmin |r0 + A z|^2 + ridge |z|^2 of minimum norm, the rank, and rho = r0 + A z.
//   W [R][n + 1], R = nd (ridge == 0) or nd + n: the stacked block [A; sqrt(ridge) I] with c = (-r0; 0) behind it -- with a ridge the
//   rank test therefore runs on the stacked block, whose singular values are sqrt(sigma^2 + ridge);
//   scr: lsq_scratch_doubles(n) doubles; the answer is z = scr + 2 n;
//   rho comes from the intact r0 and rows of A formed a second time (the items in o_wD and Dh survive the solve), not from the
//   transformed right-hand side; it is left in W[i (n + 1) + n], i < nd.
// solve: this team has a problem.  Returns the rank; ok as lsq_solve sets it (rho is not formed without an answer), and false too
// for a rho that is not finite: as in the augmented kernels, every word of the answer is scanned.
template <int TEAM, class CORE, class PROG>
TG_HD int inverse_lsq_stage(const CORE &core, const PROG &P, const double *S, int lane, bool solve, const double *r0, const double *Dh,
                            bool minus, double ridge, double rcond, double *W, double *scr, bool &ok) {
    const int nd = P.nd, n = P.nu + P.nc, ld = n + 1, R = nd + (ridge > 0.0 ? n : 0);
    int *perm = (int *)scr;
    double *nrm = scr + n, *z = scr + 2 * n, *tau2 = scr + 3 * n;
    if (solve) TG_FOR(i, R * ld) W[i] = 0.0;
    TG_SYNC();
    if (solve) {
        TG_FOR(i, nd) { inverse_row(core, P, S, i, W + i * ld, Dh, minus); W[i * ld + n] = -r0[i]; }
        if (ridge > 0.0) { const double s = sqrt(ridge); TG_FOR(j, n) W[(nd + j) * ld + j] = s; }
    }
    TG_SYNC();
    const int r = lsq_solve<TEAM>(solve, W, R, n, ld, rcond, perm, nrm, z, tau2, lane, ok);
    if (solve && ok) TG_FOR(i, nd) {
        double *row = W + i * ld;
        for (int j = 0; j < n; j++) row[j] = 0.0;
        inverse_row(core, P, S, i, row, Dh, minus);
        double acc = r0[i];
        for (int j = 0; j < n; j++) acc = fma(row[j], z[j], acc);
        row[n] = acc;
    }
    TG_SYNC();
    if (solve && ok) for (int i = 0; i < nd; i++) if (!(fabs(W[i * ld + n]) <= DBL_MAX)) ok = false;      // (every lane scans the same words: team-uniform)
    return r;
}

// The solve stage of the _bounded kernels: z = argmin |r0 + A z|^2 + ridge |z|^2 subject to lo <= z <= hi (bvls_solve.hpp), the
// first solve's rank, and rho = r0 + A z.
//   W: the PRISTINE stacked block [R][n + 1], assembled ONCE as inverse_lsq_stage assembles it (word for word) and only read by the
//   solver; rho comes from r0 and its rows and is left in W[i (n + 1) + n], i < nd, as there;
//   scr: bvls_scratch_doubles(R, n) doubles; the answer is bvls_scratch(scr, R, n).z, the bound states .bnd;
//   lo, hi: this team's box [n] in global memory, in the units of the caller; the first nu entries are multiplied by u_scale (the
//   discrete kernel's unknowns are the impulses dt_k u; an infinite bound stays infinite).
// solve: this team has a problem.  status: TG_OK, TG_NOT_CONVERGED (z is the last feasible iterate, rho belongs to it) or
// TG_SINGULAR (no answer: the first solve lost rank, or something is not finite -- then the returned rank is 0 too).
template <int TEAM, class CORE, class PROG>
TG_HD int inverse_bounded_stage(const CORE &core, const PROG &P, const double *S, int lane, bool solve, const double *r0, const double *Dh,
                                bool minus, double ridge, double rcond, const double *lo, const double *hi, double u_scale, int max_solves,
                                double *W, double *scr, int &solves, int &status) {
    const int nd = P.nd, n = P.nu + P.nc, ld = n + 1, R = nd + (ridge > 0.0 ? n : 0);
    const BvlsScratch X = bvls_scratch(scr, R, n);
    if (solve) TG_FOR(i, R * ld) W[i] = 0.0;
    TG_SYNC();
    if (solve) {
        TG_FOR(i, nd) { inverse_row(core, P, S, i, W + i * ld, Dh, minus); W[i * ld + n] = -r0[i]; }
        if (ridge > 0.0) { const double s = sqrt(ridge); TG_FOR(j, n) W[(nd + j) * ld + j] = s; }
        TG_FOR(j, n) { const double s = j < P.nu ? u_scale : 1.0; X.lo[j] = lo[j] * s; X.hi[j] = hi[j] * s; }
    }
    TG_SYNC();
    bool finite = true;
#if defined(TG_HELPER_WAVES)
    constexpr bool VOTE = false;
#else
    constexpr bool VOTE = true;      // (the generic kernels are one wavefront per workgroup: __launch_bounds__(64))
#endif
    int r = bvls_solve<TEAM, VOTE>(solve, W, R, n, ld, rcond, max_solves, scr, lane, solves, status, finite);
    const bool answer = solve && status != BVLS_SINGULAR;
    if (answer) TG_FOR(i, nd) {
        double *row = W + i * ld;
        double acc = r0[i];
        for (int j = 0; j < n; j++) acc = fma(row[j], X.z[j], acc);
        row[n] = acc;
    }
    TG_SYNC();
    if (answer) for (int i = 0; i < nd; i++) if (!(fabs(W[i * ld + n]) <= DBL_MAX)) { status = BVLS_SINGULAR; finite = false; }      // (team-uniform)
    if (!finite) r = 0;
    return r;
}

}  // namespace tg
