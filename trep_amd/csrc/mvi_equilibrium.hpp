// mvi_equilibrium.hpp -- MODE_EQUILIBRIUM: batched equilibrium search, one team per pose (tg_batch_minimize_potential).
//
// Per pose (the reference's System.minimize_potential_energy, trep/system.py:215-272): minimise V(q) over the FREE configs F subject
// to h(q) = 0, the other configs held at their input values.  A safeguarded Newton iteration on the KKT conditions; the numpy
// iteration of tests/equilibrium_reference.py is the specification and this file follows it decision for decision.
// At a point (q, mu): h, D = Dh[:, F], V, g = V_q[F] + D' mu, W = V_qq[F, F] + sum_c mu_c h_c,qq[F, F]  (Core::potential_lds and
// Core::con_d2 over the pair list, as the projection).  From q = q0 with the least-squares multipliers of the start
// ([[I, D'], [D, 0]] (d, mu) = (-V_q[F], 0); zero where that solve is rejected), tau = 0, rho = 0:
//   converged when max |h| <= tolerance and max |g| <= tolerance (written so that a NaN fails it); otherwise a TRIAL, each of which
//   counts toward max_iterations and is rejected if it fails any of
//   (1) definiteness: W + tau I + sigma D'D has an unpivoted Cholesky factor, sigma = 1e8 wmax / max diag(D'D),
//       wmax = max |diag W| -- sufficient (Finsler) for W + tau I being positive on the null space of D;
//   (2) the solve [[W + tau I, D'], [D, 0]] (d, dmu) = -(g, h) by gauss_jordan: the matrix accepted, the step finite;
//   (3) acceptance at the trial point (q_F + d, mu + dmu): with rho+ = max(rho, 2 |mu + dmu|inf) and phi = V + rho+ |h|_1 on both
//       sides, phi_trial <= phi + 64 eps max(1, |phi|); or, while tau <= 1e-3 wmax, the KKT residual max(|h|inf, |g|inf) at the trial
//       point is at most half the current one.
//   Accepted: tau /= 4, and 0 once under 1e-6 wmax.  Rejected: tau = max(4 tau, 1e-3 wmax); tau > 1e9 wmax ends the search.
// Status per pose: TG_OK converged; TG_NOT_CONVERGED the budget is used, q = the last accepted iterate; TG_SINGULAR tau ran out, or
// nothing is free and the input does not pass the test.  No constraint is a normal case (D empty).
//
// Every decision reads LDS words that the whole team sees, so it is team-uniform without a vote; the teams of a wavefront leave
// together (__all) and a finished team idles through the phases.  A rejected trial puts q and mu back and evaluates the point
// again: the same arithmetic on the same input, so the state is the one before the trial bit for bit.
// LDS of a team: the rollout slice (sweeps, h, the sparse Dh; mu in its lambda area) and behind it the frame's scratch (mvi_pose.hpp:
// the KKT image, q0, the solver's row scales, the free configs' places) with the search's own regions in it: behind the image
// W [nF][nF] and the Cholesky work area [nF][nF]; behind q0 the pose and multipliers before the trial [nq + nc], V_q [nq], g [nq]
// and V (2 words).
// Compiled by hipcc (trepamd_equilibrium.hip: k_equilibrium) and, with TEAM = 1, by g++ for the CPU tests (tests/emu_pose).
#pragma once
#include <cfloat>

#include "mvi_pose.hpp"

namespace tg {

constexpr int MODE_EQUILIBRIUM = 10;

// (the fields of the frame, mvi_pose.hpp, V and the search's own regions)
struct EquilibriumArgs {
    const int *free_mask;        // [nq] device, non-zero = free; null: every config
    const double *q0;            // [batch][nq]
    double *q, *mu, *v;          // [batch][nq], [batch][nc] (or null), [batch][2]: V at the start and at the returned pose (or null)
    int o_kkt, o_w, o_chol, o_q0, o_keep, o_vq, o_g, o_v, o_scal, o_idx;   // LDS offsets (doubles) behind the rollout slice
    int lds_per_team;            // doubles per team: what the kernel strides its teams by
};

inline void equilibrium_layout(int rollout_lds_per_team, int nq, int nc, EquilibriumArgs &J) {
    pose_layout(rollout_lds_per_team, nq, nc, J, {{&J.o_w, nq * nq}, {&J.o_chol, nq * nq}},
                {{&J.o_keep, nq + nc}, {&J.o_vq, nq}, {&J.o_g, nq}, {&J.o_v, 2}});
}

template <int TEAM, bool SPRINGS, bool PAR, class PROG, class ARGS>
TG_HD void run_equilibrium(PROG &P, ARGS &A, const EquilibriumArgs &J, const ParTable T, double *S, int lane, int traj) {
    const int nq = P.nq, nd = P.nd, nc = P.nc;
    PoseFrame<TEAM, PROG, EquilibriumArgs> F(P, J, S, lane, traj, A.batch);
    const bool live = F.live;
    const size_t t = F.t;
    Core<TEAM, SPRINGS, PROG, double, PAR> core(P, S, lane, 1.0);
    if constexpr (PAR) core.par = T.rows + (t / (size_t)T.group) * (size_t)T.stride + 4 * P.n_bodies;
    else (void)T;
    core.init_sweep_schedule(false);
    double *K = F.K, *W = S + J.o_w, *C = S + J.o_chol, *keep = S + J.o_keep, *Vq = S + J.o_vq, *G = S + J.o_g;
    double *Vs = S + J.o_v, *scal = F.scal;
    int *idx = F.idx;
    const int nF = F.index_free(), n = nF + nc, ld = n + 1;
    F.load_pose();

    // everything the iteration reads at (q2, lambda area): h, Dh, V, V_q, W with the multipliers' curvature, g
    auto evaluate = [&](bool on) {
        if (!pose_any(on)) return;
        core.potential_lds(on, S + P.o_Dh2, Vs, Vq, W, nF, idx);
        if (on) F.add_curvature(core, W, nF);
        if (on) TG_FOR(k, nq) {
            const int a = idx[k];
            if (a < 0) continue;
            double g = Vq[k];
            for (int c = 0; c < nc; c++) { const int m = P.dh_lookup[c * nq + k]; if (m >= 0) g = fma(S[P.o_Dh2 + m], S[P.o_lam + c], g); }
            G[a] = g;
        }
        TG_SYNC();
    };
    // max(|h|inf, |g|inf) (a NaN stays one) and |h|_1 of the evaluated point: every lane scans the same words
    auto measure = [&](double &kkt, double &h1) {
        bool nan = false;
        kkt = 0.0; h1 = 0.0;
        for (int a = 0; a < nF; a++) { const double v = fabs(G[a]); if (v != v) nan = true; if (v > kkt) kkt = v; }
        for (int c = 0; c < nc; c++) { const double v = fabs(S[P.o_f + nd + c]); if (v != v) nan = true; if (v > kkt) kkt = v; h1 += v; }
        if (nan) kkt = NAN;
    };
    // the image [[Wblock, D'], [D, 0]] with the right-hand side -(first | second): Wblock = W + tau I, or the identity
    auto assemble = [&](bool on, bool identity, double tau, const double *first, bool second) {
        if (on) TG_FOR(i, n * ld) K[i] = 0.0;
        TG_SYNC();
        if (on) {
            F.scatter_dh(nF, ld);
            TG_FOR(e, nF * nF) { const int a = e / nF, b = e % nF; K[a * ld + b] = identity ? (a == b ? 1.0 : 0.0) : W[e] + (a == b ? tau : 0.0); }
            TG_FOR(a, nF) K[a * ld + n] = -first[a];
            TG_FOR(c, nc) K[(nF + c) * ld + n] = second ? -S[P.o_f + nd + c] : 0.0;
        }
        TG_SYNC();
    };
    auto finite_step = [&]() {
        bool ok = true;
        for (int i = 0; i < n; i++) if (!(fabs(K[i * ld + n]) <= DBL_MAX)) ok = false;
        return ok;
    };
    // unpivoted, right-looking Cholesky of the image's W block + sigma D'D in the work area, carried out by the team
    auto definite = [&](bool on, double sigma) {
        if (on) TG_FOR(e, nF * nF) {
            const int a = e / nF, b = e % nF;
            double s = 0.0;
            for (int c = 0; c < nc; c++) s = fma(K[(nF + c) * ld + a], K[(nF + c) * ld + b], s);
            C[e] = K[a * ld + b] + sigma * s;
        }
        TG_SYNC();
        bool ok = on;
        for (int k = 0; k < nF; k++) {
            const double piv = ok ? C[k * nF + k] : 1.0;
            if (!(piv > 0.0)) ok = false;             // (a NaN fails it)
            const double r = sqrt(piv);
            const int m = nF - k - 1;
            TG_SYNC();                                // every lane has the pivot before its column is scaled
            if (ok) TG_FOR(j, m + 1) C[(k + j) * nF + k] /= r;
            TG_SYNC();
            if (ok) TG_FOR(e, m * m) {
                const int i = k + 1 + e / m, j = k + 1 + e % m;
                if (i >= j) C[i * nF + j] -= C[i * nF + k] * C[j * nF + k];
            }
            TG_SYNC();
        }
        return ok;
    };

    int status = TG_OK, iterations = 0;
    bool done = !live;
    double tau = 0.0, rho = 0.0;
    evaluate(!done);
    const double v_start = Vs[0];
    if (nc > 0 && nF > 0) {      // the least-squares multipliers of the start; W and g then belong to them
        assemble(!done, true, 0.0, G, false);        // (with mu = 0, g is V_q over the free places)
        const bool ok = core.gauss_jordan(!done, K, n, 1, ld, scal) && finite_step();
        if (!done && ok) TG_FOR(c, nc) S[P.o_lam + c] = K[(nF + c) * ld + n];
        TG_SYNC();
        evaluate(!done && ok);
    }
    for (;;) {
        double kkt, h1, wmax = 0.0;
        measure(kkt, h1);
        const double V = Vs[0];
        for (int a = 0; a < nF; a++) { const double v = fabs(W[a * nF + a]); if (v > wmax) wmax = v; }
        if (!done) {
            if (kkt <= A.tolerance) done = true;
            else if (nF == 0) { done = true; status = TG_SINGULAR; }
            else if (iterations >= A.max_iterations) { done = true; status = TG_NOT_CONVERGED; }
            else if (tau > 1e9 * wmax) { done = true; status = TG_SINGULAR; }
        }
        if (pose_all(done)) break;       // the teams of a wavefront leave together: a finished one idles through the phases
        if (!done) iterations++;
        assemble(!done, false, tau, G, true);
        double dmax = 0.0;
        if (!done) for (int a = 0; a < nF; a++) {
            double s = 0.0;
            for (int c = 0; c < nc; c++) s = fma(K[(nF + c) * ld + a], K[(nF + c) * ld + a], s);
            if (s > dmax) dmax = s;
        }
        bool ok = definite(!done, dmax > 0.0 ? 1e8 * wmax / dmax : 0.0);
        ok = core.gauss_jordan(ok, K, n, 1, ld, scal) && ok;
        ok = ok && finite_step();
        if (ok) {
            TG_FOR(k, nq) {
                const int a = idx[k];
                const double v = S[P.o_q2 + k];
                keep[k] = v;
                if (a >= 0) { S[P.o_q1 + k] = v + K[a * ld + n]; S[P.o_q2 + k] = v + K[a * ld + n]; }
            }
            TG_FOR(c, nc) { const double v = S[P.o_lam + c]; keep[nq + c] = v; S[P.o_lam + c] = v + K[(nF + c) * ld + n]; }
        }
        TG_SYNC();
        evaluate(ok);
        bool take = false;
        if (ok) {
            double kkt_t, h1_t, mu_inf = 0.0;
            measure(kkt_t, h1_t);
            for (int c = 0; c < nc; c++) { const double v = fabs(S[P.o_lam + c]); if (v > mu_inf) mu_inf = v; }
            const double rho_t = rho > 2.0 * mu_inf ? rho : 2.0 * mu_inf;
            const double phi = V + rho_t * h1, phi_t = Vs[0] + rho_t * h1_t;
            take = phi_t <= phi + 64.0 * DBL_EPSILON * (fabs(phi) > 1.0 ? fabs(phi) : 1.0);
            if (!take && tau <= 1e-3 * wmax) take = kkt_t <= 0.5 * kkt;
            if (take) rho = rho_t;
        }
        TG_SYNC();                                    // the decision is read before the pose is put back
        const bool back = ok && !take;
        if (back) {
            TG_FOR(k, nq) { S[P.o_q1 + k] = keep[k]; S[P.o_q2 + k] = keep[k]; }
            TG_FOR(c, nc) S[P.o_lam + c] = keep[nq + c];
        }
        TG_SYNC();
        evaluate(back);
        if (!done) {
            if (take) { tau *= 0.25; if (tau < 1e-6 * wmax) tau = 0.0; }
            else tau = 4.0 * tau > 1e-3 * wmax ? 4.0 * tau : 1e-3 * wmax;
        }
    }
    if (live && lane == 0 && J.v) { J.v[2 * t] = v_start; J.v[2 * t + 1] = Vs[0]; }
    F.store(A, iterations, status);
}

}  // namespace tg
