// mvi_modes.hpp -- MODE_MODES: batched normal modes, one team per pose (tg_batch_normal_modes).
//
// Per pose: the small-oscillation eigenproblem K phi = omega^2 M phi on the tangent space of the constraints, over the FREE configs F
// (the launch's mask: dynamic configs only), the other configs held.  tests/normal_modes_reference.py is the specification and this
// file follows it decision for decision.
//   1. At rest (dq = 0): V_q, V_qq[F, F], h, D = Dh[:, F] (Core::potential_lds) and M = L_ddqddq[F, F] (Core::mass_lds).
//   2. mu as supplied, or the minimum-norm minimiser of |V_q[F] + D' mu| (lsq_solve under rcond).  residual = |V_q[F] + D' mu|inf.
//   3. K = V_qq[F, F] + sum_c mu_c h_c,qq[F, F] (PoseFrame::add_curvature: the sign conventions of mvi_equilibrium.hpp's W).
//   4. Column-pivoted Householder QR of D' (nF x nc) with the identity carried along (lsq_factor<TEAM, true>, extra = nF): the carried
//      block ends as Q'.  r = the rank under rcond; Z = the last nm = nF - r columns of Q (rows r .. nF - 1 of the carried block).
//   5. M_r = Z'MZ, K_r = Z'KZ, both symmetrised; unpivoted Cholesky M_r = LL' (a pivot that is not > 0 ends the pose: TG_SINGULAR);
//      C = L^-1 K_r L^-T, symmetrised.
//   6. Jacobi eigen-solve of C (sym_eig.hpp); a pose that uses max_sweeps sweeps without passing the test is TG_NOT_CONVERGED and
//      its current answer is still written.
//   7. lambda ascending (ranked by counting, equal values in column order), Phi = Z L^-T Y scattered to [nF][nq] with zeros at the held
//      configs, the component of largest magnitude of every shape positive (of equal magnitudes the lowest config index decides).
// A pose whose q is not finite, whose multipliers or C are not finite or whose M_r has no Cholesky factor is TG_SINGULAR and every
// numeric output of it is zero.
// Every decision reads LDS words that the whole team sees, so it is team-uniform without a vote; nF is the launch's (the mask is), so
// it counts every loop with a fence; a team's rank and nm are predicates.
// LDS of a team: the rollout slice and behind it the frame's scratch (mvi_pose.hpp) with the regions of this kernel: behind the image
// (which holds [D' | -V_q] for the multipliers, then [D' | I] for the null space) K, M [nF][nF] and four [nF][ld] images, ld = nF | 1
// (sym_eig.hpp): the work area T, K_r -> C, M_r -> L, Y; behind q0: V_q, g, V, the least-squares scratch, the (c, s) of a Jacobi set,
// the eigenvalues and their places.
// Compiled by hipcc (trepamd_modes.hip: k_modes) and, with TEAM = 1, by g++ for the CPU tests (tests/emu_modes).
#pragma once
#include <cfloat>

#include "lsq_solve.hpp"
#include "mvi_pose.hpp"
#include "sym_eig.hpp"

namespace tg {

constexpr int MODE_MODES = 15;

// (the fields of the frame, mvi_pose.hpp, and the kernel's own)
struct ModesArgs {
    const int *free_mask;        // [nq] device, non-zero = free (never null here: the host clears the kinematic configs)
    const double *q0;            // [batch][nq]
    const double *mu_in;         // [batch][nc] multipliers to take as they are, or null: least squares
    double *q, *mu;              // unused (null) / [batch][nc] out (or null): the frame's names
    double *omega2, *modes;      // [batch][n_free], [batch][n_free][nq]
    double *residual;            // [batch] (or null)
    int *count, *rank;           // [batch] each (or null)
    double rcond;
    int n_free, max_sweeps;
    int o_kkt, o_w, o_m, o_t, o_kr, o_mr, o_y, o_q0, o_vq, o_g, o_v, o_lsq, o_cs, o_lam, o_scal, o_idx;   // LDS offsets (doubles)
    int lds_per_team;
};

inline void modes_layout(int rollout_lds_per_team, int nq, int nc, ModesArgs &J) {
    const int im = nq * sym_eig_ld(nq);
    pose_layout(rollout_lds_per_team, nq, nc, J, {{&J.o_w, nq * nq}, {&J.o_m, nq * nq}, {&J.o_t, im}, {&J.o_kr, im}, {&J.o_mr, im}, {&J.o_y, im}},
                {{&J.o_vq, nq}, {&J.o_g, nq}, {&J.o_v, 2}, {&J.o_lsq, lsq_scratch_doubles(nc) + 2}, {&J.o_cs, sym_eig_scratch_doubles(nq)},
                 {&J.o_lam, 2 * nq}});
}

template <int TEAM, bool SPRINGS, bool PAR, class PROG, class ARGS>
TG_HD void run_modes(PROG &P, ARGS &A, const ModesArgs &J, const ParTable T, double *S, int lane, int traj) {
    const int nq = P.nq, nc = P.nc;
    PoseFrame<TEAM, PROG, ModesArgs> F(P, J, S, lane, traj, A.batch);
    const bool live = F.live;
    const size_t t = F.t;
    Core<TEAM, SPRINGS, PROG, double, PAR> core(P, S, lane, 1.0);
    if constexpr (PAR) core.par = T.rows + (t / (size_t)T.group) * (size_t)T.stride + 4 * P.n_bodies;
    else (void)T;
    core.init_sweep_schedule(false);
    double *K = F.K, *W = S + J.o_w, *M = S + J.o_m, *Tw = S + J.o_t, *Kr = S + J.o_kr, *Mr = S + J.o_mr, *Y = S + J.o_y;
    double *Vq = S + J.o_vq, *G = S + J.o_g, *Vs = S + J.o_v, *cs = S + J.o_cs, *lam = S + J.o_lam;
    double *nrm = S + J.o_lsq, *z = nrm + nc, *tau2 = z + nc;
    int *perm = (int *)(tau2 + nc), *place = (int *)(lam + nq);
    int *idx = F.idx;
    const int nF = F.index_free(), ld = nc + nF, jl = sym_eig_ld(nF);      // (nF == J.n_free: the launch's)
    F.load_pose();

    bool go = live;
    for (int k = 0; k < nq; k++) if (!(fabs(F.Q0[k]) <= DBL_MAX)) go = false;      // (every lane scans the same words: team-uniform)
    if (J.mu_in && live) TG_FOR(c, nc) S[P.o_lam + c] = J.mu_in[t * nc + c];
    TG_SYNC();
    if (pose_any(live)) {
        core.potential_lds(live, S + P.o_Dh2, Vs, Vq, W, nF, idx);
        core.mass_lds(live, M, nF, idx);
    }
    // D' into the image, rows the free configs, columns the constraints; `unit`: the identity behind it, else -V_q[F] in column nc
    auto image = [&](bool unit) {
        if (live) TG_FOR(i, nF * ld) K[i] = 0.0;
        TG_SYNC();
        if (live) {
            TG_FOR(m, P.n_dh) {
                const int c = P.dh_pack[8 * (size_t)m], a = idx[P.dh_pack[8 * (size_t)m + 1]];
                if (a >= 0) K[a * ld + c] = S[P.o_Dh2 + m];
            }
            TG_FOR(k, nq) {
                const int a = idx[k];
                if (a < 0) continue;
                if (unit) K[a * ld + nc + a] = 1.0; else K[a * ld + nc] = -Vq[k];
            }
        }
        TG_SYNC();
    };
    if (!J.mu_in && nc > 0 && nF > 0) {
        image(false);
        bool ok = true;
        lsq_solve<TEAM>(go, K, nF, nc, ld, J.rcond, perm, nrm, z, tau2, lane, ok);
        if (go && !ok) go = false;
        if (go) TG_FOR(c, nc) S[P.o_lam + c] = z[c];
        TG_SYNC();
    }
    if (go) for (int c = 0; c < nc; c++) if (!(fabs(S[P.o_lam + c]) <= DBL_MAX)) go = false;
    // g = V_q[F] + D' mu and the stiffness
    if (live) {
        F.add_curvature(core, W, nF);
        TG_FOR(k, nq) {
            const int a = idx[k];
            if (a < 0) continue;
            double g = Vq[k];
            for (int c = 0; c < nc; c++) { const int m = P.dh_lookup[c * nq + k]; if (m >= 0) g = fma(S[P.o_Dh2 + m], S[P.o_lam + c], g); }
            G[a] = g;
        }
    }
    TG_SYNC();
    double residual = 0.0;
    for (int a = 0; a < nF; a++) { const double v = fabs(G[a]); if (v > residual) residual = v; if (v != v) go = false; }
    // the null space
    int r = 0;
    if (nF > 0) {
        image(true);
        if (nc > 0) {
            if (go) TG_FOR(c, nc) perm[c] = c;
            bool bad = false;
            TG_SYNC();
            const int own = nF < nc ? nF : nc;
            r = lsq_factor<TEAM, true>(go, K, ld, 1, nF, nc, nF, own, own, J.rcond, perm, nrm, nullptr, lane, bad);
            TG_SYNC();
            if (bad) go = false;
        }
    }
    const int nm = go ? nF - r : 0;
    auto Zc = [&](int a, int j) { return K[(r + j) * ld + nc + a]; };      // Z (a, j)
    // X_r = Z' X Z, symmetrised, into R [nm][jl]
    auto reduce = [&](const double *X, double *R) {
        if (go) TG_FOR(e, nF * nm) {
            const int a = e / nm, j = e % nm;
            double s = 0.0;
            for (int b = 0; b < nF; b++) s = fma(X[a * nF + b], Zc(b, j), s);
            Tw[a * jl + j] = s;
        }
        TG_SYNC();
        if (go) TG_FOR(e, nm * nm) {
            const int i = e / nm, j = e % nm;
            double s = 0.0;
            for (int a = 0; a < nF; a++) s = fma(Zc(a, i), Tw[a * jl + j], s);
            R[i * jl + j] = s;
        }
        TG_SYNC();
    };
    auto symmetrise = [&](double *R) {
        if (go) TG_FOR(e, nm * nm) {
            const int i = e / nm, j = e % nm;
            if (i < j) { const double v = 0.5 * (R[i * jl + j] + R[j * jl + i]); R[i * jl + j] = v; R[j * jl + i] = v; }
        }
        TG_SYNC();
    };
    reduce(M, Mr); symmetrise(Mr);
    reduce(W, Kr); symmetrise(Kr);
    // unpivoted, right-looking Cholesky of M_r in place (mvi_equilibrium.hpp: definite)
    {
        bool ok = go;
        for (int k = 0; k < nF; k++) {
            const bool in = ok && k < nm;
            const double piv = in ? Mr[k * jl + k] : 1.0;
            if (!(piv > 0.0)) ok = false;             // (a NaN fails it)
            const double rt = sqrt(piv);
            const int m = nm - k - 1;
            TG_SYNC();                                // every lane has the pivot before its column is scaled
            if (ok && in) TG_FOR(j, m + 1) Mr[(k + j) * jl + k] /= rt;
            TG_SYNC();
            if (ok && in) TG_FOR(e, m * m) {
                const int i = k + 1 + e / m, j = k + 1 + e % m;
                if (i >= j) Mr[i * jl + j] -= Mr[i * jl + k] * Mr[j * jl + k];
            }
            TG_SYNC();
        }
        if (go && !ok) go = false;
    }
    // C = L^-1 K_r L^-T in place: the columns forwards (one lane each), then the rows, then symmetrised
    if (go) TG_FOR(j, nm) for (int i = 0; i < nm; i++) {
        double s = Kr[i * jl + j];
        for (int k = 0; k < i; k++) s = fma(-Mr[i * jl + k], Kr[k * jl + j], s);
        Kr[i * jl + j] = s / Mr[i * jl + i];
    }
    TG_SYNC();
    if (go) TG_FOR(i, nm) for (int j = 0; j < nm; j++) {
        double s = Kr[i * jl + j];
        for (int k = 0; k < j; k++) s = fma(-Kr[i * jl + k], Mr[j * jl + k], s);
        Kr[i * jl + j] = s / Mr[j * jl + j];
    }
    TG_SYNC();
    symmetrise(Kr);
    if (go) for (int e = 0; e < nm * nm; e++) if (!(fabs(Kr[(e / nm) * jl + e % nm]) <= DBL_MAX)) { go = false; break; }
    const int n_eig = go ? nm : 0;
    if (go) TG_FOR(e, nm * nm) Y[(e / nm) * jl + e % nm] = e / nm == e % nm ? 1.0 : 0.0;
    TG_SYNC();
    bool converged = false;
    const int sweeps = sym_eig_jacobi<TEAM>(go, Kr, Y, n_eig, nF, jl, J.max_sweeps, cs, lane, converged, [](bool f) { return pose_all(f); });
    // the eigenvalues and their places in ascending order (counted, equal values in column order)
    if (go) TG_FOR(j, nm) lam[j] = Kr[j * jl + j];
    TG_SYNC();
    if (go) TG_FOR(j, nm) {
        int at = 0;
        for (int i = 0; i < nm; i++) if (lam[i] < lam[j] || (lam[i] == lam[j] && i < j)) at++;
        place[j] = at;
    }
    // U = L^-T Y in place, one lane per column, backwards
    if (go) TG_FOR(j, nm) for (int i = nm - 1; i >= 0; i--) {
        double s = Y[i * jl + j];
        for (int k = i + 1; k < nm; k++) s = fma(-Mr[k * jl + i], Y[k * jl + j], s);
        Y[i * jl + j] = s / Mr[i * jl + i];
    }
    TG_SYNC();
    // Phi (mode j, free config a) = sum_b Z (a, b) U (b, j) into the work area [nm][jl], then the sign of every shape
    if (go) TG_FOR(e, nm * nF) {
        const int j = e / nF, a = e % nF;
        double s = 0.0;
        for (int b = 0; b < nm; b++) s = fma(Zc(a, b), Y[b * jl + j], s);
        Tw[j * jl + a] = s;
    }
    TG_SYNC();
    if (go) TG_FOR(j, nm) {
        double best = -1.0, sign = 1.0;
        for (int a = 0; a < nF; a++) { const double v = Tw[j * jl + a]; if (fabs(v) > best) { best = fabs(v); sign = v < 0.0 ? -1.0 : 1.0; } }
        cs[j] = sign;      // (the Jacobi scratch is free again)
    }
    TG_SYNC();
    if (live) {
        double *o2 = J.omega2 + t * (size_t)nF, *om = J.modes + t * (size_t)nF * nq;
        const int rows = go ? nm : 0;      // (a pose that failed after its null space was found writes zeros alone)
        TG_FOR(i, nF) if (i >= rows) o2[i] = 0.0;
        TG_FOR(e, nF * nq) {
            const int row = e / nq, a = idx[e % nq];
            if (row >= rows || a < 0) om[e] = 0.0;
        }
        if (go) TG_FOR(e, nm * nq) {
            const int j = e / nq, k = e % nq, a = idx[k];
            if (a >= 0) om[(size_t)place[j] * nq + k] = cs[j] * Tw[j * jl + a];
        }
        if (go) TG_FOR(j, nm) o2[place[j]] = lam[j];
        if (J.mu) TG_FOR(c, nc) J.mu[t * nc + c] = go ? S[P.o_lam + c] : 0.0;
        if (lane == 0) {
            if (J.residual) J.residual[t] = go ? residual : 0.0;
            if (J.count) J.count[t] = rows;
            if (J.rank) J.rank[t] = go ? r : 0;
            A.iters[t] = go ? sweeps : 0;
            A.status[t] = !go ? TG_SINGULAR : (converged ? TG_OK : TG_NOT_CONVERGED);
        }
    }
}

}  // namespace tg
