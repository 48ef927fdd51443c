// mvi_response.hpp -- MODE_RESPONSE: batched static response, one team per pose (tg_batch_static_response).
//
// Per pose: how a rest pose and its multipliers move with the held configs (the drive response) and under a load on the free configs
// (the compliance and the reaction), over the FREE configs F of the launch's mask, H the held ones, E the driven held configs.
// tests/static_response_reference.py is the specification and this file follows it decision for decision.
//   1. At rest (dq = 0): V_q, V_qq over ALL configs (Core::potential_lds with the identity index), h and the sparse Dh.
//   2. mu as supplied, or the minimum-norm minimiser of |V_q[F] + D_F' mu| (lsq_solve under rcond: mvi_modes.hpp's step 2).
//      residual = |V_q[F] + D_F' mu|inf.
//   3. W = V_qq + sum_c mu_c h_c,qq over all config pairs (PoseFrame::add_curvature with the identity index).
//   4. Column-pivoted Householder QR of D_F' (nF x nc) with the identity carried along: D_F' P = Q [T; 0], T = [R11 R12] of r rows,
//      r the rank under rcond; Z = the last nm = nF - r columns of Q.  r < nc: T' = Q2 [U; 0] by r more reflections (lsq_factor
//      without pivoting, strides exchanged, as lsq_solve does it).  The pseudo-inverse in the pivoted order, Pp = Q2 [U'^-1 Q1'; 0]
//      (r == nc: R11^-1 Q1'), [nc][nF]: row j belongs to constraint perm[j].  Every right-hand side below goes through this one
//      factorisation.
//   5. K_r = Z' W_FF Z, symmetrised; unpivoted Cholesky K_r = LL' (a pivot that is not > 0 ends the pose: TG_SINGULAR).
//   6. N = nD (+ nF with the compliance) columns (x_p, f): a driven config e: x_p = -Pp' D_H e, f = -W_FH e; a unit load on free
//      config a: x_p = 0, f = e_a.  x = x_p + Z K_r^-1 Z' (f - W_FF x_p), y = Pp (f - W_FF x).  Drive columns: dq = x, dmu = y;
//      load columns: C = x, R = y.  defect = |D_F X + D_H E|inf.
// A pose whose q, multipliers or answer is not finite or whose K_r has no Cholesky factor is TG_SINGULAR and every numeric output of
// it is zero.
// Every decision reads LDS words that the whole team sees, so it is team-uniform without a vote; nF, nc and nD are the launch's, so
// they count every loop with a fence; a team's rank and nm are predicates.
// LDS of a team: the rollout slice and behind it the frame's scratch (mvi_pose.hpp) with the regions of this kernel: behind the image
// (which holds [D_F' | -V_q] for the multipliers, then [D_F' | I] for the factorisation) W [nq][nq], Pp [nc][max(nF, nD)], K_r -> L
// [nF][nF | 1], a work area (Z'-products [nF][nF | 1], then [max(nF, nc)][N]), X and G [nF][N]; behind q0: V_q, V, the least-squares
// scratch, the free configs' list and the identity index.
// Compiled by hipcc (trepamd_response.hip: k_response) and, with TEAM = 1, by g++ for the CPU tests (tests/emu_response).
#pragma once
#include <cfloat>

#include "lsq_solve.hpp"
#include "mvi_pose.hpp"

namespace tg {

constexpr int MODE_RESPONSE = 16;

// (the fields of the frame, mvi_pose.hpp, and the kernel's own)
struct ResponseArgs {
    const int *free_mask;        // [nq] device, non-zero = free (never null here)
    const int *drive;            // [n_drive] device: the driven configs, all of them held
    const double *q0;            // [batch][nq]
    const double *mu_in;         // [batch][nc] multipliers to take as they are, or null: least squares
    double *q, *mu;              // unused (null) / [batch][nc] out (or null): the frame's names
    double *dq, *dmu;            // [batch][n_drive][nq], [batch][n_drive][nc]
    double *compliance, *reaction;      // [batch][nq][nq], [batch][nq][nc]; read only with `loads`
    double *residual, *defect;   // [batch] each (or null)
    int *rank;                   // [batch] (or null)
    double rcond;
    int n_free, n_drive, loads;  // loads: the load columns (compliance, reaction) are asked for
    int o_kkt, o_w, o_pinv, o_kr, o_t, o_x, o_g, o_q0, o_vq, o_v, o_lsq, o_fl, o_idn, o_scal, o_idx;   // LDS offsets (doubles)
    int lds_per_team;
};

TG_HD int response_ld(int n) { return n | 1; }

// n_free, n_drive and loads are the launch's: the regions are as large as this launch needs them
inline void response_layout(int rollout_lds_per_team, int nq, int nc, int n_free, int n_drive, bool loads, ResponseArgs &J) {
    const int nF = n_free, N = n_drive + (loads ? nF : 0), cols = N > 1 ? N : 1, wide = nF > nc ? nF : nc;
    const int work = nF * response_ld(nF) > wide * N ? nF * response_ld(nF) : wide * N;
    pose_layout(rollout_lds_per_team, nq, nc, J,
                {{&J.o_w, nq * nq}, {&J.o_pinv, nc * (nF > n_drive ? nF : n_drive)}, {&J.o_kr, nF * response_ld(nF)}, {&J.o_t, work}, {&J.o_x, nF * cols}, {&J.o_g, nF * cols}},
                {{&J.o_vq, nq}, {&J.o_v, 2}, {&J.o_lsq, lsq_scratch_doubles(nc) + 2}, {&J.o_fl, (nq + 1) / 2}, {&J.o_idn, (nq + 1) / 2}});
}

template <int TEAM, bool SPRINGS, bool PAR, class PROG, class ARGS>
TG_HD void run_response(PROG &P, ARGS &A, const ResponseArgs &J, const ParTable T, double *S, int lane, int traj) {
    const int nq = P.nq, nc = P.nc;
    PoseFrame<TEAM, PROG, ResponseArgs> F(P, J, S, lane, traj, A.batch);
    const bool live = F.live;
    const size_t t = F.t;
    Core<TEAM, SPRINGS, PROG, double, PAR> core(P, S, lane, 1.0);
    if constexpr (PAR) core.par = T.rows + (t / (size_t)T.group) * (size_t)T.stride + 4 * P.n_bodies;
    else (void)T;
    core.init_sweep_schedule(false);
    double *K = F.K, *W = S + J.o_w, *Pp = S + J.o_pinv, *Kr = S + J.o_kr, *Tw = S + J.o_t, *X = S + J.o_x, *G = S + J.o_g;
    double *Vq = S + J.o_vq, *Vs = S + J.o_v;
    double *nrm = S + J.o_lsq, *z = nrm + nc, *tau2 = z + nc;
    int *perm = (int *)(tau2 + nc), *fl = (int *)(S + J.o_fl), *idn = (int *)(S + J.o_idn);
    int *idx = F.idx;
    const bool loads = J.loads != 0;
    const int nF = F.index_free(), nD = J.n_drive, ld = nc + nF, jl = response_ld(nF);      // (nF == J.n_free: the launch's)
    const int N = nD + (loads ? nF : 0), own = nF < nc ? nF : nc;
    TG_FOR(k, nq) idn[k] = k;
    F.load_pose();
    TG_FOR(k, nq) if (idx[k] >= 0) fl[idx[k]] = k;

    bool go = live;
    for (int k = 0; k < nq; k++) if (!(fabs(F.Q0[k]) <= DBL_MAX)) go = false;      // (every lane scans the same words: team-uniform)
    if (J.mu_in && live) TG_FOR(c, nc) S[P.o_lam + c] = J.mu_in[t * nc + c];
    if (live) TG_FOR(c, nc) perm[c] = c;
    TG_SYNC();
    if (pose_any(live)) core.potential_lds(live, S + P.o_Dh2, Vs, Vq, W, nq, idn);
    // D_F' into the image, rows the free configs, columns the constraints; `unit`: the identity behind it, else -V_q[F] in column nc
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
    auto dh = [&](int c, int k) { const int m = P.dh_lookup[c * nq + k]; return m >= 0 ? S[P.o_Dh2 + m] : 0.0; };      // Dh (c, k)
    if (!J.mu_in && nc > 0 && nF > 0) {
        image(false);
        bool ok = true;
        lsq_solve<TEAM>(go, K, nF, nc, ld, J.rcond, perm, nrm, z, tau2, lane, ok);
        if (go && !ok) go = false;
        if (go) TG_FOR(c, nc) S[P.o_lam + c] = z[c];
        TG_SYNC();
    }
    if (go) for (int c = 0; c < nc; c++) if (!(fabs(S[P.o_lam + c]) <= DBL_MAX)) go = false;
    // g = V_q[F] + D_F' mu (into G) and W
    if (live) {
        F.add_curvature(core, W, nq, idn);
        TG_FOR(k, nq) {
            const int a = idx[k];
            if (a < 0) continue;
            double g = Vq[k];
            for (int c = 0; c < nc; c++) g = fma(dh(c, k), S[P.o_lam + c], g);
            G[a] = g;
        }
    }
    TG_SYNC();
    double residual = 0.0;
    for (int a = 0; a < nF; a++) { const double v = fabs(G[a]); if (v > residual) residual = v; if (v != v) go = false; }
    TG_SYNC();
    // the factorisation and the pseudo-inverse
    int r = 0;
    if (nF > 0) {
        image(true);
        if (nc > 0) {
            if (go) TG_FOR(c, nc) perm[c] = c;
            bool bad = false;
            TG_SYNC();
            r = lsq_factor<TEAM, true>(go, K, ld, 1, nF, nc, nF, own, own, J.rcond, perm, nrm, nullptr, lane, bad);
            TG_SYNC();
            const bool deficient = go && r < nc;
            const int r2 = lsq_factor<TEAM, false>(deficient, K, 1, ld, nc, r, 0, r, own, 0.0, nullptr, nullptr, tau2, lane, bad);
            TG_SYNC();
            if (bad || (deficient && r2 != r)) go = false;
            // one lane per column a of Q1': the triangle in place in the carried block, then Q2 on (y; 0)
            if (go) TG_FOR(a, nF) {
                double *B = K + nc + a;      // B (i) = B[i * ld]
                if (deficient) for (int i = 0; i < r; i++) {
                    double s = B[i * ld];
                    for (int k = 0; k < i; k++) s = fma(-K[i * ld + k], B[k * ld], s);
                    B[i * ld] = s / K[i * ld + i];
                } else for (int i = r - 1; i >= 0; i--) {
                    double s = B[i * ld];
                    for (int k = i + 1; k < r; k++) s = fma(-K[i * ld + k], B[k * ld], s);
                    B[i * ld] = s / K[i * ld + i];
                }
                for (int j = 0; j < nc; j++) Pp[j * nF + a] = j < r ? B[j * ld] : 0.0;
                if (deficient) for (int k = r - 1; k >= 0; k--) {
                    double dot = Pp[k * nF + a];
                    for (int i = k + 1; i < nc; i++) dot = fma(K[k * ld + i], Pp[i * nF + a], dot);
                    const double w = tau2[k] * dot;
                    Pp[k * nF + a] -= w;
                    for (int i = k + 1; i < nc; i++) Pp[i * nF + a] = fma(-w, K[k * ld + i], Pp[i * nF + a]);
                }
            }
            TG_SYNC();
        }
    }
    const int nm = go ? nF - r : 0;
    auto Zc = [&](int a, int j) { return K[(r + j) * ld + nc + a]; };      // Z (a, j)
    auto Wff = [&](int a, int b) { return W[fl[a] * nq + fl[b]]; };
    // K_r = Z' W_FF Z, symmetrised, [nm][jl]
    if (go) TG_FOR(e, nF * nm) {
        const int a = e / nm, j = e % nm;
        double s = 0.0;
        for (int b = 0; b < nF; b++) s = fma(Wff(a, b), Zc(b, j), s);
        Tw[a * jl + j] = s;
    }
    TG_SYNC();
    if (go) TG_FOR(e, nm * nm) {
        const int i = e / nm, j = e % nm;
        double s = 0.0;
        for (int a = 0; a < nF; a++) s = fma(Zc(a, i), Tw[a * jl + j], s);
        Kr[i * jl + j] = s;
    }
    TG_SYNC();
    if (go) TG_FOR(e, nm * nm) {
        const int i = e / nm, j = e % nm;
        if (i < j) { const double v = 0.5 * (Kr[i * jl + j] + Kr[j * jl + i]); Kr[i * jl + j] = v; Kr[j * jl + i] = v; }
    }
    TG_SYNC();
    // unpivoted, right-looking Cholesky of K_r in place (mvi_modes.hpp's of M_r)
    {
        bool ok = go;
        for (int k = 0; k < nF; k++) {
            const bool in = ok && k < nm;
            const double piv = in ? Kr[k * jl + k] : 1.0;
            if (!(piv > 0.0)) ok = false;             // (a NaN fails it)
            const double rt = sqrt(piv);
            const int m = nm - k - 1;
            TG_SYNC();                                // every lane has the pivot before its column is scaled
            if (ok && in) TG_FOR(j, m + 1) Kr[(k + j) * jl + k] /= rt;
            TG_SYNC();
            if (ok && in) TG_FOR(e, m * m) {
                const int i = k + 1 + e / m, j = k + 1 + e % m;
                if (i >= j) Kr[i * jl + j] -= Kr[i * jl + k] * Kr[j * jl + k];
            }
            TG_SYNC();
        }
        if (go && !ok) go = false;
    }
    // the columns: x_p into X [nF][N], f - W_FF x_p into G [nF][N]
    auto force = [&](int a, int j) { return j < nD ? -W[fl[a] * nq + J.drive[j]] : (a == j - nD ? 1.0 : 0.0); };
    if (go) TG_FOR(e, nF * N) {
        const int a = e / N, j = e % N;
        double s = 0.0;
        if (j < nD) { const int k = J.drive[j]; for (int c = 0; c < nc; c++) s = fma(-Pp[c * nF + a], dh(perm[c], k), s); }
        X[e] = s;
    }
    TG_SYNC();
    auto unbalanced = [&]() {
        if (go) TG_FOR(e, nF * N) {
            const int a = e / N, j = e % N;
            double s = force(a, j);
            for (int b = 0; b < nF; b++) s = fma(-Wff(a, b), X[b * N + j], s);
            G[e] = s;
        }
        TG_SYNC();
    };
    unbalanced();
    // Z' G into the work area [nm][N]; L L' solved in place, one lane per column; X += Z (.)
    if (go) TG_FOR(e, nm * N) {
        const int i = e / N, j = e % N;
        double s = 0.0;
        for (int a = 0; a < nF; a++) s = fma(Zc(a, i), G[a * N + j], s);
        Tw[e] = s;
    }
    TG_SYNC();
    if (go) TG_FOR(j, N) {
        for (int i = 0; i < nm; i++) {
            double s = Tw[i * N + j];
            for (int k = 0; k < i; k++) s = fma(-Kr[i * jl + k], Tw[k * N + j], s);
            Tw[i * N + j] = s / Kr[i * jl + i];
        }
        for (int i = nm - 1; i >= 0; i--) {
            double s = Tw[i * N + j];
            for (int k = i + 1; k < nm; k++) s = fma(-Kr[k * jl + i], Tw[k * N + j], s);
            Tw[i * N + j] = s / Kr[i * jl + i];
        }
    }
    TG_SYNC();
    if (go) TG_FOR(e, nF * N) {
        const int a = e / N, j = e % N;
        double s = X[e];
        for (int i = 0; i < nm; i++) s = fma(Zc(a, i), Tw[i * N + j], s);
        X[e] = s;
    }
    TG_SYNC();
    unbalanced();
    // y = Pp G into the work area [nc][N] (row c belongs to constraint perm[c]); the defect into Pp's place once Pp is read
    if (go) TG_FOR(e, nc * N) {
        const int c = e / N, j = e % N;
        double s = 0.0;
        for (int a = 0; a < nF; a++) s = fma(Pp[c * nF + a], G[a * N + j], s);
        Tw[e] = s;
    }
    TG_SYNC();
    if (go) TG_FOR(e, nc * nD) {
        const int c = e / nD, j = e % nD;
        double s = dh(c, J.drive[j]);
        for (int a = 0; a < nF; a++) s = fma(dh(c, fl[a]), X[a * N + j], s);
        Pp[e] = s;
    }
    TG_SYNC();
    double defect = 0.0;
    if (go) {
        for (int e = 0; e < nF * N; e++) if (!(fabs(X[e]) <= DBL_MAX)) { go = false; break; }
        for (int e = 0; e < nc * N; e++) if (!(fabs(Tw[e]) <= DBL_MAX)) { go = false; break; }
        for (int e = 0; e < nc * nD; e++) { const double v = fabs(Pp[e]); if (v > defect) defect = v; if (v != v) go = false; }
    }
    if (live) {
        double *odq = J.dq + t * (size_t)nD * nq, *odm = J.dmu + t * (size_t)nD * nc;
        TG_FOR(e, nD * nq) {
            const int j = e / nq, k = e % nq, a = idx[k];
            odq[e] = !go ? 0.0 : (a >= 0 ? X[a * N + j] : (k == J.drive[j] ? 1.0 : 0.0));
        }
        TG_FOR(e, nD * nc) {
            const int j = e / nc, c = e % nc;
            odm[(size_t)j * nc + perm[c]] = go ? Tw[c * N + j] : 0.0;
        }
        if (loads) {
            double *oc = J.compliance + t * (size_t)nq * nq, *orc = J.reaction + t * (size_t)nq * nc;
            TG_FOR(e, nq * nq) {
                const int a = idx[e / nq], b = idx[e % nq];
                oc[e] = go && a >= 0 && b >= 0 ? X[a * N + nD + b] : 0.0;
            }
            TG_FOR(e, nq * nc) {
                const int k = e / nc, c = e % nc, a = idx[k];
                orc[(size_t)k * nc + perm[c]] = go && a >= 0 ? Tw[c * N + nD + a] : 0.0;
            }
        }
        if (J.mu) TG_FOR(c, nc) J.mu[t * nc + c] = go ? S[P.o_lam + c] : 0.0;
        if (lane == 0) {
            if (J.residual) J.residual[t] = go ? residual : 0.0;
            if (J.defect) J.defect[t] = go ? defect : 0.0;
            if (J.rank) J.rank[t] = go ? r : 0;
            A.iters[t] = 0;
            A.status[t] = go ? TG_OK : TG_SINGULAR;
        }
    }
}

}  // namespace tg
