// mvi_project.hpp -- MODE_PROJECT: batched constraint projection, one team per trajectory (tg_batch_project_constraints).
//
// Per trajectory (the reference's System.satisfy_constraints, trep/system.py:158-214, as an equality-constrained least-squares
// problem):  minimise 1/2 |q - q0|^2 over the FREE configs F subject to h(q) = 0, the other configs held at their input values.
// Newton on the KKT conditions with the constraint curvature.  From q = q0, mu = 0; with D = Dh(q)[:, F] and
// g = (q - q0)_F + D' mu every iteration
//   (1) sweeps the poses and attach points at q and evaluates h and Dh (Core::eval_constraints, the rollout's own code);
//   (2) tests max |h| <= tolerance and max |g| <= tolerance (every lane scans the right-hand side: team-uniform without a vote);
//   (3) adds sum_c mu_c h_c,qq over the (constraint, a <= b) pair list (Core::con_d2, as constraint_hessian_rhs does, but over all
//       free configs) to the identity and solves  [[I + sum mu_c h_c,qq, D'], [D, 0]] (dq_F, dmu) = -(g, h)  with the pivoting
//       Gauss-Jordan solver, one right-hand side.
// Without the curvature term the iteration is a sequential linearisation: 13-26 steps on the puppet under keep_kinematic at 0.02 rad
// of noise where this one takes at most 5 (tests/test_projection_cpu.py pins the count).
// Status per trajectory: TG_OK converged; TG_NOT_CONVERGED max_iterations steps taken, q = the last iterate; TG_SINGULAR the solver
// rejected the matrix, q = the iterate before that solve.  With an empty free set or no constraint there is nothing to solve: TG_OK if
// the input passes the test, else TG_SINGULAR, q unchanged.
// Velocity part (dq0 given, converged trajectories): the nearest rates with D(q) dq = 0 and the fixed rates kept --
// [[I, D'], [D, 0]] (d, nu) = (0, -Dh(q) dq0), dq_F = dq0_F + d -- through the same matrix image and solver.
//
// LDS of a team: the rollout slice (the sweeps and the constraint evaluation work in it; mu lives in its lambda area, the sparse Dh in
// its Dh2 area) and behind it the frame's scratch alone (mvi_pose.hpp): the KKT image, q0, the solver's row scales, the free configs'
// places in the image.
// Compiled by hipcc (trepamd_project.hip: k_project) and, with TEAM = 1, by g++ for the CPU tests (tests/emu_pose).
#pragma once
#include "mvi_pose.hpp"

namespace tg {

constexpr int MODE_PROJECT = 9;

// (the fields of the frame, mvi_pose.hpp, and the rates)
struct ProjectArgs {
    const int *free_mask;        // [nq] device, non-zero = free; null: every config
    const double *q0, *dq0;      // [batch][nq]; dq0 null: no velocity part
    double *q, *dq, *mu;         // [batch][nq], [batch][nq] (null without dq0), [batch][nc] (or null)
    int o_kkt, o_q0, o_scal, o_idx;   // LDS offsets (doubles) behind the rollout slice
    int lds_per_team;            // doubles per team: what the kernel strides its teams by
};

inline void project_layout(int rollout_lds_per_team, int nq, int nc, ProjectArgs &J) { pose_layout(rollout_lds_per_team, nq, nc, J); }

template <int TEAM, bool SPRINGS, class PROG, class ARGS>
TG_HD void run_project(PROG &P, ARGS &A, const ProjectArgs &J, double *S, int lane, int traj) {
    const int nq = P.nq, nd = P.nd, nc = P.nc;
    Core<TEAM, SPRINGS, PROG, double> core(P, S, lane, 1.0);
    core.init_sweep_schedule(false);
    PoseFrame<TEAM, PROG, ProjectArgs> F(P, J, S, lane, traj, A.batch);
    const bool live = F.live;
    const size_t t = F.t;
    double *K = F.K, *Q0 = F.Q0, *scal = F.scal;
    int *idx = F.idx;
    const int nF = F.index_free(), n = nF + nc, ld = n + 1;
    F.load_pose();

    // the image without the curvature block: zeros, D and D' from the sparse Dh, the identity, the right-hand side -(g | h)
    auto assemble = [&](bool on, bool velocity) {
        if (on) TG_FOR(i, n * ld) K[i] = 0.0;
        TG_SYNC();
        if (on) {
            F.scatter_dh(nF, ld);
            TG_FOR(k, nq) { const int a = idx[k]; if (a >= 0) K[a * ld + a] = 1.0; }
        }
        TG_SYNC();
        if (on && !velocity) {
            TG_FOR(k, nq) {
                const int a = idx[k];
                if (a < 0) continue;
                double g = S[P.o_q2 + k] - Q0[k];
                for (int c = 0; c < nc; c++) g = fma(K[a * ld + nF + c], S[P.o_lam + c], g);
                K[a * ld + n] = -g;
            }
            TG_FOR(c, nc) K[(nF + c) * ld + n] = -S[P.o_f + nd + c];
        }
        if (on && velocity) TG_FOR(c, nc) {      // -Dh(q) dq0 over ALL configs: the fixed rates stay
            double r = 0.0;
            for (int k = 0; k < nq; k++) { const int m = P.dh_lookup[c * nq + k]; if (m >= 0) r = fma(S[P.o_Dh2 + m], J.dq0[t * nq + k], r); }
            K[(nF + c) * ld + n] = -r;
        }
        TG_SYNC();
    };

    int status = TG_OK, iterations = 0;
    bool done = !live;
    for (;;) {
        core.eval_constraints(!done, 2, true, S + P.o_Dh2);
        assemble(!done, false);
        if (!done) {
            bool conv = true;      // (written so that a NaN fails the test)
            for (int i = 0; i < n; i++) if (!(fabs(K[i * ld + n]) <= A.tolerance)) conv = false;
            if (conv) done = true;
            else if (nF == 0 || nc == 0) { done = true; status = TG_SINGULAR; }
            else if (iterations >= A.max_iterations) { done = true; status = TG_NOT_CONVERGED; }
        }
        if (pose_all(done)) break;       // the teams of a wavefront leave together: a finished one idles through the phases
        if (!done) F.add_curvature(core, K, ld);
        TG_SYNC();
        const bool ok = core.gauss_jordan(!done, K, n, 1, ld, scal);
        if (!done && !ok) { done = true; status = TG_SINGULAR; }
        if (!done) {
            TG_FOR(k, nq) { const int a = idx[k]; if (a >= 0) { const double v = S[P.o_q2 + k] + K[a * ld + n]; S[P.o_q1 + k] = v; S[P.o_q2 + k] = v; } }
            TG_FOR(c, nc) S[P.o_lam + c] += K[(nF + c) * ld + n];
            iterations++;
        }
        TG_SYNC();
    }
    // velocity part at the converged pose (its Dh is the last evaluation's); nothing to solve without constraints or free configs
    if (J.dq0) {
        const bool von = live && status == TG_OK && nc > 0 && nF > 0;
        assemble(von, true);
        const bool ok = core.gauss_jordan(von, K, n, 1, ld, scal);
        if (von && !ok) status = TG_SINGULAR;
        if (live) TG_FOR(k, nq) {
            const int a = idx[k];
            const double v = J.dq0[t * nq + k];
            J.dq[t * nq + k] = (von && ok && a >= 0) ? v + K[a * ld + n] : v;
        }
    }
    F.store(A, iterations, status);
}

}  // namespace tg
