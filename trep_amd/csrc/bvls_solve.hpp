// bvls_solve.hpp -- bounded-variable least squares in LDS: an active-set loop (Stark-Parker BVLS) around lsq_solve.hpp.
//
// The solve stage of the _bounded kernels (mvi_dyn_inverse.hpp, mvi_inverse.hpp; tests/bounded_reference.py is the specification).
// A team holds a PRISTINE row block Wp [R][ld], ld = n + 1, in LDS: columns 0 .. n - 1 the matrix W, column n the right-hand side c.
// Answer: z = argmin |c - W z| subject to lo <= z <= hi (either bound may be infinite per variable), the bound state of every
// variable (-1 at lo, +1 at hi, 0 free; lo == hi reports -1), the number of least-squares solves taken and the rank of the first.
// Wp is only read: every solve destroys a WORKING copy, gathered from Wp -- the free columns in ascending index order, and behind
// them c minus the bound columns times their bounds.
//   Start: z = the point of the box nearest 0, every variable free except those with lo == hi (never freed).  With nothing bound the
//   working copy equals Wp word for word, so the first solve is lsq_solve on the problem the _lsq kernels solve: with all bounds
//   infinite the answer has their bits.  A first solve of rank < (number of free columns) at rcond means a problem that is not
//   strictly convex: BVLS_SINGULAR (use a ridge).  A free subset of a full-column-rank block has full column rank, so later solves
//   cannot fail that test; it stays on every solve as a guard.
//   Each trip: solve on the free set for the trial s.
//     s outside the box: alpha = min over the violators of (bound_j - z_j) / (s_j - z_j), in [0, 1]; z += alpha (s - z) on the free
//     set; every violator whose own ratio is <= alpha is set on its bound exactly and bound.  (The one that set alpha always is: its
//     ratio is recomputed from the same words.)  Next trip.
//     s inside: z = s.  g = W'(W z - c) from Wp.  Among the bound variables with lo < hi, those with g_j < 0 at lo or g_j > 0 at hi
//     lower the objective by leaving; the one of largest |g_j| is freed, next trip.  None: the KKT conditions hold, BVLS_OK.
//   z is feasible at all times (an update is clamped into the box against the last rounding).
// Determinism: both selections (the step's minimum ratio, as the maximum of its negative, and the largest gradient) go through
// team_argmax and its first-maximum rule; every sum is one lane's, rows or columns ascending.  A problem's bits depend neither on
// its neighbours nor on TEAM.
// Control flow: teams of a workgroup differ in the number of solves they need, and TG_SYNC is a workgroup barrier.  Every TG_SYNC
// here and in lsq_solve sits in a loop whose trip count is the launch's (max_solves, and min(R, n) inside the solver), each team
// working under its own predicate `run`; none sits behind a team-dependent branch, trip count or return.  max_solves is the cap:
// a team still running after it reports BVLS_NOT_CONVERGED with its last (feasible) iterate.  The callers pass 3 n + 3.
// Early exit (VOTE): the trip loop is left when NO lane of the workgroup has a team still running.  The vote is a wavefront ballot,
// which is workgroup-wide exactly when the workgroup is one wavefront: VOTE may be set only by kernels that carry
// __launch_bounds__(64) on this wave64 part (a launch with more threads then fails instead of running) -- all generic kernels do,
// and launch_kernel starts them with 64 threads.  The ballot's result is the same in every lane, so the break is uniform.  In a
// build with helper waves (several wavefronts per workgroup) there is no vote, and on the host the team is alone.
// Not finite: any entry of Wp that is not finite reaches the first working copy (as a free column or through c) and lsq_solve
// reports it: BVLS_SINGULAR, rank 0.  Bounds must be numbers with lo <= hi, lo < +inf, hi > -inf: the caller's duty (the host
// refuses others).
// Scratch (bvls_scratch_doubles): the working block [R][ld], lo, hi, z, g [n] each, bnd and idx [n] ints each, lsq_solve's 4 n.
// Compiled by hipcc for TEAM = 1, 4, 16, 64 and, with TEAM = 1, by g++ for the CPU tests (tests/emu_bvls).
#pragma once
#include "lanes.hpp"
#include "lsq_solve.hpp"

namespace tg {

// the values of TG_OK, TG_NOT_CONVERGED, TG_SINGULAR (trep_amd.h), which this header does not see
constexpr int BVLS_OK = 0, BVLS_NOT_CONVERGED = 1, BVLS_SINGULAR = 2;

TG_HD int bvls_max_solves(int n) { return 3 * n + 3; }

// doubles of scratch bvls_solve needs beside the pristine block Wp [R][n + 1]
TG_HD int bvls_scratch_doubles(int R, int n) { return R * (n + 1) + 5 * n + lsq_scratch_doubles(n); }

struct BvlsScratch {
    double *Wk, *lo, *hi, *z, *g, *lsq;
    int *bnd, *idx;
};
TG_HD BvlsScratch bvls_scratch(double *scr, int R, int n) {
    BvlsScratch X;
    X.Wk = scr; X.lo = X.Wk + R * (n + 1); X.hi = X.lo + n; X.z = X.hi + n; X.g = X.z + n;
    X.bnd = (int *)(X.g + n); X.idx = X.bnd + n;
    X.lsq = X.g + 2 * n;
    return X;
}

// does any lane of the workgroup say yes?  (see the head of the file for when the ballot is workgroup-wide)
TG_HD bool bvls_any(bool yes) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(TG_HELPER_WAVES)
    return __builtin_amdgcn_ballot_w64(yes) != 0ull;
#else
    return yes;
#endif
}

// The solve described at the head of the file.  on: this team has a problem (an idle team still takes part in every TG_SYNC and
// vote).  The caller has filled X.lo and X.hi (X = bvls_scratch(scr, R, n)) and fenced.  Returns the first solve's rank; X.z [n]
// holds the answer (the last feasible iterate unless status == BVLS_OK; not to be used with BVLS_SINGULAR), X.bnd [n] the bound
// states, X.g the gradient of the variables that were bound at the last test; finite is false when the solver met a number that
// is not finite (status is then BVLS_SINGULAR).  All results are team-uniform.
template <int TEAM, bool VOTE>
TG_HD int bvls_solve(bool on, const double *Wp, int R, int n, int ld, double rcond, int max_solves, double *scr, int lane, int &solves, int &status,
                     bool &finite) {
    const BvlsScratch X = bvls_scratch(scr, R, n);
    int *perm = (int *)X.lsq;
    double *nrm = X.lsq + n, *zs = X.lsq + 2 * n, *tau2 = X.lsq + 3 * n, *resid = X.Wk;
    if (on) for (int j = lane; j < n; j += TEAM) {
        const double l = X.lo[j], h = X.hi[j];
        X.z[j] = l > 0.0 ? l : (h < 0.0 ? h : 0.0);
        X.g[j] = 0.0;
        X.bnd[j] = l == h ? -1 : 0;
    }
    TG_SYNC();
    bool run = on;
    int rank0 = 0;
    solves = 0; status = BVLS_OK; finite = true;
    for (int t = 0; t < max_solves; t++) {
        // ---- the working copy: free columns ascending, c less the bound columns at their bounds (every lane scans the same words) --
        int nf = 0;
        if (run) {
            for (int j = 0; j < n; j++) if (X.bnd[j] == 0) { if (lane == 0) X.idx[nf] = j; nf++; }
            for (int i = lane; i < R; i += TEAM) {
                const double *src = Wp + i * ld;
                double *dst = X.Wk + i * ld;
                double acc = src[n];
                int k = 0;
                for (int j = 0; j < n; j++) { if (X.bnd[j] == 0) dst[k++] = src[j]; else acc = fma(-src[j], X.z[j], acc); }
                dst[k] = acc;
            }
        }
        TG_SYNC();
        bool ok = true;
        const int r = lsq_solve<TEAM>(run, X.Wk, R, nf, ld, rcond, perm, nrm, zs, tau2, lane, ok, n);
        if (run) {
            solves++;
            if (t == 0) rank0 = r;
            if (!ok) { finite = false; status = BVLS_SINGULAR; run = false; }
            else if (r < nf) { status = BVLS_SINGULAR; run = false; }
        }
        // ---- the trial against the box: the smallest step ratio among the violators (as the largest negative) ----------------------
        double best = -2.0;
        int piv = 0;
        if (run) for (int k = lane; k < nf; k += TEAM) {
            const int j = X.idx[k];
            const double sj = zs[k], zj = X.z[j];
            double a;
            if (sj < X.lo[j]) a = (X.lo[j] - zj) / (sj - zj);
            else if (sj > X.hi[j]) a = (X.hi[j] - zj) / (sj - zj);
            else continue;
            a = a > 0.0 ? (a < 1.0 ? a : 1.0) : 0.0;
            if (-a > best) { best = -a; piv = j; }
        }
        team_argmax<TEAM>(best, piv);
        const bool step = run && best > -2.0, kkt = run && !step;
        const double alpha = -best;
        if (run) for (int k = lane; k < nf; k += TEAM) {      // (lane k owns z, bnd of its variable until the fence)
            const int j = X.idx[k];
            const double sj = zs[k];
            if (!step) { X.z[j] = sj; continue; }
            const double zj = X.z[j], l = X.lo[j], h = X.hi[j];
            double a = 2.0;
            int side = 0;
            if (sj < l) { a = (l - zj) / (sj - zj); side = -1; }
            else if (sj > h) { a = (h - zj) / (sj - zj); side = 1; }
            if (side) a = a > 0.0 ? (a < 1.0 ? a : 1.0) : 0.0;
            if (side && a <= alpha) { X.z[j] = side < 0 ? l : h; X.bnd[j] = side; }
            else { const double zn = fma(alpha, sj - zj, zj); X.z[j] = zn < l ? l : (zn > h ? h : zn); }
        }
        TG_SYNC();
        // ---- a feasible trial: the residual W z - c and the gradient of the bound variables, from the pristine block ------------------
        if (kkt) for (int i = lane; i < R; i += TEAM) {
            const double *src = Wp + i * ld;
            double acc = -src[n];
            for (int j = 0; j < n; j++) acc = fma(src[j], X.z[j], acc);
            resid[i] = acc;
        }
        TG_SYNC();
        double gain = 0.0;
        int leave = -1;
        if (kkt) for (int j = lane; j < n; j += TEAM) {
            if (X.bnd[j] == 0 || !(X.lo[j] < X.hi[j])) continue;
            double gj = 0.0;
            for (int i = 0; i < R; i++) gj = fma(Wp[i * ld + j], resid[i], gj);
            X.g[j] = gj;
            const double fall = X.bnd[j] < 0 ? -gj : gj;      // > 0: the objective falls as the variable leaves its bound
            if (fall > gain) { gain = fall; leave = j; }
        }
        team_argmax<TEAM>(gain, leave);
        if (kkt) {
            if (gain > 0.0) { if (lane == 0) X.bnd[leave] = 0; }
            else run = false;      // the KKT conditions hold
        }
        TG_SYNC();
        if (VOTE && !bvls_any(run)) break;
    }
    if (run) status = BVLS_NOT_CONVERGED;
    return rank0;
}

}  // namespace tg
