// lsq_solve.hpp -- rank-revealing least squares in LDS: column-pivoted Householder QR with a minimum-norm completion.
//
// The solve stage of the _lsq kernels (mvi_dyn_inverse.hpp, mvi_inverse.hpp; tests/min_norm_reference.py is the specification).
// A team holds a row block W [R][ld], ld >= n + 1, in LDS: columns 0 .. n - 1 the matrix, column n the right-hand side c.  Answer:
// z = argmin |c - W z|, of minimum |z| among the minimisers (numpy.linalg.lstsq's), and the rank r.
//   Stage one, W P = Q [R11 R12; 0 0] (Businger-Golub).  At step k the squared norms of the trailing columns, rows k .. R - 1, are
//   summed from scratch (no downdate, so no cancellation to guard) and team_argmax picks the largest; of equal norms the column of
//   the SMALLER index wins (lanes.hpp: the first maximum, as a serial scan finds it -- a duplicated column keeps its first copy).
//   nrm0 is the first pivot's norm; the factorisation stops with r = k when the pivot norm is zero or <= rcond nrm0.  A column norm
//   that is not a number or not finite is NOT a norm below the cut: it is taken for the largest, and the team that meets one, in
//   either stage, stops with ok == false (step 0 sums every entry of the matrix, so any such entry is met there).
//   Otherwise the pivot column is swapped in (perm records it), the reflector H = I - tau v v', v_k = 1, is formed in place and
//   applied to the trailing columns and to c, and the column is cleared below its diagonal.
//   r == n: back-substitution R11 z_p = (Q'c)[:n].
//   r < n (every n > R problem among them): the n x r transpose of the trapezoid [R11 R12] is factored by r more reflections without
//   pivoting (the same routine, strides exchanged; the triangle is well conditioned after stage one): [R11 R12] = [U' 0] Q2'.  U'
//   lands in the lower triangle of W, the reflectors in the rows to the right of it.  U' y = (Q'c)[:r] forwards, z_p = Q2 (y; 0).
//   z[perm[j]] = z_p[j].  I + W'W is never formed.
// Every dot product and update is one lane's, over the rows in ascending order (one lane per column): a problem's bits do not depend
// on the team's neighbours in the wavefront, nor on TEAM (the order of every sum and the tie rule are the same at every team size).
// Control flow is wave-uniform: teams of a wavefront differ in rank, so every loop runs min(R, n) trips (R and n are the launch's) under
// a per-team predicate, as gauss_jordan carries `go`; no TG_SYNC sits behind a team-dependent branch or trip count.
// Rank 0 (W == 0): z = 0, ok.  ok == false when a column norm, an entry of c or the answer is not finite, and for nothing else (z is
// then left as computed: the caller zeroes its outputs and the rank).
// Range: the norms are plain sums of squares, not scaled.  Entries whose squares leave the range of a double are outside the
// solver's: a matrix of scale 1e-160 and below counts as zero (rank 0, z = 0, ok) and one of scale 1e154 and above overflows
// (ok == false).  Between about 1e-140 and 1e140 -- forces, Jacobians and sqrt(ridge) in any unit system are well inside -- nothing is lost.
// Scratch beside W: perm [n] ints, nrm [n] (the column norms of the current step, then z_p), z [n] (the answer), tau2 [n] (the scalars
// of the second stage's reflectors; those of the first are consumed within their step).
// Compiled by hipcc for TEAM = 1, 4, 16, 64 and, with TEAM = 1, by g++ for the CPU tests (tests/emu_lsq).
#pragma once
#include <cfloat>
#include <cmath>

#include "lanes.hpp"

namespace tg {

// doubles of scratch lsq_solve needs beside the block W [R][n + 1]
TG_HD int lsq_scratch_doubles(int n) { return 4 * n; }

// Householder QR of M (i, j) = X[i rs + j cs], rows x cols, `extra` more columns behind it transformed along.  `steps` reflections at
// the most (this team's), `trips` loop trips (the wavefront's).  PIVOT: column pivoting with the rcond stop, columns cleared below
// the diagonal; otherwise the reflectors stay below the diagonal (v_k = 1 implied) and their scalars go to tau.  Returns the number
// of reflections made; bad is set (never cleared) when a column norm is not finite.  The caller fences before and after.
template <int TEAM, bool PIVOT>
TG_HD int lsq_factor(bool on, double *X, int rs, int cs, int rows, int cols, int extra, int steps, int trips, double rcond, int *perm,
                     double *nrm2, double *tau, int lane, bool &bad) {
    int rank = 0;
    bool go = on;
    double nrm0 = 0.0;
    for (int k = 0; k < trips; k++) {
        go = go && k < steps;
        double best = -1.0;
        int piv = k;
        if (go) for (int j = k + lane; j < (PIVOT ? cols : k + 1); j += TEAM) {
            double s = 0.0;
            for (int i = k; i < rows; i++) { const double a = X[i * rs + j * cs]; s = fma(a, a, s); }
            if (!(s <= DBL_MAX)) s = INFINITY;      // (not a number, or overflowed: the largest of all, so that the arg-max shows it to the team)
            if (PIVOT) nrm2[j] = s;
            if (s > best) { best = s; piv = j; }
        }
        team_argmax<TEAM>(best, piv);
        if (go && !(best <= DBL_MAX)) { bad = true; go = false; }      // (team-uniform: every lane holds the team's maximum)
        const double nrm = sqrt(best);      // (not a number in a team that is not going)
        if (k == 0) nrm0 = nrm;
        if (go && !(nrm > 0.0 && nrm > rcond * nrm0)) go = false;
        if (go) rank = k + 1;
        if (PIVOT) {
            if (go && piv != k) {
                for (int i = lane; i < rows; i += TEAM) { const double t = X[i * rs + k * cs]; X[i * rs + k * cs] = X[i * rs + piv * cs]; X[i * rs + piv * cs] = t; }
                if (lane == 0) { const int t = perm[k]; perm[k] = perm[piv]; perm[piv] = t; }
            }
            TG_SYNC();
        }
        // the reflector: beta = -sign(alpha) |x|, tau = (beta - alpha) / beta, v = x / (alpha - beta) below the diagonal (every lane
        // forms the scalars from the same words; nobody writes M (k, k) in this phase)
        double t = 0.0, beta = 0.0;
        if (go) {
            const double alpha = X[k * rs + k * cs];
            beta = -copysign(nrm, alpha);
            t = (beta - alpha) / beta;
            const double sc = 1.0 / (alpha - beta);
            for (int i = k + 1 + lane; i < rows; i += TEAM) X[i * rs + k * cs] *= sc;
        }
        TG_SYNC();
        if (go) {
            for (int j = k + 1 + lane; j < cols + extra; j += TEAM) {
                double dot = X[k * rs + j * cs];
                for (int i = k + 1; i < rows; i++) dot = fma(X[i * rs + k * cs], X[i * rs + j * cs], dot);
                const double w = t * dot;
                X[k * rs + j * cs] -= w;
                // rows four at a time, all loads issued before the first store: the compiler must assume that a store may alias
                // the next load, so load-store-load-store would pay the full LDS latency per row (as in gauss_jordan)
                int i = k + 1;
                for (; i + 3 < rows; i += 4) {
                    const double v0 = X[i * rs + k * cs], v1 = X[(i + 1) * rs + k * cs], v2 = X[(i + 2) * rs + k * cs], v3 = X[(i + 3) * rs + k * cs];
                    const double a0 = X[i * rs + j * cs], a1 = X[(i + 1) * rs + j * cs], a2 = X[(i + 2) * rs + j * cs], a3 = X[(i + 3) * rs + j * cs];
                    X[i * rs + j * cs] = fma(-w, v0, a0); X[(i + 1) * rs + j * cs] = fma(-w, v1, a1);
                    X[(i + 2) * rs + j * cs] = fma(-w, v2, a2); X[(i + 3) * rs + j * cs] = fma(-w, v3, a3);
                }
                for (; i < rows; i++) X[i * rs + j * cs] = fma(-w, X[i * rs + k * cs], X[i * rs + j * cs]);
            }
            if (lane == 0) { X[k * rs + k * cs] = beta; if (!PIVOT) tau[k] = t; }
        }
        TG_SYNC();
        // (no fence behind this: until the next one nobody reads or writes column k below its diagonal)
        if (PIVOT && go) for (int i = k + 1 + lane; i < rows; i += TEAM) X[i * rs + k * cs] = 0.0;
    }
    return rank;
}

// The solve described at the head of the file.  on: this team has a problem (an idle team still takes part in every TG_SYNC).
// Returns the rank; z [n] holds the answer, ok whether it is finite.  W, perm, nrm and tau2 are left as the factorisation left them.
// n is THIS TEAM's column count (0 is allowed: rank 0, nothing written), n_trips >= n the launch's, which alone sets the trip count of
// every loop with a fence in it (bvls_solve.hpp: the free set's size is a team's own); -1: n, the _lsq kernels' case.
template <int TEAM>
TG_HD int lsq_solve(bool on, double *W, int R, int n, int ld, double rcond, int *perm, double *nrm, double *z, double *tau2, int lane, bool &ok,
                    int n_trips = -1) {
    if (n_trips < 0) n_trips = n;
    const int trips = R < n_trips ? R : n_trips, own = R < n ? R : n;
    if (on) for (int j = lane; j < n; j += TEAM) perm[j] = j;
    bool bad = false;
    if (on) for (int i = 0; i < R; i++) if (!(fabs(W[i * ld + n]) <= DBL_MAX)) bad = true;      // (every lane scans the same words: team-uniform)
    TG_SYNC();
    const int r = lsq_factor<TEAM, true>(on, W, ld, 1, R, n, 1, own, trips, rcond, perm, nrm, nullptr, lane, bad);
    TG_SYNC();
    const bool deficient = on && r < n;
    const int r2 = lsq_factor<TEAM, false>(deficient, W, 1, ld, n, r, 0, r, trips, 0.0, nullptr, nullptr, tau2, lane, bad);
    // the triangle: R11 z_p = c backwards (r == n), U' y = c forwards (r < n; U' is the lower triangle of W).  c_j stays undivided:
    // whoever needs y_j divides for themselves, and nobody writes c_j in the phase that reads it
    for (int s = 0; s < trips; s++) {
        if (on && s < r) {
            const int j = deficient ? s : r - 1 - s;
            const double y = W[j * ld + n] / W[j * ld + j];
            if (deficient) for (int i = j + 1 + lane; i < r; i += TEAM) W[i * ld + n] = fma(-W[i * ld + j], y, W[i * ld + n]);
            else for (int i = lane; i < j; i += TEAM) W[i * ld + n] = fma(-W[i * ld + j], y, W[i * ld + n]);
        }
        TG_SYNC();
    }
    double *zp = deficient ? nrm : z;      // (r == n: z_p is unpermuted straight away)
    if (on) for (int j = lane; j < n; j += TEAM) {
        const double y = j < r ? W[j * ld + n] / W[j * ld + j] : 0.0;
        if (deficient) zp[j] = y; else zp[perm[j]] = y;
    }
    TG_SYNC();
    // z_p = Q2 (y; 0) = H_0 (H_1 (... H_{r-1} (y; 0))): every lane sums the same dot product, then the lanes share the update
    for (int s = 0; s < trips; s++) {
        const int k = r - 1 - s;
        const bool act = deficient && k >= 0;
        double w = 0.0;
        if (act) {
            double dot = zp[k];
            for (int i = k + 1; i < n; i++) dot = fma(W[k * ld + i], zp[i], dot);
            w = tau2[k] * dot;
        }
        TG_SYNC();
        if (act) for (int i = k + lane; i < n; i += TEAM) zp[i] = i == k ? zp[i] - w : fma(-w, W[k * ld + i], zp[i]);
        TG_SYNC();
    }
    if (deficient) for (int j = lane; j < n; j += TEAM) z[perm[j]] = zp[j];
    TG_SYNC();
    ok = !bad && !(deficient && r2 != r);
    if (on) for (int j = 0; j < n; j++) if (!(fabs(z[j]) <= DBL_MAX)) ok = false;      // (every lane scans the same words: team-uniform)
    return r;
}

}  // namespace tg
