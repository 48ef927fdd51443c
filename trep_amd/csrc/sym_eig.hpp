// sym_eig.hpp -- symmetric eigen-solve in LDS: cyclic Jacobi in the round-robin (Brent-Luk) parallel ordering.
//
// The solve stage of the normal-modes kernel (mvi_modes.hpp; tests/normal_modes_reference.py is the specification).  A team holds a
// symmetric matrix A [n][ld] and a vector block Y [n][ld] in LDS.  Answer: A brought to diagonal form by plane rotations, A <- J'AJ,
// Y <- Y J: with Y = I at the start the columns of Y are the eigenvectors of the eigenvalues left on the diagonal.
//   Ordering: m = n rounded up to even; a sweep has m - 1 sets of m / 2 disjoint pairs.  Set s: pair 0 is (m - 1, s), pair k >= 1 is
//   ((s + k) mod (m - 1), (s - k) mod (m - 1)); a pair is ordered p < q, and one that holds the dummy index n (odd n) is left out.
//   A set: every pair's (c, s) is formed from the CURRENT matrix -- theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| +
//   hypot(theta, 1)), c = 1 / sqrt(t t + 1), s = t c; a pair with |a_pq| <= kJacobiSkip eps scale is skipped (c = 1, s = 0), scale =
//   max |entry| at the start of the sweep -- then all row rotations (row_p, row_q) <- (c row_p - s row_q, s row_p + c row_q), then,
//   behind a fence, all column rotations of A and the same ones of Y; a rotated pair's own entries a_pq, a_qp are then set to zero.
//   Sweeps go on until max |off-diagonal| <= eps max |entry|, tested at the start of a sweep; max_sweeps at the most.
// One lane per (pair, column) item in the row phase, one per (row, pair) item in the column phase: every entry's update is one lane's,
// from two products in a fixed order, so a problem's bits depend neither on TEAM nor on the team's neighbours in the wavefront (the
// two maxima of the test are exact whatever the order they are taken in).
// Control flow is wave-uniform: the sets of a sweep are counted by n_trips (the launch's), the sweeps by max_sweeps and a vote of the
// wavefront's teams (pose_all: they leave together, a finished team idles through the phases); a team's own n and its convergence are
// predicates.  No fence sits behind a team-dependent branch.
// Leading dimension: ld = n_trips | 1, ODD.  In the column phase neighbouring lanes hold neighbouring rows i, i + 1, ... of one pair and
// read A [i][p], A [i][q]: addresses a fixed ld doubles apart.  An 8-byte LDS read takes the bank pair (a / 4) mod 64 and conflicts
// within a 32-lane half, an 8-byte write within 16 lanes modulo 32 banks: the lanes' double indices i ld must differ modulo 32
// (reads) and modulo 16 (writes), which every odd ld gives and an even one does not (ld = 16 would put all rows on one bank pair).
// In the row phase neighbouring lanes hold neighbouring columns of one row: consecutive doubles, conflict-free at any ld.
// Scratch beside A and Y: cs [n_trips + 2] doubles (sym_eig_scratch_doubles), the (c, s) of a set's pairs.
// Compiled by hipcc for TEAM = 1, 4, 16, 64 and, with TEAM = 1, by g++ for the CPU tests (tests/emu_modes).
#pragma once
#include <cfloat>
#include <cmath>

#include "lanes.hpp"

namespace tg {

constexpr double kJacobiSkip = 0.0625;      // a pair under kJacobiSkip eps scale is not rotated: well under the stopping test

TG_HD int sym_eig_ld(int n_trips) { return n_trips | 1; }
TG_HD int sym_eig_scratch_doubles(int n_trips) { return n_trips + 2; }

// the maximum over the team (exact: no rounding, so the order does not matter)
template <int TEAM>
TG_HD double team_max(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int m = TEAM / 2; m >= 1; m >>= 1) { const double o = __shfl_xor(v, m, TEAM); if (o > v) v = o; }
#endif
    return v;
}

// pair k of set s in the ordering of m (even) players; false: the pair holds the dummy index
TG_HD bool sym_eig_pair(int m, int n, int s, int k, int &p, int &q) {
    int a, b;
    if (k == 0) { a = m - 1; b = s; }
    else { a = (s + k) % (m - 1); b = (s - k + (m - 1)) % (m - 1); }
    p = a < b ? a : b; q = a < b ? b : a;
    return q < n;
}

// The solve described at the head of the file.  on: this team has a problem (an idle team still takes part in every fence and vote).
// n is THIS TEAM's order, n_trips >= n the launch's.  Returns the sweeps made; converged says whether the test was passed.
// ALL: the wavefront's vote (mvi_pose.hpp: pose_all), passed in so that this header needs lanes.hpp alone.
template <int TEAM, class ALL>
TG_HD int sym_eig_jacobi(bool on, double *A, double *Y, int n, int n_trips, int ld, int max_sweeps, double *cs, int lane, bool &converged, ALL all) {
    const int m = (n + 1) & ~1, mt = (n_trips + 1) & ~1, half = m / 2;
    int sweeps = 0;
    bool done = !on;
    converged = false;
    for (;;) {
        double off = 0.0, big = 0.0;
        if (!done) for (int e = lane; e < n * n; e += TEAM) {
            const int i = e / n, j = e % n;
            const double v = fabs(A[i * ld + j]);
            if (v > big) big = v;
            if (i != j && v > off) off = v;
        }
        off = team_max<TEAM>(off); big = team_max<TEAM>(big);
        if (!done) {
            if (off <= DBL_EPSILON * big) { done = true; converged = true; }
            else if (sweeps >= max_sweeps) done = true;
        }
        if (all(done)) break;
        if (!done) sweeps++;
        const double cut = kJacobiSkip * DBL_EPSILON * big;
        for (int s = 0; s < mt - 1; s++) {
            const bool act = !done && s < m - 1;
            if (act) for (int k = lane; k < half; k += TEAM) {
                int p, q;
                double c = 1.0, sn = 0.0;
                if (sym_eig_pair(m, n, s, k, p, q)) {
                    const double apq = A[p * ld + q];
                    if (fabs(apq) > cut) {
                        const double theta = (A[q * ld + q] - A[p * ld + p]) / (2.0 * apq);
                        const double t = copysign(1.0, theta) / (fabs(theta) + hypot(theta, 1.0));
                        c = 1.0 / sqrt(fma(t, t, 1.0));
                        sn = t * c;
                    }
                }
                cs[2 * k] = c; cs[2 * k + 1] = sn;
            }
            TG_SYNC();
            if (act) for (int e = lane; e < half * n; e += TEAM) {
                const int k = e / n, j = e % n;
                int p, q;
                if (!sym_eig_pair(m, n, s, k, p, q)) continue;
                const double c = cs[2 * k], sn = cs[2 * k + 1], x = A[p * ld + j], y = A[q * ld + j];
                A[p * ld + j] = c * x - sn * y;
                A[q * ld + j] = sn * x + c * y;
            }
            TG_SYNC();
            if (act) for (int e = lane; e < half * n; e += TEAM) {
                const int k = e / n, i = e % n;
                int p, q;
                if (!sym_eig_pair(m, n, s, k, p, q)) continue;
                const double c = cs[2 * k], sn = cs[2 * k + 1];
                const double x = A[i * ld + p], y = A[i * ld + q];
                // (the pair's own entry is set to the zero the rotation was made for: its computed value is rounding noise of the order
                // of eps scale, which the stopping test would otherwise meet again in every sweep)
                A[i * ld + p] = (i == q && sn != 0.0) ? 0.0 : c * x - sn * y;
                A[i * ld + q] = (i == p && sn != 0.0) ? 0.0 : sn * x + c * y;
                const double u = Y[i * ld + p], v = Y[i * ld + q];
                Y[i * ld + p] = c * u - sn * v;
                Y[i * ld + q] = sn * u + c * v;
            }
            TG_SYNC();
        }
    }
    return sweeps;
}

}  // namespace tg
