// mvi_pose.hpp -- the frame of the pose solvers: the constraint projection (mvi_project.hpp) and the equilibrium search (mvi_equilibrium.hpp).
//
// A pose solver puts one team on one pose and runs Newton on a KKT system over the FREE configs F (the other configs held at their
// input values), mu in the rollout slice's lambda area, the sparse Dh in its Dh2 area, its own scratch behind the rollout slice at
// offsets the host computes.  What the solvers share is here, once: the scratch regions both have (pose_layout), the free configs'
// places in the KKT image, the loading of the pose, the scatter of Dh into the image, the multipliers' curvature sum_c mu_c h_c,qq over the (constraint, a <= b) pair list, the votes of a wavefront's teams and the write-back.  Each
// solver keeps its own iteration, its own right-hand sides and its own g.
#pragma once
#include <initializer_list>

#include "mvi_core.hpp"

namespace tg {

// ProjectArgs and EquilibriumArgs each list their fields themselves, in an order of their own (the order is the kernel-argument layout,
// which the compiled kernels are sensitive to).  The frame is a template over the argument struct and reads the fields both have:
//   const int *free_mask        [nq] device, non-zero = free; null: every config
//   const double *q0            [batch][nq]
//   double *q, *mu              [batch][nq], [batch][nc] (or null)
//   int o_kkt, o_q0, o_scal, o_idx    LDS offsets (doubles) behind the rollout slice
//   int lds_per_team            doubles per team: what the kernel strides its teams by
// They are passed beside RunArgs (whose layout the host emulation mirrors), as ParTable is.  RunArgs supplies batch, tolerance,
// max_iterations, the remap fields and the iteration / status words (iters, status: the call's own, not the integrator's).

// The scratch layout of one team for a system of the given sizes (host; the same numbers for the device launch and the emulation):
// the KKT image [n][n + 1], n <= nq + nc; a solver's own regions; q0 [nq]; a solver's own regions; the solver's row scales
// [nq + nc]; the free configs' places (int [nq]).
struct PoseRegion { int *at, doubles; };
template <class POSE>
inline void pose_layout(int rollout_lds_per_team, int nq, int nc, POSE &J, std::initializer_list<PoseRegion> after_kkt = {},
                        std::initializer_list<PoseRegion> after_q0 = {}) {
    const int n = nq + nc;
    int off = (rollout_lds_per_team + 1) & ~1;
    J.o_kkt = off; off += n * (n + 1);
    for (const PoseRegion &r : after_kkt) { *r.at = off; off += r.doubles; }
    J.o_q0 = off; off += nq;
    for (const PoseRegion &r : after_q0) { *r.at = off; off += r.doubles; }
    J.o_scal = off; off += n;
    off = (off + 1) & ~1;
    J.o_idx = off; off += (nq + 1) / 2;
    J.lds_per_team = (off + 1) & ~1;
}

// a phase no team of the wavefront needs is skipped by all of them; the teams of a wavefront leave together
TG_HD bool pose_any(bool f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __any(f ? 1 : 0) != 0;
#else
    return f;
#endif
}
TG_HD bool pose_all(bool f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __all(f ? 1 : 0) != 0;
#else
    return f;
#endif
}

template <int TEAM, class PROG, class POSE>
struct PoseFrame {
    PROG &P;
    const POSE &J;
    double *const S;
    const int lane;
    const bool live;
    const size_t t;
    double *const K, *const Q0, *const scal;     // the KKT image, the input pose, the solver's row scales
    int *const idx;                              // the free configs' places in the image, -1: held

    TG_HD PoseFrame(PROG &P_, const POSE &J_, double *S_, int lane_, int traj, int batch)
        : P(P_), J(J_), S(S_), lane(lane_), live(traj < batch), t((size_t)(live ? traj : 0)), K(S_ + J_.o_kkt), Q0(S_ + J_.o_q0),
          scal(S_ + J_.o_scal), idx((int *)(S_ + J_.o_idx)) {}

    // the free configs' places in the image, in config order; nF (every lane counts: uniform)
    TG_HD int index_free() {
        const int nq = P.nq;
        int nF = 0;
        for (int k = 0; k < nq; k++) nF += (!J.free_mask || J.free_mask[k]) ? 1 : 0;
        TG_FOR(k, nq) {
            int at = 0;
            for (int j = 0; j < k; j++) at += (!J.free_mask || J.free_mask[j]) ? 1 : 0;
            idx[k] = (!J.free_mask || J.free_mask[k]) ? at : -1;
        }
        return nF;
    }
    // q = q0, mu = 0, no Dh yet; ends the phase
    TG_HD void load_pose() {
        const int nq = P.nq, nc = P.nc;
        if (live) {
            TG_FOR(i, nq) { const double v = J.q0[t * nq + i]; Q0[i] = v; S[P.o_q1 + i] = v; S[P.o_q2 + i] = v; }
            TG_FOR(c, nc) S[P.o_lam + c] = 0.0;
            TG_FOR(i, P.n_dh) S[P.o_Dh2 + i] = 0.0;
        }
        TG_SYNC();
    }
    // D and D' of the image (nF free configs, leading dimension ld) from the sparse Dh
    TG_HD void scatter_dh(int nF, int ld) {
        TG_FOR(m, P.n_dh) {
            const int c = P.dh_pack[8 * (size_t)m], k = P.dh_pack[8 * (size_t)m + 1], a = idx[k];
            const double v = S[P.o_Dh2 + m];
            if (a >= 0) { K[(nF + c) * ld + a] = v; K[a * ld + nF + c] = v; }
        }
    }
    // curvature: M [.][ldm] += sum_c mu_c h_c,qq(a, b) over the free configs (several constraints reach the same entry: LDS atomics)
    template <class CORE>
    TG_HD void add_curvature(CORE &core, double *M, int ldm) {
        for (int pp = tg_opaque(lane); pp < P.n_cpair; pp += TEAM) {
            const int *pw = P.cpair4 + 4 * (size_t)pp;
            const int c = pw[0], na = pw[1], nb = pw[2], a = idx[pw[3] & 0xFFFF], b = idx[pw[3] >> 16];
            if (a < 0 || b < 0) continue;
            const double h = S[P.o_lam + c] * core.con_d2(c, na, nb);
            lds_add(&M[b * ldm + a], h);
            if (na != nb) lds_add(&M[a * ldm + b], h);
        }
    }
    // the same over the places `at` [nq] gives the configs (-1: left out) instead of the frame's own: the identity for every config pair,
    // kinematic configs included (mvi_response.hpp)
    template <class CORE>
    TG_HD void add_curvature(CORE &core, double *M, int ldm, const int *at) {
        for (int pp = tg_opaque(lane); pp < P.n_cpair; pp += TEAM) {
            const int *pw = P.cpair4 + 4 * (size_t)pp;
            const int c = pw[0], na = pw[1], nb = pw[2], a = at[pw[3] & 0xFFFF], b = at[pw[3] >> 16];
            if (a < 0 || b < 0) continue;
            const double h = S[P.o_lam + c] * core.con_d2(c, na, nb);
            lds_add(&M[b * ldm + a], h);
            if (na != nb) lds_add(&M[a * ldm + b], h);
        }
    }
    // the answer of a live team: the pose, the multipliers, the iteration and status words
    template <class ARGS>
    TG_HD void store(ARGS &A, int iterations, int status) {
        const int nq = P.nq, nc = P.nc;
        if (live) {
            TG_FOR(i, nq) J.q[t * nq + i] = S[P.o_q2 + i];
            if (J.mu) TG_FOR(c, nc) J.mu[t * nc + c] = S[P.o_lam + c];
            if (lane == 0) { A.iters[t] = iterations; A.status[t] = status; }
        }
    }
};

}  // namespace tg
