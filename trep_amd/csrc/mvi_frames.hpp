// mvi_frames.hpp -- MODE_FRAMES: batched frame kinematics, one team per state (tg_batch_frame_kinematics).
//
// Given configurations Q [B][n_states][nq] (and rates dQ), for every selected frame F of every state: the world pose g_F = (R_F | p_F),
// the body velocity, and the Jacobians of the position and of the body velocity with respect to every config (reference frame.py:
// g(), vb(), p_dq(), vb_ddq(); tests/frame_kinematics_reference.py is the specification).  With K the frame config k drives, a_k the
// world direction of K's joint axis (column x / y / z of R_K) and o_k = p_K, the world-frame twist column of k at F is
//   (a_k x (p_F - o_k), a_k) for a rotary k on F's path,   (a_k, 0) for a prismatic one,   0 off the path   (DESIGN.md 3.1),
// and   JP_k = its linear part,   JB_k = (R_F' JP_k, R_F' a_k),   VB = sum_k JB_k dq_k = R_F' (sum_k column_k dq_k), k ascending.
// Per team: q (and dq) of its row into the rollout slice, Core::pose_sweep for the world poses of all joints, then the selected frames
// in passes of kFramePass: g_F = G[anchor] * offset (offset alone for a frame with no variable ancestor) staged in LDS and stored,
// the world twist sum_k column_k dq_k staged and rotated into VB, then one item per OUTPUT ENTRY of JP and of JB -- consecutive lanes
// store consecutive addresses, and every entry of a requested output is written, zeros included.
// The frame table (FrameArgs::tab, ::off) is made on the host from the program's anchor / offset of every frame and the joint tree:
// per selected frame 12 * its anchor joint (or -1), the number of path configs, one word per config: -1 off the path, else
// 12 * joint | axis << 16 | rotary << 18, and the path as a list in ascending config order, word | config << 19: what the velocity
// sum walks, one independent load per term.
//
// No team reads what another writes: a state's answer does not depend on B, n_states or the team's neighbours in the wavefront.
// LDS of a team: the rollout slice and behind it kFramePass poses [12] and world twists [6], whatever the number of selected frames.
// Kinematics know no masses, forces or step sizes: one kernel for every batch, no parameter twin.
// Compiled by hipcc (trepamd_frames.hip: k_frames) and, with TEAM = 1, by g++ for the CPU tests (tests/emu_frames).
#pragma once
#include <algorithm>
#include <vector>

#include "mvi_core.hpp"

namespace tg {

constexpr int MODE_FRAMES = 12;
constexpr int kFramePass = 8;      // frames staged per pass (16: 6 % off the all-frames case on the puppet, not taken)

// passed beside RunArgs (whose layout stays), as InverseArgs is; RunArgs supplies batch = B
struct FrameArgs {
    const double *Q, *dQ;        // row (b, m) at Q + (b n_states + m) q_stride, dQ likewise with dq_stride; dQ may be null
    double *G, *VB, *JP, *JB;    // [B][n_states][F][12], [..][F][6], [..][F][nq][3], [..][F][nq][6]; each may be null
    const int *tab;              // [F][2 + 2 nq] frame table: anchor word, path length, path word of every config, the path as a list
    const double *off;           // [F][12] constant transform from the anchor joint
    size_t q_stride, dq_stride;  // doubles between consecutive rows
    int n_states, n_frames;
    int o_g, o_w;                // LDS offsets (doubles) behind the rollout slice
    int lds_per_team;            // doubles per team: what the kernel strides its teams by
};

// the scratch layout of one team (host; the same numbers for the device launch and the emulation)
inline void frames_layout(int rollout_lds_per_team, FrameArgs &J) {
    int off = (rollout_lds_per_team + 1) & ~1;
    J.o_g = off; off += 12 * kFramePass;
    J.o_w = off; off += 6 * kFramePass;
    J.lds_per_team = (off + 1) & ~1;
}

// The frame table of a selection (host), from the host program (schedule.hpp, HostProgram: a template parameter here because the
// kernel translation unit sees DevProg alone): anchor word and offset of every selected frame of the descriptor's frame list, and
// the path words of the joints from its anchor up to the world.  The indices must lie inside the system.  (The words hold 12 * joint
// in 16 bits and a config in 12: a system whose joint poses fit the LDS at all -- 12 doubles per joint -- has under 1707 of either.)
template <class HOSTPROG>
inline void frames_table(const HOSTPROG &H, int n_frames, const int32_t *frames, std::vector<int> &tab, std::vector<double> &off) {
    const size_t nq = (size_t)H.p.nq, tw = 2 + 2 * nq;
    tab.assign((size_t)n_frames * tw, -1);
    off.resize(12 * (size_t)n_frames);
    for (int s = 0; s < n_frames; s++) {
        const int f = frames[s], a = H.frame_anchor[f];
        tab[s * tw] = a < 0 ? -1 : 12 * a;
        std::copy_n(&H.frame_offset[12 * (size_t)f], 12, &off[12 * (size_t)s]);
        for (int j = a; j >= 0; j = H.j_parent[j]) {
            const int kind = H.j_kind[j], rotary = kind >= TG_RX ? 1 : 0;
            tab[s * tw + 2 + H.j_cfg[j]] = (12 * j) | ((kind - (rotary ? TG_RX : TG_TX)) << 16) | (rotary << 18);
        }
        int n_path = 0;
        for (size_t k = 0; k < nq; k++) if (tab[s * tw + 2 + k] >= 0) tab[s * tw + 2 + nq + n_path++] = tab[s * tw + 2 + k] | ((int)k << 19);
        tab[s * tw + 1] = n_path;
    }
}

// entry c of the world-frame twist column (v [3], omega [3]) of a path config at a frame: wd its path word, G the joint poses, gf the frame's pose
TG_HD double frame_twist_entry(int wd, const double *G, const double *gf, int c) {
    const double *gk = G + (wd & 0xFFFF);
    const int ax = (wd >> 16) & 3;
    const bool rotary = (wd >> 18) & 1;
    if (c >= 3) return rotary ? gk[4 * (c - 3) + ax] : 0.0;
    if (!rotary) return gk[4 * c + ax];
    const int c1 = c == 2 ? 0 : c + 1, c2 = c == 0 ? 2 : c - 1;
    return gk[4 * c1 + ax] * (gf[4 * c2 + 3] - gk[4 * c2 + 3]) - gk[4 * c2 + ax] * (gf[4 * c1 + 3] - gk[4 * c1 + 3]);
}

// team index i = b * n_states + m; i >= batch * n_states: an idle team, which still takes part in every TG_SYNC
template <int TEAM, class PROG, class ARGS>
TG_HD void run_frames(PROG &P, ARGS &A, const FrameArgs &J, double *S, int lane, long long team_index) {
    const int nq = P.nq, F = J.n_frames, tw = 2 + 2 * nq;
    const bool live = team_index < (long long)A.batch * J.n_states;
    const size_t i = (size_t)(live ? team_index : 0);
    Core<TEAM, false, PROG, double, false> core(P, S, lane, 1.0);
    core.init_sweep_schedule(false);
    if (live) TG_FOR(c, nq) {
        const double v = J.Q[i * J.q_stride + c];
        S[P.o_q1 + c] = v; S[P.o_q2 + c] = v;
        S[P.o_dq + c] = J.dQ ? J.dQ[i * J.dq_stride + c] : 0.0;
    }
    TG_SYNC();
    core.pose_sweep(live, 2);
    const double *G = S + P.o_G, *dq = S + P.o_dq;
    double *g = S + J.o_g, *w = S + J.o_w;

    for (int f0 = 0; f0 < F; f0 += kFramePass) {      // (F is the launch's: every team makes the same passes)
        const int nf = F - f0 < kFramePass ? F - f0 : kFramePass;
        const size_t at = i * (size_t)F + f0;      // the pass's first frame in the outputs
        // ---- poses of the pass's frames ----------------------------------------------------------------------------------------
        if (live) TG_FOR(e, 12 * nf) {
            const int fl = e / 12, r = (e % 12) >> 2, c = e & 3;
            const int oa = J.tab[(size_t)(f0 + fl) * tw];
            const double *o = J.off + 12 * (size_t)(f0 + fl);
            double v = o[4 * r + c];
            if (oa >= 0) {
                const double *ga = G + oa + 4 * r;
                v = ga[0] * o[c] + ga[1] * o[4 + c] + ga[2] * o[8 + c];
                if (c == 3) v += ga[3];
            }
            g[e] = v;
            if (J.G) J.G[at * 12 + e] = v;
        }
        TG_SYNC();
        // ---- body velocities: the world twist sum_k column_k dq_k, then R_F' of its two halves ------------------------------------
        if (J.VB) {
            if (live) TG_FOR(e, 6 * nf) {
                const int fl = e / 6, c = e % 6;
                const int *row = J.tab + (size_t)(f0 + fl) * tw;
                double s = 0.0;
                for (int p = 0; p < row[1]; p++) {
                    const int wk = row[2 + nq + p];
                    s += frame_twist_entry(wk & 0x7FFFF, G, g + 12 * fl, c) * dq[wk >> 19];
                }
                w[e] = s;
            }
            TG_SYNC();
            if (live) TG_FOR(e, 6 * nf) {
                const int fl = e / 6, c = e % 6, r = c % 3;
                const double *gf = g + 12 * fl, *wf = w + 6 * fl + (c - r);
                J.VB[at * 6 + e] = gf[r] * wf[0] + gf[4 + r] * wf[1] + gf[8 + r] * wf[2];
            }
        }
        // ---- the Jacobians, one item per entry -----------------------------------------------------------------------------------
        if (J.JP && live) {
            const int n3 = 3 * nq;
            TG_FOR(e, n3 * nf) {
                const int fl = e / n3, rest = e - fl * n3, k = rest / 3, c = rest - 3 * k;
                const int wd = J.tab[(size_t)(f0 + fl) * tw + 2 + k];
                J.JP[at * n3 + e] = wd >= 0 ? frame_twist_entry(wd, G, g + 12 * fl, c) : 0.0;
            }
        }
        if (J.JB && live) {
            const int n6 = 6 * nq;
            TG_FOR(e, n6 * nf) {
                const int fl = e / n6, rest = e - fl * n6, k = rest / 6, c = rest - 6 * k, r = c % 3;
                const int wd = J.tab[(size_t)(f0 + fl) * tw + 2 + k];
                double v = 0.0;
                if (wd >= 0 && (c < 3 || ((wd >> 18) & 1))) {
                    const double *gf = g + 12 * fl;
                    v = gf[r] * frame_twist_entry(wd, G, gf, c - r) + gf[4 + r] * frame_twist_entry(wd, G, gf, c - r + 1) +
                        gf[8 + r] * frame_twist_entry(wd, G, gf, c - r + 2);
                }
                J.JB[at * n6 + e] = v;
            }
        }
        TG_SYNC();      // (the next pass restages g and w)
    }
}

}  // namespace tg
