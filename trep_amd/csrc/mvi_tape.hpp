// mvi_tape.hpp -- MODE_TAPE: batched tape measures, one team per state (tg_batch_tape_measures).
//
// A tape measure is the length of the broken line through the origins of a list of frames (reference tapemeasure.py,
// _trep/tapemeasure.c; the host class trep_amd.TapeMeasure is the specification).  Given Q [B][n_states][nq] (and rates dQ), for every
// selected measure of every state: its length L, its rate V, the gradients LQ = dL/dq and VQ = dV/dq, and the Hessian LQQ.
// For a segment from frame a to frame b:  d = p_b - p_a,  l = |d|;  with JP_F[k] = dp_F/dq_k (the linear part of the twist column of
// mvi_frames.hpp) and a_j the world axis of the joint config j drives, the second derivative of a point is, for j and k both on F's
// path and j the one nearer the world (or j == k),
//   P_F[j,k] = a_j x JP_F[k]  for a rotary j,   0 for a prismatic j,   0 if either is off the path;   symmetric.
// Only the configs on exactly ONE endpoint's path move a segment (a common ancestor moves both ends rigidly): for those
//   d_k = +JP_b[k] or -JP_a[k],   d_jk = +P_b[j,k] or -P_a[j,k] (0 when j and k sit on different ends),
//   l_k = d . d_k / l,   l_jk = (d_j . d_k + d . d_jk - l_j l_k) / l,   ddot = sum_k d_k dq_k,   v = d . ddot / l,   v_k = sum_j l_jk dq_j,
// and every other derivative entry is an exact 0.0.  A measure's outputs are the sums over its segments, segments ascending, configs
// ascending within a sum.  A segment of zero length divides by zero as on the host: the measure's outputs are then not finite.
//
// Per team: q (and dq) of its row into the rollout slice and Core::pose_sweep, as run_frames does; then the selection in PASSES, each a
// run of whole measures with at most `cap` = max(kTapePass, longest measure) segments, cut on the host (no sum crosses a pass).
// Per pass the end points p_a, p_b = (G[anchor] offset) column 4, then d, 1/l, l and ddot of every segment are staged in LDS behind the
// rollout slice (kTapeStage doubles per segment); then one item per OUTPUT ENTRY, numbered as the output is laid out, so consecutive
// lanes store consecutive addresses and every entry of a requested output is written, zeros included.  Each entry recomputes its
// d_k, d_jk and l_k from the joint poses, the table words and the staged points: plain loops over at most two short paths.
//
// The table (tape_table, host; shared with the emulation) extends frames_table: the unique end-point frames with anchor word, path words
// and offset; per segment its two end-point rows, the number of exclusive configs, per config -1 or the config's path word at its end
// point | side << 19 (side 1: the end a, whose terms enter negated), and the exclusive configs as an ascending list; per measure its
// segment range; the pass cuts as measure indices.
// No team reads what another writes.  Kinematics know no masses, forces or step sizes: one kernel for every batch, no parameter twin.
// Compiled by hipcc (trepamd_tape.hip: k_tape) and, with TEAM = 1, by g++ for the CPU tests (tests/emu_tape).
#pragma once
#include <algorithm>
#include <vector>

#include "mvi_frames.hpp"

namespace tg {

constexpr int MODE_TAPE = 13;
constexpr int kTapePass = 16;      // segments a pass holds at the least (a longer measure widens it: a measure is never cut)
constexpr int kTapeStage = 14;     // staged doubles per segment: p_a [3], p_b [3], d [3], 1/l, l, ddot [3]

// passed beside RunArgs (whose layout stays), as FrameArgs is; RunArgs supplies batch = B
struct TapeArgs {
    const double *Q, *dQ;          // row (b, m) at Q + (b n_states + m) q_stride, dQ likewise with dq_stride; dQ may be null
    double *L, *V, *LQ, *VQ, *LQQ; // [B][n_states][T], [..][T], [..][T][nq], [..][T][nq], [..][T][nq][nq]; each may be null
    const int *ftab;               // [U][2 + 2 nq] frame table of the unique end points (frames_table)
    const double *off;             // [U][12] their constant transforms from the anchor joint
    const int *seg;                // [S][3 + 2 nq] row of a, row of b, exclusive configs, word per config, the exclusive configs as a list
    const int *mstart;             // [T + 1] segment range of every measure
    const int *cuts;               // [n_pass + 1] measure range of every pass
    size_t q_stride, dq_stride;    // doubles between consecutive rows
    int n_states, n_measures, n_pass;
    int o_stage;                   // LDS offset (doubles) behind the rollout slice
    int lds_per_team;              // doubles per team: what the kernel strides its teams by
};

// segments a pass is sized for, given the longest measure of the selection
inline int tape_pass_capacity(int longest_measure_segments) { return std::max(kTapePass, longest_measure_segments); }

// the scratch layout of one team (host; the same numbers for the device launch and the emulation)
inline void tape_layout(int rollout_lds_per_team, int longest_measure_segments, TapeArgs &J) {
    int off = (rollout_lds_per_team + 1) & ~1;
    J.o_stage = off; off += kTapeStage * tape_pass_capacity(longest_measure_segments);
    J.lds_per_team = (off + 1) & ~1;
}

// the table of a selection, as one block of words (offsets into it) and the offsets' doubles
struct TapeTable {
    std::vector<int> words;
    std::vector<double> off;
    int o_seg = 0, o_mstart = 0, o_cuts = 0;      // where seg, mstart and cuts begin in words (ftab begins at 0)
    int n_unique = 0, n_segments = 0, n_pass = 0, longest = 0;
};

// The table of a selection (host): measure t is frames[measure_start[t] .. measure_start[t + 1]), at least two of them, consecutive
// ones different, all inside the system (the callers check).
template <class HOSTPROG>
inline void tape_table(const HOSTPROG &H, int n_measures, const int32_t *measure_start, const int32_t *frames, TapeTable &K) {
    const int nq = H.p.nq, tw = 2 + 2 * nq, sw = 3 + 2 * nq;
    std::vector<int32_t> unique;
    std::vector<int> row_of(H.frame_anchor.size(), -1);
    for (int i = measure_start[0]; i < measure_start[n_measures]; i++)
        if (row_of[frames[i]] < 0) { row_of[frames[i]] = (int)unique.size(); unique.push_back(frames[i]); }
    std::vector<int> ftab;
    frames_table(H, (int)unique.size(), unique.data(), ftab, K.off);
    std::vector<int> seg, mstart(1, 0), cuts(1, 0);
    K.longest = 0;
    for (int t = 0; t < n_measures; t++) {
        for (int i = measure_start[t]; i + 1 < measure_start[t + 1]; i++) {
            const int ra = row_of[frames[i]], rb = row_of[frames[i + 1]];
            const size_t at = seg.size();
            seg.resize(at + sw, -1);
            seg[at] = ra; seg[at + 1] = rb;
            int n = 0;
            for (int k = 0; k < nq; k++) {
                const int wa = ftab[(size_t)ra * tw + 2 + k], wb = ftab[(size_t)rb * tw + 2 + k];
                if ((wa >= 0) == (wb >= 0)) continue;      // on neither path, or a common ancestor
                seg[at + 3 + k] = wa >= 0 ? (wa | 1 << 19) : wb;
                seg[at + 3 + nq + n++] = k;
            }
            seg[at + 2] = n;
        }
        const int total = (int)(seg.size() / sw), mine = total - mstart.back();
        mstart.push_back(total);
        K.longest = std::max(K.longest, mine);
    }
    const int cap = tape_pass_capacity(K.longest);
    for (int t = 0; t < n_measures; t++)      // a pass: whole measures while their segments fit
        if (mstart[t + 1] - mstart[cuts.back()] > cap) cuts.push_back(t);
    cuts.push_back(n_measures);
    K.n_unique = (int)unique.size(); K.n_segments = mstart.back(); K.n_pass = (int)cuts.size() - 1;
    K.words = ftab;
    K.o_seg = (int)K.words.size(); K.words.insert(K.words.end(), seg.begin(), seg.end());
    K.o_mstart = (int)K.words.size(); K.words.insert(K.words.end(), mstart.begin(), mstart.end());
    K.o_cuts = (int)K.words.size(); K.words.insert(K.words.end(), cuts.begin(), cuts.end());
}

// component c of dp/dq_k of a point p [3] for the path word wd of config k: the arithmetic of frame_twist_entry(wd, G, g_F, c < 3)
TG_HD double tape_point_dq(int wd, const double *G, const double *p, int c) {
    const double *gk = G + (wd & 0xFFFF);
    const int ax = (wd >> 16) & 3;
    if (!((wd >> 18) & 1)) return gk[4 * c + ax];
    const int c1 = c == 2 ? 0 : c + 1, c2 = c == 0 ? 2 : c - 1;
    return gk[4 * c1 + ax] * (p[c2] - gk[4 * c2 + 3]) - gk[4 * c2 + ax] *(p[c1] - gk[4 * c1 + 3]);
}

// d_k [3] of a segment for the word w of an exclusive config: +JP_b[k] or -JP_a[k]; st the segment's staged block
TG_HD void tape_dk(int w, const double *G, const double *st, double *out) {
    const bool at_a = (w >> 19) & 1;
    const double *p = st + (at_a ? 0 : 3);
    for (int c = 0; c < 3; c++) { const double v = tape_point_dq(w & 0x7FFFF, G, p, c); out[c] = at_a ? -v : v; }
}

// l_jk of a segment for the words wj, wk of two of its exclusive configs (symmetric to the bit)
TG_HD double tape_ljk(int wj, int wk, const double *G, const double *st) {
    double dj[3], dk[3];
    tape_dk(wj, G, st, dj);
    tape_dk(wk, G, st, dk);
    const double *d = st + 6, inv = st[9];
    double s = dj[0] * dk[0] + dj[1] * dk[1] + dj[2] * dk[2];
    if (((wj ^ wk) >> 19 & 1) == 0) {      // both on the same end: d_jk = +-a_n x JP[f], n the one nearer the world
        const bool swap = (wk & 0xFFFF) < (wj & 0xFFFF);
        const int wn = swap ? wk : wj;
        if ((wn >> 18) & 1) {
            const double *far = swap ? dj : dk, *gn = G + (wn & 0xFFFF);
            const int ax = (wn >> 16) & 3;
            const double a0 = gn[ax], a1 = gn[4 + ax], a2 = gn[8 + ax];
            s += d[0] * (a1 * far[2] - a2 * far[1]) + d[1] * (a2 * far[0] - a0 * far[2]) + d[2] * (a0 * far[1] - a1 * far[0]);
        }
    }
    const double lj = (d[0] * dj[0] + d[1] * dj[1] + d[2] * dj[2]) * inv, lk = (d[0] * dk[0] + d[1] * dk[1] + d[2] * dk[2]) * inv;
    return (s - lj * lk) * inv;
}

// team index i = b * n_states + m; i >= batch * n_states: an idle team, which still takes part in every TG_SYNC
template <int TEAM, class PROG, class ARGS>
TG_HD void run_tape(PROG &P, ARGS &A, const TapeArgs &J, double *S, int lane, long long team_index) {
    const int nq = P.nq, T = J.n_measures, tw = 2 + 2 * nq, sw = 3 + 2 * nq;
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
    double *stage = S + J.o_stage;
    const bool rates = J.dQ && (J.V || J.VQ);

    for (int pass = 0; pass < J.n_pass; pass++) {      // (the launch's: every team makes the same passes)
        const int t0 = J.cuts[pass], nt = J.cuts[pass + 1] - t0;
        const int s0 = J.mstart[t0], ns = J.mstart[t0 + nt] - s0;
        const int *ms = J.mstart + t0;
        const size_t at = i * (size_t)T + t0;      // the pass's first measure in the outputs
        // ---- the end points of the pass's segments -----------------------------------------------------------------------------
        if (live) TG_FOR(e, 6 * ns) {
            const int sl = e / 6, c = e - 6 * sl, r = c % 3;
            const int row = J.seg[(size_t)(s0 + sl) * sw + c / 3];
            const int oa = J.ftab[(size_t)row * tw];
            const double *o = J.off + 12 * (size_t)row;
            double v = o[4 * r + 3];
            if (oa >= 0) {
                const double *ga = G + oa + 4 * r;
                v = ga[0] * o[3] + ga[1] * o[7] + ga[2] * o[11] + ga[3];
            }
            stage[kTapeStage * sl + c] = v;
        }
        TG_SYNC();
        if (live) TG_FOR(sl, ns) {
            double *st = stage + kTapeStage * sl;
            const double d0 = st[3] - st[0], d1 = st[4] - st[1], d2 = st[5] - st[2];
            const double l = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
            st[6] = d0; st[7] = d1; st[8] = d2; st[9] = 1.0 / l; st[10] = l;
        }
        TG_SYNC();
        if (rates) {
            if (live) TG_FOR(e, 3 * ns) {
                const int sl = e / 3, c = e - 3 * sl;
                const int *row = J.seg + (size_t)(s0 + sl) * sw;
                const double *st = stage + kTapeStage * sl;
                double s = 0.0;
                for (int n = 0; n < row[2]; n++) {
                    const int k = row[3 + nq + n], w = row[3 + k];
                    const double v = tape_point_dq(w & 0x7FFFF, G, st + ((w >> 19) & 1 ? 0 : 3), c) * dq[k];
                    s += (w >> 19) & 1 ? -v : v;
                }
                stage[kTapeStage * sl + 11 + c] = s;
            }
            TG_SYNC();
        }
        // ---- lengths and rates, one item per measure ---------------------------------------------------------------------------
        if (live && (J.L || J.V)) TG_FOR(tl, nt) {
            double sl_ = 0.0, sv = 0.0;
            for (int s = ms[tl] - s0; s < ms[tl + 1] - s0; s++) {
                const double *st = stage + kTapeStage * s;
                sl_ += st[10];
                if (rates) sv += (st[6] * st[11] + st[7] * st[12] + st[8] * st[13]) * st[9];
            }
            if (J.L) J.L[at + tl] = sl_;
            if (J.V) J.V[at + tl] = sv;
        }
        // ---- the gradients, one item per entry ---------------------------------------------------------------------------------
        if (live && J.LQ) TG_FOR(e, nq * nt) {
            const int tl = e / nq, k = e - tl * nq;
            double sum = 0.0;
            for (int s = ms[tl] - s0; s < ms[tl + 1] - s0; s++) {
                const int w = J.seg[(size_t)(s0 + s) * sw + 3 + k];
                if (w < 0) continue;
                const double *st = stage + kTapeStage * s;
                double dk[3];
                tape_dk(w, G, st, dk);
                sum += (st[6] * dk[0] + st[7] * dk[1] + st[8] * dk[2]) * st[9];
            }
            J.LQ[at * nq + e] = sum;
        }
        if (live && J.VQ) TG_FOR(e, nq * nt) {
            const int tl = e / nq, k = e - tl * nq;
            double sum = 0.0;
            for (int s = ms[tl] - s0; s < ms[tl + 1] - s0; s++) {
                const int *row = J.seg + (size_t)(s0 + s) * sw;
                const int w = row[3 + k];
                if (w < 0) continue;
                const double *st = stage + kTapeStage * s;
                double vk = 0.0;
                for (int n = 0; n < row[2]; n++) {
                    const int j = row[3 + nq + n];
                    vk += tape_ljk(row[3 + j], w, G, st) * dq[j];
                }
                sum += vk;
            }
            J.VQ[at * nq + e] = sum;
        }
        // ---- the Hessian, one item per entry -----------------------------------------------------------------------------------
        if (live && J.LQQ) {
            const int n2 = nq * nq;
            TG_FOR(e, n2 * nt) {
                const int tl = e / n2, rest = e - tl * n2, j = rest / nq, k = rest - j * nq;
                double sum = 0.0;
                for (int s = ms[tl] - s0; s < ms[tl + 1] - s0; s++) {
                    const int *row = J.seg + (size_t)(s0 + s) * sw;
                    const int wj = row[3 + j], wk = row[3 + k];
                    if (wj < 0 || wk < 0) continue;
                    sum += tape_ljk(wj, wk, G, stage + kTapeStage * s);
                }
                J.LQQ[at * n2 + e] = sum;
            }
        }
        TG_SYNC();      // (the next pass restages)
    }
}

}  // namespace tg
