// Host emulation of the tape-measure kernel (TEST INFRASTRUCTURE ONLY).
//
// trep_amd/csrc/mvi_tape.hpp compiled with g++ and TEAM = 1: every state of the call runs run_tape, the body of the device's k_tape,
// one after the other, with the scratch layout the device launch uses (tape_layout) and the table the library builds (tape_table).
// Not part of the product.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../trep_amd/csrc/mvi_tape.hpp"

namespace {
struct Emu {
    tg::HostProgram H;
    tg::DevProg P;
    // the table of the selection of the call before, kept as the library keeps it (emu_tape, reuse = 1)
    std::vector<int> start, sel;
    tg::TapeTable K;
};

bool same_selection(const Emu *e, int n_measures, const int *start, const int *frames) {
    if (e->start.size() != (size_t)n_measures + 1 || e->sel.size() != (size_t)(start[n_measures] - start[0])) return false;
    for (int t = 0; t <= n_measures; t++) if (e->start[t] != start[t] - start[0]) return false;
    return std::equal(e->sel.begin(), e->sel.end(), frames + start[0]);
}
}  // namespace

extern "C" {

void *emu_create(const tg_system_desc *d) {
    Emu *e = new Emu();
    try {
        e->H = tg::build_program(d);
    } catch (...) {
        delete e;
        return nullptr;
    }
    e->P = e->H.p;
    e->H.bind(e->P, e->H.ipool.data(), e->H.dpool.data());
    return e;
}

void emu_destroy(void *h) { delete (Emu *)h; }

// doubles of LDS per team of the tape-measure kernel for a longest measure of `longest` segments, of the rollout slice, frames of the system
void emu_tape_lds(void *h, int longest, int *out) {
    Emu *e = (Emu *)h;
    tg::TapeArgs J{};
    tg::tape_layout(e->P.lds_per_team, longest, J);
    out[0] = J.lds_per_team; out[1] = e->P.lds_per_team; out[2] = (int)e->H.frame_anchor.size();
}

// the table of a selection: out = unique end points, segments, passes, segments of the longest measure; cuts [n_measures + 1] gets the pass cuts
void emu_tape_table(void *h, int n_measures, const int *start, const int *frames, int *out, int *cuts) {
    Emu *e = (Emu *)h;
    tg::TapeTable K;
    tg::tape_table(e->H, n_measures, start, frames, K);
    out[0] = K.n_unique; out[1] = K.n_segments; out[2] = K.n_pass; out[3] = K.longest;
    std::copy_n(&K.words[K.o_cuts], K.n_pass + 1, cuts);
}

// Q (and dQ, or null) rows q_stride (dq_stride) doubles apart, batch * n_states of them; measures as tg_batch_tape_measures (checked by
// the caller); outputs likewise (any may be null).  reuse: keep the table of the call before if the selection is the same.
// poison: the scratch of every team starts as NaN instead of zero (the device's LDS is not cleared either).  Returns 1 if the table was built.
int emu_tape(void *h, int batch, int n_states, const double *Q, long long q_stride, const double *dQ, long long dq_stride, int n_measures,
             const int *start, const int *frames, double *L, double *V, double *LQ, double *VQ, double *LQQ, int reuse, int poison) {
    Emu *e = (Emu *)h;
    int built = 0;
    if (!reuse || !same_selection(e, n_measures, start, frames)) {
        tg::tape_table(e->H, n_measures, start, frames, e->K);
        e->sel.assign(frames + start[0], frames + start[n_measures]);
        e->start.clear();
        for (int t = 0; t <= n_measures; t++) e->start.push_back(start[t] - start[0]);
        built = 1;
    }
    const tg::TapeTable &K = e->K;
    tg::RunArgs A{};
    A.batch = batch; A.n_steps = n_states; A.mode = tg::MODE_TAPE; A.group_size = 1;
    tg::TapeArgs J{};
    tg::tape_layout(e->P.lds_per_team, K.longest, J);
    J.Q = Q; J.dQ = dQ; J.L = L; J.V = V; J.LQ = LQ; J.VQ = VQ; J.LQQ = LQQ;
    J.ftab = K.words.data(); J.off = K.off.data();
    J.seg = K.words.data() + K.o_seg; J.mstart = K.words.data() + K.o_mstart; J.cuts = K.words.data() + K.o_cuts;
    J.q_stride = (size_t)q_stride; J.dq_stride = (size_t)dq_stride; J.n_states = n_states; J.n_measures = n_measures; J.n_pass = K.n_pass;
    std::vector<double> lds((size_t)J.lds_per_team);
    for (long long i = 0; i < (long long)batch * n_states; i++) {
        std::fill(lds.begin(), lds.end(), poison ? NAN : 0.0);
        tg::run_tape<1>(static_cast<tg::CProg &>(e->P), A, J, lds.data(), 0, i);
    }
    return built;
}
}
