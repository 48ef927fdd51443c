// Host emulation of the frame-kinematics kernel (TEST INFRASTRUCTURE ONLY).
//
// trep_amd/csrc/mvi_frames.hpp compiled with g++ and TEAM = 1: every state of the call runs run_frames, the body of the device's
// k_frames, one after the other, with the scratch layout the device launch uses (frames_layout) and the frame table the library
// builds (frames_table).  Not part of the product.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../trep_amd/csrc/mvi_frames.hpp"

namespace {
struct Emu {
    tg::HostProgram H;
    tg::DevProg P;
};
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

// doubles of LDS per team of the frame-kinematics kernel, of the rollout slice it extends, and the frames of the system
void emu_frames_lds(void *h, int *out) {
    Emu *e = (Emu *)h;
    tg::FrameArgs J{};
    tg::frames_layout(e->P.lds_per_team, J);
    out[0] = J.lds_per_team; out[1] = e->P.lds_per_team; out[2] = (int)e->H.frame_anchor.size();
}

// anchor joint (-1: none) of every frame of the descriptor
void emu_frame_anchors(void *h, int *out) {
    Emu *e = (Emu *)h;
    std::copy(e->H.frame_anchor.begin(), e->H.frame_anchor.end(), out);
}

// Q (and dQ, or null) rows q_stride (dq_stride) doubles apart, batch * n_states of them; frames [n_frames] inside the system;
// outputs as tg_batch_frame_kinematics (any may be null).
// poison: the scratch of every team starts as NaN instead of zero (the device's LDS is not cleared either)
void emu_frames(void *h, int batch, int n_states, const double *Q, long long q_stride, const double *dQ, long long dq_stride, int n_frames,
                const int *frames, double *G, double *VB, double *JP, double *JB, int poison) {
    Emu *e = (Emu *)h;
    tg::RunArgs A{};
    A.batch = batch; A.n_steps = n_states; A.mode = tg::MODE_FRAMES; A.group_size = 1;
    tg::FrameArgs J{};
    tg::frames_layout(e->P.lds_per_team, J);
    std::vector<int> tab;
    std::vector<double> off;
    tg::frames_table(e->H, n_frames, frames, tab, off);
    J.Q = Q; J.dQ = dQ; J.G = G; J.VB = VB; J.JP = JP; J.JB = JB; J.tab = tab.data(); J.off = off.data();
    J.q_stride = (size_t)q_stride; J.dq_stride = (size_t)dq_stride; J.n_states = n_states; J.n_frames = n_frames;
    std::vector<double> lds((size_t)J.lds_per_team);
    for (long long i = 0; i < (long long)batch * n_states; i++) {
        std::fill(lds.begin(), lds.end(), poison ? NAN : 0.0);
        tg::run_frames<1>(static_cast<tg::CProg &>(e->P), A, J, lds.data(), 0, i);
    }
}
}
