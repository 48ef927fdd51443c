// Host emulation of the computed-torque kernel (TEST INFRASTRUCTURE ONLY).
//
// trep_amd/csrc/mvi_dyn_inverse.hpp compiled with g++ and TEAM = 1: every (trajectory, state) of the call runs run_dyn_inverse, the body
// of the device's k_dyn_inverse, one after the other, with the scratch layout the device launch uses (dyn_inverse_layout).  Not part of
// the product.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../trep_amd/csrc/mvi_dyn_inverse.hpp"

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

// doubles of LDS per team of the computed-torque kernel, of the rollout slice it extends, and the three offsets behind it
void emu_dyn_inverse_lds(void *h, int *out) {
    Emu *e = (Emu *)h;
    tg::DynInverseArgs J{};
    tg::dyn_inverse_layout(e->P.lds_per_team, e->P.nq, e->P.nd, e->P.nu, e->P.nc, J);
    out[0] = J.lds_per_team; out[1] = e->P.lds_per_team; out[2] = J.o_kkt; out[3] = J.o_ddq; out[4] = J.o_scal;
}

// rows of Q, dQ, ddQ q_stride, dq_stride, ddq_stride doubles apart; outputs as tg_batch_dynamics_inverse (any may be null);
// rows (or null): a parameter table of `stride` doubles per row, trajectory b using row b / group (the PAR twin).
// poison: the scratch of every team starts as NaN instead of zero (the device's LDS is not cleared either)
void emu_dyn_inverse(void *h, int batch, int n_states, const double *Q, long long q_stride, const double *dQ, long long dq_stride,
                     const double *ddQ, long long ddq_stride, double ridge, double *U, double *LAM, double *RHO, double *TAU, double *ACC,
                     int *status, const double *rows, int group, int stride, int poison) {
    Emu *e = (Emu *)h;
    tg::RunArgs A{};
    A.batch = batch; A.n_steps = n_states; A.mode = tg::MODE_DYN_INVERSE; A.group_size = 1;
    tg::DynInverseArgs J{};
    tg::dyn_inverse_layout(e->P.lds_per_team, e->P.nq, e->P.nd, e->P.nu, e->P.nc, J);
    J.Q = Q; J.dQ = dQ; J.ddQ = ddQ; J.U = U; J.LAM = LAM; J.RHO = RHO; J.TAU = TAU; J.ACC = ACC; J.status = status;
    J.ridge = ridge; J.q_stride = (size_t)q_stride; J.dq_stride = (size_t)dq_stride; J.ddq_stride = (size_t)ddq_stride; J.n_states = n_states;
    const tg::ParTable T{rows, group > 0 ? group : 1, stride};
    std::vector<double> lds((size_t)J.lds_per_team);
    for (long long i = 0; i < (long long)batch * n_states; i++) {
        std::fill(lds.begin(), lds.end(), poison ? NAN : 0.0);
        if (rows) tg::run_dyn_inverse<1, true, true>(static_cast<tg::CProg &>(e->P), A, J, T, lds.data(), 0, i);
        else tg::run_dyn_inverse<1, true, false>(static_cast<tg::CProg &>(e->P), A, J, T, lds.data(), 0, i);
    }
}
}
