// Host emulation of the inverse-dynamics kernel (TEST INFRASTRUCTURE ONLY).
//
// trep_amd/csrc/mvi_inverse.hpp compiled with g++ and TEAM = 1: every (trajectory, step) of the call runs run_inverse, the body of the
// device's k_inverse, one after the other, with the scratch layout the device launch uses (inverse_layout).  Not part of the product.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../trep_amd/csrc/mvi_inverse.hpp"

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

// doubles of LDS per team of the inverse-dynamics kernel, and of the rollout slice it extends
void emu_inverse_lds(void *h, int *out) {
    Emu *e = (Emu *)h;
    tg::InverseArgs J{};
    tg::inverse_layout(e->P.lds_per_team, e->P.nd, e->P.nu, e->P.nc, J);
    out[0] = J.lds_per_team; out[1] = e->P.lds_per_team;
}

// Q rows q_stride doubles apart; dt_steps [n_steps] or null (dt); p0 or null; outputs as tg_batch_inverse_dynamics (any may be null);
// rows (or null): a parameter table of `stride` doubles per row, trajectory b using row b / group (the PAR twin).
// poison: the scratch of every team starts as NaN instead of zero (the device's LDS is not cleared either)
void emu_inverse(void *h, int batch, int n_steps, double dt, const double *dt_steps, const double *Q, long long q_stride, const double *p0,
                 double ridge, double *U, double *LAM, double *Pout, double *RHO, double *Hout, int *status, const double *rows, int group,
                 int stride, int poison) {
    Emu *e = (Emu *)h;
    tg::RunArgs A{};
    A.batch = batch; A.n_steps = n_steps; A.mode = tg::MODE_INVERSE; A.group_size = 1;
    tg::InverseArgs J{};
    tg::inverse_layout(e->P.lds_per_team, e->P.nd, e->P.nu, e->P.nc, J);
    J.Q = Q; J.p0 = p0; J.dt_steps = dt_steps; J.U = U; J.LAM = LAM; J.P = Pout; J.RHO = RHO; J.H = Hout; J.status = status;
    J.dt = dt; J.ridge = ridge; J.q_stride = (size_t)q_stride; J.n_steps = n_steps;
    const tg::ParTable T{rows, group > 0 ? group : 1, stride};
    std::vector<double> lds((size_t)J.lds_per_team);
    for (long long i = 0; i < (long long)batch * n_steps; i++) {
        std::fill(lds.begin(), lds.end(), poison ? NAN : 0.0);
        if (rows) tg::run_inverse<1, true, true>(static_cast<tg::CProg &>(e->P), A, J, T, lds.data(), 0, i);
        else tg::run_inverse<1, true, false>(static_cast<tg::CProg &>(e->P), A, J, T, lds.data(), 0, i);
    }
}
}
