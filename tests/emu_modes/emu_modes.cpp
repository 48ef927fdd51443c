// Host emulation of the normal-modes kernel (TEST INFRASTRUCTURE ONLY).
//
// trep_amd/csrc/mvi_modes.hpp compiled with g++ and TEAM = 1: every pose of the batch runs run_modes, the body of the device's
// k_modes, one after the other, with the scratch layout the device launch uses (modes_layout).  Not part of the product.
#include <algorithm>
#include <vector>

#include "../../trep_amd/csrc/mvi_modes.hpp"

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

int emu_sizeof_run_args(void) { return (int)sizeof(tg::RunArgs); }

// doubles of LDS per team of the normal-modes kernel, and of the rollout slice it extends
void emu_modes_lds(void *h, int *out) {
    Emu *e = (Emu *)h;
    tg::ModesArgs J{};
    tg::modes_layout(e->P.lds_per_team, e->P.nq, e->P.nc, J);
    out[0] = J.lds_per_team; out[1] = e->P.lds_per_team;
}

// args: batch, iters (sweeps), status; free_mask [nq] (kinematic configs cleared, n_free ones); q0 [batch][nq]; mu_in [batch][nc] or
// null; the outputs of tg_batch_normal_modes; rows (or null): a parameter table, pose t using row t / group (the PAR twin)
void emu_modes(void *h, const tg::RunArgs *args, const int *free_mask, int n_free, const double *q0, const double *mu_in, double rcond, int max_sweeps,
               double *omega2, double *modes, int *count, int *rank, double *mu, double *residual, const double *rows, int group, int stride) {
    Emu *e = (Emu *)h;
    tg::ModesArgs J{};
    tg::modes_layout(e->P.lds_per_team, e->P.nq, e->P.nc, J);
    J.free_mask = free_mask; J.q0 = q0; J.mu_in = mu_in; J.mu = mu; J.omega2 = omega2; J.modes = modes; J.residual = residual;
    J.count = count; J.rank = rank; J.rcond = rcond; J.n_free = n_free; J.max_sweeps = max_sweeps;
    const tg::ParTable T{rows, group > 0 ? group : 1, stride};
    std::vector<double> lds((size_t)J.lds_per_team);
    for (int t = 0; t < args->batch; t++) {
        std::fill(lds.begin(), lds.end(), 0.0);
        if (rows) tg::run_modes<1, true, true>(static_cast<tg::CProg &>(e->P), *args, J, T, lds.data(), 0, t);
        else tg::run_modes<1, true, false>(static_cast<tg::CProg &>(e->P), *args, J, T, lds.data(), 0, t);
    }
}
}
