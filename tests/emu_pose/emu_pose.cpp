// Host emulation of the pose-solver kernels: constraint projection and equilibrium search (TEST INFRASTRUCTURE ONLY).
//
// trep_amd/csrc/mvi_project.hpp and mvi_equilibrium.hpp compiled with g++ and TEAM = 1: every pose of the batch runs run_project /
// run_equilibrium, the bodies of the device's k_project / k_equilibrium, one after the other, with the scratch layout the device
// launch uses (project_layout, equilibrium_layout).  Not part of the product.
#include <algorithm>
#include <vector>

#include "../../trep_amd/csrc/mvi_equilibrium.hpp"
#include "../../trep_amd/csrc/mvi_project.hpp"

namespace {
struct Emu {
    tg::HostProgram H;
    tg::DevProg P;
};

// every pose of the batch through `run`, each on a cleared LDS slice of the given size
template <class Run>
void each_pose(const tg::RunArgs *args, int lds_per_team, Run run) {
    std::vector<double> lds((size_t)lds_per_team);
    for (int t = 0; t < args->batch; t++) {
        std::fill(lds.begin(), lds.end(), 0.0);
        run(lds.data(), t);
    }
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

// sizeof(tg::RunArgs) as the kernels see it: the ctypes mirror of tests/emu_harness.py must agree
int emu_sizeof_run_args(void) { return (int)sizeof(tg::RunArgs); }

// doubles of LDS per team of the projection kernel, and of the rollout slice it extends
void emu_project_lds(void *h, int *out) {
    Emu *e = (Emu *)h;
    tg::ProjectArgs J{};
    tg::project_layout(e->P.lds_per_team, e->P.nq, e->P.nc, J);
    out[0] = J.lds_per_team; out[1] = e->P.lds_per_team;
}

// args: batch, tolerance, max_iterations, iters, status; free_mask [nq] or null; q0, dq0 (or null) [batch][nq]; q, dq, mu outputs
void emu_project(void *h, const tg::RunArgs *args, const int *free_mask, const double *q0, const double *dq0, double *q, double *dq, double *mu) {
    Emu *e = (Emu *)h;
    tg::ProjectArgs J{};
    tg::project_layout(e->P.lds_per_team, e->P.nq, e->P.nc, J);
    J.free_mask = free_mask; J.q0 = q0; J.dq0 = dq0; J.q = q; J.dq = dq; J.mu = mu;
    each_pose(args, J.lds_per_team, [&](double *lds, int t) { tg::run_project<1, true>(static_cast<tg::CProg &>(e->P), *args, J, lds, 0, t); });
}

// doubles of LDS per team of the equilibrium kernel, and of the rollout slice it extends
void emu_equilibrium_lds(void *h, int *out) {
    Emu *e = (Emu *)h;
    tg::EquilibriumArgs J{};
    tg::equilibrium_layout(e->P.lds_per_team, e->P.nq, e->P.nc, J);
    out[0] = J.lds_per_team; out[1] = e->P.lds_per_team;
}

// args: batch, tolerance, max_iterations, iters, status; free_mask [nq] or null; q0 [batch][nq]; q, mu, v outputs;
// rows (or null): a parameter table of `stride` doubles per row, pose t using row t / group (the PAR twin)
void emu_equilibrium(void *h, const tg::RunArgs *args, const int *free_mask, const double *q0, double *q, double *mu, double *v,
                     const double *rows, int group, int stride) {
    Emu *e = (Emu *)h;
    tg::EquilibriumArgs J{};
    tg::equilibrium_layout(e->P.lds_per_team, e->P.nq, e->P.nc, J);
    J.free_mask = free_mask; J.q0 = q0; J.q = q; J.mu = mu; J.v = v;
    const tg::ParTable T{rows, group > 0 ? group : 1, stride};
    each_pose(args, J.lds_per_team, [&](double *lds, int t) {
        if (rows) tg::run_equilibrium<1, true, true>(static_cast<tg::CProg &>(e->P), *args, J, T, lds, 0, t);
        else tg::run_equilibrium<1, true, false>(static_cast<tg::CProg &>(e->P), *args, J, T, lds, 0, t);
    });
}
}
