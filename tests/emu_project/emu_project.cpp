// Host emulation of the constraint-projection kernel (TEST INFRASTRUCTURE ONLY).
//
// trep_amd/csrc/mvi_project.hpp compiled with g++ and TEAM = 1: every trajectory of the batch runs run_project, the body of the
// device's k_project, one after the other, with the scratch layout the device launch uses (project_layout).  Not part of the product.
#include <algorithm>
#include <vector>

#include "../../trep_amd/csrc/mvi_project.hpp"

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
    std::vector<double> lds((size_t)J.lds_per_team);
    for (int t = 0; t < args->batch; t++) {
        std::fill(lds.begin(), lds.end(), 0.0);
        tg::run_project<1, true>(static_cast<tg::CProg &>(e->P), *args, J, lds.data(), 0, t);
    }
}
}
