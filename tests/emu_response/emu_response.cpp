// Host emulation of the static-response kernel (TEST INFRASTRUCTURE ONLY).
//
// trep_amd/csrc/mvi_response.hpp compiled with g++ and TEAM = 1: every pose of the batch runs run_response, the body of the device's
// k_response, one after the other, with the scratch layout the device launch uses (response_layout).  Not part of the product.
#include <algorithm>
#include <vector>

#include "../../trep_amd/csrc/mvi_response.hpp"

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

// doubles of LDS per team of the static-response kernel, and of the rollout slice it extends
void emu_response_lds(void *h, int n_free, int n_drive, int with_compliance, int *out) {
    Emu *e = (Emu *)h;
    tg::ResponseArgs J{};
    tg::response_layout(e->P.lds_per_team, e->P.nq, e->P.nc, n_free, n_drive, with_compliance != 0, J);
    out[0] = J.lds_per_team; out[1] = e->P.lds_per_team;
}

// args: batch, iters, status; free_mask [nq] (n_free ones); drive [n_drive]; q0 [batch][nq]; mu_in [batch][nc] or null; the outputs
// of tg_batch_static_response (compliance and reaction are written with with_compliance alone); rows (or null): a parameter table, pose t using
// row t / group (the PAR twin)
void emu_response(void *h, const tg::RunArgs *args, const int *free_mask, int n_free, const int *drive, int n_drive, const double *q0, const double *mu_in,
                  double rcond, int with_compliance, double *dq, double *dmu, double *compliance, double *reaction, int *rank, double *mu, double *residual, double *defect,
                  const double *rows, int group, int stride) {
    Emu *e = (Emu *)h;
    tg::ResponseArgs J{};
    tg::response_layout(e->P.lds_per_team, e->P.nq, e->P.nc, n_free, n_drive, with_compliance != 0, J);
    J.free_mask = free_mask; J.drive = drive; J.q0 = q0; J.mu_in = mu_in; J.mu = mu; J.dq = dq; J.dmu = dmu; J.compliance = compliance;
    J.reaction = reaction; J.residual = residual; J.defect = defect; J.rank = rank; J.rcond = rcond; J.n_free = n_free; J.n_drive = n_drive; J.loads = with_compliance;
    const tg::ParTable T{rows, group > 0 ? group : 1, stride};
    std::vector<double> lds((size_t)J.lds_per_team);
    for (int t = 0; t < args->batch; t++) {
        std::fill(lds.begin(), lds.end(), 0.0);
        if (rows) tg::run_response<1, true, true>(static_cast<tg::CProg &>(e->P), *args, J, T, lds.data(), 0, t);
        else tg::run_response<1, true, false>(static_cast<tg::CProg &>(e->P), *args, J, T, lds.data(), 0, t);
    }
}
}
