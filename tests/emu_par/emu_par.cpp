// Host emulation of the per-trajectory parameter kernels (TEST INFRASTRUCTURE ONLY).
//
// The same as tests/emu/emu.cpp -- trep_amd/csrc/mvi_core.hpp compiled with g++ and TEAM = 1 -- plus a parameter table: while one
// is set (emu_set_parameters), every trajectory runs run_trajectory<..., PAR = true> on its row (mvi_core.hpp, ParTable), as the
// device's k_run_par does.  Not part of the product.
#include <algorithm>
#include <vector>

#include "../../trep_amd/csrc/mvi_core.hpp"

namespace {
struct Emu {
    tg::HostProgram H;
    tg::DevProg P;
    std::vector<double> table;   // rows of ParTable layout; empty: the default kernels
    int group = 1, stride = 0;
};

template <bool PAR> void run_all(Emu *e, const tg::RunArgs *args) {
    std::vector<double> lds((size_t)std::max(std::max(std::max(e->P.lds_per_team, e->P.d_lds_per_team), e->P.e_lds_per_team), e->P.g_lds_per_team));
    const tg::ParTable T{e->table.data(), e->group, e->stride};
    for (int t = 0; t < args->batch; t++) {
        std::fill(lds.begin(), lds.end(), 0.0);
#define EMU_RUN(M) tg::run_trajectory<1, M, true, tg::DevProg, const tg::RunArgs, -1, PAR>(e->P, *args, lds.data(), 0, t, 0, 1, T)
        switch (args->mode) {
        case tg::MODE_ROLLOUT: EMU_RUN(tg::MODE_ROLLOUT); break;
        case tg::MODE_CALC_P2: EMU_RUN(tg::MODE_CALC_P2); break;
        case tg::MODE_CALC_F: EMU_RUN(tg::MODE_CALC_F); break;
        case tg::MODE_DERIV1: EMU_RUN(tg::MODE_DERIV1); break;
        case tg::MODE_DYNAMICS: EMU_RUN(tg::MODE_DYNAMICS); break;
        case tg::MODE_DYN_DERIV1: EMU_RUN(tg::MODE_DYN_DERIV1); break;
        case tg::MODE_ENERGY: EMU_RUN(tg::MODE_ENERGY); break;
        case tg::MODE_LAGRANGIAN: EMU_RUN(tg::MODE_LAGRANGIAN); break;
        default: EMU_RUN(tg::MODE_DERIV2Z); break;
        }
#undef EMU_RUN
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

// rows x [inertia 4 n_bodies | gravity 3 | damping nd] (complete rows); rows == 0 clears
void emu_set_parameters(void *h, int rows, int group, const double *table) {
    Emu *e = (Emu *)h;
    e->stride = 4 * e->P.n_bodies + 3 + e->P.nd;
    e->group = group;
    e->table.assign(table, table + (size_t)rows * e->stride);
}

// the system's own values in one row of that layout
void emu_base_row(void *h, double *row) {
    Emu *e = (Emu *)h;
    const int nb = e->P.n_bodies;
    for (int i = 0; i < 4 * nb; i++) row[i] = e->H.b_inertia[i];
    for (int k = 0; k < 3; k++) row[4 * nb + k] = e->P.grav[k];
    for (int i = 0; i < e->P.nd; i++) row[4 * nb + 3 + i] = e->H.damp.empty() ? 0.0 : e->H.damp[i];
}

void emu_run(void *h, const tg::RunArgs *args) {
    Emu *e = (Emu *)h;
    if (e->table.empty()) run_all<false>(e, args);
    else run_all<true>(e, args);
}
}
