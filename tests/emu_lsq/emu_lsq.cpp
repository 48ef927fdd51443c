// Host emulation of the rank-revealing least-squares solver and of the two kernels that end in it (TEST INFRASTRUCTURE ONLY).
//
// trep_amd/csrc/lsq_solve.hpp, mvi_dyn_inverse.hpp and mvi_inverse.hpp compiled with g++ and TEAM = 1: the solver alone on
// caller-supplied problems (what tg_batch_debug_lsq_solve runs on the device), and every team of a call through the LSQ
// instantiations of run_dyn_inverse / run_inverse, one after the other, with the scratch layouts the device launches use
// (dyn_inverse_lsq_layout, inverse_lsq_layout).  Not part of the product.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../trep_amd/csrc/mvi_dyn_inverse.hpp"
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

// `count` problems of one shape: A [count][rows][cols], c [count][rows]; z [count][cols], rank and status [count].
// poison: the scratch starts as NaN
void emu_lsq_solve(int count, int rows, int cols, const double *A, const double *c, double rcond, double *z, int *rank, int *status, int poison) {
    const int ld = cols + 1;
    std::vector<double> lds((size_t)rows * ld + tg::lsq_scratch_doubles(cols));
    for (int p = 0; p < count; p++) {
        std::fill(lds.begin(), lds.end(), poison ? NAN : 0.0);
        double *W = lds.data(), *scr = W + (size_t)rows * ld;
        for (int i = 0; i < rows; i++) {
            for (int j = 0; j < cols; j++) W[i * ld + j] = A[((size_t)p * rows + i) * cols + j];
            W[i * ld + cols] = c[(size_t)p * rows + i];
        }
        bool ok = true;
        const int r = tg::lsq_solve<1>(true, W, rows, cols, ld, rcond, (int *)scr, scr + cols, scr + 2 * cols, scr + 3 * cols, 0, ok);
        for (int j = 0; j < cols; j++) z[(size_t)p * cols + j] = ok ? scr[2 * cols + j] : 0.0;
        rank[p] = ok ? r : 0;
        status[p] = ok ? TG_OK : TG_SINGULAR;
    }
}

// doubles of LDS per team of the two LSQ kernels and of the layouts they replace, and the rollout slice: out[0..4] = computed torque
// LSQ, computed torque, inverse dynamics LSQ, inverse dynamics, rollout; out[5..7] the offsets o_kkt, o_ddq, o_scal of the first
void emu_lsq_lds(void *h, int *out) {
    Emu *e = (Emu *)h;
    tg::DynInverseArgs D{}, D0{};
    tg::dyn_inverse_lsq_layout(e->P.lds_per_team, e->P.nq, e->P.nd, e->P.nu, e->P.nc, D);
    tg::dyn_inverse_layout(e->P.lds_per_team, e->P.nq, e->P.nd, e->P.nu, e->P.nc, D0);
    tg::InverseArgs I{}, I0{};
    tg::inverse_lsq_layout(e->P.lds_per_team, e->P.nd, e->P.nu, e->P.nc, I);
    tg::inverse_layout(e->P.lds_per_team, e->P.nd, e->P.nu, e->P.nc, I0);
    out[0] = D.lds_per_team; out[1] = D0.lds_per_team; out[2] = I.lds_per_team; out[3] = I0.lds_per_team; out[4] = e->P.lds_per_team;
    out[5] = D.o_kkt; out[6] = D.o_ddq; out[7] = D.o_scal;
}

// as emu_dyn_inverse (tests/emu_dyn_inverse), with rcond and rank
void emu_dyn_inverse_lsq(void *h, int batch, int n_states, const double *Q, long long q_stride, const double *dQ, long long dq_stride,
                         const double *ddQ, long long ddq_stride, double ridge, double rcond, double *U, double *LAM, double *RHO, double *TAU,
                         double *ACC, int *rank, int *status, const double *rows, int group, int stride, int poison) {
    Emu *e = (Emu *)h;
    tg::RunArgs A{};
    A.batch = batch; A.n_steps = n_states; A.mode = tg::MODE_DYN_INVERSE; A.group_size = 1;
    tg::DynInverseArgs J{};
    tg::dyn_inverse_lsq_layout(e->P.lds_per_team, e->P.nq, e->P.nd, e->P.nu, e->P.nc, J);
    J.Q = Q; J.dQ = dQ; J.ddQ = ddQ; J.U = U; J.LAM = LAM; J.RHO = RHO; J.TAU = TAU; J.ACC = ACC; J.status = status;
    J.ridge = ridge; J.q_stride = (size_t)q_stride; J.dq_stride = (size_t)dq_stride; J.ddq_stride = (size_t)ddq_stride; J.n_states = n_states;
    J.rcond = rcond; J.rank = rank;
    const tg::ParTable T{rows, group > 0 ? group : 1, stride};
    std::vector<double> lds((size_t)J.lds_per_team);
    for (long long i = 0; i < (long long)batch * n_states; i++) {
        std::fill(lds.begin(), lds.end(), poison ? NAN : 0.0);
        if (rows) tg::run_dyn_inverse<1, true, true, true>(static_cast<tg::CProg &>(e->P), A, J, T, lds.data(), 0, i);
        else tg::run_dyn_inverse<1, true, false, true>(static_cast<tg::CProg &>(e->P), A, J, T, lds.data(), 0, i);
    }
}

// as emu_inverse (tests/emu_invdyn), with rcond and rank
void emu_inverse_lsq(void *h, int batch, int n_steps, double dt, const double *dt_steps, const double *Q, long long q_stride, const double *p0,
                     double ridge, double rcond, double *U, double *LAM, double *Pout, double *RHO, double *Hout, int *rank, int *status,
                     const double *rows, int group, int stride, int poison) {
    Emu *e = (Emu *)h;
    tg::RunArgs A{};
    A.batch = batch; A.n_steps = n_steps; A.mode = tg::MODE_INVERSE; A.group_size = 1;
    tg::InverseArgs J{};
    tg::inverse_lsq_layout(e->P.lds_per_team, e->P.nd, e->P.nu, e->P.nc, J);
    J.Q = Q; J.p0 = p0; J.dt_steps = dt_steps; J.U = U; J.LAM = LAM; J.P = Pout; J.RHO = RHO; J.H = Hout; J.status = status;
    J.dt = dt; J.ridge = ridge; J.q_stride = (size_t)q_stride; J.n_steps = n_steps;
    J.rcond = rcond; J.rank = rank;
    const tg::ParTable T{rows, group > 0 ? group : 1, stride};
    std::vector<double> lds((size_t)J.lds_per_team);
    for (long long i = 0; i < (long long)batch * n_steps; i++) {
        std::fill(lds.begin(), lds.end(), poison ? NAN : 0.0);
        if (rows) tg::run_inverse<1, true, true, true>(static_cast<tg::CProg &>(e->P), A, J, T, lds.data(), 0, i);
        else tg::run_inverse<1, true, false, true>(static_cast<tg::CProg &>(e->P), A, J, T, lds.data(), 0, i);
    }
}
}
