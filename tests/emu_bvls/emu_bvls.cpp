// Host emulation of the bounded least-squares solver and of the two kernels that end in it (TEST INFRASTRUCTURE ONLY).
//
// trep_amd/csrc/bvls_solve.hpp, mvi_dyn_inverse.hpp and mvi_inverse.hpp compiled with g++ and TEAM = 1: the solver alone on
// caller-supplied problems (what tg_batch_debug_bvls_solve runs on the device), and every team of a call through the BND
// instantiations of run_dyn_inverse / run_inverse, one after the other, with the scratch layouts the device launches use
// (dyn_inverse_bounded_layout, inverse_bounded_layout).  Not part of the product.
// With -DEMU_BVLS_MAIN the file is a program of its own that runs the solver on a fixed set of problems (for a sanitizer build:
// g++ -fsanitize=address,undefined -DEMU_BVLS_MAIN emu_bvls.cpp); it prints a checksum and exits 0.
#include <algorithm>
#include <cmath>
#include <cstdio>
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

// `count` problems of one shape: A [count][rows][cols], c [count][rows], lo and hi [count][cols]; z and active [count][cols], solves,
// rank and status [count].  max_solves 0: 3 cols + 3.  poison: the scratch starts as NaN
void emu_bvls_solve(int count, int rows, int cols, const double *A, const double *c, const double *lo, const double *hi, double rcond,
                    int max_solves, double *z, int *active, int *solves, int *rank, int *status, int poison) {
    const int ld = cols + 1;
    std::vector<double> lds((size_t)rows * ld + tg::bvls_scratch_doubles(rows, cols));
    for (int p = 0; p < count; p++) {
        std::fill(lds.begin(), lds.end(), poison ? NAN : 0.0);
        double *W = lds.data(), *scr = W + (size_t)rows * ld;
        const tg::BvlsScratch X = tg::bvls_scratch(scr, rows, cols);
        for (int i = 0; i < rows; i++) {
            for (int j = 0; j < cols; j++) W[i * ld + j] = A[((size_t)p * rows + i) * cols + j];
            W[i * ld + cols] = c[(size_t)p * rows + i];
        }
        for (int j = 0; j < cols; j++) { X.lo[j] = lo[(size_t)p * cols + j]; X.hi[j] = hi[(size_t)p * cols + j]; }
        int n_solves = 0, st = TG_OK;
        bool finite = true;
        const int r = tg::bvls_solve<1, true>(true, W, rows, cols, ld, rcond, max_solves ? max_solves : tg::bvls_max_solves(cols), scr, 0, n_solves, st, finite);
        const bool answer = st != TG_SINGULAR;
        for (int j = 0; j < cols; j++) { z[(size_t)p * cols + j] = answer ? X.z[j] : 0.0; active[(size_t)p * cols + j] = answer ? X.bnd[j] : 0; }
        solves[p] = n_solves; rank[p] = finite ? r : 0; status[p] = st;
    }
}

// doubles of LDS per team: out[0..4] = computed torque BND, computed torque LSQ, inverse dynamics BND, inverse dynamics LSQ, rollout
// slice; out[5..7] the offsets o_kkt, o_ddq, o_scal of the first
void emu_bvls_lds(void *h, int *out) {
    Emu *e = (Emu *)h;
    tg::DynInverseArgs D{}, D0{};
    tg::dyn_inverse_bounded_layout(e->P.lds_per_team, e->P.nq, e->P.nd, e->P.nu, e->P.nc, D);
    tg::dyn_inverse_lsq_layout(e->P.lds_per_team, e->P.nq, e->P.nd, e->P.nu, e->P.nc, D0);
    tg::InverseArgs I{}, I0{};
    tg::inverse_bounded_layout(e->P.lds_per_team, e->P.nd, e->P.nu, e->P.nc, I);
    tg::inverse_lsq_layout(e->P.lds_per_team, e->P.nd, e->P.nu, e->P.nc, I0);
    out[0] = D.lds_per_team; out[1] = D0.lds_per_team; out[2] = I.lds_per_team; out[3] = I0.lds_per_team; out[4] = e->P.lds_per_team;
    out[5] = D.o_kkt; out[6] = D.o_ddq; out[7] = D.o_scal;
}

// as emu_dyn_inverse_lsq (tests/emu_lsq), with the box lo, hi [bound_rows][nu + nc] and the outputs active and solves
void emu_dyn_inverse_bounded(void *h, int batch, int n_states, const double *Q, long long q_stride, const double *dQ, long long dq_stride,
                             const double *ddQ, long long ddq_stride, double ridge, double rcond, const double *lo, const double *hi,
                             int bound_rows, double *U, double *LAM, double *RHO, double *TAU, double *ACC, int *active, int *solves, int *rank,
                             int *status, const double *rows, int group, int stride, int poison) {
    Emu *e = (Emu *)h;
    tg::RunArgs A{};
    A.batch = batch; A.n_steps = n_states; A.mode = tg::MODE_DYN_INVERSE; A.group_size = 1;
    tg::DynInverseArgs J{};
    tg::dyn_inverse_bounded_layout(e->P.lds_per_team, e->P.nq, e->P.nd, e->P.nu, e->P.nc, J);
    J.Q = Q; J.dQ = dQ; J.ddQ = ddQ; J.U = U; J.LAM = LAM; J.RHO = RHO; J.TAU = TAU; J.ACC = ACC; J.status = status;
    J.ridge = ridge; J.q_stride = (size_t)q_stride; J.dq_stride = (size_t)dq_stride; J.ddq_stride = (size_t)ddq_stride; J.n_states = n_states;
    J.rcond = rcond; J.rank = rank;
    J.lo = lo; J.hi = hi; J.bound_rows = bound_rows; J.active = active; J.solves = solves; J.max_solves = tg::bvls_max_solves(e->P.nu + e->P.nc);
    const tg::ParTable T{rows, group > 0 ? group : 1, stride};
    std::vector<double> lds((size_t)J.lds_per_team);
    for (long long i = 0; i < (long long)batch * n_states; i++) {
        std::fill(lds.begin(), lds.end(), poison ? NAN : 0.0);
        if (rows) tg::run_dyn_inverse<1, true, true, false, true>(static_cast<tg::CProg &>(e->P), A, J, T, lds.data(), 0, i);
        else tg::run_dyn_inverse<1, true, false, false, true>(static_cast<tg::CProg &>(e->P), A, J, T, lds.data(), 0, i);
    }
}

// as emu_inverse_lsq (tests/emu_lsq), likewise
void emu_inverse_bounded(void *h, int batch, int n_steps, double dt, const double *dt_steps, const double *Q, long long q_stride, const double *p0,
                         double ridge, double rcond, const double *lo, const double *hi, int bound_rows, double *U, double *LAM, double *Pout,
                         double *RHO, double *Hout, int *active, int *solves, int *rank, int *status, const double *rows, int group, int stride,
                         int poison) {
    Emu *e = (Emu *)h;
    tg::RunArgs A{};
    A.batch = batch; A.n_steps = n_steps; A.mode = tg::MODE_INVERSE; A.group_size = 1;
    tg::InverseArgs J{};
    tg::inverse_bounded_layout(e->P.lds_per_team, e->P.nd, e->P.nu, e->P.nc, J);
    J.Q = Q; J.p0 = p0; J.dt_steps = dt_steps; J.U = U; J.LAM = LAM; J.P = Pout; J.RHO = RHO; J.H = Hout; J.status = status;
    J.dt = dt; J.ridge = ridge; J.q_stride = (size_t)q_stride; J.n_steps = n_steps;
    J.rcond = rcond; J.rank = rank;
    J.lo = lo; J.hi = hi; J.bound_rows = bound_rows; J.active = active; J.solves = solves; J.max_solves = tg::bvls_max_solves(e->P.nu + e->P.nc);
    const tg::ParTable T{rows, group > 0 ? group : 1, stride};
    std::vector<double> lds((size_t)J.lds_per_team);
    for (long long i = 0; i < (long long)batch * n_steps; i++) {
        std::fill(lds.begin(), lds.end(), poison ? NAN : 0.0);
        if (rows) tg::run_inverse<1, true, true, false, true>(static_cast<tg::CProg &>(e->P), A, J, T, lds.data(), 0, i);
        else tg::run_inverse<1, true, false, false, true>(static_cast<tg::CProg &>(e->P), A, J, T, lds.data(), 0, i);
    }
}
}

#if defined(EMU_BVLS_MAIN)
// the solver alone on pseudo-random problems of several shapes, boxes that bind none, some and all variables, one-sided and
// degenerate (lo == hi) bounds, a rank-deficient and a non-finite problem; every scratch array is sized exactly, so that an
// address sanitizer sees any access outside it
int main() {
    unsigned long long s = 88172645463325252ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
    const int shapes[][2] = {{1, 1}, {2, 1}, {3, 3}, {5, 2}, {9, 4}, {22, 18}, {40, 18}, {7, 7}};
    double sum = 0.0;
    int problems = 0, most = 0;
    for (const auto &sh : shapes) {
        const int rows = sh[0], cols = sh[1];
        for (int kind = 0; kind < 8; kind++) {
            std::vector<double> A((size_t)rows * cols), c(rows), lo(cols), hi(cols), z(cols);
            std::vector<int> active(cols);
            for (double &a : A) a = rnd();
            for (double &v : c) v = 3.0 * rnd();
            for (int j = 0; j < cols; j++) {
                const double w = kind == 0 ? INFINITY : (kind == 1 ? 100.0 : (kind == 2 ? 0.3 : 0.01));
                lo[j] = -w * (0.5 + 0.5 * fabs(rnd())); hi[j] = w * (0.5 + 0.5 * fabs(rnd()));
                if (kind == 4) lo[j] = -INFINITY;
                if (kind == 5 && j == 0) lo[j] = hi[j] = 0.25;
            }
            if (kind == 6 && cols > 1) for (int i = 0; i < rows; i++) A[(size_t)i * cols + 1] = A[(size_t)i * cols];
            if (kind == 7) A[0] = NAN;
            int solves = 0, rank = 0, status = 0;
            emu_bvls_solve(1, rows, cols, A.data(), c.data(), lo.data(), hi.data(), 1e-9, 0, z.data(), active.data(), &solves, &rank, &status, 1);
            for (int j = 0; j < cols; j++) sum += z[j] + active[j];
            sum += solves + rank + status;
            most = std::max(most, solves);
            problems++;
        }
    }
    std::printf("emu_bvls: %d problems, at most %d solves, checksum %.17g\n", problems, most, sum);
    return 0;
}
#endif
