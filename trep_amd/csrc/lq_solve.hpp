// lq_solve.hpp -- the gamma solvers of the matrix-core LQ sweeps (dopt.hip: k_tv_lq_mfma, k_tv_lq_ds): [C | K] = gamma^-1 [B'b + r | Kpart]
// with gamma = R_k + B'PB (nU x nU, nU <= NR <= 32) and 1 + nX right-hand sides, all in LDS as G [nU][ldw] = [gamma | rhs].
//   lq_factor_rows       pivoted elimination of gamma alone, one row per lane; leaves multipliers (over gamma) and the table LqFac
//   lq_apply_rows        a wave replays those steps on its slice of the right-hand sides
//   lq_factor_rows_spd2  unpivoted, guarded in-place inversion, two rows per lane on a 16-lane DPP row; leaves gamma^-1 over gamma
//   (the product gamma^-1 [rhs] on the matrix cores that goes with it is phase 4 of k_tv_lq_ds: "the inverse product")
//   lq_factor_call, lq_factor_pivoted_call   the factorisation as calls (k_tv_lq_ds), the first one choosing between the two forms
// Needs lanes.hpp only (tg_rcp, tg_max_u32_lanes32, tg_readlane_f64).  LqFac is seen by the host as well (the LDS layouts size the
// table with it); the solvers exist in the device pass only, like those of gj_solve.hpp.
#pragma once
#include "lanes.hpp"

namespace tg {

// The factorisation table `fac` in LDS, offsets in doubles: what lq_factor_rows leaves for lq_apply_rows, then the form flag by
// which k_tv_lq_ds chooses between the replay and the inverse product.
struct LqFac {
    static constexpr int ROWS = 32;                 // rows a solver holds at most (NR <= ROWS)
    static constexpr int DINV = 0;                  // ROWS doubles: reciprocal pivot of the row each lane holds
    static constexpr int COL = DINV + ROWS;         // ROWS ints: the column that row solved (-1: none)
    static constexpr int PIV = COL + ROWS / 2;      // ROWS ints: the pivot lane of each step
    static constexpr int FORM = PIV + ROWS / 2;     // one int (lq_factor_call): 1 = gamma's block of G holds gamma^-1 (the inverse product),
                                                    // 0 = the multipliers of the pivoted factorisation (lq_apply_rows)
    static constexpr int SIZE = FORM;               // doubles without the flag (k_tv_lq_mfma: always the replay) ...
    static constexpr int SIZE_WITH_FORM = FORM + 2; // ... and with it
};

#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
typedef __attribute__((address_space(3))) double lq_lds_double;
typedef __attribute__((address_space(3))) int lq_lds_int;
__device__ __forceinline__ lq_lds_double *lq_fac_dinv(const double *fac) { return (lq_lds_double *)fac + LqFac::DINV; }
__device__ __forceinline__ lq_lds_int *lq_fac_col(const double *fac) { return (lq_lds_int *)((lq_lds_double *)fac + LqFac::COL); }
__device__ __forceinline__ lq_lds_int *lq_fac_piv(const double *fac) { return (lq_lds_int *)((lq_lds_double *)fac + LqFac::PIV); }
__device__ __forceinline__ int *lq_fac_form(double *fac) { return reinterpret_cast<int *>(fac + LqFac::FORM); }

// Gauss-Jordan on gamma with one matrix ROW per lane (lanes 0 .. NR-1) and the columns in registers.  A pivot step is: one 32-lane DPP
// max over |a_ik| (LAPACK's rule: largest magnitude of the column among the rows not used yet; near ties within 2^-17 go to the lower
// row), the pivot row broadcast with v_readlane (two entries ahead of their two FMAs), one FMA per remaining column -- no LDS
// traffic, no dynamic register index.  Rows / columns nU .. NR-1 are an identity block.  The elimination is in two parts, so that
// the dependent pivot steps (search -> reciprocal -> multipliers) are done ONCE per Riccati step instead of once per wavefront.
// lq_factor_rows: the matrix alone; the multiplier of (row i, step k) goes over the dead entry G[i][k], the pivot lanes / solved
// columns / reciprocal pivots to `fac` (LqFac).  lq_apply_rows: a wave replays the steps on its slice of right-hand sides (columns
// rhs_lo .. rhs_lo + rhs_n - 1 of the block behind gamma; at most SL): per step one multiplier read, and per column two v_readlane
// + one FMA.  Solutions go to Cs [nU] (rhs 0) and Ks [nU][ldx] (rhs 1 + j), in variable order.
template <int NR>
__device__ __forceinline__ void lq_factor_rows(double *G_generic, int ldw, int nU, int lane, double *fac, int *sing) {
    static_assert(NR <= LqFac::ROWS, "the factorisation table holds 32 rows");
    lq_lds_double *G = (lq_lds_double *)G_generic, *dinv_s = lq_fac_dinv(fac);
    lq_lds_int *col_s = lq_fac_col(fac), *piv_s = lq_fac_piv(fac);
    const bool mine = lane < nU, ident = lane >= nU && lane < NR;
    double m[NR];
#pragma unroll
    for (int j = 0; j < NR; j++) m[j] = mine ? (j < nU ? G[lane * ldw + j] : 0.0) : ((ident && j == lane) ? 1.0 : 0.0);
    int mycol = -1;
    double diag = 1.0;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < NR; k++) if (k < nU) {      // (steps nU .. NR-1 are the identity block: they change nothing; a uniform branch per unrolled step)
        const bool free_row = (mine || ident) && mycol < 0;
        const float cand = free_row ? (float)fabs(m[k]) : 0.0f;
        const unsigned int best = tg_max_u32_lanes32((__float_as_uint(cand) & ~0x3Fu) | (unsigned int)(63 - lane));
        const int src = 63 - (int)(best & 0x3Fu);
        if (!(__uint_as_float(best & ~0x3Fu) > 0.0f)) ok = false;
        const bool is_piv = lane == src;
        const double inv = tg_rcp(tg_readlane_f64(m[k], src));      // (the multipliers need not be correctly rounded)
        const double l = (ok && !is_piv) ? m[k] * inv : 0.0;
#pragma unroll
        for (int j = k + 1; j < NR; j += 2) {
            const double p0 = tg_readlane_f64(m[j], src), p1 = tg_readlane_f64(m[j + 1 < NR ? j + 1 : j], src);
            m[j] = fma(-l, p0, m[j]);
            if (j + 1 < NR) m[j + 1] = fma(-l, p1, m[j + 1]);
        }
        if (is_piv) { mycol = k; diag = m[k]; }
        if (mine) G[lane * ldw + k] = l;
        if (lane == 0) piv_s[k] = src;
    }
    if (!ok && lane == 0) *sing = 1;
    if (lane < LqFac::ROWS) { col_s[lane] = mycol; dinv_s[lane] = 1.0 / diag; }
}

template <int NR, int SL>
__device__ __forceinline__ void lq_apply_rows(const double *G_generic, int ldw, int nU, int rhs_lo, int rhs_n, double *Ks_generic, int ldx,
                                              double *Cs_generic, int lane, const double *fac) {
    const lq_lds_double *G = (const lq_lds_double *)G_generic, *dinv_s = lq_fac_dinv(fac);
    const lq_lds_int *col_s = lq_fac_col(fac), *piv_s = lq_fac_piv(fac);
    lq_lds_double *Ks = (lq_lds_double *)Ks_generic, *Cs = (lq_lds_double *)Cs_generic;
    const bool mine = lane < nU;
    double b[SL];
#pragma unroll
    for (int c = 0; c < SL; c++) b[c] = (mine && c < rhs_n) ? G[lane * ldw + nU + rhs_lo + c] : 0.0;
    for (int k = 0; k < nU; k++) {
        const int src = __builtin_amdgcn_readfirstlane(piv_s[k]);
        const double l = mine ? G[lane * ldw + k] : 0.0;
#pragma unroll
        for (int c = 0; c < SL; c += 2) {
            const double p0 = tg_readlane_f64(b[c], src), p1 = tg_readlane_f64(b[c + 1 < SL ? c + 1 : c], src);
            b[c] = fma(-l, p0, b[c]);
            if (c + 1 < SL) b[c + 1] = fma(-l, p1, b[c + 1]);
        }
    }
    const int mycol = lane < LqFac::ROWS ? col_s[lane] : -1;
    if (mine && mycol >= 0 && mycol < nU) {       // row `lane` was the pivot of variable mycol: its right-hand sides / pivot are that variable's solution
        const double dinv = dinv_s[lane];
#pragma unroll
        for (int c = 0; c < SL; c++) {
            if (c < rhs_n) {
                const int g = rhs_lo + c;
                const double x = b[c] * dinv;
                if (g == 0) Cs[mycol] = x; else Ks[mycol * ldx + g - 1] = x;
            }
        }
    }
}

// gamma = R_k + B'PB is symmetric and, with a positive definite R_k, positive definite: it can be eliminated in index order without a
// pivot search (the pivoted factorisation is ~20 k cycles of the ~70 k of a Riccati step, executed by one wave while seven wait at
// the barrier).  TWO matrix rows per lane (rows 2 i and 2 i + 1 in lane i < NR / 2 <= 16): the pivot row of step k sits in lane
// k / 2 of the first 16-lane DPP row, and the elimination is `v_fmac_f64_dpp ... row_newbcast:k/2` -- one instruction per (row,
// column) instead of two v_readlane + one FMA, no SGPR hazards.  It leaves gamma^-1 itself (in-place Gauss-Jordan inversion, over
// gamma in G) instead of the multipliers: the replay of the elimination on the 1 + nX right-hand sides -- 18 steps of two v_readlane
// + one FMA per column on 18 of 64 lanes, the longest phase of the step (17 k cycles) -- becomes a product gamma^-1 [r | Kpart] on
// the matrix cores (the inverse product in phase 4 of k_tv_lq_ds).  Every pivot is guarded -- |pivot| must exceed 2^-20 of the largest entry of its row (the
// Newton model's R_k + HZ_uu can be indefinite far from the optimum) -- and nothing is written before all guards have passed: on
// failure (false) the caller runs lq_factor_rows on the untouched matrix.
template <int L>
__device__ __forceinline__ double lq_bcast16(double v) {
    return __longlong_as_double(__builtin_amdgcn_update_dpp((long long)0, __double_as_longlong(v), 0x150 + L, 0xf, 0xf, true));
}
template <int L>
__device__ __forceinline__ void lq_fmac16(double &a, double b, double c) {      // a += (lane L's b) * c
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(a) : "v"(b), "v"(c), "n"(L));
}
template <int K, int NR>
__device__ __forceinline__ void lq_spd2_steps(double (&m0)[NR], double (&m1)[NR], int lane, int nU, double &inv0, double &inv1) {
    if constexpr (K < NR) {
        if (K < nU) {      // (uniform)
            constexpr int L = K >> 1;
            constexpr bool ODD = (K & 1) != 0;
            const double inv = tg_rcp(lq_bcast16<L>(ODD ? m1[K] : m0[K]));
            const bool pl = lane == L;
            double n0 = -(m0[K] * inv), n1 = -(m1[K] * inv);      // minus the multipliers of the lane's two rows
            if (ODD) { n1 = pl ? 0.0 : n1; inv1 = pl ? inv : inv1; } else { n0 = pl ? 0.0 : n0; inv0 = pl ? inv : inv0; }
            // IN-PLACE Gauss-Jordan inversion: column K of the matrix is dead after this step and becomes column K of the inverse's
            // numerator (pivot row: 1, other rows: minus their multiplier); the columns j < K already are such columns and are updated
            // like the live matrix columns j > K
#pragma unroll
            for (int j = 0; j < NR; j++) {
                if (j == K) continue;
                if (ODD) { lq_fmac16<L>(m0[j], m1[j], n0); lq_fmac16<L>(m1[j], m1[j], n1); }
                else { lq_fmac16<L>(m1[j], m0[j], n1); lq_fmac16<L>(m0[j], m0[j], n0); }
            }
            m0[K] = (!ODD && pl) ? 1.0 : n0; m1[K] = (ODD && pl) ? 1.0 : n1;
        }
        lq_spd2_steps<K + 1, NR>(m0, m1, lane, nU, inv0, inv1);
    }
}
template <int NR>
__device__ __forceinline__ bool lq_factor_rows_spd2(double *G_generic, int ldw, int nU, int lane) {
    static_assert(NR % 2 == 0 && NR <= 32, "two rows per lane on one 16-lane DPP row");
    lq_lds_double *G = (lq_lds_double *)G_generic;
    const int r0 = 2 * (lane & 15), r1 = r0 + 1;
    const bool have = lane < NR / 2, in0 = have && r0 < nU, in1 = have && r1 < nU;
    double m0[NR], m1[NR], a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int j = 0; j < NR; j++) {
        const double x0 = G[(in0 ? r0 : 0) * ldw + (j < nU ? j : 0)], x1 = G[(in1 ? r1 : 0) * ldw + (j < nU ? j : 0)];
        m0[j] = (in0 && j < nU) ? x0 : ((have && !in0 && j == r0) ? 1.0 : 0.0);
        m1[j] = (in1 && j < nU) ? x1 : ((have && !in1 && j == r1) ? 1.0 : 0.0);
        a0 = fmax(a0, fabs(m0[j])); a1 = fmax(a1, fabs(m1[j]));
    }
    double inv0 = 0.0, inv1 = 0.0;
    lq_spd2_steps<0, NR>(m0, m1, lane, nU, inv0, inv1);
    // the guards: |pivot| > 2^-20 of the row's largest entry, from the reciprocal kept by each row (a zero pivot gives inf / NaN: fails)
    const bool bad = (in0 && !(fabs(inv0) * (9.5367431640625e-07 * a0) < 1.0)) || (in1 && !(fabs(inv1) * (9.5367431640625e-07 * a1) < 1.0));
    if (__any(bad ? 1 : 0)) return false;
#pragma unroll
    for (int k = 0; k < NR; k++) if (k < nU) {      // gamma^-1 [row][k] = numerator / pivot of the row
        if (in0) G[r0 * ldw + k] = m0[k] * inv0;
        if (in1) G[r1 * ldw + k] = m1[k] * inv1;
    }
    return true;
}

// (the pivoted fallback as a call of its own: its code is only fetched when a guard failed)
template <int NR>
__device__ __noinline__ void lq_factor_pivoted_call(double *G, int ldw, int nU, int lane, double *fac, int *sing) {
    ldw = __builtin_amdgcn_readfirstlane(ldw); nU = __builtin_amdgcn_readfirstlane(nU);
    lq_factor_rows<NR>(G, ldw, nU, lane, fac, sing);
}

// gamma's factorisation as a CALL: one wave of eight runs it, and inlined its 2 x 20 matrix registers (unpivoted attempt + pivoted fallback)
// are part of the sweep kernel's register allocation (158 spilled VGPRs).  Leaves the form it took in the table's flag (LqFac::FORM).
template <int NR>
__device__ __noinline__ void lq_factor_call(double *G, int ldw, int nU, int lane, double *fac, int *sing) {
    // (arguments of a call travel in vector registers: say that the sizes are wave-uniform, or every `k < nU` becomes a divergent branch)
    ldw = __builtin_amdgcn_readfirstlane(ldw); nU = __builtin_amdgcn_readfirstlane(nU);
    const bool inverse = lq_factor_rows_spd2<NR>(G, ldw, nU, lane);
    if (!inverse) lq_factor_pivoted_call<NR>(G, ldw, nU, lane, fac, sing);
    if (lane == 0) *lq_fac_form(fac) = inverse ? 1 : 0;
}
#endif

}  // namespace tg
