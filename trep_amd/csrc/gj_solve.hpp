// gj_solve.hpp -- the register-resident dense Gauss-Jordan solvers with scaled partial pivoting: gj_rows_exact / gj_rows (one row per
// lane), gj_panel / gj_panel_rhs (matrix-core panels, full-wave teams) and gj_cols (two columns per lane, many right-hand sides).
// Siblings of the structured solve (bbd_solve.hpp); the LDS fallback Core::gauss_jordan stays in mvi_core.hpp.  Device pass only.
// TEAM is the team size of the caller (lanes per trajectory); beyond it the solvers use their arguments and lanes.hpp (tg_rcp,
// tg_max_u32_lanes32, TG_SYNC), nothing of the integrator core.  gj_panel / gj_panel_rhs are full-wave only and take no TEAM;
// gj_cols is full-wave only as well, but its call sites are compiled for every team size, so it keeps the parameter.
#pragma once
#include "lanes.hpp"
#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
namespace tg {

// ---- Gauss-Jordan with one matrix ROW PER LANE held in registers (n <= N <= TEAM) ---------------------
//      Same pivot rule as gauss_jordan() but pivoting "in place": rows never move, the lane that owns
//      the pivot row of step k broadcasts it (v_readlane for a full-wave team, ds_bpermute otherwise)
//      and every other lane eliminates in registers.  No LDS traffic inside the k loop.  N is the
//      matrix size rounded up to a multiple of 4 (identity padding), so every loop bound is a
//      compile-time constant and the body carries no guards.
//      Reads [A | rhs(1 column)] from LDS, leaves x in A[i*ld + n] like gauss_jordan().
// Slow path of the pivot search (out of line: the 28-times unrolled solver must stay small enough for the instruction
// cache): exact maximum of the candidates' doubles and, among the rows that attain it, the first in the reference's order.
template <int TEAM>
__device__ __noinline__ int pivot_exact(double cand64, bool cand_ok, int pos, int lane) {
    unsigned long long best = cand_ok ? (unsigned long long)__double_as_longlong(cand64) : 0ull;   // non-negative doubles order like their bits
    if (TEAM == 64) {
        best = __ockl_wfred_max_u64(best);
    } else {
#pragma unroll
        for (int m = TEAM / 2; m >= 1; m >>= 1) {
            const unsigned long long o = __shfl_xor(best, m, TEAM);
            best = o > best ? o : best;
        }
    }
    const bool at_max = cand_ok && (unsigned long long)__double_as_longlong(cand64) == best;
    unsigned int k2 = at_max ? ((unsigned int)(63 - pos) << 6) | (unsigned int)(lane & 63) : 0u;   // position first, lane to identify the row
    if (TEAM == 64) {
        k2 = __ockl_wfred_max_u32(k2);
    } else {
#pragma unroll
        for (int m = TEAM / 2; m >= 1; m >>= 1) {
            const unsigned int o = __shfl_xor(k2, m, TEAM);
            k2 = o > k2 ? o : k2;
        }
    }
    int piv = (int)(k2 & 0x3Fu);
    if (TEAM != 64) piv = (piv & (TEAM - 1));
    return piv;
}

template <int TEAM, int N, bool TRACE = false>
__device__ __noinline__ bool gj_rows_exact(bool on, double *A_generic, int n, int ld, int lane, int *trace = nullptr) {
    typedef __attribute__((address_space(3))) double lds_double;
    lds_double *A = (lds_double *)A_generic;
    double row[N], rhs = 0.0, scale = 0.0, diag = 1.0;
    int mycol = -1;
    // position of this lane's row in the reference's row order (math-code.c swaps rows physically; here rows never move):
    // only needed to break EXACT ties the way the reference's strict `>` scan does -- first row in its current order
    int pos = lane;
    const bool mine = on && lane < N;
    const int wl = (int)(threadIdx.x & 63u), team_base = wl - lane;
#pragma unroll
    for (int j = 0; j < N; j++)
        row[j] = (mine && lane < n && j < n) ? A[lane * ld + j] : ((mine && lane >= n && j == lane) ? 1.0 : 0.0);
    if (mine) {
        rhs = lane < n ? A[lane * ld + n] : 0.0;
        double s = -1.0;
#pragma unroll
        for (int j = 0; j < N; j++) { const double a = fabs(row[j]); s = a > s ? a : s; }
        scale = 1.0 / s;
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < N; k++) {
        // arg-max of |a_ik| * scale_i over the rows not yet used as pivots, ties to the row that comes first in the
        // reference's (swapped) row order -- its scan uses a strict `>`.  The candidates are ranked by ONE 32-bit wave max
        // of (single-precision magnitude with the 6 low mantissa bits replaced by 63 - position): cast and mask are
        // monotonic, so the exact fp64 maximum is among the lanes that attain the truncated maximum, and among EXACTLY
        // equal candidates (mirror-symmetric mechanisms produce them all the time) the key already prefers the smallest
        // position.  Only if several lanes share the truncated maximum with DIFFERENT doubles (within 2^-17 relative, rare)
        // the slow path compares the doubles exactly.
        const bool cand_ok = mine && mycol < 0;
        const double cand64 = cand_ok ? fabs(row[k] * scale) : 0.0;
        // key = magnitude (22 bits) | 31 - position | lane: N <= 32, so position and lane take 5 bits each
        const unsigned int tkey = __float_as_uint((float)cand64) & ~0x3FFu;
        unsigned int key = tkey | ((unsigned int)(31 - (pos & 31)) << 5) | (unsigned int)(lane & 31);
        if (TEAM == 64) {
            key = __ockl_wfred_max_u32(key);
        } else {
#pragma unroll
            for (int m = TEAM / 2; m >= 1; m >>= 1) {
                const unsigned int o = __shfl_xor(key, m, TEAM);
                key = o > key ? o : key;
            }
        }
        const unsigned long long team_mask = TEAM == 64 ? ~0ull : (((1ull << TEAM) - 1ull) << team_base);
        const bool at_tmax = cand_ok && tkey == (key & ~0x3FFu);
        const unsigned long long tied = __ballot(at_tmax) & team_mask;
        int piv = (int)(key & 31u);
        if (TEAM < 32) piv &= (TEAM - 1);
        if (__any((tied & (tied - 1ull)) != 0ull ? 1 : 0)) {   // some team has several lanes at the truncated maximum
            const double w = TEAM == 64 ? __longlong_as_double(((long long)__builtin_amdgcn_readlane((int)(__double_as_longlong(cand64) >> 32), piv) << 32) |
                                                               (unsigned int)__builtin_amdgcn_readlane((int)(__double_as_longlong(cand64) & 0xFFFFFFFFLL), piv))
                                        : __shfl(cand64, piv, TEAM);
            if (__any((at_tmax && cand64 != w) ? 1 : 0))       // ... and they are not all exactly equal: exact comparison
                piv = pivot_exact<TEAM>(cand64, cand_ok, pos, lane);
        }
        // singular test (math-code.c:393: scaled pivot <= 1e-20): decided by the truncated maximum unless that lies within a
        // factor of two of the threshold -- only then the winner's exact value is looked at
        const int src = (TEAM == 64) ? __builtin_amdgcn_readfirstlane(piv) : piv;
        const float best = __uint_as_float(key & ~0x3FFu);
        if (__any((best < 2.0e-20f && best > 0.5e-20f) ? 1 : 0)) {
            const unsigned long long big = __ballot(cand64 > 1.0e-20);
            if (on && ok && !((big >> (team_base + src)) & 1ull)) ok = false;
        } else if (on && ok && !(best > 1.0e-20f)) ok = false;
        const bool go = on && ok;
        // broadcast the pivot row (columns k..N-1 and the rhs)
        auto bcast = [&](double v) -> double {
            if (TEAM == 64) {
                const long long b = __double_as_longlong(v);
                const int lo = __builtin_amdgcn_readlane((int)(b & 0xFFFFFFFFLL), src);
                const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
                return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
            }
            return __shfl(v, src, TEAM);
        };
        const double pkk = bcast(row[k]);
        const double prhs = bcast(rhs);
        const bool is_piv = mine && (lane & (TEAM - 1)) == src;
        // bookkeeping of the reference's row order: it swaps the pivot row with the row at position k
        {
            const int pos_p = (TEAM == 64) ? __builtin_amdgcn_readlane(pos, src) : __shfl(pos, src, TEAM);
            if (__any(pos_p != k ? 1 : 0)) {     // (wave-uniform) almost never taken: the pivot usually is the row at position k
                if (pos == k) pos = pos_p;
                if (is_piv) pos = k;
            }
        }
        if (TRACE && go && is_piv) trace[k] = lane;
        // 1/pivot: hardware seed + two Newton steps (the multipliers need not be correctly rounded)
        double rp = tg_rcp(pkk);
        const double l = (go && mine && !is_piv) ? row[k] * rp : 0.0;
#pragma unroll
        for (int j = k + 1; j < N; j++) row[j] = fma(-l, bcast(row[j]), row[j]);
        rhs = fma(-l, prhs, rhs);
        if (go && is_piv) { mycol = k; diag = row[k]; }
        // Keep the elimination pivot-major: left alone, the instruction selector linearises the fully
        // unrolled body column by column (fma -> readlane of the same register -> fma ...): one long
        // dependent chain padded with hazard s_nops.  Passing the updated row through ordered empty asm
        // statements pins step k before step k+1; inside a step the broadcasts and fmas are independent.
#pragma unroll
        for (int j = k + 1; j < N; j += 8) {
            if (j + 7 < N) asm volatile("" : "+v"(row[j]), "+v"(row[j + 1]), "+v"(row[j + 2]), "+v"(row[j + 3]),
                                             "+v"(row[j + 4]), "+v"(row[j + 5]), "+v"(row[j + 6]), "+v"(row[j + 7]));
            else {
#pragma unroll
                for (int jj = j; jj < N; jj++) asm volatile("" : "+v"(row[jj]));
            }
        }
    }
    if (mine && ok && mycol >= 0 && mycol < n) A[mycol * ld + n] = rhs / diag;
    __syncthreads();
    return ok;
}

// ---- the default solver: same elimination, pivot candidates ranked in single precision -------------------------------
//      One 32-bit wave max per step over (float bits of |a_ik| * scale_i with the 6 low mantissa bits replaced by
//      63 - lane) and no branch anywhere in the unrolled body.  Candidates closer than 2^-17 relative are taken in lane
//      (= original row) order.  That is NOT always the reference's choice: every row's largest entry scales to 1 +- 1 ulp,
//      so whenever two rows have their largest entry in the same column (two string constraints and a shared torso
//      config: 95 % of the puppet's Newton systems) the reference's strict `>` scan decides by that last ulp.  Either
//      row is an exact arg-max to 16 digits and the solutions agree to rounding (1e-13 relative on the test matrices), but
//      the pivot SEQUENCE can differ; gj_rows_exact() reproduces it exactly (RunArgs::exact_pivot, tg_batch_set_pivot_rule)
//      at +9 % rollout time -- each variant of an in-line exact test (position bookkeeping +2.3 %, tie block +3.4 %, exact
//      singular test +3.7 %; a branch-free "detect and redo" fires on 95 % of the solves) was measured and rejected.
#if defined(TG_GJ_INLINE)
#define TG_GJ_ATTR __forceinline__
#else
#define TG_GJ_ATTR __noinline__
#endif
template <int TEAM, int N, bool TRACE = false>
__device__ TG_GJ_ATTR bool gj_rows(bool on, double *A_generic, int n, int ld, int lane, int *trace = nullptr) {
    typedef __attribute__((address_space(3))) double lds_double;
    lds_double *A = (lds_double *)A_generic;
    double row[N], rhs = 0.0, scale = 0.0, diag = 1.0;
    int mycol = -1;
    const bool mine = on && lane < N;
#pragma unroll
    for (int j = 0; j < N; j++)
        row[j] = (mine && lane < n && j < n) ? A[lane * ld + j] : ((mine && lane >= n && j == lane) ? 1.0 : 0.0);
    if (mine) {
        rhs = lane < n ? A[lane * ld + n] : 0.0;
        double s = -1.0;
#pragma unroll
        for (int j = 0; j < N; j++) { const double a = fabs(row[j]); s = a > s ? a : s; }
        scale = 1.0 / s;
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < N; k++) {
        const float cand = (mine && mycol < 0) ? (float)fabs(row[k] * scale) : 0.0f;
        unsigned int key = (__float_as_uint(cand) & ~0x3Fu) | (unsigned int)(63 - (lane & 63));
        if (TEAM == 64) {
            key = tg_max_u32_lanes32(key);       // N <= 32: only lanes 0..31 hold rows (the others carry key 0 | lane bits)
        } else {
#pragma unroll
            for (int m = TEAM / 2; m >= 1; m >>= 1) {
                const unsigned int o = __shfl_xor(key, m, TEAM);
                key = o > key ? o : key;
            }
        }
        int piv = 63 - (int)(key & 0x3Fu);
        const float best = __uint_as_float(key & ~0x3Fu);
        if (TEAM != 64) piv = (piv & (TEAM - 1));
        if (on && ok && !(best > 1.0e-20f)) ok = false;
        const bool go = on && ok;
        // broadcast the pivot row (columns k..N-1 and the rhs)
        const int src = (TEAM == 64) ? __builtin_amdgcn_readfirstlane(piv) : piv;
        auto bcast = [&](double v) -> double {
            if (TEAM == 64) {
                const long long b = __double_as_longlong(v);
                const int lo = __builtin_amdgcn_readlane((int)(b & 0xFFFFFFFFLL), src);
                const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
                return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
            }
            return __shfl(v, src, TEAM);
        };
        const double prhs = bcast(rhs);
        const bool is_piv = mine && (lane & (TEAM - 1)) == src;
        if (TRACE && go && is_piv) trace[k] = lane;
        const double pkk = bcast(row[k]);
        double rp = tg_rcp(pkk);          // 1/pivot (the multipliers need not be correctly rounded)
        const double l = (go && mine && !is_piv) ? row[k] * rp : 0.0;
        // two pivot-row entries are broadcast before their two FMAs: a v_readlane result cannot be consumed by the next VALU
        // instruction (two wait states), so one broadcast-FMA pair at a time costs an s_nop per column (groups of four make
        // the unroller give up on the row registers: 420 instead of 66 ms)
#pragma unroll
        for (int j = k + 1; j < N; j += 2) {
            const double b0 = bcast(row[j]);
            const double b1 = bcast(row[j + 1 < N ? j + 1 : j]);
            row[j] = fma(-l, b0, row[j]);
            if (j + 1 < N) row[j + 1] = fma(-l, b1, row[j + 1]);
        }
        rhs = fma(-l, prhs, rhs);
        if (go && is_piv) { mycol = k; diag = row[k]; }
        // keep the elimination pivot-major (see gj_rows_exact)
#pragma unroll
        for (int j = k + 1; j < N; j += 8) {
            if (j + 7 < N) asm volatile("" : "+v"(row[j]), "+v"(row[j + 1]), "+v"(row[j + 2]), "+v"(row[j + 3]),
                                             "+v"(row[j + 4]), "+v"(row[j + 5]), "+v"(row[j + 6]), "+v"(row[j + 7]));
            else {
#pragma unroll
                for (int jj = j; jj < N; jj++) asm volatile("" : "+v"(row[jj]));
            }
        }
    }
    if (mine && ok && mycol >= 0 && mycol < n) A[mycol * ld + n] = rhs / diag;
    __syncthreads();
    return ok;
}

// ---- the full-wave solver (TEAM == 64, 16 < n < 32): panels of four columns + trailing update on the matrix cores ---------
//      gj_rows keeps one matrix row per lane (28 of 64 lanes busy) and pays two v_readlane per FMA for the pivot-row
//      broadcast: ~68 VALU instructions per pivot step, and the solver is bound by exactly that instruction stream.  Here the
//      [A | b] matrix (b = column n) stays in LDS in its [n][ld] layout AND lives in the accumulator layout of
//      v_mfma_f64_16x16x4_f64 on all 64 lanes: lane (g = lane >> 4, c = lane & 15), register v of tile (TR, TC) holds entry
//      [16 TR + 4 v + g][16 TC + c] -- 16 doubles per lane instead of 29.  Per panel of four columns:
//        1. lane i < n reads the four panel entries of row i from LDS (one row per lane);
//        2. the four columns are eliminated exactly like gj_rows does it (scaled partial pivoting, rows never move, same
//           single-precision ranking) -- but the broadcasts only cover the other panel columns and the columns of Z: 3 per step;
//        3. Z [32][4] accumulates what the four elementary row operations do to any OTHER column: after the panel,
//           A' = A + Z A[R, :] with R the four pivot rows as they were at the panel's start (block Gauss-Jordan; Z[:, t] is
//           column r_t of the accumulated row-operation matrix minus the identity: z_t <- l at step t, z_s += l z_s[r_t] for s < t);
//        4. Z goes through 1 KB of LDS into A-operand form, lane group t reads pivot row r_t straight from the LDS image as
//           its B operand, the rank-4 update of the four (later two) 16 x 16 tiles is one v_mfma_f64_16x16x4_f64 each, and the
//           live tiles are written back to the LDS image.
//      No branch, no run-time register index.  Same pivot rule as gj_rows (the default rule); the trailing columns see the block
//      update instead of four rank-1 updates, so results differ from gj_rows' by rounding only.  `scratch`: 128 doubles of LDS
//      outside [A | b] (the Z table).
//      Always an out-of-line function: inlined into the 20 k-instruction rollout kernel it shares that kernel's register
//      allocation and schedule (91 instead of 53 SGPR spills, every other phase ~10 % slower: 63.3 ms per benchmark launch);
//      as a call it keeps its own (61.7 ms; gj_rows: 65.1 ms).
template <int N, bool TRACE = false>
__device__ __noinline__ bool gj_panel(bool on, double *A_generic, int n, int ld, int lane, double *scratch_generic, int *trace = nullptr) {
    static_assert(N % 4 == 0 && N > 16 && N <= 32, "gj_panel: 16 < N <= 32");
    typedef __attribute__((address_space(3))) double lds_double;
    typedef double v4d __attribute__((ext_vector_type(4)));
    lds_double *A = (lds_double *)A_generic, *WL = (lds_double *)scratch_generic;
    const int g = (lane >> 4) & 3, c = lane & 15;
    // TEAM == 64: the workgroup is ONE wavefront, whose LDS operations execute in program order -- a read issued after a write of
    // the same wave sees it, so no fence / s_waitcnt stands between the phases below; the compiler only has to keep may-alias
    // LDS accesses in program order, which it does (WL and A are both plain LDS pointers)
    auto lds_fence = [] { asm volatile("" ::: "memory"); };
    // rows 16 TR + 4 v + g of a register exist for every lane group / for none / for some (only when n is not a multiple of 4)
    auto rows_all = [&](int TR, int v) { return 16 * TR + 4 * v + 3 < n; };
    auto rows_none = [&](int TR, int v) { return 16 * TR + 4 * v >= n; };
    const bool in1 = 16 + c <= n;             // this lane's column of tile column 1 exists (b is column n)
    const int c1 = in1 ? 16 + c : 0;
    // ---- the matrix into the accumulator layout, the rows' scale factors one row per lane
    v4d T[2][2];
#pragma unroll
    for (int TR = 0; TR < 2; TR++)
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const int row = 16 * TR + 4 * v + g;
            if (rows_none(TR, v)) { T[TR][0][v] = 0.0; T[TR][1][v] = 0.0; continue; }
            const bool rin = rows_all(TR, v) || row < n;
            const int ro = rin ? row * ld : 0;
            const double a0 = A[ro + c], a1 = A[ro + c1];
            T[TR][0][v] = rin ? a0 : 0.0;
            T[TR][1][v] = (rin && in1) ? a1 : 0.0;
        }
    const bool mine = lane < n;
    const int myrow = (mine ? lane : 0) * ld;     // lanes without a row mirror row 0: finite values that end up nowhere
    double scale = 0.0;
    {
        double s = -1.0;
#pragma unroll
        for (int j = 0; j < N; j++) if (j < n) { const double a = fabs(A[myrow + j]); s = a > s ? a : s; }
        scale = 1.0 / s;
    }
    bool ok = true;
    if (!mine) scale = 0.0;
    const unsigned int lanetag = (unsigned int)(63 - (lane & 63));
    int mycol = -1;
    double rdiag = 0.0;
#pragma unroll
    for (int p = 0; p < N / 4; p++) {
        // 1. the panel's entries of this lane's row
        double cp[4], z[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int t = 0; t < 4; t++) cp[t] = A[myrow + (4 * p + t < n ? 4 * p + t : 0)];
        // 2. / 3. the four pivot steps
        int srcs[4] = {0, 0, 0, 0};
        double b0 = 0.0, b1 = 0.0;
        const bool live0 = 4 * p + 4 < 16;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int k = 4 * p + t;
            if (k < n) {
                const double own_rp = tg_rcp(cp[t]);      // every lane inverts its own candidate while the search runs
                // rows already used as pivots (and lanes without a row) carry scale 0: their key is the bare lane tag
                const float cand = (float)(cp[t] * scale);
                unsigned int key = (__float_as_uint(cand) & 0x7FFFFFC0u) | lanetag;
                key = tg_max_u32_lanes32(key);
                if (!((key & ~0x3Fu) > 0x1E3CE508u)) ok = false;     // scaled pivot <= 1e-20 (compared as bits: non-negative floats)
                const int src = __builtin_amdgcn_readfirstlane(63 - (int)(key & 0x3Fu));
                auto bcast = [&](double v) -> double {
                    const long long b = __double_as_longlong(v);
                    const int lo = __builtin_amdgcn_readlane((int)(b & 0xFFFFFFFFLL), src);
                    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
                    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
                };
                const bool is_piv = lane == src;
                if (TRACE && on && ok && is_piv) trace[k] = lane;
                srcs[t] = src;
                if (t == 3 || k == n - 1) {
                    // lane group t fetches pivot row r_t of the image (as of the panel's start) as its B operand: requested
                    // here, as soon as the last pivot row is known, so that the loads travel under the last elimination step
                    const int prow = (g == 0 ? srcs[0] : (g == 1 ? srcs[1] : (g == 2 ? srcs[2] : srcs[3]))) * ld;
                    b1 = A[prow + c1];
                    if (live0) b0 = A[prow + c];
                }
                const double rp = bcast(own_rp);
                // branch-free: a divergent if / else costs more (exec bookkeeping, two skipped-block branches) than three selects
                const double l = is_piv ? 0.0 : cp[t] * -rp;
#pragma unroll
                for (int t2 = t + 1; t2 < 4; t2++) cp[t2] = fma(l, bcast(cp[t2]), cp[t2]);
#pragma unroll
                for (int s = 0; s < t; s++) z[s] = fma(l, bcast(z[s]), z[s]);
                z[t] = l;
                mycol = is_piv ? k : mycol;
                rdiag = is_piv ? own_rp : rdiag;
                scale = is_piv ? 0.0 : scale;
            }
        }
        // 4. Z -> A-operand form; pivot rows from the LDS image (as of the panel's start); trailing update; write back
        //    (tile column 0 is dead once the panel has passed column 11)
        if (lane < 32) {
#pragma unroll
            for (int t = 0; t < 4; t++) WL[lane * 4 + t] = z[t];
        }
        lds_fence();
        const double a0 = WL[c * 4 + g], a1 = WL[(16 + c) * 4 + g];
        if (!in1) b1 = 0.0;
        if (live0) {
            T[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, T[0][0], 0, 0, 0);
            T[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, T[1][0], 0, 0, 0);
        }
        T[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, T[0][1], 0, 0, 0);
        T[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, T[1][1], 0, 0, 0);
        lds_fence();      // every lane has its operands before the image changes
        auto write_back = [&](int TC) {
#pragma unroll
            for (int TR = 0; TR < 2; TR++)
#pragma unroll
                for (int v = 0; v < 4; v++) {
                    const int row = 16 * TR + 4 * v + g;
                    if (!rows_none(TR, v) && (rows_all(TR, v) || row < n)) A[row * ld + 16 * TC + c] = T[TR][TC][v];
                }
        };
        if (live0) write_back(0);
        if (in1) write_back(1);
        lds_fence();
    }
    // x = b / pivot, row by row: the right-hand side is column n of the image
    const double xr = A[myrow + n] * rdiag;
    lds_fence();
    if (on && mine && ok && mycol >= 0) A[mycol * ld + n] = xr;
    __syncthreads();
    return ok;
}
// ---- gj_panel for MANY right-hand sides (the derivative solves: n <= 31 rows, [A | B] with w <= 16 NTC columns) ------------
//      The same panels, pivot rule and block update as gj_panel, with NTC tile columns in the accumulator layout (two tile
//      rows x NTC tiles x 4 doubles per lane) instead of two: every right-hand side rides in the rank-4 matrix-core update
//      (2 NTC v_mfma_f64_16x16x4 per panel for ~110 columns, where gj_cols spends 28 x 56 lane-wide FMAs plus the pivot-column
//      traffic per PIVOT step).  The LDS image [n][ld] is refreshed after every panel (live tile columns only); at the end every
//      lane scales its entries by the reciprocal pivot of their row and stores them in the row of the variable that row solved:
//      A[i][n + j] = x_i of right-hand side j, like gauss_jordan() / gj_cols.  `scratch`: 128 + 64 doubles of LDS outside the image.
template <int N, int NTC>
__device__ __noinline__ bool gj_panel_rhs(bool on, double *A_generic, int n, int w, int ld, int lane, double *scratch_generic) {
    static_assert(N % 4 == 0 && N > 16 && N <= 32 && NTC >= 2 && NTC <= 8, "gj_panel_rhs: 16 < N <= 32, 32 .. 128 columns");
    typedef __attribute__((address_space(3))) double lds_double;
    typedef double v4d __attribute__((ext_vector_type(4)));
    lds_double *A = (lds_double *)A_generic, *WL = (lds_double *)scratch_generic, *RD = WL + 128;
    __attribute__((address_space(3))) int *MC = (__attribute__((address_space(3))) int *)(WL + 160);
    const int g = (lane >> 4) & 3, c = lane & 15;
    auto lds_fence = [] { asm volatile("" ::: "memory"); };
    auto rows_all = [&](int TR, int v) { return 16 * TR + 4 * v + 3 < n; };
    auto rows_none = [&](int TR, int v) { return 16 * TR + 4 * v >= n; };
    // ---- [A | B] into the accumulator layout
    v4d T[2][NTC];
#pragma unroll
    for (int TR = 0; TR < 2; TR++)
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const int row = 16 * TR + 4 * v + g;
            const bool rin = !rows_none(TR, v) && (rows_all(TR, v) || row < n);
#pragma unroll
            for (int TC = 0; TC < NTC; TC++) {
                const int col = 16 * TC + c;
                const bool in = rin && col < w;
                const double a = A[in ? row * ld + col : 0];
                T[TR][TC][v] = in ? a : 0.0;
            }
        }
    const bool mine = lane < n;
    const int myrow = (mine ? lane : 0) * ld;
    double scale = 0.0;
    {
        double s = -1.0;
#pragma unroll
        for (int j = 0; j < N; j++) if (j < n) { const double a = fabs(A[myrow + j]); s = a > s ? a : s; }
        scale = 1.0 / s;
    }
    bool ok = true;
    if (!mine) scale = 0.0;
    const unsigned int lanetag = (unsigned int)(63 - (lane & 63));
    int mycol = -1;
    double rdiag = 0.0;
#pragma unroll
    for (int p = 0; p < N / 4; p++) {
        double cp[4], z[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int t = 0; t < 4; t++) cp[t] = A[myrow + (4 * p + t < n ? 4 * p + t : 0)];
        int srcs[4] = {0, 0, 0, 0};
        const int TC0 = (4 * p + 4) >> 4;        // first tile column with columns right of this panel
        double bop[NTC];
#pragma unroll
        for (int TC = 0; TC < NTC; TC++) bop[TC] = 0.0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int k = 4 * p + t;
            if (k < n) {
                const double own_rp = tg_rcp(cp[t]);
                const float cand = (float)(cp[t] * scale);
                unsigned int key = (__float_as_uint(cand) & 0x7FFFFFC0u) | lanetag;
                key = tg_max_u32_lanes32(key);
                if (!((key & ~0x3Fu) > 0x1E3CE508u)) ok = false;
                const int src = __builtin_amdgcn_readfirstlane(63 - (int)(key & 0x3Fu));
                auto bcast = [&](double v) -> double {
                    const long long b = __double_as_longlong(v);
                    const int lo = __builtin_amdgcn_readlane((int)(b & 0xFFFFFFFFLL), src);
                    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
                    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
                };
                const bool is_piv = lane == src;
                srcs[t] = src;
                if (t == 3 || k == n - 1) {   // B operands: lane group t takes pivot row r_t of the image as of the panel's start
                    const int prow = (g == 0 ? srcs[0] : (g == 1 ? srcs[1] : (g == 2 ? srcs[2] : srcs[3]))) * ld;
#pragma unroll
                    for (int TC = 0; TC < NTC; TC++) if (TC >= TC0) { const int col = 16 * TC + c; bop[TC] = A[prow + (col < w ? col : 0)]; }
                }
                const double rp = bcast(own_rp);
                const double l = is_piv ? 0.0 : cp[t] * -rp;
#pragma unroll
                for (int t2 = t + 1; t2 < 4; t2++) cp[t2] = fma(l, bcast(cp[t2]), cp[t2]);
#pragma unroll
                for (int s = 0; s < t; s++) z[s] = fma(l, bcast(z[s]), z[s]);
                z[t] = l;
                mycol = is_piv ? k : mycol;
                rdiag = is_piv ? own_rp : rdiag;
                scale = is_piv ? 0.0 : scale;
            }
        }
        if (lane < 32) {
#pragma unroll
            for (int t = 0; t < 4; t++) WL[lane * 4 + t] = z[t];
        }
        lds_fence();
        const double a0 = WL[c * 4 + g], a1 = WL[(16 + c) * 4 + g];
#pragma unroll
        for (int TC = 0; TC < NTC; TC++) if (TC >= TC0) {
            const double b = 16 * TC + c < w ? bop[TC] : 0.0;
            T[0][TC] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, T[0][TC], 0, 0, 0);
            T[1][TC] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, T[1][TC], 0, 0, 0);
        }
        lds_fence();
        if (p + 1 < N / 4) {        // refresh the image (the last panel's result leaves through the scaled store below)
#pragma unroll
            for (int TC = 0; TC < NTC; TC++) if (TC >= TC0 && 16 * TC + c < w) {
#pragma unroll
                for (int TR = 0; TR < 2; TR++)
#pragma unroll
                    for (int v = 0; v < 4; v++) {
                        const int row = 16 * TR + 4 * v + g;
                        if (!rows_none(TR, v) && (rows_all(TR, v) || row < n)) A[row * ld + 16 * TC + c] = T[TR][TC][v];
                    }
            }
        }
        lds_fence();
    }
    // x = B / pivot, row by row, into the row of the variable each row solved
    if (mine) { RD[lane] = rdiag; MC[lane] = mycol; }
    lds_fence();
    if (on && ok) {
#pragma unroll
        for (int TR = 0; TR < 2; TR++)
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const int row = 16 * TR + 4 * v + g;
                if (rows_none(TR, v) || !(rows_all(TR, v) || row < n)) continue;
                const double rd = RD[row];
                const int mc = MC[row];
#pragma unroll
                for (int TC = 0; TC < NTC; TC++) {
                    const int col = 16 * TC + c;
                    if (col >= n && col < w && mc >= 0) A[mc * ld + col] = T[TR][TC][v] * rd;
                }
            }
    }
    TG_SYNC();
    return ok;
}

// ---- Gauss-Jordan with two matrix COLUMNS PER LANE in registers: few rows, many right-hand sides --------------
//      (the derivative solves: n <= NR <= 32 rows, up to 128 columns [A | rhs]).  Lane c holds columns c and
//      c + 64 of every row.  Per pivot column k: lane k publishes its column in LDS (NR doubles); lane i < NR
//      scales entry i and one 32-bit wave max picks the pivot row r; every lane reads the multipliers back with
//      uniform (broadcast) LDS reads.  Rows never move and r is only known at run time, so a lane picks its
//      pivot-row entries with a 0/1-weighted FMA sum over its rows instead of an indexed register read.  The
//      matrix itself never touches LDS during the elimination.  Leaves x_i in A[i*ld + n + rhs] like
//      gauss_jordan().  `scal` is 4*NR doubles of scratch (scale factors, pivot reciprocals, row -> variable
//      map, current column).
template <int TEAM, int NR>
__device__ TG_GJ_ATTR bool gj_cols(bool on, double *A_generic, int n, int w, int ld, double *scal_generic, int lane) {
    typedef __attribute__((address_space(3))) double lds_double;
    lds_double *A = (lds_double *)A_generic, *scal = (lds_double *)scal_generic;
    lds_double *dinv = scal + NR;                      // pivot reciprocal of physical row i
    double a0[NR], a1[NR];
    const bool c0 = on && lane < w, c1 = on && lane + 64 < w;
    // implicit scaling factors 1 / max_j |a_ij| over the matrix columns: lane i < n owns row i
    if (on && lane < NR) {
        double s = -1.0;
        if (lane < n) for (int j = 0; j < n; j++) { const double v = fabs(A[lane * ld + j]); s = v > s ? v : s; }
        scal[lane] = lane < n ? 1.0 / s : 0.0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
#pragma unroll
    for (int i = 0; i < NR; i++) {
        a0[i] = (c0 && i < n) ? A[i * ld + lane] : 0.0;
        a1[i] = (c1 && i < n) ? A[i * ld + lane + 64] : 0.0;
    }
    bool ok = true;
    unsigned int used = 0u;
    lds_double *colbuf = scal + 3 * NR;                // column k of the current step, published by its lane
    for (int k = 0; k < n; k++) {
        if (lane == k) {
#pragma unroll
            for (int i = 0; i < NR; i++) colbuf[i] = a0[i];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
        // scaled pivot search, one row per lane: the magnitude only ranks candidates, so single precision with the
        // lane in the low mantissa bits and one 32-bit wave max (scal is 0 for padding rows)
        float mf = 0.0f;
        if (lane < NR && !((used >> lane) & 1u)) mf = (float)(fabs(colbuf[lane]) * scal[lane]);
        const unsigned int key = __ockl_wfred_max_u32((__float_as_uint(mf) & ~0x3Fu) | (unsigned int)(63 - lane));
        const int r = __builtin_amdgcn_readfirstlane(63 - (int)(key & 0x3Fu));
        if (on && ok && !(__uint_as_float(key & ~0x3Fu) > 1.0e-20f)) ok = false;
        used |= 1u << r;
        // the pivot column in registers first (wave-uniform addresses: LDS broadcasts, all in flight together): a load inside
        // a `(i == r) ? .. : ..` arm turns into a scalar branch with its own s_waitcnt per row
        double cb[NR];
#pragma unroll
        for (int i = 0; i < NR; i++) cb[i] = colbuf[i];
        // this lane's pivot-row entries and the pivot: r is wave-uniform but not a compile-time register index, so a chain of
        // uniform branches picks them (a 0/1-weighted FMA sum is NR dependent fp64 FMAs at ~30 cycles each)
        double p0 = 0.0, p1 = 0.0, piv = 1.0;
#pragma unroll
        for (int i = 0; i < NR; i++) if (i == r) { p0 = a0[i]; p1 = a1[i]; piv = cb[i]; }
        double inv = tg_rcp(piv);
        if (lane == 0 && on) { ((__attribute__((address_space(3))) int *)(scal + 2 * NR))[r] = k; dinv[r] = 1.0 / piv; }
        const double ginv = (on && ok) ? inv : 0.0;
#pragma unroll
        for (int i = 0; i < NR; i++) {
            const double l = cb[i] * ((i == r) ? 0.0 : ginv);
            a0[i] = fma(-l, p0, a0[i]); a1[i] = fma(-l, p1, a1[i]);
        }
        // the next step overwrites colbuf: its reads above are ordered before those writes (same wavefront, in-order LDS)
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    // physical row i solved variable var_i; write x = a / pivot into the row of the variable (right-hand sides only)
    if (on && ok) {
        const __attribute__((address_space(3))) int *var = (const __attribute__((address_space(3))) int *)(scal + 2 * NR);
#pragma unroll
        for (int i = 0; i < NR; i++) {
            if (i < n) {
                const int v = var[i];
                const double d = dinv[i];
                if (c0 && lane >= n) A[v * ld + lane] = a0[i] * d;
                if (c1) A[v * ld + lane + 64] = a1[i] * d;
            }
        }
    }
    TG_SYNC();
    return ok;
}

}  // namespace tg
#endif
