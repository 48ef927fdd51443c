// lanes.hpp -- what the kernels use to talk across the lanes of a team: the phase-boundary fences (TG_SYNC / TG_WSYNC), the DPP and
// v_readlane moves on doubles, the 32-lane maximum and the team arg-max, and the refined reciprocal the register solvers share.
// Nothing here reads the schedule, the launch arguments or Core; the solver headers (bbd_solve.hpp, gj_solve.hpp) need only this file.
// Compiled by hipcc and, with TEAM = 1, by g++ for the host emulation of the CPU tests (the device-only parts are guarded).
#pragma once

#if defined(__HIPCC__)
#define TG_HD __host__ __device__ __forceinline__
// Phase boundary.  Lanes of a team exchange data through LDS only, so the fence is restricted to the LDS address
// space: a plain __syncthreads() also waits for every outstanding GLOBAL store (s_waitcnt vmcnt(0)), which puts
// the HBM write latency of the result rows on the critical path of the next phase.
// Helper waves (-DTG_HELPER_WAVES=n, system-specialised builds of full-wave teams): the second-derivative kernel runs n wavefronts per
// trajectory.  Wave 0 owns every wave-scoped phase (sweeps, register solvers, DPP searches); the flat pair / tile loops -- which
// only read LDS tables and accumulate with LDS atomics -- are shared by all n waves (TG_FORW) between workgroup barriers (TG_WSYNC).
// A phase boundary INSIDE wave 0's part must then not be a workgroup barrier: TG_SYNC becomes a wave-local fence (in a one-wave
// workgroup that is all s_barrier ever was).
#if defined(__HIP_DEVICE_COMPILE__)
#define TG_WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local"); __builtin_amdgcn_s_barrier(); \
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local"); } while (0)
// TG_RSYNC: the phase boundary of code that only the ROLLOUT runs (eval_world, newton_matrix_world, the rollout loop of
// run_trajectory, pose_sweep_dual on the rollout's lists).  In a build with helper waves the team is a full wavefront and the rollout's
// workgroup is that one wave: nobody else reads its LDS slice, and the LDS operations of a wave execute in the order they were issued.  A
// wavefront-scope fence is then enough -- it orders the compiler's accesses and emits no instruction, where each workgroup-scope release
// drains every LDS operation in flight (s_waitcnt lgkmcnt(0)); a read is still waited for, counted, before its value is used.
// Everywhere else it is TG_SYNC.
#if defined(TG_HELPER_WAVES)
#define TG_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local"); __builtin_amdgcn_wave_barrier(); \
                       __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local"); } while (0)
#define TG_RSYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local"); __builtin_amdgcn_wave_barrier(); \
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local"); } while (0)
#else
#define TG_SYNC() TG_WSYNC()
#define TG_RSYNC() TG_SYNC()
#endif
#else
#define TG_SYNC() ((void)0)
#define TG_WSYNC() ((void)0)
#define TG_RSYNC() ((void)0)
#endif
#else
#define TG_HD inline
#define TG_SYNC() ((void)0)
#define TG_WSYNC() ((void)0)
#define TG_RSYNC() ((void)0)
#endif

#if defined(__HIPCC__)
// ROCm device-library wavefront reduction (DPP based); declared in hip/amd_detail only behind an opt-in macro
extern "C" __device__ __attribute__((const)) unsigned long long __ockl_wfred_max_u64(unsigned long long);
extern "C" __device__ __attribute__((const)) unsigned int __ockl_wfred_max_u32(unsigned int);
#endif

#if defined(__HIP_DEVICE_COMPILE__)
// 1/p to full precision: hardware seed (4.6e-8 relative, tools/micro/rcp_f64_accuracy.hip) and ONE cubic refinement
// r (1 + e + e^2), e = 1 - p r: three dependent fp64 operations instead of the four of two Newton steps (a dependent fp64
// operation costs ~30 cycles on this part); the error is e^3 ~ 1e-22 plus rounding.
__device__ __forceinline__ double tg_rcp(double p) {
    const double r = __builtin_amdgcn_rcp(p);
    const double e = fma(-p, r, 1.0);
    return fma(r, fma(e, e, e), r);
}
// max over lanes 0..31 of a wavefront (the register solvers hold at most 32 rows): four row-shift steps leave each 16-lane
// row's maximum in its last lane; the two row maxima are combined on the scalar unit.  Two DPP steps shorter than the
// library's full-wave reduction, and this sits on the critical path of every pivot step.
__device__ __forceinline__ unsigned int tg_max_u32_lanes32(unsigned int v) {
    unsigned int t;
    t = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true); v = t > v ? t : v;   // row_shr:1
    t = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true); v = t > v ? t : v;   // row_shr:2
    t = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true); v = t > v ? t : v;   // row_shr:4
    t = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true); v = t > v ? t : v;   // row_shr:8
    const unsigned int a = (unsigned int)__builtin_amdgcn_readlane((int)v, 15), b = (unsigned int)__builtin_amdgcn_readlane((int)v, 31);
    return a > b ? a : b;
}
#endif

namespace tg {
// lane K of every quad (four neighbouring lanes) to the whole quad: two 32-bit DPP moves (quad_perm has no 64-bit form)
#if defined(__HIP_DEVICE_COMPILE__)
template <int CTRL> __device__ __forceinline__ double tg_dpp_f64(double x) {      // any DPP control on a double (lanes without a source read 0)
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double tg_readlane_f64(double x, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}
template <int K> __device__ __forceinline__ double tg_quad_bcast(double x) {
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(0, lo, K * 0x55, 0xF, 0xF, true);     // (bound_ctrl: no tied `old` operand, hence no copy ahead of the move)
    hi = __builtin_amdgcn_update_dpp(0, hi, K * 0x55, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
#endif

// smallest c with 2^c >= cols, capped at log2(TEAM)
template <int TEAM>
TG_HD int tile_log2(int cols) {
    int c = 0;
    while ((1 << c) < cols && (1 << c) < TEAM) c++;
    return c;
}

// arg-max over the team; ties resolve to the smaller index (first maximum, as a serial scan finds)
template <int TEAM>
TG_HD void team_argmax(double &v, int &i) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int m = TEAM / 2; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(v, m, TEAM);
        const int oi = __shfl_xor(i, m, TEAM);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
#else
    (void)v; (void)i;
#endif
}

}  // namespace tg
