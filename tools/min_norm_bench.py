#!/usr/bin/env python3
"""Measurement record of the rank-revealing least-squares kernels against the augmented-image ones they stand beside
(BatchMidpointVI.dynamics_inverse_device with and without rcond=; k_dyn_inverse, LSQ and not), by the protocol of
tools/dynamics_inverse_bench.py: --batch x --states states on the device (recorded poses plus noise, rates and accelerations of
order one), one launch per call with all five outputs and the status words (the rank words on top for the new kernel), the kernel
time from tg_batch_timing (HIP events on the batch's stream around the launch), the median over --launches launches after --warmup,
with the spread.  puppet40 at ridge 0 (full rank: both kernels answer the same question) and puppet_forces at ridge 1e-4 (the
existing kernel needs the ridge there); the new kernel on puppet_forces at ridge 0 too, which the existing one cannot run.  Both
kernels run on the same states and write the same outputs; their answers are compared (the worst difference of z relative to
max(1, |z|inf)).  DESIGN.md section 3.7f expected roughly m^3 / (nd n^2) between the two solves; what comes out is recorded whichever
way it points.  Writes profiles/min_norm_bench.json.  It gates nothing; anything that could not be run is recorded as "not measured".

    python tools/min_norm_bench.py [--cpu-only] [--batch 8192] [--states 25] [--out profiles/min_norm_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SYSTEMS = (("puppet40", 0.0, True), ("puppet_forces", 1e-4, True), ("puppet_forces", 0.0, False))     # (name, ridge, the existing kernel runs it)
RCOND = 1e-9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "min_norm_bench.json"))
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--states", type=int, default=25)
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import common
    import dynamics_inverse_reference as dr

    out = dict(batch=args.batch, states_per_trajectory=args.states, rcond=RCOND, device="not measured", systems="not measured")
    if not args.cpu_only:
        from trep_amd import BatchMidpointVI, _lib
        L = _lib.lib()
        B, M = args.batch, args.states
        rows = B * M
        systems_out = {}
        for name, ridge, both in SYSTEMS:
            system = common.build(name)[0]
            Q, dQ, ddQ = dr.draw_states(name, B, M, 0)
            mvi = BatchMidpointVI(system, B, specialize=False)
            nd, nu, nc = mvi.nd, mvi.nu, mvi.nc
            n, m = nu + nc, nd + nu + nc
            Q_dev, dQ_dev, ddQ_dev = mvi.device_array(Q), mvi.device_array(dQ), mvi.device_array(ddQ)
            widths = (nu, nc, nd, nd, nc)
            bufs = [mvi.device_empty(w * rows) if w else None for w in widths]
            words, ranks = L.tg_device_alloc(0, 4 * rows), L.tg_device_alloc(0, 4 * rows)
            assert words and ranks
            old = lambda: mvi.dynamics_inverse_device(M, Q_dev, dQ_dev, ddQ_dev, None, None, None, ridge, *bufs, words)
            new = lambda: mvi.dynamics_inverse_device(M, Q_dev, dQ_dev, ddQ_dev, None, None, None, ridge, *bufs, words, rcond=RCOND, rank_dev=ranks)

            def timed(fn):
                mvi.timing(reset=True)
                for _ in range(args.warmup):
                    fn()
                mvi.timing(reset=True)
                ms = []
                for _ in range(args.launches):
                    fn()
                    count, t = mvi.timing(reset=True)
                    assert count == 1
                    ms.append(t)
                mvi.synchronize()
                return ms

            def answer():
                z = np.concatenate([mvi.download(bufs[i], (rows, widths[i])) if widths[i] else np.zeros((rows, 0)) for i in (0, 1)], axis=1)
                status = np.zeros(rows, dtype=np.int32)
                _lib.check(L.tg_memcpy_d2h(0, status.ctypes.data, words, 4 * rows))
                return z, mvi.download(bufs[2], (rows, nd)), status
            row = dict(nd=nd, nu=nu, nc=nc, n=n, image_size=m, ridge=ridge, team=mvi.kernel_info()["team"], states=rows,
                       expected_ratio_m3_over_nd_n2=float(m) ** 3 / (nd * float(n) ** 2))
            lds = np.zeros(4, dtype=np.int32)
            if both:
                ms_old = timed(old)
                z_old, rho_old, status_old = answer()
                L.tg_system_dynamics_inverse_lds(mvi._sys_h, lds.ctypes.data_as(_lib._c_ip))
                row.update(augmented_ms_median=float(np.median(ms_old)), augmented_ms_min=float(min(ms_old)), augmented_ms_max=float(max(ms_old)),
                           augmented_lds_bytes_per_workgroup=int(lds[2]), augmented_status_ok=int((status_old == 0).sum()))
            ms_new = timed(new)
            z_new, rho_new, status_new = answer()
            rank = np.zeros(rows, dtype=np.int32)
            _lib.check(L.tg_memcpy_d2h(0, rank.ctypes.data, ranks, 4 * rows))
            L.tg_system_dynamics_inverse_lsq_lds(mvi._sys_h, lds.ctypes.data_as(_lib._c_ip))
            row.update(lsq_ms_median=float(np.median(ms_new)), lsq_ms_min=float(min(ms_new)), lsq_ms_max=float(max(ms_new)),
                       lsq_lds_bytes_per_workgroup=int(lds[2]), lsq_status_ok=int((status_new == 0).sum()), lsq_states_per_s=rows / (1e-3 * float(np.median(ms_new))),
                       rank_histogram={str(int(k)): int(v) for k, v in zip(*np.unique(rank, return_counts=True))})
            if both:
                scale = max(1.0, float(np.abs(z_new).max()))
                row.update(augmented_over_lsq=float(np.median(ms_old)) / float(np.median(ms_new)),
                           z_difference=float(np.abs(z_new - z_old).max()) / scale, rho_difference=float(np.abs(rho_new - rho_old).max()) / scale)
            L.tg_device_free(0, words)
            L.tg_device_free(0, ranks)
            mvi.close()
            systems_out["%s_ridge_%g" % (name, ridge)] = row
            print(name, ridge, row, flush=True)
        out.update(device="MI355X", systems=systems_out)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
