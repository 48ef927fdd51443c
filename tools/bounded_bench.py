#!/usr/bin/env python3
"""Measurement record of the bounded computed-torque kernel against the rank-revealing one it is built around
(BatchMidpointVI.dynamics_inverse_device with bounds_dev= and with rcond= alone; k_dyn_inverse, BND and LSQ), by the protocol of
tools/min_norm_bench.py: --batch x --states states on the device (recorded poses plus noise, rates and accelerations of order one),
one launch per call with all five outputs, the status and the rank words on the same states (active and solves on top for the new
kernel), the kernel time from tg_batch_timing (HIP events on the batch's stream around the launch), the median over --launches
launches after --warmup, with the spread.  puppet40 at ridge 0 with tension bounds; puppet_forces at ridge 1e-4 with the box of
tests/bounded_reference.py's table (tension bounds and |u_i| <= half the median |u| of the unbounded answer, taken from the first
--box-states states).  Every timing comes with the histogram of `solves`.  Writes profiles/bounded_bench.json.  It gates nothing;
anything that could not be run is recorded as "not measured".

    python tools/bounded_bench.py [--cpu-only] [--batch 8192] [--states 25] [--out profiles/bounded_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SYSTEMS = (("puppet40", 0.0, "tension"), ("puppet_forces", 1e-4, "tension+inputs"))
RCOND = 1e-9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bounded_bench.json"))
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--states", type=int, default=25)
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--box-states", type=int, default=4096)
    args = ap.parse_args()
    import numpy as np
    import common
    import dynamics_inverse_reference as dr

    out = dict(batch=args.batch, states_per_trajectory=args.states, rcond=RCOND, device="not measured", systems="not measured",
               early_exit_vote=True)
    if not args.cpu_only:
        from trep_amd import BatchMidpointVI, _lib
        L = _lib.lib()
        B, M = args.batch, args.states
        rows = B * M
        systems_out = {}
        for name, ridge, rule in SYSTEMS:
            system = common.build(name)[0]
            Q, dQ, ddQ = dr.draw_states(name, B, M, 0)
            mvi = BatchMidpointVI(system, B, specialize=False)
            nd, nu, nc = mvi.nd, mvi.nu, mvi.nc
            n = nu + nc
            Q_dev, dQ_dev, ddQ_dev = mvi.device_array(Q), mvi.device_array(dQ), mvi.device_array(ddQ)
            widths = (nu, nc, nd, nd, nc)
            bufs = [mvi.device_empty(w * rows) if w else None for w in widths]
            words = {k: L.tg_device_alloc(0, 4 * rows * w) for k, w in (("status", 1), ("rank", 1), ("solves", 1), ("active", n))}
            assert all(words.values())
            lsq = lambda: mvi.dynamics_inverse_device(M, Q_dev, dQ_dev, ddQ_dev, None, None, None, ridge, *bufs, words["status"], rcond=RCOND,
                                                      rank_dev=words["rank"])

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

            def ints(key, width=1):
                a = np.zeros(rows * width, dtype=np.int32)
                _lib.check(L.tg_memcpy_d2h(0, a.ctypes.data, words[key], 4 * a.size))
                return a
            ms_lsq = timed(lsq)
            u_free = mvi.download(bufs[0], (rows, nu)) if nu else np.zeros((rows, 0))
            lo, hi = mvi.tension_bounds("dynamics_inverse")
            if rule == "tension+inputs":
                half = 0.5 * float(np.median(np.abs(u_free[:args.box_states])))
                lo[:nu], hi[:nu] = -half, half
            box = (mvi.device_array(lo[None]), mvi.device_array(hi[None]), 1)
            bnd = lambda: mvi.dynamics_inverse_device(M, Q_dev, dQ_dev, ddQ_dev, None, None, None, ridge, *bufs, words["status"], rcond=RCOND,
                                                      rank_dev=words["rank"], bounds_dev=box, active_dev=words["active"], solves_dev=words["solves"])
            ms_bnd = timed(bnd)
            solves, status, active = ints("solves"), ints("status"), ints("active", n).reshape(rows, n)
            lds = np.zeros(4, dtype=np.int32)
            row = dict(nd=nd, nu=nu, nc=nc, n=n, ridge=ridge, box=rule, team=mvi.kernel_info()["team"], states=rows,
                       lsq_ms_median=float(np.median(ms_lsq)), lsq_ms_min=float(min(ms_lsq)), lsq_ms_max=float(max(ms_lsq)),
                       bounded_ms_median=float(np.median(ms_bnd)), bounded_ms_min=float(min(ms_bnd)), bounded_ms_max=float(max(ms_bnd)),
                       bounded_over_lsq=float(np.median(ms_bnd)) / float(np.median(ms_lsq)),
                       bounded_states_per_s=rows / (1e-3 * float(np.median(ms_bnd))),
                       solves_histogram={str(int(k)): int(v) for k, v in zip(*np.unique(solves, return_counts=True))},
                       solves_mean=float(solves.mean()), solves_max=int(solves.max()),
                       status_histogram={str(int(k)): int(v) for k, v in zip(*np.unique(status, return_counts=True))},
                       states_with_an_active_bound=int((active != 0).any(axis=1).sum()))
            L.tg_system_dynamics_inverse_lsq_lds(mvi._sys_h, lds.ctypes.data_as(_lib._c_ip))
            row["lsq_lds_bytes_per_workgroup"] = int(lds[2])
            L.tg_system_dynamics_inverse_bounded_lds(mvi._sys_h, lds.ctypes.data_as(_lib._c_ip))
            row["bounded_lds_bytes_per_workgroup"] = int(lds[2])
            for w in words.values():
                L.tg_device_free(0, w)
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
