#!/usr/bin/env python3
"""Measurement record of the batched computed torque (BatchMidpointVI.dynamics_inverse_device, k_dyn_inverse) on the two puppets:
puppet_forces (22 dynamic configs, 18 inputs, rank deficient: ridge 1e-4) and puppet40 (22 dynamic and 18 kinematic configs, 6
constraints), --batch x --states states each (recorded poses plus noise, rates and accelerations of order one, as the tests draw them),
every array on the device, one launch per call with all five outputs and the status words.  Per system: the kernel time from
tg_batch_timing (HIP events on the batch's stream around the launch), the median over --launches launches after --warmup, with the
spread; the bytes written, from the shapes.  Next to it, in the same process:
  the forward kernel (tg_batch_dynamics_device, MODE_DYNAMICS) on the same states, a batch of batch x states trajectories, timed the
  same way: the same evaluation phases plus the assembly of M, against the assembly of A -- and a solve of size nd + nc against one of
  nd + nu + nc;
  a device-to-device copy of the bytes the computed-torque launch writes (tg_copy_rows, wall clock around the copy and a device
  synchronisation).
Writes profiles/dynamics_inverse.json.  It gates nothing; anything that could not be run is recorded as "not measured".

    python tools/dynamics_inverse_bench.py [--cpu-only] [--batch 8192] [--states 25] [--out profiles/dynamics_inverse.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SYSTEMS = (("puppet_forces", 1e-4), ("puppet40", 0.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dynamics_inverse.json"))
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--states", type=int, default=25)
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import common
    import dynamics_inverse_reference as dr

    out = dict(batch=args.batch, states_per_trajectory=args.states, device="not measured", systems="not measured")
    if not args.cpu_only:
        from trep_amd import BatchMidpointVI, _lib
        L = _lib.lib()
        B, M = args.batch, args.states
        rows = B * M
        systems_out = {}
        for name, ridge in SYSTEMS:
            system = common.build(name)[0]
            Q, dQ, ddQ = dr.draw_states(name, B, M, 0)
            mvi = BatchMidpointVI(system, B, specialize=False)
            nq, nd, nu, nc, nk = mvi.nq, mvi.nd, mvi.nu, mvi.nc, mvi.nk
            Q_dev, dQ_dev, ddQ_dev = mvi.device_array(Q), mvi.device_array(dQ), mvi.device_array(ddQ)
            per_state = nu + nc + nd + nd + nc            # U, lam, rho, tau, acc (the status word on top: 4 bytes)
            whole = mvi.device_empty(per_state * rows)      # one block, the outputs behind one another: the copy's target afterwards
            at, bufs = whole, []
            for width in (nu, nc, nd, nd, nc):
                bufs.append(at if width else None)
                at += 8 * width * rows
            words = L.tg_device_alloc(0, 4 * rows)
            assert words
            call = lambda: mvi.dynamics_inverse_device(M, Q_dev, dQ_dev, ddQ_dev, None, None, None, ridge, bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], words)

            def timed(batch, fn):
                batch.timing(reset=True)
                for _ in range(args.warmup):
                    fn()
                batch.timing(reset=True)
                ms = []
                for _ in range(args.launches):
                    fn()
                    n, t = batch.timing(reset=True)
                    assert n == 1
                    ms.append(t)
                batch.synchronize()
                return ms
            ms = timed(mvi, call)
            status = np.zeros(rows, dtype=np.int32)
            _lib.check(L.tg_memcpy_d2h(0, status.ctypes.data, words, 4 * rows))
            rho = mvi.download(bufs[2], (rows, nd))
            tau = mvi.download(bufs[3], (rows, nd))
            # the copy of the same bytes
            src = mvi.device_empty(per_state * rows)
            copy_ms = []
            for i in range(args.warmup + args.launches):
                _lib.check(L.tg_device_synchronize(0))
                t0 = time.perf_counter()
                _lib.check(L.tg_copy_rows(0, B, per_state * M, None, None, src, whole))
                _lib.check(L.tg_device_synchronize(0))
                if i >= args.warmup:
                    copy_ms.append(1e3 * (time.perf_counter() - t0))
            team = mvi.kernel_info()["team"]
            lds = np.zeros(4, dtype=np.int32)
            L.tg_system_dynamics_inverse_lds(mvi._sys_h, lds.ctypes.data_as(_lib._c_ip))
            L.tg_device_free(0, words)
            mvi.close()
            # the forward kernel on the same states: one trajectory per state
            fwd = BatchMidpointVI(system, rows, specialize=False)
            q_f, dq_f = fwd.device_array(Q.reshape(rows, nq)), fwd.device_array(dQ.reshape(rows, nq))
            k_f = fwd.device_array(ddQ.reshape(rows, nq)[:, nd:]) if nk else None
            u_f = fwd.device_array(np.zeros((rows, nu))) if nu else None
            ddq_f, lam_f = fwd.device_empty(rows * nd), (fwd.device_empty(rows * nc) if nc else None)
            fwd_ms = timed(fwd, lambda: _lib.check(L.tg_batch_dynamics_device(fwd._h, q_f, dq_f, u_f, k_f, ddq_f, lam_f, None)))
            fwd.close()
            med, cmed, fmed = float(np.median(ms)), float(np.median(copy_ms)), float(np.median(fwd_ms))
            nbytes = 8 * per_state * rows + 4 * rows
            systems_out[name] = dict(
                nq=nq, nd=nd, nu=nu, nc=nc, ridge=ridge, team=team, lds_doubles_per_team=int(lds[1]), lds_bytes_per_workgroup=int(lds[2]),
                image_size=nd + nu + nc, forward_image_size=nd + nc, states=rows, bytes_written=nbytes, bytes_read=3 * 8 * nq * rows,
                launches=len(ms), kernel_ms_median=med, kernel_ms_min=float(min(ms)), kernel_ms_max=float(max(ms)), states_per_s=rows / (1e-3 * med),
                forward_kernel_ms_median=fmed, forward_kernel_ms_min=float(min(fwd_ms)), forward_kernel_ms_max=float(max(fwd_ms)),
                kernel_over_forward=med / fmed, copy_ms_median=cmed, copy_ms_min=float(min(copy_ms)), copy_ms_max=float(max(copy_ms)),
                kernel_over_copy=med / cmed, status_ok=int((status == 0).sum()), rho_inf=float(np.abs(rho).max()), tau_inf=float(np.abs(tau).max()))
            print(name, systems_out[name], flush=True)
        out.update(device="MI355X", systems=systems_out,
                   copy_note="tg_copy_rows of the byte count of the five double outputs, wall clock around the copy and a device synchronisation; it reads as much as it writes",
                   forward_note="tg_batch_dynamics_device on batch x states trajectories, u = 0, the same q, dq and kinematic accelerations; HIP events like the kernel's")
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
