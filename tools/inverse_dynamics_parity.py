#!/usr/bin/env python3
"""Parity record of the batched inverse dynamics (BatchMidpointVI.inverse_dynamics): runs the case table of the tests
(tests/inverse_dynamics_reference.py::CASES), with and without p0, and writes per case
  the floors e_ref of the specification (its QR and augmented-system solves against each other) and the bound max(1e-10, 64 e_ref),
  the margin |z~|inf the errors are relative to and the largest |rho|,
  the worst error of the emulated kernel (tests/emu_invdyn, TEAM = 1) and of the device per quantity (z~, rho, P, h),
to profiles/inverse_dynamics_parity.json.  "throughput": seconds per call of `inverse_dynamics_device` on puppet-40 paths of
--steps steps for --batch trajectories, Q on the device, one launch and one synchronisation per call.  No figure existed before this
kernel did ("before": unmeasured); it gates nothing.

    python tools/inverse_dynamics_parity.py [--cpu-only] [--batch 8192] [--steps 200] [--out profiles/inverse_dynamics_parity.json]

--cpu-only writes the half that needs no GPU and marks the device fields unmeasured.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inverse_dynamics_parity.json"))
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    import numpy as np
    import common
    import emu_invdyn_harness
    import inverse_dynamics_reference as ir

    cases = {}
    for c in ir.CASES:
        p = ir.case_paths(c)
        dt = ir.step_sizes(c) if c.pattern != "uniform" else ir.DT
        for with_p0 in (True, False):
            ref = ir.case_reference(c, with_p0)
            p0 = p["p0"] if with_p0 else None
            f = ir.floors(ref)
            row = dict(system=c.name, B=c.B, N=c.N, ridge=c.ridge, steps=c.pattern, p0=with_p0, covers=c.covers, floor_z=f["z"], floor_rho=f["rho"],
                       margin=f["scale"], bound=ir.bound(ref), rho_inf=float(np.abs(ref.rho).max(initial=0.0)))
            emu = emu_invdyn_harness.EmuInverse(p["d"]).inverse_dynamics(p["Q"], dt, p0, c.ridge)
            row["emulation_error"] = ir.errors(c, ref, emu)
            row["device_error"] = None
            if not args.cpu_only:
                from trep_amd import BatchMidpointVI
                mvi = BatchMidpointVI(common.build(c.name)[0], c.B, specialize=False)
                row["device_error"] = ir.errors(c, ref, mvi.inverse_dynamics(p["Q"], dt, p0, c.ridge))
                row["team"] = mvi.kernel_info()["team"]
                mvi.close()
            cases["%s_%s" % (ir.case_id(c), "p0" if with_p0 else "no_p0")] = row
            print(ir.case_id(c), row)

    throughput = None
    if not args.cpu_only:
        from trep_amd import BatchMidpointVI, systems
        B, N, dt = args.batch, args.steps, 0.01
        system = systems.puppet()
        Q0 = systems.puppet_initial_conditions(system, B, seed=1)
        K = systems.puppet_string_schedule(system, Q0[:, system.nQd:], N, dt)
        mvi = BatchMidpointVI(system, B)
        mvi.initialize_from_configs(0.0, Q0, dt, Q0)
        X_dev = mvi.device_empty(B * (N + 1) * mvi.nX)
        mvi.rollout_device(N, dt, None, mvi.device_array(K), X_dev)
        mvi.synchronize()
        lam, P, rho = mvi.device_empty(B * N * mvi.nc), mvi.device_empty(B * (N + 1) * mvi.nd), mvi.device_empty(B * N * mvi.nd)
        times = []
        for i in range(8):
            t0 = time.perf_counter()
            mvi.inverse_dynamics_device(N, dt, X_dev, mvi.nX, None, 0.0, None, lam, P, rho)
            mvi.synchronize()
            times.append(time.perf_counter() - t0)
        times = times[3:]
        worst_rho = float(np.abs(mvi.download(rho, (B, N, mvi.nd))).max())
        mvi.close()
        med = float(np.median(times))
        throughput = dict(system="puppet40", trajectories=B, steps=N, samples=len(times), seconds_median=med, seconds_min=float(min(times)),
                          seconds_max=float(max(times)), steps_per_second=B * N / med, rho_inf=worst_rho, before="unmeasured: the kernel is new",
                          includes="per call: one launch reading the rollout's X on the device, synchronisation; no host copies")
        print("throughput", throughput)

    out = dict(tolerance=ir.TOL, margin=ir.MARGIN, device="unmeasured" if args.cpu_only else "MI355X", cases=cases, throughput=throughput)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
