#!/usr/bin/env python3
"""Parity record of the batched computed torque (BatchMidpointVI.dynamics_inverse): runs the case table of the tests
(tests/dynamics_inverse_reference.py::CASES) and writes per case
  the floors e_ref of the specification (its QR and augmented-system solves against each other), the bound max(1e-10, 64 e_ref) of z
  and rho and the bound 1e-10 of tau and acc,
  the margin |z|inf the errors of z and rho are relative to, the largest |rho| and |tau| and the smallest singular value of A,
  the worst error of the emulated kernel (tests/emu_dyn_inverse, TEAM = 1) and of the device per quantity (z, rho, tau, acc),
to profiles/dynamics_inverse_parity.json.  It gates nothing.

    python tools/dynamics_inverse_parity.py [--cpu-only] [--out profiles/dynamics_inverse_parity.json]

--cpu-only writes the half that needs no GPU and marks the device fields unmeasured.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dynamics_inverse_parity.json"))
    ap.add_argument("--cpu-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import common
    import dynamics_inverse_reference as dr
    import emu_dyn_inverse_harness

    cases = {}
    for c in dr.CASES:
        p = dr.case_states(c)
        ref = dr.case_reference(c)
        f = dr.floors(ref)
        smin = dr.sigma_min(ref)
        row = dict(system=c.name, B=c.B, M=c.M, ridge=c.ridge, draw=c.draw, covers=c.covers, floor_z=f["z"], floor_rho=f["rho"], margin=f["scale"],
                   bound=dr.bound(ref), bound_direct=dr.TOL_DIRECT, rho_inf=float(np.abs(ref.rho).max(initial=0.0)),
                   tau_inf=float(np.abs(ref.tau).max(initial=0.0)), acc_inf=float(np.abs(ref.acc).max(initial=0.0)),
                   sigma_min=None if np.isinf(smin) else smin)
        emu = emu_dyn_inverse_harness.EmuDynInverse(p["d"]).dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], c.ridge)
        row["emulation_error"] = dr.errors(ref, emu)
        row["device_error"] = None
        if not args.cpu_only:
            from trep_amd import BatchMidpointVI
            mvi = BatchMidpointVI(common.build(c.name)[0], c.B, specialize=False)
            row["device_error"] = dr.errors(ref, mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], c.ridge))
            row["team"] = mvi.kernel_info()["team"]
            mvi.close()
        cases[dr.case_id(c)] = row
        print(dr.case_id(c), row, flush=True)

    out = dict(tolerance=dr.TOL, margin=dr.MARGIN, tolerance_direct=dr.TOL_DIRECT, device="unmeasured" if args.cpu_only else "MI355X", cases=cases)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
