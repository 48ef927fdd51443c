#!/usr/bin/env python3
"""Parity record of the batched constraint projection (BatchMidpointVI.satisfy_constraints): runs the case table of the tests
(tests/projection_reference.py::CASES) and writes, per case,

    floor            -- max |q_ref(tolerance 1e-10) - q_ref(tolerance 1e-13)| of the numpy reference: what the stopping rule leaves open
    bound            -- 64 max(floor, 1e-13): the bound on |q - q_ref|
    reference_steps  -- the most Newton steps the reference takes on a row of the case
    emulation_error / emulation_steps / emulation_residual -- worst |q - q_ref|, most steps and the worst answer residual (in its
                        bounds, tests/projection_reference.py::residuals) of the kernel compiled for the host (one lane)
    device_error / device_steps / device_residual -- the same of the kernel on the GPU at the system's own team size (null: not measured)

to profiles/projection_parity.json.

    python tools/projection_parity.py [--cpu-only] [--out profiles/projection_parity.json]

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projection_parity.json"))
    ap.add_argument("--cpu-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import common
    import emu_pose_harness
    import projection_reference as pr

    def measured(name, case, got, ref):
        Q0, dQ0, free = pr.case_inputs(*case)
        return float(np.abs(got.Q - ref.Q).max()), int(got.iterations.max()), pr.worst(pr.residuals(name, Q0, dQ0, free, got))

    cases = {}
    for case in pr.CASES:
        name, mask, noise = case
        Q0, dQ0, free = pr.case_inputs(*case)
        ref = pr.case_reference(*case)
        row = dict(system=name, mask=mask, noise=noise, rows=len(Q0), floor=pr.case_floor(*case), bound=pr.case_bound(*case),
                   reference_steps=int(ref.iterations.max()))
        emu = emu_pose_harness.EmuProjection(common.build(name)[1]).project(Q0, dQ0, free, tolerance=pr.TOL)
        row["emulation_error"], row["emulation_steps"], row["emulation_residual"] = measured(name, case, emu, ref)
        row["device_error"] = row["device_steps"] = row["device_residual"] = None
        if not args.cpu_only:
            from trep_amd import BatchMidpointVI
            mvi = BatchMidpointVI(common.build(name)[0], len(Q0), specialize=False)
            kw = dict(keep_kinematic=mask == "keep_kinematic", constant_q_list=pr.constant_list(name) if mask == "constant" else None)
            got = mvi.satisfy_constraints(Q0, dQ0, tolerance=pr.TOL, **kw)
            row["device_error"], row["device_steps"], row["device_residual"] = measured(name, case, got, ref)
            mvi.close()
        cases[pr.case_id(case)] = row
        print(pr.case_id(case), row)
    out = dict(tolerance=pr.TOL, margin=pr.MARGIN, device="unmeasured" if args.cpu_only else "MI355X", cases=cases)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
