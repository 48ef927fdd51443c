#!/usr/bin/env python3
"""Parity record of the batched equilibrium search (BatchMidpointVI.minimize_potential_energy): runs the case table of the tests
(tests/equilibrium_reference.py::CASES) and writes, per case,

    floor            -- max |q_ref(tolerance 1e-10) - q_ref(tolerance 1e-13)| of the numpy reference: what the stopping rule leaves open
    bound            -- 64 max(floor, 1e-13): the bound on |q - q_ref|
    reference_steps  -- the fewest and the most trials the reference makes on a row of the case (the rest row's 0 left out)
    reference_margin -- the reference's smallest relative margin of an accept / reject or Cholesky decision on the case
    thin_rows        -- rows whose margin is under 1e-6 (compared at the end point only)
    draw             -- which draw of the case's seed the table uses
    emulation_error / emulation_mu_error / emulation_v_error / emulation_steps -- worst |q - q_ref|, |mu - mu_ref|,
                        |V - V_ref| / max(1, |V_ref|) and most trials of the kernel compiled for the host (one lane)
    device_error / device_mu_error / device_v_error / device_steps -- the same of the kernel on the GPU at the system's own team
                        size (null: not measured)

and, under "puppet40", how the reference fares on puppet40 under keep_kinematic over three draws of each noise level (rows that
stall: not TG_OK within the budget), to profiles/equilibrium_parity.json.  "throughput" holds poses per second of 8192
puppet_basic poses at 0.02 of noise (null: not measured; no threshold goes with it).

    python tools/equilibrium_parity.py [--cpu-only] [--out profiles/equilibrium_parity.json]

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "equilibrium_parity.json"))
    ap.add_argument("--cpu-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import common
    import emu_pose_harness
    import equilibrium_reference as er

    def measured(got, ref):
        return (float(np.abs(got.Q - ref.Q).max()), float(np.abs(got.mu - ref.mu).max(initial=0.0)),
                float((np.abs(got.V - ref.V) / np.maximum(1.0, np.abs(ref.V))).max()), int(got.iterations.max()))

    def keywords(name, mask):
        return dict(keep_kinematic=mask == "keep_kinematic", constant_q_list=er.CONSTANT[name] if mask == "constant" else None)

    cases = {}
    for case in er.CASES:
        name, mask, noise = case
        Q0, free = er.case_inputs(*case)
        ref = er.case_reference(*case)
        steps = np.delete(ref.iterations, er.EQUILIBRIUM % len(Q0))
        row = dict(system=name, mask=mask, noise=noise, rows=len(Q0), floor=er.case_floor(*case), bound=er.case_bound(*case),
                   reference_steps=[int(steps.min()), int(steps.max())], reference_margin=float(ref.margin.min()),
                   thin_rows=int((~er.firm_rows(ref)).sum()), draw=er.DRAW.get(case, 0),
                   certified=bool(er.certified(name, ref, free).all()))
        emu = emu_pose_harness.EmuEquilibrium(common.build(name)[1]).minimize(Q0, free, tolerance=er.TOL)
        row["emulation_error"], row["emulation_mu_error"], row["emulation_v_error"], row["emulation_steps"] = measured(emu, ref)
        row["device_error"] = row["device_mu_error"] = row["device_v_error"] = row["device_steps"] = None
        if not args.cpu_only:
            from trep_amd import BatchMidpointVI
            mvi = BatchMidpointVI(common.build(name)[0], len(Q0), specialize=False)
            got = mvi.minimize_potential_energy(Q0, tolerance=er.TOL, **keywords(name, mask))
            row["device_error"], row["device_mu_error"], row["device_v_error"], row["device_steps"] = measured(got, ref)
            mvi.close()
        cases[er.case_id(case)] = row
        print(er.case_id(case), row)

    # the open point of the prototype: puppet40 under keep_kinematic
    puppet40 = {}
    for noise in (0.02, 0.1):
        case = ("puppet40", "keep_kinematic", noise)
        keep = er.DRAW.get(case)
        rows = stalled = 0
        for draw in range(3):
            er.DRAW[case] = draw
            er.case_inputs.cache_clear()
            er.case_reference.cache_clear()
            ref = er.case_reference(*case)
            Q0, free = er.case_inputs(*case)
            good = er.certified(case[0], ref, free)
            rows += len(good)
            stalled += int((~good).sum())
        if keep is None:
            del er.DRAW[case]
        else:
            er.DRAW[case] = keep
        er.case_inputs.cache_clear()
        er.case_reference.cache_clear()
        puppet40["%g" % noise] = dict(rows=rows, stalled=stalled, draws=3)
    print("puppet40", puppet40)

    throughput = None
    if not args.cpu_only:
        from trep_amd import BatchMidpointVI
        name, mask, noise = "puppet_basic", "all", 0.02
        B, calls = 8192, 100
        rng = np.random.default_rng(7)
        eq = er.equilibria(name, mask)
        Q = eq[rng.integers(len(eq), size=B)].copy()
        Q += noise * rng.standard_normal(Q.shape)
        mvi = BatchMidpointVI(common.build(name)[0], B, specialize=False)
        for _ in range(10):
            got = mvi.minimize_potential_energy(Q)
        times = []
        for _ in range(10):                         # a sample is `calls` whole calls back to back: about half a second of work
            t0 = time.perf_counter()
            for _ in range(calls):
                got = mvi.minimize_potential_energy(Q)
            times.append((time.perf_counter() - t0) / calls)
        mvi.close()
        med = float(np.median(times))
        throughput = dict(system=name, poses=B, noise=noise, samples=len(times), calls_per_sample=calls, seconds_median=med,
                          seconds_min=float(min(times)), seconds_max=float(max(times)), poses_per_second=B / med,
                          converged=int((got.status == 0).sum()), most_trials=int(got.iterations.max()),
                          includes="per call: host copies in and out, one launch, synchronisation")
        print("throughput", throughput)

    out = dict(tolerance=er.TOL, margin=er.MARGIN, thin=er.THIN, device="unmeasured" if args.cpu_only else "MI355X", cases=cases,
               puppet40=puppet40, throughput=throughput)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
