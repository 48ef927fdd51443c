#!/usr/bin/env python3
"""Parity record of the rank-revealing least-squares path of the two inverse questions (BatchMidpointVI.dynamics_inverse and
inverse_dynamics with rcond=): runs both tables of the tests (tests/min_norm_reference.py: CT_CASES, ID_CASES with and without p0)
and writes per case
  the ranks met, the singular-value gap (the least sigma_r / sigma_1 above the cut and the worst sigma_{r+1} / sigma_1 below it),
  the floor e_ref of the specification (its SVD and complete-orthogonal-decomposition routes against each other), the bound
  max(1e-10, 64 e_ref) of z and rho and the bound 1e-10 of the direct quantities, the margin |z|inf the errors are relative to,
  the worst error of the emulated kernel (tests/emu_lsq, TEAM = 1) and of the device per quantity, and whether their ranks are the
  specification's,
to profiles/min_norm_parity.json.  It gates nothing.

    python tools/min_norm_parity.py [--cpu-only] [--out profiles/min_norm_parity.json]

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "min_norm_parity.json"))
    ap.add_argument("--cpu-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import common
    import dynamics_inverse_reference as dr
    import emu_lsq_harness
    import inverse_dynamics_reference as ir
    import min_norm_reference as mr

    def head(ref, **more):
        fl, scale = mr.floor(ref)
        row = dict(ranks=sorted(set(int(r) for r in ref.rank.ravel())), gap_above=None if np.isinf(ref.gap_above) else float(ref.gap_above),
                   gap_below=float(ref.gap_below), floor=fl, margin=scale, bound=mr.bound(ref), bound_direct=mr.TOL_DIRECT, device_error=None,
                   device_rank_equal=None)
        row.update(more)
        return row

    def batch(name, B):
        from trep_amd import BatchMidpointVI
        return BatchMidpointVI(common.build(name)[0], B, specialize=False)
    cases = {}
    for c in mr.CT_CASES:
        base = mr.ct_base(c)
        p, ref = dr.case_states(base), mr.ct_reference(c)
        row = head(ref, table="computed torque", system=c.name, B=base.B, M=base.M, ridge=c.ridge, covers=c.covers)
        run = lambda f: f(p["Q"], p["dQ"], p["ddQ"], c.ridge, rcond=mr.RCOND)
        err = lambda g: (mr.errors(ref, dr.unknowns(g.U, g.lam), g.rho, {"tau": g.tau, "acc": g.acc}), bool(np.array_equal(g.rank, ref.rank)))
        row["emulation_error"], row["emulation_rank_equal"] = err(run(emu_lsq_harness.EmuLsq(p["d"]).dynamics_inverse))
        if not args.cpu_only:
            mvi = batch(c.name, base.B)
            row["device_error"], row["device_rank_equal"] = err(run(mvi.dynamics_inverse))
            row["team"] = mvi.kernel_info()["team"]
            mvi.close()
        cases["ct_" + mr.ct_id(c)] = row
        print(mr.ct_id(c), row, flush=True)
    for c in mr.ID_CASES:
        p = ir.case_paths(c.base)
        nu = int(p["d"].n_inputs)
        dt = p["dts"] if c.base.pattern != "uniform" else ir.DT
        for with_p0 in (True, False):
            ref = mr.id_reference(c, with_p0)
            p0 = p["p0"] if with_p0 else None
            row = head(ref, table="discrete", system=c.base.name, B=c.base.B, N=c.base.N, ridge=c.ridge, pattern=c.base.pattern, p0=with_p0)
            err = lambda g: (mr.errors(ref, ir.impulses(nu, g.U, g.lam, p["dts"]), g.rho, {"P": g.P, "h": g.h}), bool(np.array_equal(g.rank, ref.rank)))
            row["emulation_error"], row["emulation_rank_equal"] = err(emu_lsq_harness.EmuLsq(p["d"]).inverse_dynamics(p["Q"], p["dts"], p0, c.ridge, mr.RCOND))
            if not args.cpu_only:
                mvi = batch(c.base.name, c.base.B)
                row["device_error"], row["device_rank_equal"] = err(mvi.inverse_dynamics(p["Q"], dt, p0, c.ridge, rcond=mr.RCOND))
                row["team"] = mvi.kernel_info()["team"]
                mvi.close()
            key = "id_%s_%s" % (mr.id_id(c), "p0" if with_p0 else "nop0")
            cases[key] = row
            print(key, row, flush=True)

    out = dict(rcond=mr.RCOND, tolerance=mr.TOL, margin=mr.MARGIN, tolerance_direct=mr.TOL_DIRECT, gap_above_required=mr.GAP_ABOVE,
               gap_below_required=mr.GAP_BELOW, device="unmeasured" if args.cpu_only else "MI355X", cases=cases)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
