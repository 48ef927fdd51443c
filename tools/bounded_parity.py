#!/usr/bin/env python3
"""Parity record of the bounded inverse questions (tests/bounded_reference.py): per case of both tables the floors e_ref, the bound,
the admissibility margins and the coverage of the specification, two mutation factors (one variable wrongly bound; the unbounded answer
clipped to the box -- the error of the mutated answer over the bound, the smallest over the states that have an active bound and,
for clipping, on which clipping is not exact), and the worst error per quantity of the emulated kernels (tests/emu_bvls) and of the
device, with the histogram of `solves`.  Writes profiles/bounded_parity.json.  It gates nothing (the tests do); anything that could
not be run is recorded as "not measured".

    python tools/bounded_parity.py [--cpu-only] [--out profiles/bounded_parity.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bounded_parity.json"))
    ap.add_argument("--cpu-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import bounded_reference as br
    import common
    import dynamics_inverse_reference as cref
    import emu_bvls_harness
    import inverse_dynamics_reference as dref

    def mutations(t, solved, scale_of):
        wrong, clip, exact, total = np.inf, np.inf, 0, 0
        for b, s in zip(*np.nonzero(solved)):
            lo = (t.lo[b] if t.lo.ndim == 2 else t.lo) * scale_of(s)
            hi = (t.hi[b] if t.hi.ndim == 2 else t.hi) * scale_of(s)
            if not (t.active[b, s][lo < hi] != 0).any():
                continue
            total += 1
            unit = br.floors(t)["scale"] * br.bound(t)
            e = float(np.abs(np.clip(t.ref.z[b, s], lo, hi) - t.z[b, s]).max()) / unit
            if e < 1.0:
                exact += 1
            else:
                clip = min(clip, e)
            for j in range(len(lo)):
                if t.active[b, s, j] == 0 and (np.isfinite(lo[j]) or np.isfinite(hi[j])):
                    a = t.active[b, s].copy()
                    a[j] = -1 if (t.z[b, s, j] - lo[j] <= hi[j] - t.z[b, s, j]) else 1
                    wrong = min(wrong, float(np.abs(br.polish(t.ref.A[b, s], t.ref.r0[b, s], t.case.ridge, lo, hi, a)[0] - t.z[b, s]).max()) / unit)
        fin = lambda v: float(v) if np.isfinite(v) else "no such state"
        return dict(one_variable_wrongly_bound=fin(wrong), clipped_unbounded_answer=fin(clip), states_with_an_active_bound=total, clipping_exact_on=exact)

    def spec(t, solved, scale_of):
        m = t.margins
        least = lambda k: float(min((x[k] for x in m), default=np.inf)) if m and np.isfinite(min((x[k] for x in m), default=np.inf)) else "no such state"
        f = br.floors(t)
        return dict(draw=t.draw, floor_z=f["z"], floor_rho=f["rho"], scale=f["scale"], bound=br.bound(t), margin_z=least("margin_z"), margin_g=least("margin_g"),
                    sigma_ratio=least("sigma"), worst_free_gradient=float(max((x["free_gradient"] for x in m), default=0.0)),
                    active_bounds_per_state=np.bincount((t.active != 0).sum(-1)[solved]).tolist(), mutation_factors=mutations(t, solved, scale_of))

    def run(kind, t, got, tag):
        e = (br.compare_continuous if kind == "c" else br.compare_discrete)(t, got, tag)
        e["solves"] = np.bincount(np.asarray(got.solves).ravel()).tolist()
        return e

    device = not args.cpu_only
    if device:
        from trep_amd import BatchMidpointVI
    out = dict(device="MI355X" if device else "not measured", continuous={}, discrete={})
    for c in br.CONTINUOUS:
        if c.expect != "ok":
            continue
        t = br.continuous_table(c)
        p = t.inputs
        solved = np.ones((c.B, c.M), dtype=bool)
        row = spec(t, solved, lambda s: np.ones(t.z.shape[-1]))
        emu = emu_bvls_harness.EmuBvls(common.build(c.name)[1])
        row["emulated"] = run("c", t, emu.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], t.lo, t.hi, c.ridge, br.RCOND), "emulated ")
        row["device"] = "not measured"
        if device:
            mvi = BatchMidpointVI(common.build(c.name)[0], c.B, specialize=False)
            row["device"] = run("c", t, mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], c.ridge, bounds=(t.lo, t.hi)), "device ")
            row["device"]["team"] = mvi.kernel_info()["team"]
            mvi.close()
        out["continuous"][br.ccase_id(c)] = row
    for c in br.DISCRETE:
        for with_p0 in (True, False):
            t = br.discrete_table(c, with_p0)
            p = t.inputs
            nu = int(p["d"].n_inputs)
            solved = np.ones((c.B, c.N), dtype=bool)
            solved[:, 0] = with_p0
            row = spec(t, solved, lambda k: np.concatenate([np.full(nu, p["dts"][k]), np.ones(t.z.shape[-1] - nu)]))
            emu = emu_bvls_harness.EmuBvls(common.build(c.name)[1])
            row["emulated"] = run("d", t, emu.inverse_dynamics(p["Q"], p["dts"], t.lo, t.hi, p["p0"] if with_p0 else None, c.ridge, br.RCOND), "emulated ")
            row["device"] = "not measured"
            if device:
                mvi = BatchMidpointVI(common.build(c.name)[0], c.B, specialize=False)
                dt = p["dts"] if c.pattern != "uniform" else dref.DT
                row["device"] = run("d", t, mvi.inverse_dynamics(p["Q"], dt, p["p0"] if with_p0 else None, c.ridge, bounds=(t.lo, t.hi)), "device ")
                row["device"]["team"] = mvi.kernel_info()["team"]
                mvi.close()
            out["discrete"][br.dcase_id(c) + ("_p0" if with_p0 else "_no_p0")] = row
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
