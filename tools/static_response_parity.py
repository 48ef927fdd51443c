#!/usr/bin/env python3
"""Record the parity of the static-response kernel over the case table of tests/static_response_reference.py: per case the floors
(the specification's change under the curvature ladder's rival and its distance from LAPACK, per array), the bounds, the invariant
bounds and the worst error of every array for the host emulation and, with --device, for the kernel on the GPU.  With --device also
one throughput figure: puppet40, B = 8192, with and without the compliance, milliseconds per launch through the device entry point
(warmed up, a host clock around launches that end in a synchronise, the two variants alternating, median and spread of the rounds).

    python tools/static_response_parity.py [--device] [--out profiles/static_response_parity.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import common
import emu_response_harness
import static_response_reference as sr

THROUGHPUT = dict(system="puppet40", batch=8192, launches=100, rounds=7, warmup=3)


def plain(x):
    if isinstance(x, dict):
        return dict((k, plain(v)) for k, v in x.items())
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x.item() if isinstance(x, np.generic) else x


def mask_arguments(case):
    return dict(keep_kinematic=sr.CASES[case][1] == "keep_kinematic", constant_q_list=sr.constant_names(case))


def throughput():
    import trep_amd
    t = dict(THROUGHPUT)
    case, B = t["system"], t["batch"]
    Q0, free = sr.case_inputs(case)
    Q = Q0[np.arange(B) % len(Q0)]
    mvi = trep_amd.BatchMidpointVI(common.build(case)[0], B, specialize=False)
    nq, nc, nD = mvi.nq, mvi.nc, int((~free).sum())
    q_dev = mvi.device_array(Q)
    out = dict(dq_dev=mvi.device_empty(B * nD * nq), dmu_dev=mvi.device_empty(B * nD * nc), compliance_dev=mvi.device_empty(B * nq * nq),
               reaction_dev=mvi.device_empty(B * nq * nc))

    def launches(compliance, n):
        for _ in range(n):
            mvi.static_response_device(q_dev, compliance=compliance, **out, **mask_arguments(case))
        mvi.synchronize()
    times = {True: [], False: []}
    for compliance in (True, False):
        launches(compliance, t["warmup"])
    for _ in range(t["rounds"]):
        for compliance in (True, False):
            t0 = time.perf_counter()
            launches(compliance, t["launches"])
            times[compliance].append(1e3 * (time.perf_counter() - t0) / t["launches"])
    t.update(team=mvi.kernel_info()["team"], n_free=int(free.sum()), n_drive=nD,
             ms_with_compliance=float(np.median(times[True])), ms_without_compliance=float(np.median(times[False])),
             ms_with_compliance_range=[min(times[True]), max(times[True])], ms_without_compliance_range=[min(times[False]), max(times[False])])
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "static_response_parity.json"))
    args = ap.parse_args()
    cases = {}
    for case in sr.CASES:
        name = sr.system_of(case)
        Q, free = sr.case_inputs(case)
        ref = sr.case_reference(case)
        row = dict(system=name, poses=len(Q), minima=len(sr.minima(case)), n_free=int(free.sum()), n_drive=int((~free).sum()),
                   rank=[int(ref.rank.min()), int(ref.rank.max())], floors=sr.case_floors(case), bounds=sr.case_bounds(case))
        fig = sr.compare(case, emu_response_harness.EmuResponse(common.build(name)[1]).static_response(Q, free))
        row["invariant_bounds"] = fig["invariant_bounds"]
        row["emulation"] = dict(errors=fig["errors"], invariants=fig["invariants"])
        if args.device:
            import trep_amd
            mvi = trep_amd.BatchMidpointVI(common.build(name)[0], len(Q), specialize=False)
            row["team"] = mvi.kernel_info()["team"]
            fig = sr.compare(case, mvi.static_response(Q, **mask_arguments(case)))
            row["device"] = dict(errors=fig["errors"], invariants=fig["invariants"])
        cases[case] = row
    prof = dict(margin=sr.MARGIN, tolerance=sr.TOL, invariant_minimum=sr.INVARIANT_MIN, device=bool(args.device), cases=cases)
    if args.device:
        prof["throughput"] = throughput()
    elif os.path.exists(args.out):      # (a record without a device keeps the throughput figure it had)
        with open(args.out) as f:
            prof["throughput"] = json.load(f).get("throughput")
    with open(args.out, "w") as f:
        json.dump(plain(prof), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
