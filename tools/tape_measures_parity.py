#!/usr/bin/env python3
"""Parity record of the batched tape measures: per system of tests/tape_measure_reference.py and per output array the floor (the
disagreement of the host TapeMeasure accessors and the closed formulas, two independent fp64 evaluations, relative to max(1, |want|inf),
on the CPU), the tolerance max(project tolerance, 64 x floor) and its margin over the floor, and the error of the emulated kernel
(mvi_tape.hpp compiled for the host) and of the device kernel at the system's own team size, each as a fraction of its bound.  Writes
profiles/tape_measures_parity.json.  It gates nothing (the tests assert the same bounds); without a device the device errors are
recorded as "not measured".

    python tools/tape_measures_parity.py [--cpu-only] [--out profiles/tape_measures_parity.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def ratios(tr, name, got, want):
    import numpy as np
    out = {}
    for f in tr.FIELDS:
        a, w = getattr(got, f), getattr(want, f)
        err = float(np.abs(a - w).max())
        out[f] = dict(error=err, bound=tr.tolerance(name, f) * max(1.0, float(np.abs(w).max())))
        out[f]["error_over_bound"] = err / out[f]["bound"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tape_measures_parity.json"))
    ap.add_argument("--cpu-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import emu_tape_harness
    import tape_measure_reference as tr

    B, M = 5, 3
    out = dict(tolerances=tr.TOL, floor_note="host accessors against formulas(), relative to max(1, |want|inf), over the table's states",
               states_per_launch=[B, M], systems={})
    for name in tr.SYSTEMS:
        ms = [list(m) for m in tr.measures(name)]
        floors = tr.floors(name)
        Q, dQ, at = tr.batch_states(name, B, M)
        want = tr.expected(name, at)
        rec = dict(measures=ms, states=len(tr.states(name)[0]), shortest_segment=float(tr.segment_lengths(name).min()),
                   floor=floors, tolerance={f: tr.tolerance(name, f) for f in tr.FIELDS},
                   margin_over_floor={f: (tr.tolerance(name, f) / floors[f]) if floors[f] > 0 else "floor is zero" for f in tr.FIELDS},
                   emulated=ratios(tr, name, emu_tape_harness.EmuTape(tr.system_of(name)[1]).tape_measures(Q, dQ, ms), want), device="not measured")
        if not args.cpu_only:
            from trep_amd import BatchMidpointVI
            mvi = BatchMidpointVI(tr.system_of(name)[0], B, specialize=False)
            got = mvi.tape_measures(Q, dQ, ms, gradients=True, hessians=True)
            rec["device"] = ratios(tr, name, tr.Arrays(*got), want)
            rec["device_team"] = mvi.kernel_info()["team"]
            mvi.close()
        out["systems"][name] = rec
        print(name, json.dumps(rec["emulated"]), json.dumps(rec["device"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
