#!/usr/bin/env python3
"""Record the parity of the normal-modes kernel over the case table of tests/normal_modes_reference.py: per system the floors (the
eigenvalue change under the curvature ladder's floor, the specification's distance from LAPACK), the bounds, the reference's worst
sweep count and the worst error of every quantity for the host emulation and, with --device, for the kernel on the GPU.

    python tools/normal_modes_parity.py [--device] [--out profiles/normal_modes_parity.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import common
import emu_modes_harness
import normal_modes_reference as nr


def plain(x):
    if isinstance(x, dict):
        return dict((k, plain(v)) for k, v in x.items())
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x.item() if isinstance(x, np.generic) else x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normal_modes_parity.json"))
    args = ap.parse_args()
    cases = {}
    for name in nr.SYSTEMS:
        Q = nr.case_inputs(name)
        row = dict(poses=len(Q), floors=nr.case_floors(name), eig_bound=nr.eig_bound(name), invariant_bounds=nr.invariant_bounds(name),
                   reference_sweeps=int(nr.case_reference(name).sweeps.max()), max_sweeps=nr.MAX_SWEEPS)
        row["emulation"] = nr.compare(name, emu_modes_harness.EmuModes(common.build(name)[1]).normal_modes(Q))
        if args.device:
            import trep_amd
            mvi = trep_amd.BatchMidpointVI(common.build(name)[0], len(Q), specialize=False)
            row["team"] = mvi.kernel_info()["team"]
            row["device"] = nr.compare(name, mvi.normal_modes(Q))
        cases[name] = row
    with open(args.out, "w") as f:
        json.dump(plain(dict(margin=nr.MARGIN, tolerance=nr.TOL, invariant_minimum=nr.INVARIANT_MIN, gap=nr.GAP, device=bool(args.device),
                             cases=cases)), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
