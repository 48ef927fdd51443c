#!/usr/bin/env python3
"""Parity record of the LQ sweep kernels (GPU): runs the size-class table of the tests (tests/common.py::LQ_CASES -- LQR, affine LQ
and the Newton model of every case) and the solver-branch problems (indefinite gamma, a zero leading pivot) on the device, against the
long-double sweep of tests/lq_reference.py, and writes per kernel class

    floor  -- the worst distance of the fp64 host sweep (dlqr.py, LAPACK) from the long-double one: what correct fp64 arithmetic gives
    worst  -- the worst distance of the kernel from the long-double sweep, per output (K, C, P0, b0, and K entry by entry)

to profiles/lq_parity.json.  The tests bound every output by max(64 floor, 1e-13); this file is where that setting can be checked.

    python tools/lq_parity.py [--out profiles/lq_parity.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = ("k_tv_lq", "k_tv_lq_mfma", "k_tv_lq_ds")
OUTPUTS = ("K", "C", "P0", "b0", "K_per_entry")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lq_parity.json"))
    args = ap.parse_args()
    import common
    import lq_reference as ref
    from trep_amd import _lib
    L = _lib.lib()
    classes, branches = {}, {}

    def record(table, key, floors, got, want):
        row = table.setdefault(key, dict(floor=0.0, worst=dict((o, 0.0) for o in OUTPUTS), problems=0))
        row["problems"] += 1
        row["floor"] = max([row["floor"]] + [e for e in floors if e is not None])
        for name, g, w in zip(OUTPUTS, got, want):
            if w is not None:
                row["worst"][name] = max(row["worst"][name], ref.relerr(g, w))
        row["worst"]["K_per_entry"] = max(row["worst"]["K_per_entry"], ref.entry_relerr(got[0], want[0]))

    def set_env(env):
        for k in ("TREPAMD_LQ_LEGACY", "TREPAMD_LQ_DENSE"):
            os.environ.pop(k, None)
        os.environ.update(env)

    def launch(p):
        rc, plan, _, _ = common.lq_plan(p)
        assert rc == 0
        _lib.check(L.tg_tv_lq(0, ctypes.byref(p)))
        return "%s<%d, %d>" % (KERNELS[plan[0]], plan[1], plan[2]) if plan[0] else "%s<TS = %d>" % (KERNELS[0], plan[1])

    for case in common.LQ_CASES:
        set_env(case.env)
        S, N, nX, nU, nxh = case.S, case.N, case.nX, case.nU, common.lq_case_nxh(case)
        names = "A B Q Qf R q r hz".split()
        pool = common.device_pool()
        try:
            dev = dict((k, pool.upload(v)) for k, v in zip(names, common.lq_case_problem(case)))
            for mode in common.LQ_MODES:
                p = common.lq_struct(S, N, nX, nU, dev, affine=mode != "lqr", hz=(nxh + nU, nxh) if mode == "newton" else None, ds=case.ds)
                out = common.LqOutputs(pool, S, N, nX, nU)
                key = launch(out.bind(p))
                K, C, P0, b0, st = out.get()
                assert (st == 0).all()
                for s in range(S):
                    want, floors, _ = common.lq_case_reference(case, mode, s)
                    record(classes, key, floors, (K[s], C[s], P0[s], b0[s]), want)
        finally:
            pool.close()
    problems = (("indefinite gamma", lambda ds: common.lq_indefinite_problem(ds)),
                ("zero leading pivot", lambda ds: common.lq_zero_pivot_problem(ds, 6, 2, 5)))
    for kernel, (env, _) in common.LQ_KERNELS.items():
        set_env(env)
        for title, make in problems:
            for ds in common.LQ_SPECIAL_SIZES:
                pr = make(ds)
                S, N, nX, nU, nxh = pr["S"], pr["N"], pr["nX"], pr["nU"], pr["nxh"]
                pool = common.device_pool()
                try:
                    dev = dict((k, pool.upload(pr[k])) for k in "A B Q Qf R q r hz".split())
                    out = common.LqOutputs(pool, S, N, nX, nU)
                    key = launch(out.bind(common.lq_struct(S, N, nX, nU, dev, hz=(nxh + nU, nxh), ds=ds)))
                    K, C, P0, b0, st = out.get()
                    assert (st == 0).all()
                    for s in range(S):
                        want, floors, _, _ = common.lq_special_reference(pr, s)
                        record(branches, "%s, %s" % (title, key), floors, (K[s], C[s], P0[s], b0[s]), want)
                finally:
                    pool.close()
    set_env({})
    worst = max(max(r["worst"].values()) for r in list(classes.values()) + list(branches.values()))
    floor = max(r["floor"] for r in list(classes.values()) + list(branches.values()))
    doc = dict(command="python tools/lq_parity.py", reference="tests/lq_reference.py (np.longdouble, eps %.3g)" % float(np.finfo(np.longdouble).eps),
               metric="max |a - ref| / max(1, max |ref|) per output; K_per_entry: max |a - ref| / (|ref| + rowmax |ref|)",
               bound="max(64 floor, 1e-13) per output and problem", worst_floor=floor, worst_error=worst,
               size_classes=dict(sorted(classes.items())), solver_branches=dict(sorted(branches.items())))
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=False)
        f.write("\n")
    print("%d size classes, %d solver-branch rows: worst floor %.3e, worst kernel error %.3e -> %s" % (len(classes), len(branches), floor, worst, args.out))


if __name__ == "__main__":
    main()
