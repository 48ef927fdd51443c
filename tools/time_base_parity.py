#!/usr/bin/env python3
"""Parity record of the non-uniform time base (GPU): runs the case table of the tests (tests/common.py::TB_SYSTEMS x TB_PATTERNS) --
the open-loop rollout with the non-rollout modes behind it, the closed loops, the one-step-per-trajectory horizon batches, on the
generic kernels and on the prebuilt specialised ones -- through the very functions of tests/test_gpu_time_base.py, and writes per case

    margins -- how far the oracle on a wrong time base (uniform mean, list one step forward / back) is from the oracle on the right
               one: the smallest relerr(X) over the case's trajectories (the tests ask for >= 1e-4)
    e_ref   -- the oracle's response to one unit in the last place of the start, per quantity
    worst   -- the worst distance of the kernels from the oracle per quantity, next to its bound max(tolerance, 64 e_ref)

to profiles/time_base_parity.json.  The counterpart of tools/lq_parity.py.

    python tools/time_base_parity.py [--out profiles/time_base_parity.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class _Env(object):
    """The part of pytest's monkeypatch the test functions use."""

    def delenv(self, name, raising=True):
        os.environ.pop(name, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_base_parity.json"))
    args = ap.parse_args()
    import common as C
    import test_gpu_time_base as T
    env = _Env()
    cases = {}
    for name, pattern in C.TB_CASES:
        c, ref = C.tb_case(name, pattern), C.tb_reference(name, pattern)
        margins = {}
        for kind, dts in C.tb_wrong_step_sizes(c["dts"]).items():
            margins[kind] = min(C.relerr(C.tb_oracle_rollout(c["d"], c["Q0"][b], c["Q1"][b], dts, c["U"][b], c["K"][b])["X"], ref[b]["X"])
                                for b in range(c["B"]))
        e_ref = C.tb_e_ref(name, pattern)
        row = dict(team=C.TB_SYSTEMS[name][0], trajectories=c["B"], steps=c["N"], margins=margins, e_ref=dict(e_ref), runs={})
        if name in C.TB_CLOSED_LOOP:
            row["e_ref_closed_loop"] = dict(C.tb_e_ref(name, pattern, closed_loop=True))
        cases["%s / %s" % (name, pattern)] = row

    def with_bounds(worst, e_ref, tol=None):
        return dict((q, dict(worst=e, bound=C.tb_bound(q, e_ref) if q in C.TB_TOL else (tol or {}).get(q))) for q, e in sorted(worst.items()))

    for pattern in C.TB_PATTERNS:
        for name, spec in C.TB_KINDS:
            row = cases["%s / %s" % (name, pattern)]
            kind = "specialised" if spec else "generic"
            row["runs"]["open loop, " + kind] = with_bounds(T.run_open_loop(env, name, spec, pattern), row["e_ref"])
        for name, spec in T.LOOP_KINDS:
            row = cases["%s / %s" % (name, pattern)]
            kind = "specialised" if spec else "generic"
            row["runs"]["closed loop, " + kind] = with_bounds(T.run_closed_loop(env, name, spec, pattern), row["e_ref_closed_loop"])
        for name, spec in T.HORIZON_KINDS:
            row = cases["%s / %s" % (name, pattern)]
            kind = "specialised" if spec else "generic"
            tol = dict(q2=C.TB_TOL["X"], p2=C.TB_TOL["X"])
            row["runs"]["one step per trajectory, " + kind] = with_bounds(T.run_horizon(env, name, spec, pattern), None, tol)
    every = [(q, v["worst"], v["bound"]) for row in cases.values() for run in row["runs"].values() for q, v in run.items()]
    doc = dict(command="python tools/time_base_parity.py", reference="oracle/trep_oracle.c stepped with o.step(o.times()[1] + dts[k], ...)",
               metric="max |a - ref| / max(1, max |ref|) per quantity, worst over the case's trajectories",
               bound="max(project tolerance, 64 e_ref) per case and quantity", step_sizes="DT = %g x (0.6, 1.5, 0.6, ...) / DT x (0.6 + 0.9 r)" % C.TB_DT,
               smallest_margin=min(min(r["margins"].values()) for r in cases.values()),
               worst_error_over_bound=max(e / b for _, e, b in every), cases=cases)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=False)
        f.write("\n")
    print("%d cases: smallest margin %.3e, worst error / bound %.3e -> %s" % (len(cases), doc["smallest_margin"], doc["worst_error_over_bound"], args.out))


if __name__ == "__main__":
    main()
