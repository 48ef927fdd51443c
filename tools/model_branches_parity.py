#!/usr/bin/env python3
"""Parity record of the model-branch cases (tests/common.py, MB_*): spatial_loop and mixed_loop on the generic kernels, ladder_point and
ladder_mixed on the specialised world-frame path.  Per system

    e_ref     -- the oracle's response to one unit in the last place of the start, per quantity (the floor of the bounds)
    margins   -- per mutated descriptor of tests/test_model_branches_cpu.py: "does not solve", or how many tolerances it is from the
                 right one in X, lambda and the l1_* derivatives (the tests ask for >= 1e3)
    emulated  -- worst distance of the generic kernel source at TEAM = 1 (host build) from the oracle, per quantity
    device    -- worst distance of the kernels on the GPU from the oracle, per quantity, through the very functions of
                 tests/test_gpu_model_branches.py and tests/test_gpu_world_frame_shapes.py; null until run on a GPU

to profiles/model_branches_parity.json.

    python tools/model_branches_parity.py [--cpu-only] [--out profiles/model_branches_parity.json]
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


def emulated(C, name):
    from emu_harness import EmuBatch
    c, ref = C.mb_case(name), C.mb_reference(name)
    d, B = c["d"], 3
    Z, ZL = C.mb_contraction(name)
    e = EmuBatch(d, B)
    e.initialize_from_configs(0.0, c["Q0"][:B], C.TB_DT, c["Q1"][:B])
    X = e.rollout(C.MB_N, C.TB_DT, c["U"][:B] if d.n_inputs else None, c["K"][:B] if d.n_kin else None)
    d1 = e.deriv1()
    HZ = e.deriv2z(Z[:B], ZL[:B])
    worst = {}
    for b in range(B):
        r = ref[b]
        for q, v in (("X", C.relerr(X[b], r["X"])), ("p2", C.relerr(e.p2[b], r["p2"])), ("lambda1", C.relerr(e.lam[b], r["lambda1"])),
                     ("d1", max(C.relerr(d1[n][b], r["d1"][n]) for n in C.D1)), ("hz", C.relerr(HZ[b], r["hz"]))):
            worst[q] = max(worst.get(q, 0.0), v)
    return worst


def margins(C, T, name):
    d, mutants = T._mutants(name)
    prefix, q0, U, K = C.trajectories(name)[0]
    right = T._run(d, q0, U, K)
    tol = dict(X=C.TB_TOL["X"], lam=C.TB_TOL["lambda1"], l1=C.TB_TOL["d1"])
    out = {}
    for what, changes in mutants:
        got = T._run(T._mutant(d, **changes), q0, U, K)
        out[what] = "does not solve" if got is None else dict((k, C.relerr(got[k], right[k]) / tol[k]) for k in tol)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_branches_parity.json"))
    ap.add_argument("--cpu-only", action="store_true", help="floors, margins and emulated errors only: the device figures stay null")
    args = ap.parse_args()
    import common as C
    import test_model_branches_cpu as T
    systems = {}
    for name in C.MB_GENERIC + C.MB_LADDERS:
        e_ref = C.mb_e_ref(name)
        row = dict(team=C.MB_TEAM[name], trajectories=C.mb_batch(name), steps=C.MB_N, e_ref=dict(e_ref),
                   bounds=dict((q, C.mb_bound(name, q, e_ref)) for q in e_ref), emulated=emulated(C, name), device=None)
        if name in C.MB_GENERIC:
            row["margins"] = margins(C, T, name)
        if name in C.MB_CLOSED_LOOP:
            row["e_ref_closed_loop"] = dict(C.mb_e_ref(name, closed_loop=True))
        systems[name] = row
    if not args.cpu_only:
        import test_gpu_model_branches as G
        import test_gpu_world_frame_shapes as W
        env = _Env()
        for name in C.MB_GENERIC:
            systems[name]["device"] = {"generic": G.run_generic(env, name)}
        for name in C.MB_LADDERS:
            systems[name]["device"] = {"specialised": W.run_specialised(env, name, False),
                                       "specialised, exact pivot": W.run_specialised(env, name, True)}
    doc = dict(command="python tools/model_branches_parity.py" + (" --cpu-only" if args.cpu_only else ""),
               reference="oracle/trep_oracle.c from starts on the recorded trajectories, %d steps of %g" % (C.MB_N, C.TB_DT),
               metric="max |a - ref| / max(1, max |ref|) per quantity, worst over the case's trajectories",
               bound="the project's tolerance per quantity; max(tolerance, 64 e_ref) for the quantities in second_term",
               second_term=sorted("%s / %s" % k for k in C.MB_SECOND_TERM),
               device_figures="not measured: written with --cpu-only on a machine without a GPU" if args.cpu_only else "measured",
               systems=systems)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=False)
        f.write("\n")
    print("%d systems -> %s (%s)" % (len(systems), args.out, doc["device_figures"]))


if __name__ == "__main__":
    main()
