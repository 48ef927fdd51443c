#!/usr/bin/env python3
"""Parity record of the forward-mode (dual-number) kernels: runs the case table of the tests (tests/common.py::FW_SYSTEMS x FW_KERNELS)
through the very functions of tests/test_forward_cpu.py and tests/test_gpu_forward.py and writes, per system, kernel and array,

    tolerance -- the project's figure (1e-10 dynamics, 1e-12 Lagrangian)
    e_ref     -- the floor of the reference: the ladder of half the base step against the ladder
    bound     -- max(tolerance, 64 e_ref)
    emulated  -- the worst error of the kernel compiled for the host (one lane)
    device    -- the worst error of the kernel on the GPU (null: not measured)

and per case the sensitivity margin (the smallest distance, in bounds, of the reference from the reference along the neighbouring
variable or at the neighbouring trajectory's state), next to the ladder's agreement with the reference project's own goldens and the
LDS-limit chains, to profiles/forward_parity.json.  The counterpart of tools/time_base_parity.py.

    python tools/forward_parity.py [--cpu-only] [--out profiles/forward_parity.json]

--cpu-only writes the half that needs no GPU (ladder against goldens, floors, emulated errors, margins) and marks the device fields
unmeasured.
"""
import argparse
import contextlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def quiet(fn, *args):
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        out = fn(*args)
    return out, buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forward_parity.json"))
    ap.add_argument("--cpu-only", action="store_true")
    args = ap.parse_args()
    import common as C
    import test_forward_cpu as T
    from oracle.oracle import OracleMVI
    G = None
    if not args.cpu_only:
        import test_gpu_forward as G

    goldens = {}
    for name in T.D2_NAMES:
        _, text = quiet(T.test_the_ladder_reproduces_the_second_derivatives_of_the_reference, name)
        goldens[name] = dict(dynamics2=float(text.split()[-1]))
    for name in T.CONVENTION_NAMES:
        _, text = quiet(T.test_the_ladder_reproduces_the_reference_after_its_element_conventions, name)
        w = text.replace(",", "").split()
        goldens[name] = dict(dynamics2_raw=float(w[-7]), dynamics2_with_reference_conventions=float(w[-5]))
    for name in T.HIGHER_NAMES:
        _, text = quiet(T.test_the_nested_ladder_reproduces_the_higher_lagrangian_derivatives_of_the_reference, name)
        w = text.replace(",", "").split()
        goldens.setdefault(name, {}).update(lagrangian_third_order=float(w[-4]), lagrangian_fourth_order=float(w[-1]))

    cases = {}
    for name in C.FW_SYSTEMS:
        o = OracleMVI(C.build(name)[1])
        for kernel in C.FW_KERNELS:
            c = C.fw_case(name, kernel)
            e_ref = C.fw_e_ref(name, kernel)
            emu = C.fw_errors(name, kernel, T.emulated(c, kernel))
            dev = quiet(G.run_case, name, kernel)[0] if G else None
            smallest, zeros, blind, failed = T.sensitivity(name, kernel, o)
            assert not failed
            arrays = dict((n, dict(tolerance=C.FW_TOL[kernel], e_ref=e_ref[n], bound=C.fw_bound(name, kernel, n), emulated=emu[n],
                                   device=dev[n] if dev else None)) for n in c["names"] if c["Q"].size and C.fw_reference(name, kernel)[0][0][n].size)
            ladder = C.fw_ladder_of(name, kernel)
            cases["%s / %s" % (name, kernel)] = dict(trajectories=c["B"], ladder=dict(base_step_q=ladder[0], halvings=ladder[1], step_dq_ddqk_u=C.FW_STEP_V),
                                                     sensitivity_margin=smallest, zero_references=zeros, state_blind=blind, arrays=arrays)
            print("%s / %s done" % (name, kernel), flush=True)

    chains = {}
    for kernel in C.FW_KERNELS:
        limit = C.fw_chain_limit(kernel)
        c = C.fw_chain_case(kernel, limit - 1)
        emu = T.emulated(c, kernel)
        dev = quiet(G.run_chain, kernel)[0][1] if G else None
        chains[kernel] = dict(links_refused=limit, lds_bytes_refused=C.fw_lds_bytes(C.fw_chain(limit)[1], kernel), links_run=limit - 1,
                              lds_bytes_run=C.fw_lds_bytes(C.fw_chain(limit - 1)[1], kernel),
                              arrays=dict((n, dict(tolerance=C.FW_TOL[kernel], e_ref=c["e_ref"][n], bound=max(C.FW_TOL[kernel], 64.0 * c["e_ref"][n]),
                                                   emulated=max(C.relerr(emu[n][t], c["reference"][t][0][n]) for t in range(c["B"])),
                                                   device=dev[n] if dev else None)) for n in c["names"] if c["reference"][0][0][n].size))
    every = [a for row in list(cases.values()) + list(chains.values()) for a in row["arrays"].values()]
    doc = dict(command="python tools/forward_parity.py" + (" --cpu-only" if args.cpu_only else ""),
               reference="Richardson-extrapolated central differences of OracleMVI.dynamics_deriv1 / lagrangian in long double (tests/common.py: fw_ladder), nested for two directions",
               metric="max |a - ref| / max(1, max |ref|) per array, worst over the case's trajectories",
               bound="max(project tolerance, 64 e_ref) per case and array",
               device="measured" if G else "unmeasured",
               smallest_margin=min(r["sensitivity_margin"] for r in cases.values()),
               worst_emulated_error_over_bound=max(a["emulated"] / a["bound"] for a in every),
               worst_device_error_over_bound=max(a["device"] / a["bound"] for a in every) if G else None,
               ladder_against_goldens=goldens, cases=cases, lds_limit_chains=chains)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=False)
        f.write("\n")
    print("%d cases: smallest margin %.3e, worst emulated error / bound %.3e, worst device error / bound %s -> %s" % (
        len(cases), doc["smallest_margin"], doc["worst_emulated_error_over_bound"],
        "%.3e" % doc["worst_device_error_over_bound"] if G else "unmeasured", args.out))


if __name__ == "__main__":
    main()
