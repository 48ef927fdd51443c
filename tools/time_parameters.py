#!/usr/bin/env python3
"""Cost of per-trajectory parameters on the GPU (BatchMidpointVI.set_parameters), in one process, alternating default and parameter
launches on the same batch, HIP events on the batch's stream (tg_batch_timing):
  * puppet rollout B x N (benchmark inputs): the default kernel against B distinct parameter rows;
  * deriv1 -> A, B (tg_batch_linearize) of S puppet states: default against S distinct rows;
  * a sweep of 16 parameter sets done without the table: 16 batches of B / 16 trajectories of rebuilt systems (generic kernels,
    a rebuilt system has no prebuilt specialisation), against the same sweep as one parameter launch.
python tools/time_parameters.py [--batch 8192] [--steps 200] [--states 65536] [--reps 3] [--out file.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def rows_for(system, n, seed):
    from trep_amd import parameters
    rng = np.random.default_rng(seed)
    base = parameters.base_values(system)
    return {"inertia": base["inertia"][None] * rng.uniform(0.5, 2.0, (n,) + base["inertia"].shape),
            "gravity": base["gravity"][None] * rng.uniform(0.8, 1.2, (n, 1)),
            "damping": base["damping"][None] * rng.uniform(0.0, 3.0, (n, len(base["damping"])))}


def timed(mvi, fn, reps):
    out = []
    for _ in range(reps):
        mvi.timing(reset=True)
        fn()
        mvi.synchronize()
        out.append(mvi.timing(reset=True)[1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--states", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import trep_amd
    from trep_amd import systems
    from test_parameters_cpu import rebuilt
    system = systems.puppet()
    B, N, dt, nd = args.batch, args.steps, 0.01, system.nQd
    Q0 = systems.puppet_initial_conditions(system, B, seed=20250 + 3)
    K = systems.puppet_string_schedule(system, Q0[:, nd:], N, dt)
    rows = rows_for(system, B, 1)
    out = {"system": "puppet nq=40 nd=22 nk=18 nc=6", "batch": B, "steps": N, "reps": args.reps}

    mvi = trep_amd.BatchMidpointVI(system, B)
    out["spec_library"] = bool(mvi.kernel_info()["spec_library"])
    mvi.initialize_from_configs(0.0, Q0, dt, Q0)
    mvi.snapshot()
    K_dev = mvi.device_array(K)
    X_dev = mvi.device_empty(B * (N + 1) * mvi.nX)
    mvi.timing(reset=True)

    def roll():
        mvi.restore()
        mvi.rollout_device(N, dt, None, K_dev, X_dev)
    default_ms, par_ms = [], []
    for r in range(args.reps):        # alternating: default, parameters, default, ...
        mvi.clear_parameters()
        default_ms += timed(mvi, roll, 1)
        mvi.set_parameters(**rows)
        par_ms += timed(mvi, roll, 1)
    it, st = mvi.status()
    info = mvi.kernel_info()
    out["rollout"] = {"default_ms": default_ms, "parameters_ms": par_ms, "ratio_of_medians": float(np.median(par_ms) / np.median(default_ms)),
                      "parameter_status_ok": bool((st == 0).all()), "par_spec_launched": info["par_spec_launched"],
                      "par_generic_launched": info["par_generic_launched"]}
    mvi.close()

    # deriv1 -> A, B of S states (one step of the benchmark inputs from each state, repeated over the batch)
    S = args.states
    reps = (S + B - 1) // B
    QS = np.tile(Q0, (reps, 1))[:S]
    eng = trep_amd.BatchMidpointVI(system, S)
    eng.initialize_from_configs(0.0, QS, dt, QS)
    eng.rollout(1, dt, None, np.tile(K[:, :1], (reps, 1, 1))[:S])
    nX, nU = eng.nX, eng.nU
    A_dev, B_dev = eng.device_empty(S * nX * nX), eng.device_empty(S * nX * nU)
    srows = rows_for(system, S, 2)

    def lin():
        trep_amd._lib.check(eng._L.tg_batch_linearize(eng._h, A_dev, B_dev))
    eng.timing(reset=True)
    d_ms, p_ms = [], []
    for r in range(args.reps):
        eng.clear_parameters()
        d_ms += timed(eng, lin, 1)
        eng.set_parameters(**srows)
        p_ms += timed(eng, lin, 1)
    info = eng.kernel_info()
    out["deriv1_AB"] = {"states": S, "default_ms": d_ms, "parameters_ms": p_ms, "ratio_of_medians": float(np.median(p_ms) / np.median(d_ms)),
                        "par_spec_launched": info["par_spec_launched"]}
    eng.close()

    # 16 parameter sets: 16 rebuilt batches of B / 16 trajectories, against one parameter launch of B trajectories
    n_sets, per = 16, B // 16
    set_rows = {k: v[:n_sets] for k, v in rows.items()}
    sweep_ms = 0.0
    for s in range(n_sets):
        sysr = rebuilt(systems.puppet, set_rows, s)
        m = trep_amd.BatchMidpointVI(sysr, per)
        m.initialize_from_configs(0.0, Q0[s * per:(s + 1) * per], dt, Q0[s * per:(s + 1) * per])
        Kd = m.device_array(np.ascontiguousarray(K[s * per:(s + 1) * per]))
        m.timing(reset=True)
        m.rollout_device(N, dt, None, Kd, None)
        m.synchronize()
        sweep_ms += m.timing(reset=True)[1]
        m.close()
    one = trep_amd.BatchMidpointVI(system, n_sets * per)
    one.initialize_from_configs(0.0, Q0[:n_sets * per], dt, Q0[:n_sets * per])
    one.set_parameters(group=per, **set_rows)
    Kd = one.device_array(np.ascontiguousarray(K[:n_sets * per]))
    one.timing(reset=True)
    one.rollout_device(N, dt, None, Kd, None)
    one.synchronize()
    out["sweep_16_sets"] = {"trajectories_per_set": per, "rebuilt_batches_kernel_ms": sweep_ms, "one_parameter_launch_ms": one.timing(reset=True)[1],
                            "note": "kernel time only; the rebuilt batches also pay schedule builds and, to run specialised, a hipcc build each"}
    one.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
