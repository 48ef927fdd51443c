#!/usr/bin/env python3
"""Tape measures in one launch.  First the extensor-tendon model: a tape through the points A, B, C, E and I of the spring network
is a tendon's excursion, and its gradient with respect to every config is the tendon's moment arm there (a length per radian at
the rotary configs, a ratio at the sliding ones).  BatchMidpointVI.tape_measures returns excursion and moment arms for a batch of
postures at once; one posture is checked against the host TapeMeasure.  Then the marionette: the six string lengths (control point
to hook) and their rates for every state of a batch of rollouts, read by BatchMidpointVI.tape_measures_device from the rollout's X
where it lies (row stride nX); the rates use finite-difference configuration rates made on the host.

    python examples/tendon_moment_arms.py [--batch 256] [--steps 50]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import trep_amd
from trep_amd import TapeMeasure, systems

TENDON = ("A", "B", "C", "E", "I")
STRINGS = ("upper_torso", "lower_torso", "left_arm", "right_arm", "left_leg", "right_leg")


def tendon(B):
    system = systems.extensor_tendon()
    nq = len(system.configs)
    rng = np.random.default_rng(3)
    q0 = np.array(system.q)
    Q = q0[None, :] + 0.3 * rng.uniform(-1.0, 1.0, (B, nq))                       # postures around the model's initial pose
    mvi = trep_amd.BatchMidpointVI(system, B)
    tape = TapeMeasure(system, TENDON)
    r = mvi.tape_measures(Q, measures=[tape], gradients=True)                     # length [B][1], length_dq [B][1][nq]
    arms = r.length_dq[:, 0]
    print("tendon %s over %d postures: excursion %.4f .. %.4f" % ("-".join(TENDON), B, r.length.min(), r.length.max()))
    for k, c in enumerate(system.configs):
        if np.abs(arms[:, k]).max() > 0.0:
            print("  moment arm at %-8s %+.4f .. %+.4f" % (c.name, arms[:, k].min(), arms[:, k].max()))
    b = B // 2
    system.q = Q[b]
    want = np.array([tape.length_dq(c) for c in system.configs])
    err = max(abs(r.length[b, 0] - tape.length()), float(np.abs(arms[b] - want).max()))
    print("  posture %d against the host TapeMeasure: largest difference %.1e" % (b, err))
    assert err <= 1e-11 * max(1.0, float(np.abs(want).max()))
    mvi.close()


def strings(B, N):
    dt = 0.01
    system = systems.puppet()
    Q0 = systems.puppet_initial_conditions(system, B, seed=4)
    K = systems.puppet_string_schedule(system, Q0[:, system.nQd:], N, dt)
    mvi = trep_amd.BatchMidpointVI(system, B)
    mvi.initialize_from_configs(0.0, Q0, dt, Q0)
    nX, nq = mvi.nX, mvi.nq
    X_dev = mvi.device_empty(B * (N + 1) * nX)
    mvi.rollout_device(N, dt, None, mvi.device_array(K), X_dev)
    mvi.synchronize()
    assert (mvi.status()[1] == 0).all()
    X = mvi.download(X_dev, (B, N + 1, nX))
    dQ = np.gradient(X[:, :, :nq], dt, axis=1)                                    # configuration rates along each path
    measures = [[s + "_string_control", s + "_string_hook"] for s in STRINGS]
    T = len(measures)
    L_dev, V_dev = mvi.device_empty(B * (N + 1) * T), mvi.device_empty(B * (N + 1) * T)
    mvi.tape_measures_device(N + 1, X_dev, q_row_stride=nX, dQ_dev=mvi.device_array(dQ), measures=measures, length_dev=L_dev, velocity_dev=V_dev)
    mvi.synchronize()
    L, V = mvi.download(L_dev, (B, N + 1, T)), mvi.download(V_dev, (B, N + 1, T))
    for t, s in enumerate(STRINGS):
        config = X[:, :, system.configs.index(system.get_config(s + "_string-length"))]
        print("%-12s string: length %.3f .. %.3f m, rate %+.3f .. %+.3f m/s, largest constraint residual %.1e m"
              % (s, L[:, :, t].min(), L[:, :, t].max(), V[:, :, t].min(), V[:, :, t].max(), np.abs(L[:, :, t] - np.abs(config)).max()))
    mvi.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    tendon(args.batch)
    strings(args.batch, args.steps)


if __name__ == "__main__":
    main()
