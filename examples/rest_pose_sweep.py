#!/usr/bin/env python3
"""Rest poses of a mass / gravity sweep in one launch, then a rollout from them.

A planar link hangs from a spring (systems.spring_link).  Every trajectory of the batch gets its own mass and its own gravity
(set_parameters); BatchMidpointVI.minimize_potential_energy finds each variant's own rest pose -- the host routine
System.minimize_potential_energy cannot: it sees the system's own values only -- and a rollout started there at rest stays there.

    python examples/rest_pose_sweep.py [--batch 64] [--steps 100]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trep_amd
from trep_amd import systems


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    B, N, dt = args.batch, args.steps, 0.01
    system = systems.spring_link()
    mvi = trep_amd.BatchMidpointVI(system, B)
    base = mvi.parameters()

    # ---- the sweep: masses x 0.5 .. 2, gravity x 0.5 .. 1.5 ----------------------------------------------------------------
    scale = np.linspace(0.5, 2.0, B)[:, None, None]
    gravity = base["gravity"][None] * np.linspace(0.5, 1.5, B)[::-1, None]
    mvi.set_parameters(inertia=base["inertia"][None] * scale, gravity=gravity)

    # ---- every variant's rest pose, the kinematic configs held --------------------------------------------------------------
    start = {"slide": 0.0, "a": 0.3, "b": -0.3, "d": 0.2, "e": -1.0}       # the bob hanging at its constraint's length
    Q0 = np.tile([start[c.name] for c in system.configs], (B, 1))
    rest = mvi.minimize_potential_energy(Q0, keep_kinematic=True)
    ok = rest.status == 0
    print("rest poses: %d of %d converged, %d to %d trials" % (ok.sum(), B, rest.iterations.min(), rest.iterations.max()))
    print("V start -> end, first and last variant: %.4f -> %.4f, %.4f -> %.4f" % (rest.V[0, 0], rest.V[0, 1], rest.V[-1, 0], rest.V[-1, 1]))
    print("spread of the rest poses over the sweep: %.4f" % np.abs(rest.Q - rest.Q[0]).max())

    # ---- a rollout from rest stays at rest ------------------------------------------------------------------------------------
    mvi.initialize_from_configs(0.0, rest.Q, dt, rest.Q)
    K = np.repeat(rest.Q[:, None, mvi.nq - mvi.nk:], N, axis=1)              # the kinematic slider stays where it is
    X = mvi.rollout(N, dt, None, K)
    drift = np.abs(X[:, :, :mvi.nq] - rest.Q[:, None, :]).max(axis=(1, 2))
    print("largest drift over %d steps: %.3e (converged variants)" % (N, drift[ok].max()))
    mvi.close()


if __name__ == "__main__":
    main()
