#!/usr/bin/env python3
"""Inverse dynamics of a 5-link pendulum: which inputs made this motion?

A reference motion is made by rolling the pendulum out under smooth inputs.  BatchMidpointVI.inverse_dynamics then looks at the
configurations alone and returns, for every step of every trajectory at once, the inputs that satisfy the discrete Euler-Lagrange
equations, the momenta along the path and the impulse no input could supply (zero here: the motion is feasible).  Rolling out again
from the recovered initial momentum under the recovered inputs retraces the motion; the script prints how closely.  Last, a path
moved off the dynamics: a fully actuated system still matches it exactly, with large inputs, and a ridge trades those for a
residual impulse.

Twice: the pendulum driven by a torque at every joint (ConfigForce), and the same pendulum driven by a horizontal force at every
mass (HybridWrench with one input component), where the map from inputs to joint forces changes with the pose.

    python examples/inverse_dynamics.py [--batch 32] [--steps 200]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trep_amd
from trep_amd import forces, potentials

LINKS = 5


def pendulum(drive):
    """Five unit links swinging in the x-z plane; drive = "torques" or "wrenches"."""
    system = trep_amd.System()
    tree = []
    for link in reversed(range(LINKS)):
        tree = [trep_amd.ry("theta-%d" % link, name="joint-%d" % link), [trep_amd.tz(-1.0, name="mass-%d" % link, mass=1.0)] + ([tree] if tree else [])]
    system.import_frames(tree)
    potentials.Gravity(system, (0, 0, -9.8))
    forces.Damping(system, 0.05)
    for link in range(LINKS):
        if drive == "torques":
            forces.ConfigForce(system, "theta-%d" % link, "torque-%d" % link)
        else:
            forces.HybridWrench(system, "mass-%d" % link, ("push-%d" % link, 0, 0), name="wrench-%d" % link)
    return system


def run(drive, B, N, dt):
    system = pendulum(drive)
    mvi = trep_amd.BatchMidpointVI(system, B)
    rng = np.random.default_rng(3)
    # ---- the reference motion: every trajectory its own start and its own smooth inputs --------------------------------------
    Q0 = 0.3 * rng.standard_normal((B, mvi.nq))
    t = dt * np.arange(N)
    amp, freq, phase = 3.0 * rng.standard_normal((B, 1, mvi.nu)), 1.0 + rng.random((B, 1, mvi.nu)), 6.28 * rng.random((B, 1, mvi.nu))
    U = amp * np.sin(freq * t[None, :, None] + phase)
    mvi.initialize_from_configs(0.0, Q0, dt, Q0)
    X = mvi.rollout(N, dt, U)
    assert (mvi.status()[1] == 0).all()
    Q = X[:, :, :mvi.nq]

    # ---- the inputs of that motion, from the configurations alone -----------------------------------------------------------
    inv = mvi.inverse_dynamics(Q, dt)
    assert (inv.status == 0).all()
    print("%-8s  inputs recovered to %.2e (steps 1..N-1; step 0 is absorbed into the initial momentum)" % (drive, np.abs(inv.U[:, 1:] - U[:, 1:]).max()))
    print("%-8s  largest impulse no input supplies: %.2e;  momenta against the rollout's: %.2e" % (
        drive, np.abs(inv.rho).max(), np.abs(inv.P[:, 1:] - X[:, 1:, mvi.nq:mvi.nq + mvi.nd]).max()))

    # ---- and back: the recovered initial momentum and inputs retrace the motion ---------------------------------------------
    mvi.initialize_from_state(0.0, Q[:, 0], inv.P[:, 0])
    X2 = mvi.rollout(N, dt, inv.U)
    print("%-8s  path error of the second rollout over %d steps: %.2e" % (drive, N, np.abs(X2[:, :, :mvi.nq] - Q).max()))

    # ---- a path that is off the dynamics: fully actuated, it is still feasible -- at a price a ridge keeps down -----------------
    if drive == "wrenches":
        bent = Q + 1e-3 * rng.standard_normal(Q.shape)
        for ridge in (0.0, 1e-4):
            off = mvi.inverse_dynamics(bent, dt, ridge=ridge)
            print("%-8s  the path moved by 1e-3, ridge %g: inputs up to %.1f, |rho| up to %.2e" % (drive, ridge, np.abs(off.U).max(), np.abs(off.rho).max()))
    mvi.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    for drive in ("torques", "wrenches"):
        run(drive, args.batch, args.steps, 0.01)


if __name__ == "__main__":
    main()
