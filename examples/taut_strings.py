#!/usr/bin/env python3
"""Strings only pull: can this marionette path be played?

A puppet path is made by rolling the marionette out under a string-length schedule.  BatchMidpointVI.inverse_dynamics then asks what
the six strings have to do along a PLANNED path: the same choreography played --speed times faster.  The unbounded least-squares
answer (rcond=) gives every string whatever tension the path needs, of either sign -- where the body has to come down faster than
it falls, a string would have to push, and the answer reports that as a negative tension with a small residual, i.e. as feasible.
With bounds=tension_bounds() every string is confined to the pulling side (lambda >= 0 in the discrete equations); the answer is
then the best one a real marionette can give, and what it cannot supply shows up where it belongs: in rho.

The script prints on how many steps the unbounded answer had a pushing string, and the |rho| the bounded answer reports there.

    python examples/taut_strings.py [--batch 4] [--steps 340] [--speed 4]
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
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=340)
    ap.add_argument("--speed", type=float, default=4.0)
    args = ap.parse_args()
    B, N, dt = args.batch, args.steps, 0.01
    system = systems.puppet()
    mvi = trep_amd.BatchMidpointVI(system, B)

    # ---- the choreography: a rollout under the string-length schedule ------------------------------------------------------------
    Q0 = systems.puppet_initial_conditions(system, B, seed=1)
    K = systems.puppet_string_schedule(system, Q0[:, system.nQd:], N, dt)
    mvi.initialize_from_configs(0.0, Q0, dt, Q0)
    X = mvi.rollout(N, dt, None, K)
    assert (mvi.status()[1] == 0).all()
    Q = X[:, :, :mvi.nq]

    for speed in (1.0, args.speed):
        free = mvi.inverse_dynamics(Q, dt / speed, rcond=1e-9)
        taut = mvi.inverse_dynamics(Q, dt / speed, bounds=mvi.tension_bounds("inverse_dynamics"))
        assert (taut.status == 0).all() and taut.lam.min() >= 0.0
        solved = np.ones((B, N), dtype=bool)
        solved[:, 0] = False                                # (without p0 step 0 is absorbed into the initial momentum)
        if speed == 1.0:
            solved[:, 1] = False                            # (... and step 1 starts from that momentum, not from the rollout's)
        push = (free.lam < 0.0).any(axis=2) & solved
        rho_free, rho_taut = np.abs(free.rho).max(axis=2), np.abs(taut.rho).max(axis=2)
        print("played at %gx: %d of %d steps need a pushing string in the unbounded answer (lowest tension %.3g)" % (
            speed, push.sum(), solved.sum(), free.lam[solved].min()))
        if push.any():
            print("  on those steps the unbounded answer reports |rho| up to %.2e; with taut strings |rho| is %.2e .. %.2e" % (
                rho_free[push].max(), rho_taut[push].min(), rho_taut[push].max()))
            print("  strings slack there (tension bound active): %.1f of %d on average; least-squares solves per step: %.2f on average, %d at most" % (
                (taut.active[push] != 0).sum(axis=1).mean(), mvi.nc, taut.solves[solved].mean(), taut.solves.max()))
        same = ~push & solved
        print("  on the other %d steps the two answers differ by %.1e" % (same.sum(), np.abs(taut.lam[same] - free.lam[same]).max(initial=0.0)))
    mvi.close()


if __name__ == "__main__":
    main()
