#!/usr/bin/env python3
"""Computed torque: which inputs make an arm follow a planned joint path?

The wrench_arm of the test systems -- a 3-D arm on a kinematic slider, driven by a torque at the shoulder and a two-component force at
the hand -- is to follow an analytic joint path q(t), B copies of it with amplitudes of their own.  BatchMidpointVI.dynamics_inverse
evaluates (q, dq, ddq) of the path at the midpoint of every step and returns, for all B x N states in one launch, the inputs that
produce those accelerations (the feed-forward of a tracking controller), the generalized force the motion needs in total and the part
of it the inputs cannot supply (zero here: three inputs, three dynamic configs, A = F_du of full rank along the path).

The inputs are then applied open loop: a rollout from two consecutive configurations of the path under U.  The script prints the
tracking error at two step sizes and their ratio.  What is seen is first order, a ratio of 2, not the 4 of a second-order scheme: the
integrator puts the whole impulse dt f(q_{k+1/2}, u_k) of a step into the balance at its FIRST node t_k (its momentum p_{k+1} =
D2L_d(q_k, q_{k+1}) carries no force term), so a force that varies in time acts half a step late, whichever instant of the step the
feed-forward is sampled at (the midpoint is the better of the two: a quarter of the error of sampling at t_k).  The inputs that make the
discrete equations hold exactly are BatchMidpointVI.inverse_dynamics' (examples/inverse_dynamics.py); computed torque is the
continuous answer, and it also serves where there is no time step at all -- sizing actuators, checking a plan's feasibility.  The arm
is driven by a force at its hand, which makes it unstable in open loop (an error grows about tenfold in a quarter second): the
horizon is kept short.

    python examples/computed_torque.py [--batch 32] [--time 0.5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trep_amd
from trep_amd import systems

# q = (a, b, c | slide): the centre, the amplitude and the angular frequency of every config's sine
CENTRE = np.array([0.5, -0.4, 0.8, 0.0])
AMPLITUDE = np.array([0.3, 0.2, 0.2, 0.1])
OMEGA = np.array([1.0, 1.3, 0.7, 2.0])


def path(t, gain):
    """(q, dq, ddq) [B][len(t)][nq] of the planned path at the times t; gain [B] scales the amplitudes."""
    amp = gain[:, None, None] * AMPLITUDE
    arg = OMEGA * np.asarray(t)[None, :, None]
    return CENTRE + amp * np.sin(arg), amp * OMEGA * np.cos(arg), -amp * OMEGA ** 2 * np.sin(arg)


def track(mvi, gain, T, N):
    """Feed-forward inputs at the N step midpoints and the open-loop rollout under them; returns (result, tracking error [N + 1])."""
    dt = T / N
    nd = mvi.nd
    t = dt * np.arange(-1, N + 1)                    # t_-1 and t_0 start the integrator, the N steps run from t_0 to t_N
    Q, _, _ = path(t, gain)
    inv = mvi.dynamics_inverse(*path(t[1:-1] + 0.5 * dt, gain))
    assert (inv.status == 0).all()
    # the integrator's momentum at t_0 is that of the pair (q(t_-1), q(t_0)); the sliders' planned places go in as K
    mvi.initialize_from_configs(t[0], Q[:, 0], t[1], Q[:, 1])
    X = mvi.rollout(N, dt, inv.U, Q[:, 2:, nd:])
    assert (mvi.status()[1] == 0).all()
    return inv, np.abs(X[:, :, :mvi.nq] - Q[:, 1:]).max(axis=(0, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--time", type=float, default=0.5)
    args = ap.parse_args()
    system = systems.wrench_arm()
    mvi = trep_amd.BatchMidpointVI(system, args.batch)
    gain = np.linspace(0.5, 1.5, args.batch)
    errors = []
    for N in (100, 200):
        inv, err = track(mvi, gain, args.time, N)
        errors.append(err.max())
        print("dt %.4f: %d x %d states in one launch; inputs up to %.2f, total generalized force up to %.2f, unsupplied part %.1e" % (
            args.time / N, args.batch, N, np.abs(inv.U).max(), np.abs(inv.tau).max(), np.abs(inv.rho).max()))
        print("dt %.4f: open-loop tracking error over %.1f s: %.3e (worst copy, worst config, worst step)" % (args.time / N, args.time, errors[-1]))
    print("halving the step divides the tracking error by %.2f (first order: 2, second order: 4)" % (errors[0] / errors[1]))
    mvi.close()


if __name__ == "__main__":
    main()
