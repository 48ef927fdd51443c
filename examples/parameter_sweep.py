#!/usr/bin/env python3
"""Monte-Carlo over uncertain parameters in one launch: 4096 pend-on-cart trajectories from the same initial state, each with its
own cart / pendulum masses and inertias (x U(0.5, 2)) and damping (x U(0, 3)), rolled out for 2 s as one batch
(BatchMidpointVI.set_parameters).  Without the table every parameter set would be a batch of its own.  Row 0 is checked against a
system rebuilt with its values.

    python examples/parameter_sweep.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trep_amd as trep
from trep_amd import parameters, systems

B, dt, N = 4096, 0.01, 200
system = systems.pend_on_cart()
q0 = np.array([c.q for c in system.configs], dtype=float)
q0[1] = 0.3                                   # pendulum tilted, cart at rest
Q0 = np.tile(q0, (B, 1))

rng = np.random.default_rng(7)
base = parameters.base_values(system)
inertia = base["inertia"][None] * rng.uniform(0.5, 2.0, (B,) + base["inertia"].shape)
damping = base["damping"][None] * rng.uniform(0.0, 3.0, (B, len(base["damping"])))

mvi = trep.BatchMidpointVI(system, B)
mvi.set_parameters(inertia=inertia, damping=damping)      # before initialising: the initial momenta depend on the masses
mvi.initialize_from_configs(0.0, Q0, dt, Q0)
U = np.zeros((B, N, system.nu))
t0 = time.perf_counter()
X = mvi.rollout(N, dt, U)
wall = time.perf_counter() - t0
iters, status = mvi.status()
assert (status == 0).all()
cart = X[:, -1, 0]
print("%d parameter sets x %d steps in one launch: %.1f ms (host arrays in and out)" % (B, N, wall * 1e3))
print("cart position at t = %.1f s: mean %.4f, std %.4f, range [%.4f, %.4f]" % (N * dt, cart.mean(), cart.std(), cart.min(), cart.max()))

# row 0 against the system rebuilt with its values (Frame.set_mass, Damping.set_damping_coefficient)
ref_system = systems.pend_on_cart()
for f, v in zip(ref_system.masses, inertia[0]):
    f.set_mass(*[float(x) for x in v])
damp = [f for f in ref_system.forces if isinstance(f, trep.forces.Damping)][0]
for c, v in zip(ref_system.dyn_configs, damping[0]):
    damp.set_damping_coefficient(c, float(v))
ref = trep.BatchMidpointVI(ref_system, 1)
ref.initialize_from_configs(0.0, Q0[:1], dt, Q0[:1])
Xr = ref.rollout(N, dt, U[:1])
print("row 0 against the rebuilt system: max |difference| = %.2e" % np.abs(X[0] - Xr[0]).max())
