#!/usr/bin/env python3
"""Natural frequencies of many rest poses in one launch.  256 puppets, each with its own masses and inertias (x U(0.5, 2)), come to
rest under gravity (BatchMidpointVI.minimize_potential_energy with a parameter table); the multipliers of the rest poses go into
BatchMidpointVI.normal_modes, which answers K phi = omega^2 M phi on the tangent space of the strings for every puppet at once.
A one-link pendulum is shown against its closed form, hanging and inverted.

    python examples/normal_modes.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trep_amd as trep
from trep_amd import parameters, systems

# ---- a unit point mass on a unit link: omega^2 = +-|g|
pend = systems.pendulum(1)
g = float(np.linalg.norm(parameters.base_values(pend)["gravity"]))
one = trep.BatchMidpointVI(pend, 2).normal_modes(np.array([[0.0], [np.pi]]))
print("pendulum hanging : omega^2 = %+.12f (closed form %+.12f), %.6f Hz" % (one.omega2[0, 0], g, one.frequencies[0, 0]))
print("pendulum inverted: omega^2 = %+.12f (closed form %+.12f), unstable directions: %d" % (one.omega2[1, 0], -g, one.unstable[1]))

# ---- puppets under a table of masses
B = 256
system = systems.puppet()
q0 = np.array([c.q for c in system.configs], dtype=float)
rng = np.random.default_rng(11)
base = parameters.base_values(system)
inertia = base["inertia"][None] * rng.uniform(0.5, 2.0, (B,) + base["inertia"].shape)
mvi = trep.BatchMidpointVI(system, B)
mvi.set_parameters(inertia=inertia)
t0 = time.perf_counter()
rest = mvi.minimize_potential_energy(np.tile(q0, (B, 1)), keep_kinematic=True)
t1 = time.perf_counter()
modes = mvi.normal_modes(rest.Q, mu=rest.mu)
t2 = time.perf_counter()
ok = (rest.status == 0) & (modes.status == 0)
print("%d puppets: %d at rest and solved; rest poses %.1f ms, normal modes %.1f ms (host arrays in and out)" % (
    B, int(ok.sum()), (t1 - t0) * 1e3, (t2 - t1) * 1e3))
print("modes per puppet: %d (rank of the strings %d), Jacobi sweeps %d-%d, largest residual %.2e" % (
    modes.count[ok].max(), modes.rank[ok].max(), modes.sweeps[ok].min(), modes.sweeps[ok].max(), modes.residual[ok].max()))
f = modes.frequencies[ok]
low = np.array([row[row > 1e-6][0] for row in np.nan_to_num(f)])          # the lowest frequency that is not a free motion
print("lowest natural frequency over the table: %.4f .. %.4f Hz (mean %.4f, std %.4f); unstable rest poses: %d" % (
    low.min(), low.max(), low.mean(), low.std(), int((modes.unstable[ok] > 0).sum())))
