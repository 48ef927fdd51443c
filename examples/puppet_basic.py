#!/usr/bin/env python3
"""The marionette of the reference's examples/puppet-basic.py through the drop-in API: build the system, make
the starting guess consistent with the six string constraints, integrate with the single-trajectory
MidpointVI (B = 1 shell over the batched HIP engine), then make 4096 differently perturbed poses consistent in one launch
(BatchMidpointVI.satisfy_constraints) and run them as one device-resident rollout.

    python examples/puppet_basic.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trep_amd as trep
from trep_amd import systems

dt, tf = 0.01, 2.0
system = systems.puppet_basic()           # same frame tree, masses, damping and Distance constraints as the script
system.q = systems.PUPPET_BASIC_POSE      # the script's starting guess ...
system.satisfy_constraints()              # ... made consistent with the strings
q0 = system.q

mvi = trep.MidpointVI(system)
mvi.initialize_from_configs(0.0, q0, dt, q0)
t0 = time.perf_counter()
q = [mvi.q2]
while mvi.t1 < tf:
    mvi.step(mvi.t2 + dt, (), system.qk)
    q.append(mvi.q2)
print("single trajectory: %d steps in %.2f s, TorsoZ %.4f -> %.4f" %
      (len(q) - 1, time.perf_counter() - t0, q[0][system.get_config('TorsoZ').index], q[-1][system.get_config('TorsoZ').index]))

# the same system, 4096 perturbed poses, one kernel launch
B, N = 4096, int(tf / dt)
rng = np.random.default_rng(0)
batch = trep.BatchMidpointVI(system, B)
guess = q0 + rng.uniform(-0.03, 0.03, (B, system.nQ)) * (np.arange(system.nQ) >= 3)      # B distinct poses off the strings ...
guess[0] = q0
t0 = time.perf_counter()
proj = batch.satisfy_constraints(guess)    # ... each moved to the nearest pose on them, in one launch
Q0 = proj.Q
print("projection: %d poses in %.3f s (incl. transfers), failed: %d, Newton steps at most %d" %
      (B, time.perf_counter() - t0, int((proj.status != 0).sum()), int(proj.iterations.max())))
batch.initialize_from_configs(0.0, Q0, dt, Q0)
t0 = time.perf_counter()
X = batch.rollout(N, dt)                   # [B][N+1][nX]
iters, status = batch.status()
print("batch: %d trajectories x %d steps in %.2f s (incl. transfers), failed: %d, Newton iterations/step %.2f" %
      (B, N, time.perf_counter() - t0, int((status != 0).sum()), iters.mean() / N))
