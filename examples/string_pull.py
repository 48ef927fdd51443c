#!/usr/bin/env python3
"""How a marionette's hand follows a string, from one launch.  64 puppets, each with its own masses (x U(0.5, 2)), come to rest
under gravity (BatchMidpointVI.minimize_potential_energy with a parameter table); BatchMidpointVI.static_response then gives, for
every puppet at once, the derivative of the rest pose along every string input, the change of the string tensions' multipliers and
the pose's compliance.  Composed with the hand's Jacobian (frame_kinematics(..., jacobians=True)) that is d(hand position) /
d(string length) -- the quantity a quasi-static string plan needs.  One predictor step along a string then starts the next
equilibrium search, and the trials it saves are counted.

    python examples/string_pull.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trep_amd as trep
from trep_amd import parameters, systems

B = 64
STRING, HAND, PULL = "left_arm_string-length", "lhand", -0.05       # the string shortened by 5 cm
system = systems.puppet()
names = [c.name for c in system.configs]
starts = systems.puppet_initial_conditions(system, B)       # bent limbs: from these the rest poses are strict minima
rng = np.random.default_rng(5)
base = parameters.base_values(system)
mvi = trep.BatchMidpointVI(system, B)
mvi.set_parameters(inertia=base["inertia"][None] * rng.uniform(0.5, 2.0, (B,) + base["inertia"].shape))

rest = mvi.minimize_potential_energy(starts, keep_kinematic=True)
resp = mvi.static_response(rest.Q, mu=rest.mu, keep_kinematic=True)
ok = (rest.status == 0) & (resp.status == 0)
print("%d puppets: %d at rest and answered; %d string inputs driven, rank of the strings %d, largest residual %.2e, defect %.2e" % (
    B, int(ok.sum()), resp.dq.shape[1], resp.rank[ok].max(), resp.residual[ok].max(), resp.defect[ok].max()))

# d(hand position) / d(string input) = p_dq . dq: the hand's Jacobian composed with the pose's derivative
held = [n for n, c in zip(names, system.configs) if c.kinematic]
j = held.index(STRING)
p_dq = mvi.frame_kinematics(rest.Q, frames=[HAND], jacobians=True).p_dq[:, 0]      # [B][nq][3]
hand = np.einsum("bjk,bkx->bjx", resp.dq, p_dq)                                      # [B][nD][3]
print("d(%s position) / d(%s): mean (%+.4f, %+.4f, %+.4f), spread of dz over the table %.4f .. %.4f" % (
    (HAND, STRING) + tuple(hand[ok, j].mean(axis=0)) + (hand[ok, j, 2].min(), hand[ok, j, 2].max())))
tension = resp.dmu[ok, j]
print("d(multipliers) / d(%s): largest %.3f; softest direction of the rest poses: %.4f per unit force" % (
    STRING, np.abs(tension).max(), np.abs(resp.compliance[ok]).max()))

# a predictor step along the string, then the equilibrium search from there and from the old pose
moved = rest.Q.copy()
moved[:, names.index(STRING)] += PULL
predicted = rest.Q + PULL * resp.dq[:, j]
cold = mvi.minimize_potential_energy(moved, keep_kinematic=True)
warm = mvi.minimize_potential_energy(predicted, keep_kinematic=True)
both = ok & (cold.status == 0) & (warm.status == 0)
print("string moved by %+.2f: the search needs %.1f trials from the old pose, %.1f from the predicted one (%d fewer on average); the"
      " predictor is off by %.2e, the old pose by %.2e" % (
          PULL, cold.iterations[both].mean(), warm.iterations[both].mean(), round((cold.iterations[both] - warm.iterations[both]).mean()),
          np.abs(predicted - warm.Q)[both].max(), np.abs(moved - cold.Q)[both].max()))
