#!/usr/bin/env python3
"""Where the puppet's hands and feet go: a batch of marionettes is rolled out on the device and the world paths of the four limb
ends are taken from the rollout's X where it lies -- BatchMidpointVI.frame_kinematics_device reads the configurations with the row
stride nX, one team per state, one launch for all B x (N + 1) states.  Then one string: the distance between the world positions
of its control point and its hook, both from frame_kinematics, against TapeMeasure.length() on the host at one state -- and against
the string's own length config, which the constraint holds it to.

    python examples/frame_paths.py [--batch 256] [--steps 50]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import trep_amd
from trep_amd import systems
from trep_amd.tapemeasure import TapeMeasure

ENDS = ("lhand_end", "rhand_end", "lfoot_end", "rfoot_end")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    B, N, dt = args.batch, args.steps, 0.01

    system = systems.puppet()
    Q0 = systems.puppet_initial_conditions(system, B, seed=4)
    K = systems.puppet_string_schedule(system, Q0[:, system.nQd:], N, dt)
    mvi = trep_amd.BatchMidpointVI(system, B)
    mvi.initialize_from_configs(0.0, Q0, dt, Q0)
    nX, nq = mvi.nX, mvi.nq
    X_dev = mvi.device_empty(B * (N + 1) * nX)
    mvi.rollout_device(N, dt, None, mvi.device_array(K), X_dev)

    # the limb ends of every state, straight from X on the device (nothing is copied to the host in between)
    g_dev = mvi.device_empty(B * (N + 1) * len(ENDS) * 12)
    mvi.frame_kinematics_device(N + 1, X_dev, q_row_stride=nX, frames=ENDS, g_dev=g_dev)
    mvi.synchronize()
    assert (mvi.status()[1] == 0).all()
    paths = mvi.download(g_dev, (B, N + 1, len(ENDS), 3, 4))[..., 3]            # [B][N + 1][4][3]: the fourth column of g is p
    travelled = np.linalg.norm(np.diff(paths, axis=1), axis=-1).sum(axis=1)      # [B][4]
    for i, name in enumerate(ENDS):
        print("%-10s path length over %d steps: mean %.4f m, longest %.4f m (trajectory %d), final height %.3f .. %.3f m"
              % (name, N, travelled[:, i].mean(), travelled[:, i].max(), int(travelled[:, i].argmax()), paths[:, -1, i, 2].min(), paths[:, -1, i, 2].max()))

    # one string at one state: |p(control) - p(hook)| from the device against the host's tape measure and the length config
    string = "left_arm_string"
    X = mvi.download(X_dev, (B, N + 1, nX))
    b, k = B // 3, N
    ends = mvi.frame_kinematics(np.ascontiguousarray(X[:, k, :nq]), frames=[string + "_control", string + "_hook"])
    device_length = float(np.linalg.norm(ends.g[b, 0, :, 3] - ends.g[b, 1, :, 3]))
    system.q = X[b, k, :nq]
    tape = TapeMeasure(system, [string + "_control", string + "_hook"]).length()
    config = system.get_config(string + "-length").q
    print("%s of trajectory %d at step %d: %.12f m from frame_kinematics, %.12f m by TapeMeasure.length() (difference %.1e), "
          "length config %.12f m (constraint residual %.1e)" % (string, b, k, device_length, tape, abs(device_length - tape), config, abs(device_length - config)))
    assert abs(device_length - tape) <= 1e-12 * max(1.0, tape)
    mvi.close()


if __name__ == "__main__":
    main()
