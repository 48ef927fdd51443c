"""The translation runs of the rollout's dual pose sweep (program.hpp, tr_*) in the specialised rollout kernels, against
the oracle: puppet and puppet-basic, B = 5 (one partly filled block), N = 12 steps, under the default pivot rule (k_spec<0, 0>) and the
exact one (k_spec<0, 1>).  The starts and string schedules are tests/test_gpu_floating_base.py's (common.starts with that file's velocity
and string scalings: steps of 2, 3 and 4 Newton iterations, asserted on the oracle's counts).  A second set of the puppet's has the whole
marionette and every string carrier shifted by the same (+50, -30) in x and y -- still constraint-consistent, the constraints see
differences only -- so that a swapped component or a wrong contributor of a run joint's position is far outside the tolerance.  (Puppet-
basic hangs from FIXED frames: there is no carrier to shift, its run is the torso's alone, and it runs the first set only.)
Tolerance: tests/test_gpu_floating_base.py's TOL on the states (relerr); Newton iterations equal to the oracle's."""
import functools

import numpy as np
import pytest

from common import build, relerr, starts

pytestmark = pytest.mark.gpu

DT = 0.01
TOL = 1e-10      # tests/test_gpu_floating_base.py
B, N = 5, 12
SEEDS = {"puppet40": 1, "puppet_basic": 2}
VEL_SCALE = np.array([0.0, 1.0, 3.0, 3.0, 0.0])
STRING_SCALE = np.array([1.0, 1.0, 1.0, 10.0, 10.0])
SHIFT = {"x": 50.0, "y": -30.0}
RUN_JOINTS = {"puppet40": 15, "puppet_basic": 3}


def _shift_columns(system):
    """(config index, shift) of the world-aligned translations along x and y: the torso's and the string carriers'"""
    cols = []
    for f in system.frames:
        if f.config is None:
            continue
        kind = (f.transform_type.name if hasattr(f.transform_type, "name") else str(f.transform_type)).lower()
        if kind.startswith("t") and kind[-1] in SHIFT and (f.config.kinematic or f.config.name in ("torso_tx", "torso_ty")):
            cols.append((system.configs.index(f.config), SHIFT[kind[-1]]))
    return cols


@functools.lru_cache(maxsize=None)
def _reference(name, shifted):
    """Starts on the recorded trajectories and the oracle's run from each: states and Newton iterations per step.  Computed once."""
    from oracle.oracle import OracleMVI
    system, d = build(name)
    Q0, Q1, U, K = starts(name, d, B, N, np.random.default_rng(SEEDS[name]))
    nd = d.n_dyn
    Q0, Q1 = Q0.copy(), Q1.copy()
    Q1[:, :nd] = Q0[:, :nd] + VEL_SCALE[:, None] * (Q1[:, :nd] - Q0[:, :nd])
    K = Q1[:, None, nd:] + STRING_SCALE[:, None, None] * (K - Q1[:, None, nd:])
    if shifted:
        cols = _shift_columns(system)
        assert len(cols) == 2 + 12          # torso x, y and the six carriers' x, y
        for c, s in cols:
            Q0[:, c] += s
            Q1[:, c] += s
            if c >= nd:
                K[:, :, c - nd] += s
    o = OracleMVI(d)
    X = np.zeros((B, N + 1, d.n_configs + d.n_dyn + d.n_kin))
    its = np.zeros((B, N), dtype=int)
    for b in range(B):
        o.initialize_from_configs(0.0, Q0[b], DT, Q1[b])
        X[b], total = o.rollout(N, DT, U[b], K[b])
        o.initialize_from_configs(0.0, Q0[b], DT, Q1[b])
        for k in range(N):
            its[b, k] = o.step(o.times()[1] + DT, U[b, k], K[b, k])
        assert total == its[b].sum()
    for a in (X, its, Q0, Q1, U, K):
        a.setflags(write=False)
    return system, d, Q0, Q1, U, K, X, its


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name,shifted", [("puppet40", False), ("puppet_basic", False), ("puppet40", True)])
def test_specialised_rollout_with_translation_runs_matches_oracle(name, shifted, exact):
    import trep_amd
    system, d, Q0, Q1, U, K, Xo, its = _reference(name, shifted)
    if not shifted:
        assert {2, 3, 4} <= set(its.ravel().tolist()), sorted(set(its.ravel().tolist()))       # (of the cases, not of the kernel)
    mvi = trep_amd.BatchMidpointVI(system, B, specialize=True)
    mvi.exact_pivot = exact
    mvi.initialize_from_configs(0.0, Q0, DT, Q1)
    X = mvi.rollout(N, DT, U if d.n_inputs else None, K)
    iters, status = mvi.status()
    info, kinfo = mvi.info(), mvi.kernel_info()
    mvi.close()
    assert (status == 0).all(), status
    worst = max(relerr(X[b], Xo[b]) for b in range(B))
    print("%s shifted=%d exact=%d: max relerr %.3e, iterations %s / oracle %s" % (name, shifted, exact, worst, iters.tolist(), its.sum(1).tolist()))
    assert info["tr_n"] == RUN_JOINTS[name] and kinfo["tr_n"] == RUN_JOINTS[name]
    assert "rollout" in kinfo["spec_launched"] and "rollout" not in kinfo["generic_launched"]
    assert kinfo["exact_pivot"] == exact
    for b in range(B):
        assert relerr(X[b], Xo[b]) < TOL, (name, b)
    assert np.array_equal(iters, its.sum(1))
