"""The closed forms of the floating base's translational prefix (program.hpp, fb_*) in the specialised rollout kernels,
against the oracle: puppet and puppet-basic, B = 5 (one partly filled block, a multiple of nothing), N = 12 steps -- step 0 with its own
Dh1 sweep, the later ones with the copied one, steps of 2, 3 and 4 Newton iterations among them -- under the default pivot rule
(k_spec<0, 0>, structured solve) and the exact one (k_spec<0, 1>: the dense image gets the prefix entries from phase C as well).
Tolerance: tests/test_gpu_parity.py's for the same array (its TOL on the states, relerr); Newton iterations equal to the oracle's."""
import functools

import numpy as np
import pytest

from common import build, relerr, starts

pytestmark = pytest.mark.gpu

DT = 0.01
TOL = 1e-10      # tests/test_gpu_parity.py
B, N = 5, 12
SEEDS = {"puppet40": 1, "puppet_basic": 2}
VEL_SCALE = np.array([0.0, 1.0, 3.0, 3.0, 0.0])
STRING_SCALE = np.array([1.0, 1.0, 1.0, 10.0, 10.0])


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Starts on the recorded trajectories and the oracle's run from each: states and Newton iterations per step.  Computed once."""
    from oracle.oracle import OracleMVI
    system, d = build(name)
    Q0, Q1, U, K = starts(name, d, B, N, np.random.default_rng(SEEDS[name]))
    # on the recorded trajectories every step takes three iterations: the start velocity of the dynamic configs scaled per trajectory (0: at
    # rest, two iterations) and the string schedule of the last two sped up ten times (four) -- chosen on the oracle's counts alone
    nd = d.n_dyn
    Q1 = Q1.copy()
    Q1[:, :nd] = Q0[:, :nd] + VEL_SCALE[:, None] * (Q1[:, :nd] - Q0[:, :nd])
    K = Q1[:, None, nd:] + STRING_SCALE[:, None, None] * (K - Q1[:, None, nd:])
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
@pytest.mark.parametrize("name", ["puppet40", "puppet_basic"])
def test_specialised_rollout_with_prefix_matches_oracle(name, exact):
    import trep_amd
    system, d, Q0, Q1, U, K, Xo, its = _reference(name)
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
    print("%s exact=%d: max relerr %.3e, iterations %s / oracle %s" % (name, exact, worst, iters.tolist(), its.sum(1).tolist()))
    assert info["fb_n"] == 3 and "rollout" in kinfo["spec_launched"] and "rollout" not in kinfo["generic_launched"]
    assert kinfo["exact_pivot"] == exact
    for b in range(B):
        assert relerr(X[b], Xo[b]) < TOL, (name, b)
    assert np.array_equal(iters, its.sum(1))
