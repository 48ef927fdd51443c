"""The step edge of the specialised rollout kernels (run_trajectory, csrc/mvi_core.hpp) against the oracle.

Between the converged evaluation of step k and the first evaluation of step k + 1 a full-wave team on the open-loop reference path
does p1, the X row, q1 <- q2, the kinematic targets, the rates and Dh1 <- Dh2 in one phase; step 0, the last step, the extrapolating
predictor, feedback and a failed trajectory take the separate phases.  The cases put each of those at an edge: puppet40 (18 kinematic
configs, whose targets wait on lanes nd .. nq - 1) and puppet_basic (nk = 0), B = 5 (one partly filled block), N = 1 (step 0 is also
the last: no edge at all), N = 2 (one edge, into the last step: the state's p1 is written from it) and N = 12 (ten middle edges), both
pivot rules (k_spec<0, 0> and k_spec<0, 1>), with the trajectory X and without it (then q2, p2 and lambda1 of the final state).  One
case each for the extrapolating predictor (the separate phases), a non-uniform time base (the X row takes the finished step's dt, the
rates the next one's) and two rollouts of 6 steps against one of 12, which must agree to the last bit (the write-back of q1, q2, p1,
p2 and lambda1 behind the last step, and the start from it).

Starts, inputs and the oracle runs are tests/test_gpu_translation_runs.py's first set (steps of 2, 3 and 4 Newton iterations), computed
once; a rollout of n < 12 steps is compared with the first n steps of the same oracle run.  Tolerances: TOL on the states (relerr), as
in tests/test_gpu_floating_base.py; lambda1 to common.TB_TOL["lambda1"], the project's bound for the multipliers of a run whose
iteration count equals the reference's; Newton iterations per trajectory equal to the oracle's."""
import functools

import numpy as np
import pytest

from common import TB_PREDICTOR_TOL, TB_TOL, build, relerr, tb_oracle_rollout, tb_step_sizes
from test_gpu_translation_runs import _reference as _starts

pytestmark = pytest.mark.gpu

DT = 0.01
TOL = 1e-10      # tests/test_gpu_floating_base.py
B, N = 5, 12
SYSTEMS = ("puppet40", "puppet_basic")


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The shared starts and oracle trajectory, and the oracle's multipliers after every step.  Computed once, read-only."""
    from oracle.oracle import OracleMVI
    system, d, Q0, Q1, U, K, X, its = _starts(name, False)
    lam = np.zeros((B, N, d.n_constraints))
    o = OracleMVI(d)
    for b in range(B):
        o.initialize_from_configs(0.0, Q0[b], DT, Q1[b])
        for k in range(N):
            o.step(o.times()[1] + DT, U[b, k], K[b, k])
            lam[b, k] = o.lambda1
    lam.setflags(write=False)
    return system, d, Q0, Q1, U, K, X, its, lam


def _batch(system, exact=False):
    import trep_amd
    mvi = trep_amd.BatchMidpointVI(system, B, specialize=True)
    mvi.exact_pivot = exact
    return mvi


def _inputs(d, U, K, n0, n1):
    return (np.ascontiguousarray(U[:, n0:n1]) if d.n_inputs else None, np.ascontiguousarray(K[:, n0:n1]) if d.n_kin else None)


def _assert_spec_rollout(mvi, exact=False):
    kinfo = mvi.kernel_info()
    assert "rollout" in kinfo["spec_launched"] and "rollout" not in kinfo["generic_launched"], kinfo
    assert kinfo["exact_pivot"] == exact


@pytest.mark.parametrize("with_X", [True, False], ids=["X", "noX"])
@pytest.mark.parametrize("exact", [False, True], ids=["ranked", "exact"])
@pytest.mark.parametrize("n", [1, 2, 12])
@pytest.mark.parametrize("name", SYSTEMS)
def test_rollout_of_n_steps_matches_oracle(name, n, exact, with_X):
    system, d, Q0, Q1, U, K, Xo, its, lam = _reference(name)
    nq, nd = d.n_configs, d.n_dyn
    if n == N:
        assert {2, 3, 4} <= set(its.ravel().tolist()), sorted(set(its.ravel().tolist()))       # (of the cases, not of the kernel)
    mvi = _batch(system, exact)
    mvi.initialize_from_configs(0.0, Q0, DT, Q1)
    Un, Kn = _inputs(d, U, K, 0, n)
    if with_X:
        X = mvi.rollout(n, DT, Un, Kn)
    else:
        mvi.rollout_device(n, DT, mvi.device_array(Un) if Un is not None else None, mvi.device_array(Kn) if Kn is not None else None, None)
        mvi.synchronize()
    iters, status = mvi.status()
    q2, p2, lam1 = mvi.q2, mvi.p2, mvi.lambda1
    _assert_spec_rollout(mvi, exact)
    mvi.close()
    assert (status == 0).all(), status
    worst = dict(X=0.0, q2=0.0, p2=0.0, lambda1=0.0)
    for b in range(B):
        if with_X:
            worst["X"] = max(worst["X"], relerr(X[b], Xo[b, :n + 1]))
        worst["q2"] = max(worst["q2"], relerr(q2[b], Xo[b, n, :nq]))
        worst["p2"] = max(worst["p2"], relerr(p2[b], Xo[b, n, nq:nq + nd]))
        worst["lambda1"] = max(worst["lambda1"], relerr(lam1[b], lam[b, n - 1]))
    print("%s n=%d exact=%d X=%d:" % (name, n, exact, with_X), " ".join("%s %.2e" % kv for kv in sorted(worst.items())),
          "iterations %s / oracle %s" % (iters.tolist(), its[:, :n].sum(1).tolist()))
    assert worst["X"] < TOL and worst["q2"] < TOL and worst["p2"] < TOL, (name, n, worst)
    assert worst["lambda1"] < TB_TOL["lambda1"], (name, n, worst)
    assert np.array_equal(iters, its[:, :n].sum(1))


@pytest.mark.parametrize("name,to_the_bit", [("puppet40", True), ("puppet_basic", False)])
def test_two_rollouts_of_six_steps_equal_one_of_twelve(name, to_the_bit):
    """The state a rollout leaves (q1, q2, p1, p2, lambda1, written behind its last step) is the state the edge hands to the next step
    inside a longer one.  puppet40: bit for bit -- rows, final state, iteration counts.  (Row 0 of the second rollout's X forms its v
    part with the rounded t2 - t1 of the batch's clock: that part to TOL.)
    puppet_basic: the first half and row 0 of the second bit for bit -- that is the write-back --, the rest of the second half to TOL.
    Step 0 of a launch forms Dh1 with a constraint sweep of its own at q1 (eval_constraints), a later step copies the Dh2 of the step
    before: the same point through another instruction sequence, and on this system the two differ in the last bits.  The parent commit
    shows the same figures as this tree (rows 7.878e-13, p1 7.878e-13, p2 5.969e-13, lambda1 3.8e-15 absolute): the difference is a
    property of a launch's first step, not of the edge; both runs are within TOL of the oracle."""
    system, d, Q0, Q1, U, K, Xo, its, lam = _reference(name)
    nq, nd = d.n_configs, d.n_dyn
    h = N // 2
    mvi = _batch(system)
    mvi.initialize_from_configs(0.0, Q0, DT, Q1)
    X12 = mvi.rollout(N, DT, *_inputs(d, U, K, 0, N))
    it12, st12 = mvi.status()
    end12 = (mvi.q1, mvi.q2, mvi.p1, mvi.p2, mvi.lambda1)
    mvi.initialize_from_configs(0.0, Q0, DT, Q1)
    Xa = mvi.rollout(h, DT, *_inputs(d, U, K, 0, h))
    ita, sta = mvi.status()
    Xb = mvi.rollout(h, DT, *_inputs(d, U, K, h, N))
    itb, stb = mvi.status()
    end6 = (mvi.q1, mvi.q2, mvi.p1, mvi.p2, mvi.lambda1)
    _assert_spec_rollout(mvi)
    mvi.close()
    assert (st12 == 0).all() and (sta == 0).all() and (stb == 0).all()
    print("%s: first half |dX| %.3e, second half rows 1.. %.3e, row 0 (q, p) %.3e;" % (
        name, np.abs(Xa - X12[:, :h + 1]).max(), np.abs(Xb[:, 1:] - X12[:, h + 1:]).max(), np.abs(Xb[:, 0, :nq + nd] - X12[:, h, :nq + nd]).max()),
        "final state", " ".join("%.3e" % np.abs(a - b).max() for a, b in zip(end6, end12) if a.size), "iterations", (ita + itb).tolist(), it12.tolist())
    assert np.array_equal(Xa, X12[:, :h + 1])
    assert np.array_equal(Xb[:, 0, :nq + nd], X12[:, h, :nq + nd])
    assert relerr(Xb[:, 0, nq + nd:], X12[:, h, nq + nd:]) < TOL
    if to_the_bit:
        assert np.array_equal(Xb[:, 1:], X12[:, h + 1:])
        for a, b in zip(end6, end12):
            assert np.array_equal(a, b)
    else:
        for b in range(B):
            assert relerr(Xb[b, 1:], X12[b, h + 1:]) < TOL, (name, b)
            assert relerr(Xb[b, 1:], Xo[b, h + 1:]) < TOL, (name, b)
        for a, b in zip(end6, end12):
            assert relerr(a, b) < TOL
    assert np.array_equal(ita + itb, it12) and np.array_equal(it12, its.sum(1))
    for b in range(B):
        assert relerr(X12[b], Xo[b]) < TOL, (name, b)


def test_non_uniform_time_base_across_the_edge():
    """Alternating steps of 0.6 DT and 1.5 DT: the v part of row k + 1 is (k2 - k1) / dt_k, the rates of step k + 1 are over dt_{k+1}
    -- both formed in the same phase."""
    name = "puppet40"
    system, d, Q0, Q1, U, K, Xo, its, lam = _reference(name)
    nq, nd = d.n_configs, d.n_dyn
    dts = tb_step_sizes("alternating", N)
    ref = [tb_oracle_rollout(d, Q0[b], Q1[b], dts, U[b], K[b]) for b in range(B)]
    mvi = _batch(system)
    mvi.initialize_from_configs(0.0, Q0, DT, Q1)
    X = mvi.rollout(N, dts, *_inputs(d, U, K, 0, N))
    iters, status = mvi.status()
    p1, p2 = mvi.p1, mvi.p2
    _assert_spec_rollout(mvi)
    mvi.close()
    assert (status == 0).all(), status
    errs = [relerr(X[b], r["X"]) for b, r in enumerate(ref)]
    print("non-uniform: X %.2e, iterations %s / oracle %s" % (max(errs), iters.tolist(), [r["iterations"] for r in ref]))
    for b, r in enumerate(ref):
        assert errs[b] < TOL, (b, errs[b])
        assert relerr(p1[b], r["p1"]) < TOL and relerr(p2[b], r["p2"]) < TOL, b
        v = (X[b, 1:, nd:nq] - X[b, :-1, nd:nq]) / dts[:, None]
        assert relerr(X[b, 1:, nq + nd:], v) < TOL, b
    assert np.array_equal(iters, np.array([r["iterations"] for r in ref]))


def test_extrapolating_predictor_keeps_the_separate_phases():
    """predictor = "extrapolate" takes the step set-up as it was (q2 is extrapolated from q1 before the shift).  Both sides solve to
    common.TB_PREDICTOR_TOL, as in tests/test_gpu_time_base.py: a warm start inside the tolerance ball is accepted as it is."""
    from oracle.oracle import OracleMVI
    name = "puppet40"
    system, d, Q0, Q1, U, K, Xo, its, lam = _reference(name)
    ref = []
    for b in range(B):
        o = OracleMVI(d, tolerance=TB_PREDICTOR_TOL)
        o.initialize_from_configs(0.0, Q0[b], DT, Q1[b])
        ref.append(tb_oracle_rollout(d, None, None, np.full(N, DT), U[b], K[b], o=o))
    mvi = _batch(system)
    mvi.tolerance = TB_PREDICTOR_TOL
    runs = {}
    for mode in ("reference", "extrapolate"):
        mvi.predictor = mode
        mvi.initialize_from_configs(0.0, Q0, DT, Q1)
        X = mvi.rollout(N, DT, *_inputs(d, U, K, 0, N))
        iters, status = mvi.status()
        assert (status == 0).all(), mode
        errs = [relerr(X[b], r["X"]) for b, r in enumerate(ref)]
        print(mode, "X %.2e" % max(errs), "iterations", iters.tolist(), "oracle", [r["iterations"] for r in ref])
        assert max(errs) < TOL, (mode, errs)
        runs[mode] = iters
    _assert_spec_rollout(mvi)
    mvi.close()
    # (at this tolerance a step's last residual sits near the rounding floor: the totals to one iteration, as in that file; the
    # extrapolated run has fewer by design)
    for b, r in enumerate(ref):
        assert abs(int(runs["reference"][b]) - r["iterations"]) <= 1, (b, runs["reference"][b], r["iterations"])
    assert (runs["extrapolate"] <= runs["reference"]).all(), runs
