"""Carried poses of the specialised rollout kernels (pose_sweep_dual, csrc/mvi_core.hpp; program.hpp, PoseCarry).

The first evaluation of a step the step edge has set up takes its midpoint and q2 poses from the q2 poses the converged evaluation of
the step before left in LDS: a copy per (midpoint, joint) item, the closed forms of the run joints a kinematic config moves, no sin/cos,
no chain round.  Every other evaluation -- step 0, the ones behind a Newton update, the extrapolating predictor, a failed trajectory --
sweeps as before.  Results may not move: states to TOL of the oracle, multipliers to common.TB_TOL["lambda1"], Newton iterations per
trajectory equal to the oracle's (tests/test_gpu_rollout_step_edge.py's tolerances, B = 5 and starts: steps of 2, 3 and 4 iterations).

N = 1 has no carried evaluation, N = 2 one (into the last step, whose tail takes the separate phases), N = 3 two.  The kinematic targets
either move every kinematic config at every step (by a different amount each: the twelve string joints' closed forms see a new value on
every row they copy) or stay where the start has them (then nothing at all moves across the edge but q2 itself)."""
import functools

import numpy as np
import pytest

from common import BUILDERS, TB_PREDICTOR_TOL, TB_TOL, relerr, tb_oracle_rollout, tb_state, tb_step_sizes
from test_gpu_rollout_step_edge import _reference as _edge_reference
from test_parameters_cpu import random_rows, rebuilt

pytestmark = pytest.mark.gpu

DT = 0.01
TOL = 1e-10      # tests/test_gpu_rollout_step_edge.py
B, N = 5, 3
CARRY = {"puppet40": 2, "puppet_basic": 2}       # joints without a q2 twin (tests/test_pose_carry_plan_cpu.py)
CASES = [("puppet40", "moving"), ("puppet40", "constant"), ("puppet_basic", "none")]


def _targets(d, Q1, K, kind, n):
    """K [B][n][nk]: the recorded schedule's first rows plus a step that differs per config and grows per step, or the start's values"""
    nd, nk = d.n_dyn, d.n_kin
    if nk == 0:
        return np.zeros((B, n, 0))
    if kind == "constant":
        return np.repeat(Q1[:, None, nd:], n, axis=1)
    step = 2e-4 * (1.0 + np.arange(nk) / nk) * np.where(np.arange(nk) % 2 == 0, 1.0, -1.0)
    out = K[:, :n] + (np.arange(n)[None, :, None] + 1.0) * step[None, None, :]
    assert (np.diff(np.concatenate([Q1[:, None, nd:], out], axis=1), axis=1) != 0.0).all()      # (of the case: every config moves at every step)
    return out


def _oracle_steps(d, q0, q1, dts, U, K, o=None):
    """X [n + 1], Newton iterations per step and the multipliers after every step of one trajectory"""
    from oracle.oracle import OracleMVI
    if o is None:
        o = OracleMVI(d)
        o.initialize_from_configs(0.0, q0, DT, q1)
    n = len(dts)
    X = np.zeros((n + 1, o.nq + o.nd + o.nk))
    its, lam = np.zeros(n, dtype=int), np.zeros((n, d.n_constraints))
    t1, t2 = o.times()
    X[0] = tb_state(o, t2 - t1)
    for k in range(n):
        its[k] = o.step(o.times()[1] + dts[k], U[k], K[k])
        X[k + 1] = tb_state(o, dts[k])
        lam[k] = o.lambda1
    return X, its, lam


@functools.lru_cache(maxsize=None)
def _reference(name, kind, pattern="uniform", n=N):
    """Starts, inputs, targets and the oracle's run of a case.  Computed once, read-only."""
    system, d, Q0, Q1, U, K0, _, _, _ = _edge_reference(name)
    K = _targets(d, Q1, K0, kind, n)
    dts = tb_step_sizes(pattern, n)
    runs = [_oracle_steps(d, Q0[b], Q1[b], dts, U[b, :n], K[b]) for b in range(B)]
    X, its, lam = (np.array([r[i] for r in runs]) for i in range(3))
    for a in (K, X, its, lam, dts):
        a.setflags(write=False)
    return system, d, Q0, Q1, U[:, :n], K, X, its, lam, dts


def _batch(system, exact=False, specialize=True):
    import trep_amd
    mvi = trep_amd.BatchMidpointVI(system, B, specialize=specialize)
    mvi.exact_pivot = exact
    return mvi


def _io(d, U, K, n0, n1):
    return (np.ascontiguousarray(U[:, n0:n1]) if d.n_inputs else None, np.ascontiguousarray(K[:, n0:n1]) if d.n_kin else None)


def _assert_carrying_kernel(mvi, name, par=False):
    """The specialised (parameter) rollout kernel ran and the loaded library was COMPILED with the plan's cells (tg_spec_pose_carry reports
    tg_static_carry).  It is no record that a carried evaluation ran: that also needs the step-edge path at a step that is not a launch's
    first -- which the cases provide by their N, predictor and inputs, and which the results, not this flag, bear out."""
    kinfo, info = mvi.kernel_info(), mvi.info()
    assert "rollout" in kinfo["par_spec_launched" if par else "spec_launched"], kinfo
    assert "rollout" not in kinfo["generic_launched"] and "rollout" not in kinfo["par_generic_launched"], kinfo
    assert kinfo["pose_carry"] is True and kinfo["n_carry"] == CARRY[name] and info["pose_carry"] is True and info["n_carry"] == CARRY[name], kinfo


@pytest.mark.parametrize("name,kind", CASES)
def test_rollout_matches_oracle(name, kind):
    system, d, Q0, Q1, U, K, Xo, its, lam, _ = _reference(name, kind)
    nq, nd = d.n_configs, d.n_dyn
    mvi = _batch(system)
    for n in (1, 2, 3):
        for exact in (False, True):
            for with_X in (True, False):
                mvi.exact_pivot = exact
                mvi.initialize_from_configs(0.0, Q0, DT, Q1)
                Un, Kn = _io(d, U, K, 0, n)
                if with_X:
                    X = mvi.rollout(n, DT, Un, Kn)
                else:
                    ptrs = [mvi.device_array(a) if a is not None else None for a in (Un, Kn)]
                    mvi.rollout_device(n, DT, ptrs[0], ptrs[1], None)
                    mvi.synchronize()
                iters, status = mvi.status()
                q2, p2, lam1 = mvi.q2, mvi.p2, mvi.lambda1
                assert mvi.kernel_info()["exact_pivot"] == exact
                assert (status == 0).all(), (n, exact, with_X, status)
                worst = dict(X=0.0, q2=0.0, p2=0.0, lambda1=0.0)
                for b in range(B):
                    if with_X:
                        worst["X"] = max(worst["X"], relerr(X[b], Xo[b, :n + 1]))
                    worst["q2"] = max(worst["q2"], relerr(q2[b], Xo[b, n, :nq]))
                    worst["p2"] = max(worst["p2"], relerr(p2[b], Xo[b, n, nq:nq + nd]))
                    worst["lambda1"] = max(worst["lambda1"], relerr(lam1[b], lam[b, n - 1]))
                print("%s %s n=%d exact=%d X=%d:" % (name, kind, n, exact, with_X), " ".join("%s %.2e" % kv for kv in sorted(worst.items())),
                      "iterations %s / oracle %s" % (iters.tolist(), its[:, :n].sum(1).tolist()))
                assert worst["X"] < TOL and worst["q2"] < TOL and worst["p2"] < TOL, (name, kind, n, exact, with_X, worst)
                assert worst["lambda1"] < TB_TOL["lambda1"], (name, kind, n, exact, with_X, worst)
                assert np.array_equal(iters, its[:, :n].sum(1)), (n, exact, with_X)
    _assert_carrying_kernel(mvi, name)
    mvi.close()


# the PARENT commit's figures of the stepwise witness (its specialised kernels, an MI355X; printed with %.3e): max |X1 - X12| over all rows,
# then max |difference| of q1, q2, p1, p2, lambda1 of the final state
WITNESS = {
    "puppet40": ("2.505e-13", ("1.554e-15", "3.060e-15", "7.577e-14", "1.977e-13", "2.213e-13")),
    "puppet_basic": ("1.280e-11", ("4.940e-15", "4.774e-15", "4.802e-12", "1.119e-11", "1.053e-13")),
}


def _held(value, recorded):
    """equal to the parent's recorded figure (to the digits it was recorded with), or smaller"""
    return "%.3e" % value == recorded or value <= float(recorded)


@pytest.mark.parametrize("name", ["puppet40", "puppet_basic"])
def test_twelve_launches_of_one_step_equal_one_launch_of_twelve(name):
    """A launch of one step never carries (step 0 sweeps, and it is the last step too); a launch of twelve carries eleven times.  The
    comparison is the 6 + 6 one of tests/test_gpu_rollout_step_edge.py taken to its end.  On the PARENT commit it is bit for bit in the
    first step alone (both sides run it as a launch's step 0) and not behind it, on both systems: every launch's first step forms Dh1
    with a sweep of its own where a later step of a longer launch copies Dh2 -- the same point through another instruction sequence --
    and a one-step launch has the tail's p2 where the longer one has the edge's.  What the parent shows for this very comparison is
    recorded in WITNESS, and the tree is held to it: the first step bit for bit, and the largest difference of the rows and of every
    array of the final state EQUAL TO THE PARENT'S FIGURE OR SMALLER -- a carried pose that differed from the swept one in its last
    bits would move them (the kernels are deterministic; this tree shows the parent's figures digit for digit, docs/LOG.md).  Besides:
    everything within TOL of the oracle, iteration counts equal."""
    system, d, Q0, Q1, U, K, Xo, its, lam = _edge_reference(name)
    nq, nd = d.n_configs, d.n_dyn
    n = Xo.shape[1] - 1
    mvi = _batch(system)
    mvi.initialize_from_configs(0.0, Q0, DT, Q1)
    X12 = mvi.rollout(n, DT, *_io(d, U, K, 0, n))
    it12, st12 = mvi.status()
    end12 = (mvi.q1, mvi.q2, mvi.p1, mvi.p2, mvi.lambda1)
    mvi.initialize_from_configs(0.0, Q0, DT, Q1)
    X1 = np.zeros_like(X12)
    it1 = np.zeros_like(it12)
    for k in range(n):
        Xk = mvi.rollout(1, DT, *_io(d, U, K, k, k + 1))
        it, st = mvi.status()
        assert (st == 0).all(), k
        it1 += it
        if k == 0:
            X1[:, 0] = Xk[:, 0]
        X1[:, k + 1] = Xk[:, 1]
    end1 = (mvi.q1, mvi.q2, mvi.p1, mvi.p2, mvi.lambda1)
    _assert_carrying_kernel(mvi, name)
    mvi.close()
    assert (st12 == 0).all()
    rows = float(np.abs(X1 - X12).max())
    ends = [float(np.abs(a - b).max()) for a, b in zip(end1, end12)]
    print("%s: twelve launches against one, rows |dX| %.3e;" % (name, rows), "final state", " ".join("%.3e" % e for e in ends),
          "(parent: %s; %s)" % (WITNESS[name][0], " ".join(WITNESS[name][1])), "iterations", it1.tolist(), it12.tolist())
    assert np.array_equal(X1[:, :2], X12[:, :2])          # (the first step of both is a launch's step 0)
    assert _held(rows, WITNESS[name][0]), (name, rows, WITNESS[name][0])
    for what, e, rec in zip(("q1", "q2", "p1", "p2", "lambda1"), ends, WITNESS[name][1]):
        assert _held(e, rec), (name, what, e, rec)
    assert np.array_equal(it1, it12) and np.array_equal(it12, its.sum(1))
    for b in range(B):
        assert relerr(X12[b], Xo[b]) < TOL and relerr(X1[b], Xo[b]) < TOL, (name, b)


@pytest.mark.parametrize("name,kind", [("puppet40", "moving"), ("puppet_basic", "none")])
def test_same_batch_on_the_generic_kernel(name, kind):
    system, d, Q0, Q1, U, K, Xo, its, lam, _ = _reference(name, kind)
    runs = {}
    for spec in (True, False):
        mvi = _batch(system, specialize=spec)
        mvi.initialize_from_configs(0.0, Q0, DT, Q1)
        X = mvi.rollout(N, DT, *_io(d, U, K, 0, N))
        runs[spec] = (X, mvi.status(), mvi.lambda1)
        if spec:
            _assert_carrying_kernel(mvi, name)
        else:
            assert "rollout" in mvi.kernel_info()["generic_launched"] and mvi.kernel_info()["pose_carry"] is False
        mvi.close()
    (Xs, (its_s, st_s), lam_s), (Xg, (its_g, st_g), lam_g) = runs[True], runs[False]
    print("%s: specialised against generic X %.2e lambda1 %.2e" % (name, relerr(Xs, Xg), relerr(lam_s, lam_g)))
    assert (st_s == 0).all() and (st_g == 0).all()
    for b in range(B):
        assert relerr(Xs[b], Xg[b]) < TOL, (name, b)
    assert relerr(lam_s, lam_g) < TB_TOL["lambda1"]
    assert np.array_equal(its_s, its_g) and np.array_equal(its_s, its.sum(1))


def test_a_trajectory_that_stops_converging_mid_rollout():
    """max_iterations = 2 fails every step that needs four Newton iterations: the trajectory freezes there with its status, behind one
    or more carried steps, and takes no edge any more; the others go on carrying.  Status and iterations as the generic kernel reports
    them; the trajectories that never meet such a step equal the oracle's unrestricted run."""
    name, M = "puppet40", 2
    system, d, Q0, Q1, U, K, Xo, its, lam = _edge_reference(name)
    n = its.shape[1]
    fails = (its >= M + 2)
    first = np.where(fails.any(1), fails.argmax(1), n)
    assert (first > 0).any() and (first[first < n] > 0).any() and (first == n).any(), first      # (of the cases: a failure behind an edge, a clean run)
    runs = {}
    for spec in (True, False):
        mvi = _batch(system, specialize=spec)
        mvi.initialize_from_configs(0.0, Q0, DT, Q1)
        X = mvi.rollout(n, DT, *_io(d, U, K, 0, n), max_iterations=M)
        runs[spec] = (X, mvi.status(), mvi.q2)
        if spec:
            _assert_carrying_kernel(mvi, name)
        mvi.close()
    (Xs, (its_s, st_s), q2_s), (Xg, (its_g, st_g), q2_g) = runs[True], runs[False]
    print("limited: first failing step %s, status %s / generic %s, iterations %s / generic %s" % (first.tolist(), st_s.tolist(), st_g.tolist(), its_s.tolist(), its_g.tolist()))
    assert np.array_equal(st_s, st_g) and np.array_equal(its_s, its_g)
    assert np.array_equal(st_s != 0, first < n)
    for b in range(B):
        k = int(first[b])
        assert relerr(Xs[b, :k + 1], Xo[b, :k + 1]) < TOL, b            # rows up to the failing step (all of them for a clean run)
        assert relerr(Xs[b, :k + 1], Xg[b, :k + 1]) < TOL, b
        if k == n:
            assert int(its_s[b]) == int(its[b].sum()), b
    assert relerr(q2_s[first == n], q2_g[first == n]) < TOL


def test_alternating_step_sizes_across_the_edge():
    name = "puppet40"
    system, d, Q0, Q1, U, K, Xo, its, lam, dts = _reference(name, "moving", "alternating", 4)
    assert dts[0] != dts[1]
    mvi = _batch(system)
    mvi.initialize_from_configs(0.0, Q0, DT, Q1)
    X = mvi.rollout(4, np.array(dts), *_io(d, U, K, 0, 4))
    iters, status = mvi.status()
    lam1 = mvi.lambda1
    _assert_carrying_kernel(mvi, name)
    mvi.close()
    assert (status == 0).all(), status
    print("alternating: X %.2e lambda1 %.2e iterations %s / oracle %s" % (max(relerr(X[b], Xo[b]) for b in range(B)), relerr(lam1, lam[:, -1]), iters.tolist(), its.sum(1).tolist()))
    for b in range(B):
        assert relerr(X[b], Xo[b]) < TOL, b
    assert relerr(lam1, lam[:, -1]) < TB_TOL["lambda1"]
    assert np.array_equal(iters, its.sum(1))


def test_extrapolating_predictor_takes_no_edge_and_carries_nothing():
    """predictor = "extrapolate": q2 is not q1 at a step's first evaluation, the step edge is not taken, every evaluation sweeps.  Both
    sides solve to common.TB_PREDICTOR_TOL, as in tests/test_gpu_rollout_step_edge.py."""
    from oracle.oracle import OracleMVI
    name = "puppet40"
    system, d, Q0, Q1, U, K, _, _, _, dts = _reference(name, "moving")
    ref = []
    for b in range(B):
        o = OracleMVI(d, tolerance=TB_PREDICTOR_TOL)
        o.initialize_from_configs(0.0, Q0[b], DT, Q1[b])
        ref.append(tb_oracle_rollout(d, None, None, np.array(dts), U[b], K[b], o=o))
    mvi = _batch(system)
    mvi.tolerance = TB_PREDICTOR_TOL
    runs = {}
    for mode in ("reference", "extrapolate"):
        mvi.predictor = mode
        mvi.initialize_from_configs(0.0, Q0, DT, Q1)
        X = mvi.rollout(N, DT, *_io(d, U, K, 0, N))
        iters, status = mvi.status()
        assert (status == 0).all(), mode
        errs = [relerr(X[b], r["X"]) for b, r in enumerate(ref)]
        print(mode, "X %.2e" % max(errs), "iterations", iters.tolist(), "oracle", [r["iterations"] for r in ref])
        assert max(errs) < TOL, (mode, errs)
        runs[mode] = iters
    _assert_carrying_kernel(mvi, name)
    mvi.close()
    for b, r in enumerate(ref):      # (at this tolerance a step's last residual sits near the rounding floor: the totals to one iteration, as in that file)
        assert abs(int(runs["reference"][b]) - r["iterations"]) <= 1, (b, runs["reference"][b], r["iterations"])
    assert (runs["extrapolate"] <= runs["reference"]).all(), runs


def test_puppet_under_a_parameter_table():
    """k_spec_par: every trajectory with masses, gravity and damping of its own, against the oracle of the system rebuilt with that row"""
    from oracle.oracle import OracleMVI
    from trep_amd import descriptor
    name = "puppet40"
    make = BUILDERS[name]
    system, d, Q0, Q1, U, K, _, _, _, dts = _reference(name, "moving")
    nq, nd = d.n_configs, d.n_dyn
    rows = random_rows(system, B, seed=33)
    mvi = _batch(system)
    mvi.set_parameters(**rows)
    mvi.initialize_from_configs(0.0, Q0, DT, Q1)
    X = mvi.rollout(N, DT, *_io(d, U, K, 0, N))
    iters, status = mvi.status()
    lam1 = mvi.lambda1
    _assert_carrying_kernel(mvi, name, par=True)
    mvi.close()
    assert (status == 0).all(), status
    for b in range(B):
        db = descriptor.flatten(rebuilt(make, rows, b))
        Xo, its, lam = _oracle_steps(db, Q0[b], Q1[b], dts, U[b], K[b])
        print("row %d: X %.2e lambda1 %.2e iterations %d / oracle %d" % (b, relerr(X[b], Xo), relerr(lam1[b], lam[-1]), iters[b], its.sum()))
        assert relerr(X[b], Xo) < TOL, b
        assert relerr(lam1[b], lam[-1]) < TB_TOL["lambda1"], b
        assert int(iters[b]) == int(its.sum()), b


def test_deriv1_behind_a_carrying_rollout():
    """The derivative kernels keep their own sweep of every joint (rollout_lists == false) and the LDS slice is theirs from the start:
    the first derivatives of the last step of a rollout that carried, against the oracle's."""
    from oracle.oracle import OracleMVI
    name = "puppet40"
    system, d, Q0, Q1, U, K, Xo, its, lam, dts = _reference(name, "moving")
    mvi = _batch(system)
    mvi.initialize_from_configs(0.0, Q0, DT, Q1)
    mvi.rollout(N, DT, *_io(d, U, K, 0, N))
    assert (mvi.status()[1] == 0).all()
    mvi.calc_deriv1()
    d1 = dict((n, mvi.deriv1(n)) for n in mvi.D1_NAMES)
    kinfo = mvi.kernel_info()
    _assert_carrying_kernel(mvi, name)
    mvi.close()
    assert "deriv1" in kinfo["spec_launched"], kinfo
    worst = 0.0
    for b in range(B):
        o = OracleMVI(d)
        o.initialize_from_configs(0.0, Q0[b], DT, Q1[b])
        for k in range(N):
            o.step(o.times()[1] + DT, U[b, k], K[b, k])
        o.calc_deriv1()
        for n in mvi.D1_NAMES:
            e = relerr(d1[n][b], o.deriv1(n))
            worst = max(worst, e)
            assert e < TB_TOL["d1"], (b, n, e)
    print("deriv1 behind a rollout of %d steps: worst %.2e" % (N, worst))
