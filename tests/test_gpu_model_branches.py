"""The generic kernels on the model branches only spatial_loop and mixed_loop reach, against the oracle: every component of a point
constraint (PointToPoint3D, PointToPoint2D 'yz'), a plane normal carried through a constant rotation, a const_se3 with a rotation,
kinematic rotary configs (at the root and in the middle of a chain) and a kinematic tz, a BodyWrench next to them.

One full block of teams plus a ragged one (common.mb_batch), MB_N = 12 steps from starts on the recorded trajectories.  The reference is
OracleMVI (common.mb_reference); the bounds are the project's tolerances (common.TB_TOL), raised through max(tolerance, 64 e_ref) only for
the quantities listed in common.MB_SECOND_TERM, e_ref being the oracle's own response to one ulp of the start.
test_model_branches_cpu.py shows with the oracle alone that getting one of these branches wrong is at least 1e3 tolerances away."""
import numpy as np
import pytest

from common import (D1, MB_CLOSED_LOOP, MB_GENERIC, MB_N, MB_TEAM, TB_DT, TB_GROUP, build, mb_batch, mb_bound, mb_case,
                    mb_contraction, mb_e_ref, mb_reference, oracle_hz, relerr, tb_AB, tb_closed_loop_inputs, tb_closed_loop_reference)
from oracle.oracle import OracleMVI
from test_gpu_time_base import _force, _in
from trep_amd import BatchMidpointVI

pytestmark = pytest.mark.gpu

DT = TB_DT
N = MB_N


def _batch(monkeypatch, name):
    monkeypatch.delenv("TREPAMD_TEAM", raising=False)
    system, _ = build(name)
    mvi = BatchMidpointVI(system, mb_batch(name), specialize=False)
    assert mvi.kernel_info()["team"] == MB_TEAM[name], mvi.kernel_info()
    return mvi


def _assert_generic(mvi, modes):
    info = mvi.kernel_info()
    for m in modes:
        bit = BatchMidpointVI.ALL_MODES[m]
        assert (info["generic_launch_mask"] >> bit) & 1 and not (info["spec_launch_mask"] >> bit) & 1, (m, info)
    assert info["spec_launches"] == 0 and info["par_spec_launches"] == 0 and info["par_generic_launches"] == 0, info


def run_generic(monkeypatch, name):
    """The checks of test_rollout_and_derivatives_match_oracle; returns the worst error per quantity (tools/model_branches_parity.py)."""
    c, ref, e_ref = mb_case(name), mb_reference(name), mb_e_ref(name)
    d, B = c["d"], c["B"]
    nc = d.n_constraints
    Z, ZL = mb_contraction(name)
    mvi = _batch(monkeypatch, name)
    mvi.initialize_from_configs(0.0, c["Q0"], DT, c["Q1"])
    X = mvi.rollout(N, DT, _in(c, "U", 0, N), _in(c, "K", 0, N))
    iters, status = mvi.status()
    assert (status == 0).all(), (name, status)
    p1, p2, lam = mvi.p1, mvi.p2, mvi.lambda1
    worst = {}

    def check(q, got, want, b):
        e = relerr(got, want)
        worst[q] = max(worst.get(q, 0.0), e)
        print("%s %s[%d] %.2e (bound %.2e)" % (name, q, b, e, mb_bound(name, q, e_ref)))
        assert e < mb_bound(name, q, e_ref), (name, q, b, e)
    for b, r in enumerate(ref):
        for q, got in (("X", X[b]), ("p1", p1[b]), ("p2", p2[b]), ("lambda1", lam[b])):
            check(q, got, r[q], b)
        assert int(iters[b]) == r["iterations"], (name, b, int(iters[b]), r["iterations"])
    # the non-rollout modes at exactly the oracles' last step
    _force(mvi, ref)
    f = mvi.calc_f()
    mvi.calc_p2()
    cp2 = mvi.p2
    _force(mvi, ref)
    mvi.calc_deriv1()
    d1 = dict((n, mvi.deriv1(n)) for n in D1)
    HZ = mvi.deriv2_contract(Z, ZL)
    HZ0 = mvi.deriv2_contract(Z, None)
    for b, r in enumerate(ref):
        check("f", f[b], r["f"], b)
        check("calc_p2", cp2[b], r["calc_p2"], b)
        e1 = max(relerr(d1[n][b], r["d1"][n]) for n in D1)
        worst["d1"] = max(worst.get("d1", 0.0), e1)
        assert e1 < mb_bound(name, "d1", e_ref), (name, "d1", b, e1)
        A, Bm = tb_AB(d, dict((n, d1[n][b]) for n in D1), mvi.times()[1] - mvi.times()[0])
        check("AB", np.concatenate([A.ravel(), Bm.ravel()]), np.concatenate([r["A"].ravel(), r["B"].ravel()]), b)
        check("hz", HZ[b], r["hz"], b)
        check("hz", HZ0[b], oracle_hz(r["o"], d, Z[b], np.zeros(nc)), b)         # (the oracle's tensors are still those of its last step)
    print(name, " ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    _assert_generic(mvi, ["rollout", "calc_p2", "calc_f", "deriv1", "deriv2z"])
    mvi.close()
    return worst


@pytest.mark.parametrize("name", MB_GENERIC)
def test_rollout_and_derivatives_match_oracle(monkeypatch, name):
    """calc_p2 of the start, the rollout (X with its v rows, p1, p2, lambda1, Newton iterations equal to the oracle's), calc_f, calc_p2,
    deriv1, the linearisation A / B, deriv2z with and without the lambda contraction."""
    run_generic(monkeypatch, name)


@pytest.mark.parametrize("name", MB_GENERIC)
def test_continuous_modes_match_oracle(monkeypatch, name):
    """dynamics, dynamics_deriv1, energy and lagrangian at random states near the recorded ones; every ddq_k of the kinematic (rotary)
    configs is drawn."""
    c, ref = mb_case(name), mb_reference(name)
    d, B = c["d"], c["B"]
    nq, nu, nk = d.n_configs, d.n_inputs, d.n_kin
    rng = np.random.default_rng(5 + len(name))
    Qs = np.array([r["X"][-1, :nq] for r in ref]) + 0.05 * rng.standard_normal((B, nq))
    dQs, Us, Ks = rng.standard_normal((B, nq)), rng.standard_normal((B, nu)), rng.standard_normal((B, nk))
    mvi = _batch(monkeypatch, name)
    ddq, lmb, st = mvi.dynamics(Qs, dQs, Us if nu else None, Ks)
    assert (st == 0).all()
    TV = mvi.energy(Qs, dQs)
    lag = mvi.lagrangian(Qs, dQs)
    dd1, st = mvi.dynamics_deriv1(Qs, dQs, Us if nu else None, Ks)
    assert (st == 0).all()
    keys = ("L_dq", "L_ddq", "L_dqdq", "L_ddqdq", "L_ddqddq")
    o = OracleMVI(d)                # (one of its own: the cached references' oracles stay at their last step)
    for b in range(B):
        fo, lo = o.dynamics(Qs[b], dQs[b], Us[b], Ks[b])
        assert relerr(ddq[b], fo) < 1e-9 and relerr(lmb[b], lo) < 1e-9, (name, b)
        T, V = o.energy(Qs[b], dQs[b])
        assert relerr(TV[b, 0] + TV[b, 1], T + V) < 1e-11 and relerr(TV[b, 0] - TV[b, 1], T - V) < 1e-11, (name, b)
        for key, want in zip(keys, o.lagrangian(Qs[b], dQs[b])):
            assert relerr(lag[key][b], want) < 1e-11, (name, b, key)
        for key, val in o.dynamics_deriv1(Qs[b], dQs[b], Us[b], Ks[b]).items():
            assert relerr(dd1[key.replace("lam_", "lambda_")][b], val) < 1e-9, (name, b, key)
    _assert_generic(mvi, ["dynamics", "energy", "lagrangian", "dynamics_deriv1"])
    mvi.close()


@pytest.mark.parametrize("name", MB_CLOSED_LOOP)
def test_closed_loop_rollout_matches_oracle(monkeypatch, name):
    """U_k = bU_k - K_k (X_k - bX_k) inside the rollout kernel, TB_GROUP trajectories per gain set, against the numpy loop over oracle steps."""
    c = mb_case(name)
    B = c["B"]
    Kp, bX, bU = tb_closed_loop_inputs(name, "uniform", N, B)
    ref = tb_closed_loop_reference(name, "uniform", N, B)
    e_ref = mb_e_ref(name, closed_loop=True)
    mvi = _batch(monkeypatch, name)
    mvi.initialize_from_configs(0.0, c["Q0"], DT, c["Q1"])
    X, U = mvi.rollout_closed_loop(N, DT, Kp, bX, bU, group_size=TB_GROUP)
    iters, status = mvi.status()
    assert (status == 0).all(), status
    for b, r in enumerate(ref):
        for q, got in (("X", X[b]), ("U", U[b]), ("p2", mvi.p2[b]), ("lambda1", mvi.lambda1[b])):
            e = relerr(got, r[q])
            print("%s closed loop %s[%d] %.2e" % (name, q, b, e))
            assert e < mb_bound(name, q, e_ref), (name, q, b, e)
        assert int(iters[b]) == r["iterations"], (name, b)
    _assert_generic(mvi, ["rollout"])
    mvi.close()
