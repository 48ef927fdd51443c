"""Every team size of the generic kernels (1, 4, 16 or 64 lanes per trajectory, forced with TREPAMD_TEAM) against the oracle.

A system normally gets one team size (trepamd.hip, pick_team), so most (team, feature) instantiations in the library never run on
the test systems.  Here each cell of common.TEAM_CELLS runs every kernel mode at its forced team on ragged batches whose teams in one
wavefront hold different trajectories, checks the refusals of blocks over 160 KiB of LDS, the remapped launches, the parameter
kernels, and that a trajectory that fails to converge (or sees NaN) leaves its wave neighbours bit-for-bit unchanged."""
import numpy as np
import pytest

from common import (BUILDERS, D1, NO_SECOND_ORDER, RANGE_CASES, TEAM_CELLS, build, relerr)
from common import oracle_hz as _oracle_hz, starts as _starts
from oracle.oracle import OracleError, OracleMVI
from test_parameters_cpu import random_rows, rebuilt
from trep_amd import BatchMidpointVI, _lib, descriptor
from trep_amd._lib import LibraryError

pytestmark = pytest.mark.gpu

DT = 0.01
TOL = 1e-10
CELLS = [(n, t) for n in sorted(TEAM_CELLS) for t in sorted(TEAM_CELLS[n])]
LEGAL = [(n, t) for n, t in CELLS if "rollout" not in TEAM_CELLS[n][t]]
REFUSING = [(n, t) for n, t in CELLS if TEAM_CELLS[n][t]]
BIG = ("puppet_basic",)
# Place of a system in the seeds of test_team_cell_matches_oracle.  Append a new system at the end: the draws of the others stay.
_SEED_ORDER = ["damper_link", "dual_pendulums", "pend_on_cart", "pendulum1", "pendulum5", "plane_link", "puppet_basic", "scissor4", "spring_arm",
               "spring_link", "wrench_arm", "spatial_loop", "mixed_loop"]
assert sorted(_SEED_ORDER) == sorted(TEAM_CELLS)


def _batch(monkeypatch, system, B, team):
    """A generic-kernel batch at the forced team (None: the team the system gets by itself)."""
    if team is None:
        monkeypatch.delenv("TREPAMD_TEAM", raising=False)
    else:
        monkeypatch.setenv("TREPAMD_TEAM", str(team))
    mvi = BatchMidpointVI(system, B, specialize=False)
    if team is not None:
        assert mvi.kernel_info()["team"] == team
    return mvi


def _shapes(name, team):
    tpb = 64 // team
    if name in BIG:
        return [13] if tpb == 1 else [2 * tpb + 1, 3]
    out = [2 * tpb + 1, 3 * tpb - 1, 3]
    return sorted(set(b for b in out if b > 0), reverse=True)


def _assert_generic(mvi, modes):
    info = mvi.kernel_info()
    for m in modes:
        bit = BatchMidpointVI.ALL_MODES[m]
        assert (info["generic_launch_mask"] >> bit) & 1 and not (info["spec_launch_mask"] >> bit) & 1, (m, info)
        if m in BatchMidpointVI.MODES:
            assert m in info["generic_launched"] and m not in info["spec_launched"], (m, info)


def _u(A, j):
    return A[:, j] if A.shape[2] else None


def _run_cell(monkeypatch, name, team, B, rng, refused=()):
    """Every legal mode of one (system, team, batch size) against the oracle; returns the rollout (X, iterations)."""
    system, d = build(name)
    nq, nd, nu, nk, nc = d.n_configs, d.n_dyn, d.n_inputs, d.n_kin, d.n_constraints
    N = 20 if name in BIG else 40
    S = 3                                                                   # step() calls after the rollout
    Q0, Q1, U, K = _starts(name, d, B, N, rng, extra=S)
    mvi = _batch(monkeypatch, system, B, team)
    # 1. calc_p2 + rollout
    mvi.initialize_from_configs(0.0, Q0, DT, Q1)
    P2 = mvi.p2
    X = mvi.rollout(N, DT, U[:, :N], K[:, :N])
    iters, status = mvi.status()
    assert (status == 0).all(), (name, team, B, status)
    oracles = []
    for b in range(B):
        o = OracleMVI(d)
        o.initialize_from_configs(0.0, Q0[b], DT, Q1[b])
        assert relerr(P2[b], o.p2) < 1e-12, (name, team, B, b)
        Xo, tot = o.rollout(N, DT, U[b, :N], K[b, :N])
        assert relerr(X[b], Xo) < TOL, (name, team, B, b, relerr(X[b], Xo))
        assert abs(tot - int(iters[b])) <= 1, (name, team, B, b, tot, iters[b])
        oracles.append(o)
    # 2. step() calls, lambda1; the last step starts from the oracle's state (teacher-forced) so that the derivatives below are taken
    # at the same point
    for j in range(N, N + S - 1):
        it, st = mvi.step((j + 2) * DT, _u(U, j), _u(K, j))
        assert (st == 0).all()
        for b, o in enumerate(oracles):
            ito = o.step((j + 2) * DT, U[b, j], K[b, j])
            assert abs(ito - int(it[b])) <= 1, (name, team, B, b)
    q2, p2, lam = mvi.q2, mvi.p2, mvi.lambda1
    for b, o in enumerate(oracles):
        # (lambda1 is compared at the teacher-forced step below: the scissor lift's multipliers are conditioned by 1 / dt^2, so the
        # ~1e-12 by which free-running states differ moves them by up to ~1e-9 relative, at the natural team as at the forced one)
        assert relerr(q2[b], o.q2) < TOL and relerr(p2[b], o.p2) < TOL, (name, team, B, b)
    j = N + S - 1
    t1 = (j + 1) * DT
    mvi.initialize_from_state(t1, np.array([o.q2 for o in oracles]), np.array([o.p2 for o in oracles]),
                              np.array([o.lambda1 for o in oracles]) if nc else None)
    for o in oracles:
        o.initialize_from_state(t1, o.q2.copy(), o.p2.copy(), o.lambda1.copy() if nc else None)
    it, st = mvi.step(t1 + DT, _u(U, j), _u(K, j))
    assert (st == 0).all()
    same = []
    for b, o in enumerate(oracles):
        ito = o.step(t1 + DT, U[b, j], K[b, j])
        assert abs(ito - int(it[b])) <= 1
        same.append(ito == int(it[b]))
    q2, p2, lam = mvi.q2, mvi.p2, mvi.lambda1
    for b, o in enumerate(oracles):
        assert relerr(q2[b], o.q2) < TOL and relerr(p2[b], o.p2) < TOL
        if nc and same[b]:
            assert relerr(lam[b], o.lambda1) < 3e-10, (name, team, B, b)
    # the residual and the derivatives at exactly the oracle's solution (q1, p1 are shared already)
    mvi.q2, mvi.p2 = np.array([o.q2 for o in oracles]), np.array([o.p2 for o in oracles])
    if nc:
        mvi.lambda1 = np.array([o.lambda1 for o in oracles])
    q2 = mvi.q2
    f = mvi.calc_f()
    for b, o in enumerate(oracles):
        assert relerr(f[b], o.calc_f()) < 1e-12, (name, team, B, b)
    modes = ["calc_p2", "rollout", "calc_f"]
    # 3. deriv1
    if "deriv1" not in refused:
        mvi.calc_deriv1()
        got = dict((n, mvi.deriv1(n)) for n in D1)
        for b, o in enumerate(oracles):
            o.calc_deriv1()
            for n in D1:
                assert relerr(got[n][b], o.deriv1(n)) < 1e-9, (name, team, B, b, n)
        modes.append("deriv1")
    # 4. deriv2z with random Z (and ZL)
    if "deriv2z" not in refused and name not in NO_SECOND_ORDER:
        Z = rng.standard_normal((B, nq + nd + nk))
        ZL = rng.standard_normal((B, nc))
        HZ = mvi.deriv2_contract(Z, ZL if nc else None)
        for b, o in enumerate(oracles):
            o.calc_deriv2()
            assert relerr(HZ[b], _oracle_hz(o, d, Z[b], ZL[b])) < 1e-8, (name, team, B, b)
        modes.append("deriv2z")
    elif name in NO_SECOND_ORDER:
        with pytest.raises(LibraryError, match="LinearSpring"):
            mvi.deriv2_contract(np.zeros((B, nq + nd + nk)))
    # 5. continuous dynamics, energies, Lagrangian, first derivatives of the dynamics at random states
    Qs = q2 + 0.05 * rng.standard_normal(q2.shape)
    dQs = rng.standard_normal((B, nq))
    Us = rng.standard_normal((B, nu))
    Ks = rng.standard_normal((B, nk))
    ddq, lmb, st = mvi.dynamics(Qs, dQs, Us if nu else None, Ks if nk else None)
    assert (st == 0).all()
    TV = mvi.energy(Qs, dQs)
    lag = mvi.lagrangian(Qs, dQs)
    dd1 = None
    if "dynamics_deriv1" not in refused:
        dd1, st = mvi.dynamics_deriv1(Qs, dQs, Us if nu else None, Ks if nk else None)
        assert (st == 0).all()
        modes.append("dynamics_deriv1")
    keys = ("L_dq", "L_ddq", "L_dqdq", "L_ddqdq", "L_ddqddq")
    for b, o in enumerate(oracles):
        fo, lo = o.dynamics(Qs[b], dQs[b], Us[b], Ks[b])
        assert relerr(ddq[b], fo) < 1e-9 and relerr(lmb[b], lo) < 1e-9, (name, team, B, b)
        T, V = o.energy(Qs[b], dQs[b])
        assert relerr(TV[b, 0] + TV[b, 1], T + V) < 1e-11 and relerr(TV[b, 0] - TV[b, 1], T - V) < 1e-11, (name, team, B, b)
        for key, ref in zip(keys, o.lagrangian(Qs[b], dQs[b])):
            assert relerr(lag[key][b], ref) < 1e-11, (name, team, B, b, key)
        if dd1 is not None:
            ref = o.dynamics_deriv1(Qs[b], dQs[b], Us[b], Ks[b])
            for key, val in ref.items():
                assert relerr(dd1[key.replace("lam_", "lambda_")][b], val) < 1e-9, (name, team, B, b, key)
    modes += ["dynamics", "energy", "lagrangian"]
    _assert_generic(mvi, modes)
    mvi.close()
    return X, iters


@pytest.mark.parametrize("name,team", LEGAL)
def test_team_cell_matches_oracle(monkeypatch, name, team):
    """Every mode the cell allows, at three ragged batch sizes (two full blocks and one team, three blocks less one team, a single
    partial block); the rollout also against the same system at the team it gets by itself."""
    rng = np.random.default_rng(1000 + 64 * team + _SEED_ORDER.index(name))
    refused = TEAM_CELLS[name][team]
    for B in _shapes(name, team):
        seed = int(rng.integers(1 << 30))
        X, iters = _run_cell(monkeypatch, name, team, B, np.random.default_rng(seed), refused)
        # cross-team agreement: the same batch at the natural team
        system, d = build(name)
        r = np.random.default_rng(seed)
        N = X.shape[1] - 1
        Q0, Q1, U, K = _starts(name, d, B, N, r, extra=3)
        nat = _batch(monkeypatch, system, B, None)
        nat.initialize_from_configs(0.0, Q0, DT, Q1)
        Xn = nat.rollout(N, DT, U[:, :N], K[:, :N])
        itn, stn = nat.status()
        assert (stn == 0).all()
        for b in range(B):
            assert relerr(X[b], Xn[b]) < TOL, (name, team, B, b)
            assert abs(int(iters[b]) - int(itn[b])) <= 1, (name, team, B, b)
        nat.close()


@pytest.mark.parametrize("name,team", REFUSING)
def test_team_cell_refusals(monkeypatch, name, team):
    """Blocks over 160 KiB of LDS are refused before anything is launched; the legal modes of the batch still match the oracle."""
    system, d = build(name)
    nq, nd, nu, nk, nc = d.n_configs, d.n_dyn, d.n_inputs, d.n_kin, d.n_constraints
    refused = TEAM_CELLS[name][team]
    B = 2 * (64 // team) + 1 if name not in BIG else 5
    rng = np.random.default_rng(7 + team)
    Q0, Q1, U, K = _starts(name, d, B, 4, rng)
    mvi = _batch(monkeypatch, system, B, team)
    mvi.initialize_from_state(0.0, Q0, np.zeros((B, nd)))
    mvi.set_times(0.0, DT)        # t2 != t1: the derivative entry points get as far as the launch
    Qs, dQs = Q0, np.zeros((B, nq))
    calls = {"rollout": [lambda: mvi.rollout(4, DT, U, K), lambda: mvi.calc_p2(), lambda: mvi.calc_f(),
                         lambda: mvi.step(2 * DT, _u(U, 0), _u(K, 0)), lambda: mvi.dynamics(Qs, dQs),
                         lambda: mvi.energy(Qs, dQs), lambda: mvi.lagrangian(Qs, dQs)],
             "deriv1": [lambda: mvi.calc_deriv1()],
             "deriv2z": [lambda: mvi.deriv2_contract(np.zeros((B, nq + nd + nk)))],
             "dynamics_deriv1": [lambda: mvi.dynamics_deriv1(Qs, dQs)]}
    for kind in sorted(refused):
        for call in calls[kind]:
            before = mvi.kernel_info()["generic_launches"]
            match = "LinearSpring" if kind == "deriv2z" and name in NO_SECOND_ORDER else "too large"
            with pytest.raises(LibraryError, match=match):
                call()
            assert mvi.kernel_info()["generic_launches"] == before, (name, team, kind)
    if "rollout" in refused:
        assert mvi.kernel_info()["generic_launches"] == 0
        mvi.close()
        return
    # a legal mode afterwards: calc_p2 + rollout (+ deriv1 if allowed) against the oracle
    mvi.initialize_from_configs(0.0, Q0, DT, Q1)
    X = mvi.rollout(4, DT, U, K)
    assert (mvi.status()[1] == 0).all()
    if "deriv1" not in refused:
        mvi.calc_deriv1()
    for b in range(B):
        o = OracleMVI(d)
        o.initialize_from_configs(0.0, Q0[b], DT, Q1[b])
        Xo, _ = o.rollout(4, DT, U[b], K[b])
        assert relerr(X[b], Xo) < TOL, (name, team, b)
        if "deriv1" not in refused:
            o.calc_deriv1()
            for n in D1:
                assert relerr(mvi.deriv1(n)[b], o.deriv1(n)) < 1e-9, (name, team, b, n)
    mvi.close()


# Size of the closed loop's random gains where 0.01 is too much for the reference itself: mixed_loop has kinematic configs inside a closed
# chain, and a feedback that moves them that far opens the loop -- with these inputs the oracle's own loop (common.tb_oracle_rollout) does
# not converge on trajectories 4 and 7 of the batch at team 16; at 1e-3 every trajectory takes the open loop's 30 iterations.  With gains
# that small the feedback does little: this cell checks what the test is about -- the subset launch against the full one, bit for bit --
# and the closed loop of mixed_loop itself is held to the oracle in test_gpu_model_branches.py, with gains scaled per column
# (common.tb_closed_loop_inputs) that move X by 1e-6 .. 1e-2.
_LOOP_GAIN = {"mixed_loop": 1e-3}


def _legal(name, team, kind):
    return kind not in TEAM_CELLS[name][team]


@pytest.mark.parametrize("name,team", LEGAL)
def test_team_cell_remapped_launches(monkeypatch, name, team):
    """tg_batch_deriv2_contract_device_range over step ranges that are no multiple of the teams per block equals those rows of the full
    contraction (and writes no other row); tg_batch_rollout_closed_loop_subset equals the same trajectories of the full closed loop."""
    system, d = build(name)
    nq, nd, nu, nk = d.n_configs, d.n_dyn, d.n_inputs, d.n_kin
    nX, nU, R = nq + nd + nk, nu + nk, nq + nd + nu + nk
    rng = np.random.default_rng(31 * team + 5)
    L = _lib.lib()
    if _legal(name, team, "deriv2z") and name not in NO_SECOND_ORDER:
        for seeds, horizon, k0, k1 in (RANGE_CASES if name not in BIG else RANGE_CASES[:1]):
            B = seeds * horizon
            Q0, Q1, U, K = _starts(name, d, B, 1, rng)
            mvi = _batch(monkeypatch, system, B, team)
            mvi.initialize_from_configs(0.0, Q0, DT, Q1)
            assert (mvi.step(2 * DT, _u(U, 0), _u(K, 0))[1] == 0).all()
            z = mvi.device_array(rng.standard_normal((B, nX)))
            full = mvi.device_empty(B * R * R)
            part = mvi.device_array(np.full((B, R, R), 7.0))
            _lib.check(L.tg_batch_deriv2_contract_device(mvi._h, z, full))
            _lib.check(L.tg_batch_deriv2_contract_device_range(mvi._h, z, part, horizon, k0, k1))
            mvi.synchronize()
            F, P = mvi.download(full, (B, R, R)), mvi.download(part, (B, R, R))
            rows = np.array([s * horizon + k for s in range(seeds) for k in range(k0, k1)])
            rest = np.setdiff1d(np.arange(B), rows)
            assert np.array_equal(P[rows], F[rows]), (name, team, seeds, horizon, k0, k1)
            assert (P[rest] == 7.0).all(), (name, team, seeds, horizon, k0, k1)
            assert np.abs(F).max() > 0.0
            _assert_generic(mvi, ["deriv2z"])
            mvi.close()
    # closed-loop subset: the first n trajectories of B
    tpb = 64 // team
    B = 2 * tpb + 1 if name not in BIG else 6
    n = B - 2 if B > 3 else 2
    N = 10
    Q0, Q1, U, K = _starts(name, d, B, N, rng)
    bX = np.zeros((B, N + 1, nX))
    bU = np.concatenate([U, K], axis=2)
    Kp = _LOOP_GAIN.get(name, 0.01) * rng.standard_normal((B, N, nU, nX))
    mvi = _batch(monkeypatch, system, B, team)
    mvi.initialize_from_configs(0.0, Q0, DT, Q1)
    bX[:] = np.concatenate([mvi.q2, mvi.p2, mvi.q2[:, nd:]], axis=1)[:, None, :]
    Xf, Uf = mvi.rollout_closed_loop(N, DT, Kp, bX, bU)
    itf, stf = mvi.status()
    assert (stf == 0).all()
    mvi.initialize_from_configs(0.0, Q0, DT, Q1)
    dev = [mvi.device_array(a) for a in (Kp, bX, bU)]
    Xd, Ud = mvi.device_empty(B * (N + 1) * nX), mvi.device_empty(B * N * nU)
    _lib.check(L.tg_batch_rollout_closed_loop_subset(mvi._h, n, N, DT, dev[0], 1, None, dev[1], dev[2], Xd, Ud, 200))
    mvi.synchronize()
    Xs, Us = mvi.download(Xd, (B, N + 1, nX)), mvi.download(Ud, (B, N, nU))
    its, sts = mvi.status()
    assert np.array_equal(Xs[:n], Xf[:n]) and np.array_equal(Us[:n], Uf[:n]), (name, team, n)
    assert np.array_equal(its[:n], itf[:n]) and (sts[:n] == 0).all()
    _assert_generic(mvi, ["rollout"])
    mvi.close()


@pytest.mark.parametrize("name,team", LEGAL)
@pytest.mark.parametrize("group", [1, 3])
def test_team_cell_parameter_kernels(monkeypatch, name, team, group):
    """The generic per-trajectory-parameter kernels (set_parameters) at the forced team: every trajectory against the oracle of the
    system rebuilt with its row; a group of 3 divides no team count per block."""
    make = BUILDERS[name]
    system, d = build(name)
    nq, nd, nk, nc = d.n_configs, d.n_dyn, d.n_kin, d.n_constraints
    tpb = 64 // team
    B = 2 * tpb + 1 if name not in BIG else 9       # a multiple of 3
    assert B % 3 == 0
    rows = random_rows(system, B // group, seed=40 + team + group)
    N = 10
    rng = np.random.default_rng(3 * team + group)
    Q0, Q1, U, K = _starts(name, d, B, N, rng, extra=1)
    mvi = _batch(monkeypatch, system, B, team)
    mvi.set_parameters(group=group, **rows)
    mvi.initialize_from_configs(0.0, Q0, DT, Q1)
    X = mvi.rollout(N, DT, U[:, :N], K[:, :N])
    iters, status = mvi.status()
    assert (status == 0).all()
    it, st = mvi.step((N + 2) * DT, _u(U, N), _u(K, N))
    assert (st == 0).all()
    legal1, legal2 = _legal(name, team, "deriv1"), _legal(name, team, "deriv2z") and name not in NO_SECOND_ORDER
    if legal1:
        mvi.calc_deriv1()
        got = dict((n, mvi.deriv1(n)) for n in D1)
    if legal2:
        Z = rng.standard_normal((B, nq + nd + nk))
        ZL = rng.standard_normal((B, nc))
        HZ = mvi.deriv2_contract(Z, ZL if nc else None)
    q2 = mvi.q2
    for b in range(B):
        o = OracleMVI(descriptor.flatten(rebuilt(make, rows, b // group)))
        o.initialize_from_configs(0.0, Q0[b], DT, Q1[b])
        Xo, tot = o.rollout(N, DT, U[b, :N], K[b, :N])
        assert relerr(X[b], Xo) < TOL, (name, team, group, b)
        assert abs(tot - int(iters[b])) <= 1
        o.step((N + 2) * DT, U[b, N], K[b, N])
        assert relerr(q2[b], o.q2) < TOL
        if legal1:
            o.calc_deriv1()
            for n in D1:
                assert relerr(got[n][b], o.deriv1(n)) < 1e-9, (name, team, group, b, n)
        if legal2:
            o.calc_deriv2()
            assert relerr(HZ[b], _oracle_hz(o, d, Z[b], ZL[b])) < 1e-8, (name, team, group, b)
    info = mvi.kernel_info()
    want = {"calc_p2", "rollout"} | ({"deriv1"} if legal1 else set()) | ({"deriv2z"} if legal2 else set())
    assert want <= set(info["par_generic_launched"]) and not info["par_spec_launched"], info
    assert info["generic_launches"] == 0 and info["spec_launches"] == 0, info
    mvi.close()


ISOLATION = [("pend_on_cart", 1), ("pend_on_cart", 4), ("pend_on_cart", 16), ("plane_link", 1), ("plane_link", 4),
             ("plane_link", 16), ("scissor4", 16)]


def _hinted_step(d, q, p, lam, t, u, k, hint, max_iterations):
    o = OracleMVI(d)
    o.initialize_from_state(t, q, p, lam if d.n_constraints else None)
    try:
        it = o.step(t + DT, u, k, max_iterations=max_iterations, q2_hint=hint)
    except OracleError as e:
        return str(e), o
    return it, o


@pytest.mark.parametrize("name,team", ISOLATION)
def test_failing_trajectories_leave_wave_neighbours_unchanged(monkeypatch, name, team):
    """Victims -- the first team of block 0, the last team of block 1, the last trajectory of the ragged tail -- start one step's Newton
    iteration from a far-off q2 hint and run out of iterations (the oracle says at that step, with the batch-wide max_iterations);
    one more starts from a NaN hint (the reference counts a NaN residual as solved).  Every other trajectory must be bit-for-bit what
    it is when the victims start from harmless hints instead."""
    system, d = build(name)
    nq, nd, nc = d.n_configs, d.n_dyn, d.n_constraints
    tpb = 64 // team
    B = 2 * tpb + 3
    victims = [0, 2 * tpb - 1, B - 1]
    nan_victim = tpb + 1 if tpb > 2 else 2 * tpb
    R = 3
    rng = np.random.default_rng(77 + team)
    Q0, Q1, U, K = _starts(name, d, B, R, rng, extra=1)
    mvi = _batch(monkeypatch, system, B, team)
    mvi.initialize_from_configs(0.0, Q0, DT, Q1)
    mvi.rollout(R, DT, U[:, :R], K[:, :R])
    assert (mvi.status()[1] == 0).all()
    q, p, lam = mvi.q2, mvi.p2, mvi.lambda1
    t = (R + 1) * DT
    u, k = U[:, R], K[:, R]
    # harmless hints for everyone; the oracle's iteration counts from there fix max_iterations with a margin of one each way
    safe = q[:, :nd] + 1e-4 * rng.standard_normal((B, nd))
    its = [_hinted_step(d, q[b], p[b], lam[b], t, u[b], k[b], safe[b], 200)[0] for b in range(B)]
    assert all(isinstance(i, int) for i in its), its
    M = max(its) + 1
    bad = safe.copy()
    amp = 1.0 if name == "scissor4" else 2.0
    for v in victims:
        for _ in range(200):
            h = q[v, :nd] + amp * rng.standard_normal(nd)
            it, _o = _hinted_step(d, q[v], p[v], lam[v], t, u[v], k[v], h, 200)
            if isinstance(it, int) and M + 2 <= it <= 40 and _hinted_step(d, q[v], p[v], lam[v], t, u[v], k[v], h, M)[0] == "not converged":
                bad[v] = h
                break
        else:
            pytest.fail("no victim hint found for trajectory %d" % v)
    bad[nan_victim, 0] = np.nan
    mvi.snapshot()
    runs = {}
    for kind, hints in (("safe", safe), ("bad", bad)):
        mvi.restore()
        mvi.set_times(t, t)
        it, st = mvi.step(t + DT, u if d.n_inputs else None, k if d.n_kin else None, max_iterations=M, q2_hint=hints)
        runs[kind] = (it, st, mvi.q2, mvi.p2, mvi.lambda1)
    it_s, st_s = runs["safe"][:2]
    it_b, st_b = runs["bad"][:2]
    assert (st_s == 0).all(), st_s
    for v in victims:
        assert st_b[v] == _lib.NOT_CONVERGED, (name, team, v, st_b[v], it_b[v])
    it_o, o = _hinted_step(d, q[nan_victim], p[nan_victim], lam[nan_victim], t, u[nan_victim], k[nan_victim], bad[nan_victim], M)
    assert isinstance(it_o, int) and st_b[nan_victim] == _lib.OK and int(it_b[nan_victim]) == it_o, (it_o, st_b[nan_victim])
    for got, ref in ((runs["bad"][2][nan_victim], o.q2), (runs["bad"][3][nan_victim], o.p2)):
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    others = np.setdiff1d(np.arange(B), victims + [nan_victim])
    assert np.array_equal(it_b[others], it_s[others]) and np.array_equal(st_b[others], st_s[others]), (name, team)
    for a, b_ in zip(runs["bad"][2:], runs["safe"][2:]):
        assert np.array_equal(a[others], b_[others]), (name, team)
    # and the harmless run agrees with the oracle
    for b in others:
        it, o = _hinted_step(d, q[b], p[b], lam[b], t, u[b], k[b], safe[b], M)
        assert abs(it - int(it_s[b])) <= 1 and relerr(runs["safe"][2][b], o.q2) < TOL, (name, team, b)
    if nc:
        # The convergence test votes only among teams whose dynamic residual is within the tolerance, so above a neighbour that is
        # still far off nothing is shared.  With a loose dynamic tolerance the far-started victims reach that state while their
        # constraints (held to their own 1e-10) are still off: the trajectories next to them must not notice, and every trajectory
        # takes the oracle's iterations at that tolerance.
        loose = 1e-4
        near = q[:, :nd] + 0.1 * rng.standard_normal((B, nd))
        far = safe.copy()
        far[victims] = near[victims]
        res = {}
        for kind, hints in (("safe", safe), ("far", far)):
            mvi.restore()
            mvi.set_times(t, t)
            mvi.tolerance = loose
            it, st = mvi.step(t + DT, u if d.n_inputs else None, k if d.n_kin else None, q2_hint=hints)
            assert (st == 0).all(), (name, team, kind, st)
            res[kind] = (it, mvi.q2, mvi.p2, mvi.lambda1)
        others = np.setdiff1d(np.arange(B), victims)
        for a, b_ in zip(res["far"], res["safe"]):
            assert np.array_equal(a[others], b_[others]), (name, team)
        for b in range(B):
            o = OracleMVI(d, tolerance=loose)
            o.initialize_from_state(t, q[b], p[b], lam[b])
            ito = o.step(t + DT, u[b], k[b], q2_hint=far[b])
            assert abs(ito - int(res["far"][0][b])) <= 1, (name, team, b, ito, res["far"][0][b])
    _assert_generic(mvi, ["calc_p2", "rollout"])
    mvi.close()
