"""Batched constraint projection on the device (BatchMidpointVI.satisfy_constraints, k_project): the case table of
projection_reference.py at every system's own team size and at forced ones, against the numpy reference -- the answer checks that do
not depend on the iteration, the per-case bound 64 max(floor, 1e-13) on |q - q_ref|, step counts within one of the reference's --
other batch sizes, bit-equality, the status cases, independence from the batch's library / parameter table / integrator state, the
device-pointer variant on a caller's stream, and perturbed starts projected and rolled out."""

import numpy as np
import pytest

import common
import projection_reference as pr
from oracle.oracle import OracleMVI
from trep_amd import BatchMidpointVI, _lib

pytestmark = pytest.mark.gpu

CASE_IDS = [pr.case_id(c) for c in pr.CASES]
TEAMS = [("plane_link", 4), ("plane_link", 16), ("plane_link", 64), ("scissor4", 16), ("scissor4", 64), ("puppet_basic", 64)]
PROJECT_BIT = 9
ERR_INVALID = -1


def _batch(monkeypatch, name, B, team=None, specialize=False):
    if team is None:
        monkeypatch.delenv("TREPAMD_TEAM", raising=False)
    else:
        monkeypatch.setenv("TREPAMD_TEAM", str(team))
    mvi = BatchMidpointVI(common.build(name)[0], B, specialize=specialize)
    if team is not None:
        assert mvi.kernel_info()["team"] == team
    return mvi


def _kw(name, mask):
    return dict(keep_kinematic=mask == "keep_kinematic", constant_q_list=pr.constant_list(name) if mask == "constant" else None)


def _check_case(case, got, rows=slice(None)):
    """(2), the bound of (3) and the step counts of (4) on the given rows of a case."""
    name = case[0]
    Q0, dQ0, free = pr.case_inputs(*case)
    ref = pr.case_reference(*case)
    assert (got.status == pr.OK).all(), got.status
    err = float(np.abs(got.Q - ref.Q[rows]).max())
    bound = pr.case_bound(*case)
    res = pr.residuals(name, Q0[rows], dQ0[rows], free, got)
    print(pr.case_id(case), "bound %.3e error %.3e steps %s reference %s" % (bound, err, got.iterations, ref.iterations[rows]),
          dict((k, float(v.max())) for k, v in res.items()))
    assert err <= bound
    assert (got.iterations <= ref.iterations[rows] + 1).all(), (got.iterations, ref.iterations[rows])
    assert res["fixed"].all()
    for k in ("h", "normal", "stationary", "tangent", "row_space"):
        assert res[k].max() <= 1.0, (k, res[k])


def _same(a, b, rows=slice(None)):
    for k in ("Q", "dQ", "mu", "iterations", "status"):
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None and y is None) or np.array_equal(x[rows], y), k


# ---- 1. the table on the device -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pr.CASES, ids=CASE_IDS)
def test_the_table_at_the_systems_own_team(monkeypatch, case):
    name, mask, _ = case
    Q0, dQ0, free = pr.case_inputs(*case)
    mvi = _batch(monkeypatch, name, len(Q0))
    assert np.array_equal(mvi.free_mask(**_kw(name, mask)) != 0, free)
    got = mvi.satisfy_constraints(Q0, dQ0, tolerance=pr.TOL, **_kw(name, mask))
    _check_case(case, got)
    assert got.iterations[pr.CONSISTENT] == 0 and np.array_equal(got.Q[pr.CONSISTENT], Q0[pr.CONSISTENT])
    info = mvi.kernel_info()
    assert info["generic_launch_mask"] == 1 << PROJECT_BIT and info["spec_launch_mask"] == 0 and info["generic_launches"] == 1


@pytest.mark.parametrize("name,team", TEAMS)
@pytest.mark.parametrize("mask,noise", [("constant", 0.02), ("all", 0.1)])
def test_forced_teams_one_block_and_a_ragged_batch(monkeypatch, name, team, mask, noise):
    case = (name, mask, noise)
    Q0, dQ0, free = pr.case_inputs(*case)
    per_block = 64 // team
    assert len(Q0) % per_block or per_block == 1
    mvi = _batch(monkeypatch, name, len(Q0), team)
    ragged = mvi.satisfy_constraints(Q0, dQ0, tolerance=pr.TOL, **_kw(name, mask))
    _check_case(case, ragged)
    one = _batch(monkeypatch, name, per_block, team).satisfy_constraints(Q0[:per_block], dQ0[:per_block], tolerance=pr.TOL, **_kw(name, mask))
    _check_case(case, one, slice(0, per_block))
    _same(ragged, one, slice(0, per_block))          # a trajectory does not see its neighbours


# ---- 2. other batch sizes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 300))
def test_other_batch_sizes(monkeypatch, B):
    case = ("puppet_basic", "constant", 0.02)
    name, mask, _ = case
    Q0, dQ0, free = pr.case_inputs(*case)
    pick = np.arange(B) % len(Q0)
    got = _batch(monkeypatch, name, B).satisfy_constraints(Q0[pick], dQ0[pick], tolerance=pr.TOL, **_kw(name, mask))
    table = _batch(monkeypatch, name, len(Q0)).satisfy_constraints(Q0, dQ0, tolerance=pr.TOL, **_kw(name, mask))
    _check_case(case, pr.Projection(*(x[:len(Q0)] for x in got)), slice(0, min(B, len(Q0))))
    _same(table, got, pick)


# ---- 3. bit-equality ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("scissor4", "puppet40"))
def test_equal_trajectories_give_equal_bits(monkeypatch, name):
    case = (name, "keep_kinematic", 0.02)
    Q0, dQ0, free = pr.case_inputs(*case)
    got = _batch(monkeypatch, name, len(Q0)).satisfy_constraints(Q0, dQ0, keep_kinematic=True)
    assert np.array_equal(Q0[pr.REPEAT], Q0[0])
    _same(pr.Projection(*(x[pr.REPEAT:] for x in got)), pr.Projection(*(x[:1] for x in got)))
    assert got.iterations[pr.CONSISTENT] == 0 and got.status[pr.CONSISTENT] == pr.OK
    assert np.array_equal(got.Q[pr.CONSISTENT], Q0[pr.CONSISTENT])
    again = _batch(monkeypatch, name, len(Q0)).satisfy_constraints(Q0, dQ0, keep_kinematic=True)
    _same(got, again)


# ---- 4. status --------------------------------------------------------------------------------------------------------------------
def _status_rows(name):
    Q0 = pr.case_inputs(name, "all", 0.02)[0]
    return Q0[0], pr.case_reference(name, "all", 0.02, 1e-13).Q[2:5]


@pytest.mark.parametrize("name,team", [("puppet40", None), ("scissor4", 16)])
def test_status_cases_leave_the_neighbours_alone(monkeypatch, name, team):
    bad, good = _status_rows(name)
    nq = len(bad)
    mixed = np.array([good[0], bad, good[1], good[2]])
    # plain non-convergence: one step allowed
    with_bad = _batch(monkeypatch, name, 4, team).satisfy_constraints(mixed, max_iterations=1)
    without = _batch(monkeypatch, name, 3, team).satisfy_constraints(good, max_iterations=1)
    assert list(with_bad.status) == [pr.OK, pr.NOT_CONVERGED, pr.OK, pr.OK] and list(with_bad.iterations) == [0, 1, 0, 0]
    first = pr.project_one(pr.constraints_of(name), bad, np.ones(nq, dtype=bool), max_iterations=1)
    assert np.abs(with_bad.Q[1] - first[0]).max() <= pr.MARGIN * 1e-13 and np.abs(with_bad.Q[1] - bad).max() > 1e-4
    _same(with_bad, without, [0, 2, 3])
    # a refused solve: nothing is free
    names = pr.config_names(name)
    dq = np.ones((4, nq))
    with_bad = _batch(monkeypatch, name, 4, team).satisfy_constraints(mixed, dq, constant_q_list=names)
    without = _batch(monkeypatch, name, 3, team).satisfy_constraints(good, dq[:3], constant_q_list=names)
    assert list(with_bad.status) == [pr.OK, pr.SINGULAR, pr.OK, pr.OK] and not with_bad.iterations.any()
    assert np.array_equal(with_bad.Q, mixed) and np.array_equal(with_bad.dQ, dq)
    _same(with_bad, without, [0, 2, 3])


def test_status_without_constraints(monkeypatch):
    Q = np.array([[0.3], [-1.2], [4.0]])
    dQ = np.array([[1.0], [2.0], [3.0]])
    got = _batch(monkeypatch, "pendulum1", 3).satisfy_constraints(Q, dQ)
    assert np.array_equal(got.Q, Q) and np.array_equal(got.dQ, dQ) and not got.status.any() and not got.iterations.any()
    assert got.mu.shape == (3, 0)


def test_argument_refusals_with_a_live_batch(monkeypatch):
    mvi = _batch(monkeypatch, "scissor4", 2)
    L = _lib.lib()
    q = np.zeros((2, mvi.nq))
    p = q.ctypes.data
    for tol, its, dq, dq_out in ((0.0, 50, None, None), (1e-10, -1, None, None), (1e-10, 50, None, p)):
        assert L.tg_batch_project_constraints(mvi._h, p, dq, None, tol, its, p, dq_out, None, None, None) == ERR_INVALID
    assert L.tg_batch_project_constraints(mvi._h, None, None, None, 1e-10, 50, p, None, None, None, None) == ERR_INVALID
    assert mvi.kernel_info()["generic_launches"] == 0


# ---- 5. independence from the state of the batch ------------------------------------------------------------------------------
def test_library_parameter_table_and_integrator_state_have_no_say(monkeypatch):
    name = "puppet40"
    case = (name, "keep_kinematic", 0.02)
    Q0, dQ0, free = pr.case_inputs(*case)
    B, N, DT = len(Q0), 6, 0.01
    system, d = common.build(name)
    rng = np.random.default_rng(common.tb_seed("projection state", name))
    S0, S1, U, K = common.starts(name, d, B, N, rng)
    plain = _batch(monkeypatch, name, B).satisfy_constraints(Q0, dQ0, keep_kinematic=True)

    def fresh():
        mvi = _batch(monkeypatch, name, B, specialize="auto")
        assert mvi.kernel_info()["spec_modes"]
        mvi.initialize_from_configs(0.0, S0, DT, S1)
        return mvi

    ref = fresh()
    X_ref = ref.rollout(N, DT, U, K)
    mvi = fresh()
    state = lambda: [getattr(mvi, n).copy() for n in ("q1", "q2", "p1", "p2", "lambda1")] + list(mvi.status()) + [mvi.times()]
    before = state()
    _same(plain, mvi.satisfy_constraints(Q0, dQ0, keep_kinematic=True))                       # a specialised library is loaded
    par = mvi.parameters()
    mvi.set_parameters(inertia=np.tile(1.5 * par["inertia"], (B, 1, 1)))
    _same(plain, mvi.satisfy_constraints(Q0, dQ0, keep_kinematic=True))                       # ... and a parameter table set
    mvi.clear_parameters()
    info = mvi.kernel_info()
    assert (info["generic_launch_mask"] >> PROJECT_BIT) & 1 and not (info["spec_launch_mask"] >> PROJECT_BIT) & 1
    assert "project" not in str(info["par_generic_launched"]) and info["par_generic_launches"] == 0 and info["par_spec_launches"] == 0
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)
    assert np.array_equal(mvi.rollout(N, DT, U, K), X_ref)
    assert (mvi.status()[1] == 0).all()


# ---- 6. device pointers on a caller's stream -------------------------------------------------------------------------------------
def test_device_variant_on_a_callers_stream(monkeypatch):
    L = _lib.lib()
    case = ("scissor4", "constant", 0.02)
    name, mask, _ = case
    Q0, dQ0, free = pr.case_inputs(*case)
    B = len(Q0)
    host = _batch(monkeypatch, name, B).satisfy_constraints(Q0, dQ0, **_kw(name, mask))
    mvi = _batch(monkeypatch, name, B)
    stream = L.tg_dopt_lane_stream(0, 1)
    assert stream
    mvi.set_stream(stream)
    assert mvi.stream == stream
    nq, nc = mvi.nq, mvi.nc
    q_dev, dq_dev = mvi.device_array(Q0), mvi.device_array(dQ0)
    mask_host = np.ascontiguousarray(free, dtype=np.int32)
    ints = L.tg_device_alloc(0, 4 * (nq + 2 * B))
    assert ints
    try:
        _lib.check(L.tg_memcpy_h2d(0, ints, mask_host.ctypes.data, 4 * nq))
        q_out, dq_out, mu_out = mvi.device_empty(B * nq), mvi.device_empty(B * nq), mvi.device_empty(B * nc)
        _lib.check(L.tg_batch_project_constraints_device(mvi._h, q_dev, dq_dev, ints, pr.TOL, 50, q_out, dq_out, mu_out,
                                                         ints + 4 * nq, ints + 4 * (nq + B)))
        mvi.synchronize()
        back = np.zeros(2 * B, dtype=np.int32)
        _lib.check(L.tg_memcpy_d2h(0, back.ctypes.data, ints + 4 * nq, 8 * B))
        got = pr.Projection(mvi.download(q_out, (B, nq)), mvi.download(dq_out, (B, nq)), mvi.download(mu_out, (B, nc)), back[:B], back[B:])
        _same(host, got)
    finally:
        L.tg_device_free(0, ints)
        mvi.close()


# ---- 7. end to end: perturbed starts, projected, rolled out ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ("scissor4", "puppet_basic"))
def test_shifted_starts_projected_and_rolled_out(monkeypatch, name):
    system, d = common.build(name)
    nq, nd, nc = int(d.n_configs), int(d.n_dyn), int(d.n_constraints)
    B, N, DT = 16, 20, 0.01
    rng = np.random.default_rng(common.tb_seed("projection end to end", name))
    poses = pr.golden_poses(name)
    Q = poses[rng.choice(len(poses), size=B, replace=False)] + 0.05 * rng.standard_normal((B, nq))
    dQ = 0.3 * rng.standard_normal((B, nq))
    mvi = _batch(monkeypatch, name, B)
    got = mvi.satisfy_constraints(Q, dQ)
    assert (got.status == pr.OK).all(), (got.status, got.iterations)
    assert np.abs(got.Q - Q).max() > 1e-3
    P = mvi.lagrangian(got.Q, got.dQ)["L_ddq"][:, :nd]                  # p = L_ddq at the projected state
    mvi.initialize_from_state(0.0, got.Q, P)
    X = mvi.rollout(N, DT)
    iters, status = mvi.status()
    assert (status == 0).all(), status
    o = OracleMVI(d)
    o.set_times(0.0, DT)
    tol = np.maximum(1e-10, np.asarray(d.constraint_tolerance[:nc])) + common.TB_TOL["f"]
    for k in (1, N // 2, N):
        for b in range(B):
            o.q1 = X[b, k, :nq]
            o.q2 = X[b, k, :nq]
            h = o.calc_f()[nd:]
            assert (np.abs(h) <= tol).all(), (k, b, h)
