"""Batched inverse dynamics on the device (BatchMidpointVI.inverse_dynamics, k_inverse): the case table of
inverse_dynamics_reference.py at every system's own team size and at every team size of common.TEAM_CELLS, with and without p0,
against the numpy specification with the bound of the CPU tests (max(1e-10, 64 e_ref) relative to max(1, |z~|inf)); equal bits for
a step repeated in a launch, alone in a launch, and through the host and the device entry points; the device variant reading a
rollout's X; the round trip rollout -> inverse dynamics -> rollout; the parameter twin against rebuilt systems; status, the launch
masks, the refusals and the untouched integrator state."""
import numpy as np
import pytest

import common
import inverse_dynamics_reference as ir
from trep_amd import BatchMidpointVI, _lib

pytestmark = pytest.mark.gpu

CASE_IDS = [ir.case_id(c) for c in ir.CASES]
INVERSE_BIT = 11
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
TEAM_RUNS = [(c, t) for c in ir.CASES if c.name in common.TEAM_CELLS and c.pattern == "uniform" for t in sorted(common.TEAM_CELLS[c.name])]
ROUND_TRIP_BOUND = 2.3e-9            # (test_inverse_dynamics_cpu.py)


def _batch(monkeypatch, name, B, team=None, specialize=False):
    if team is None:
        monkeypatch.delenv("TREPAMD_TEAM", raising=False)
    else:
        monkeypatch.setenv("TREPAMD_TEAM", str(team))
    mvi = BatchMidpointVI(common.build(name)[0], B, specialize=specialize)
    if team is not None:
        assert mvi.kernel_info()["team"] == team
    return mvi


def _dt(c):
    return ir.step_sizes(c) if c.pattern != "uniform" else ir.DT


def _same(a, b, fields=ir.FIELDS):
    for q in fields:
        assert np.array_equal(getattr(a, q), getattr(b, q)), q


def _fits(mvi):
    """Does a workgroup of the kernel fit the LDS at this batch's team size (tg_system_inverse_dynamics_lds)?"""
    out = np.zeros(4, dtype=np.int32)
    rc = _lib.lib().tg_system_inverse_dynamics_lds(mvi._sys_h, out.ctypes.data_as(_lib._c_ip))
    assert rc in (0, ERR_UNSUPPORTED) and out[0] == mvi.kernel_info()["team"]
    assert (rc == 0) == (int(out[2]) <= 160 * 1024)
    return rc == 0


# ---- 1. the table on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_p0", (True, False), ids=("p0", "no_p0"))
@pytest.mark.parametrize("case", ir.CASES, ids=CASE_IDS)
def test_the_table_at_the_systems_own_team(monkeypatch, case, with_p0):
    p = ir.case_paths(case)
    mvi = _batch(monkeypatch, case.name, case.B)
    got = mvi.inverse_dynamics(p["Q"], _dt(case), p["p0"] if with_p0 else None, case.ridge)
    ir.compare(case, with_p0, got)
    if not with_p0:
        for q in ("U", "lam", "rho"):
            assert not getattr(got, q)[:, 0].any(), q
    info = mvi.kernel_info()
    assert info["generic_launch_mask"] == 1 << INVERSE_BIT and info["spec_launch_mask"] == 0 and info["generic_launches"] == 1
    assert info["par_generic_launches"] == 0
    assert getattr(mvi, "_step_sizes", None) is None              # a by-step list of the call is taken off again


@pytest.mark.parametrize("case,team", TEAM_RUNS, ids=["%s_team%d" % (ir.case_id(c), t) for c, t in TEAM_RUNS])
def test_every_team_size(monkeypatch, case, team):
    p = ir.case_paths(case)
    mvi = _batch(monkeypatch, case.name, case.B, team)
    if not _fits(mvi):
        with pytest.raises(_lib.LibraryError, match="system too large for the LDS-resident inverse-dynamics kernel"):
            mvi.inverse_dynamics(p["Q"], ir.DT, p["p0"], case.ridge)
        assert mvi.kernel_info()["generic_launches"] == 0
        return
    for with_p0 in (True, False):
        ir.compare(case, with_p0, mvi.inverse_dynamics(p["Q"], ir.DT, p["p0"] if with_p0 else None, case.ridge), tag="team %d " % team)


def test_both_sides_of_the_lds_limit_are_run(monkeypatch):
    seen = set()
    for case, team in TEAM_RUNS:
        seen.add(_fits(_batch(monkeypatch, case.name, 1, team)))
    assert seen == {True, False}


# ---- 2. equal bits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("scissor4", "wrench_arm"))
def test_a_step_does_not_depend_on_its_launch(monkeypatch, name):
    """A path repeated in one launch, and one (b, k) alone in a B = 1, N = 1 launch: the same bits."""
    case = [c for c in ir.CASES if c.name == name][0]
    p = ir.case_paths(case)
    Q, p0 = p["Q"], p["p0"]
    whole = _batch(monkeypatch, name, case.B).inverse_dynamics(Q, ir.DT, p0)
    pick = np.array([3, 0, 3, 1, 3, 2, 4])
    again = _batch(monkeypatch, name, len(pick)).inverse_dynamics(Q[pick], ir.DT, p0[pick])
    for q in ir.FIELDS:
        assert np.array_equal(getattr(again, q), getattr(whole, q)[pick]), q
    b, k = 3, 7
    one = _batch(monkeypatch, name, 1).inverse_dynamics(Q[b:b + 1, k:k + 2], ir.DT, whole.P[b:b + 1, k])
    for q in ("U", "lam", "rho", "h", "status"):
        assert np.array_equal(getattr(one, q)[0, 0], getattr(whole, q)[b, k]), q
    assert np.array_equal(one.P[0, 1], whole.P[b, k + 1])


def _device_call(mvi, N, dt, Q_dev, stride, p0, ridge=0.0):
    """inverse_dynamics_device with every output, downloaded."""
    L = _lib.lib()
    B, nd, nu, nc = mvi._batch, mvi.nd, mvi.nu, mvi.nc
    p0_dev = None if p0 is None else mvi.device_array(p0)
    U, lam, P, rho, h = (mvi.device_empty(B * N * nu), mvi.device_empty(B * N * nc), mvi.device_empty(B * (N + 1) * nd),
                         mvi.device_empty(B * N * nd), mvi.device_empty(B * N * nc))
    words = L.tg_device_alloc(0, 4 * B * N)
    assert words
    try:
        mvi.inverse_dynamics_device(N, dt, Q_dev, stride, p0_dev, ridge, U, lam, P, rho, h, words)
        mvi.synchronize()
        status = np.zeros((B, N), dtype=np.int32)
        _lib.check(L.tg_memcpy_d2h(0, status.ctypes.data, words, 4 * B * N))
    finally:
        L.tg_device_free(0, words)
    return ir.Result(mvi.download(U, (B, N, nu)), mvi.download(lam, (B, N, nc)), mvi.download(P, (B, N + 1, nd)), mvi.download(rho, (B, N, nd)),
                     mvi.download(h, (B, N, nc)), status, None, None, None, None, None)


@pytest.mark.parametrize("with_p0", (True, False), ids=("p0", "no_p0"))
def test_host_and_device_variants_give_the_same_bits(monkeypatch, with_p0):
    case = [c for c in ir.CASES if c.name == "mixed_loop"][0]
    p = ir.case_paths(case)
    p0 = p["p0"] if with_p0 else None
    host = _batch(monkeypatch, case.name, case.B).inverse_dynamics(p["Q"], ir.DT, p0, case.ridge)
    mvi = _batch(monkeypatch, case.name, case.B)
    stream = _lib.lib().tg_dopt_lane_stream(0, 1)
    assert stream
    mvi.set_stream(stream)
    try:
        got = _device_call(mvi, case.N, ir.DT, mvi.device_array(p["Q"]), None, p0, case.ridge)
        _same(host, got)
        # no output asked for: still a launch, nothing written
        mvi.inverse_dynamics_device(case.N, ir.DT, mvi.device_array(p["Q"]), ridge=case.ridge)
        mvi.synchronize()
        assert mvi.kernel_info()["generic_launches"] == 2
    finally:
        mvi.close()


# ---- 3. from a rollout and back -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("wrench_arm", "puppet40"))
def test_round_trip_on_the_device(monkeypatch, name):
    """rollout_device -> inverse_dynamics_device reading X with the row stride nX -> rollout: the inputs come back within the
    derived recovery bound, P is the rollout's own momentum, and the second rollout retraces the first."""
    case = [c for c in ir.CASES if c.name == name][0]
    p = ir.case_paths(case)
    d = p["d"]
    B, N, nq, nd, nu, nk = case.B, case.N, int(d.n_configs), int(d.n_dyn), int(d.n_inputs), int(d.n_kin)
    rng = np.random.default_rng(common.tb_seed("inverse round trip", name))
    Q0, Q1, U, K = common.starts(name, d, B, N, rng)
    mvi = _batch(monkeypatch, name, B)
    mvi.initialize_from_configs(0.0, Q0, ir.DT, Q1)
    nX = mvi.nX
    X_dev = mvi.device_empty(B * (N + 1) * nX)
    mvi.rollout_device(N, ir.DT, mvi.device_array(U) if nu else None, mvi.device_array(K) if nk else None, X_dev)
    mvi.synchronize()
    assert (mvi.status()[1] == 0).all()
    X = mvi.download(X_dev, (B, N + 1, nX))
    got = _device_call(mvi, N, ir.DT, X_dev, nX, None)
    assert (got.status == ir.OK).all()
    packed = mvi.inverse_dynamics(X[:, :, :nq], ir.DT)
    _same(packed, got)                                                   # the strided read changes nothing
    ref = ir.inverse_dynamics(d, X[:, :, :nq], np.full(N, ir.DT), None)
    worst_p = float(np.abs(got.P[:, 1:] - X[:, 1:, nq:nq + nd]).max() / max(1.0, np.abs(X[:, :, nq:nq + nd]).max()))
    worst_rho = float(np.abs(got.rho).max())
    print(name, "P against the rollout's %.3e, |rho|inf %.3e" % (worst_p, worst_rho))
    assert worst_p <= 1e-10 and worst_rho <= 1e-9
    for b in range(B):                                                   # |z - z_applied| <= 2 tolerance / sigma_min, step by step
        for k in range(1, N):
            if nu:
                smin = np.linalg.svd(ref.A[b, k], compute_uv=False).min()
                z = np.concatenate([ir.DT * got.U[b, k], got.lam[b, k]])
                assert np.abs(z[:nu] - ir.DT * U[b, k]).max() <= 2 * ir.TOL / smin + ir.bound(ref)
    again = _batch(monkeypatch, name, B)
    again.initialize_from_state(0.0, X[:, 0, :nq], got.P[:, 0])
    X2 = again.rollout(N, ir.DT, got.U, X[:, 1:, nd:nq])
    assert (again.status()[1] == 0).all()
    worst = float(np.abs(X2[:, :, :nq] - X[:, :, :nq]).max())
    print(name, "round trip: worst |Q - Q_again| %.3e over %d steps" % (worst, N))
    assert worst <= ROUND_TRIP_BOUND
    Xh, Uh, r = mvi.inverse_dynamics_trajectory(X[:, :, :nq], ir.DT)
    assert Xh.shape == X.shape and Uh.shape == (B, N, nu + nk)
    assert np.array_equal(Xh[:, :, :nq], X[:, :, :nq]) and np.array_equal(Xh[:, :, nq:nq + nd], r.P) and np.array_equal(Uh[:, :, nu:], X[:, 1:, nd:nq])
    assert np.abs(Xh[:, 1:, nq + nd:] - X[:, 1:, nq + nd:]).max(initial=0.0) <= 1e-9 * max(1.0, np.abs(X[:, :, nq + nd:]).max(initial=0.0))


# ---- 4. the parameter table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_p0", (True, False), ids=("p0", "no_p0"))
def test_parameter_rows_match_rebuilt_systems(monkeypatch, with_p0):
    case = [c for c in ir.CASES if c.name == "puppet40"][0]
    p = ir.case_paths(case)
    p0 = p["p0"] if with_p0 else None
    rows = ir.parameter_rows(case.name, case.B)
    mvi = _batch(monkeypatch, case.name, case.B)
    plain = mvi.inverse_dynamics(p["Q"], ir.DT, p0)
    mvi.set_parameters(inertia=rows["inertia"], gravity=rows["gravity"], group=1)
    got = mvi.inverse_dynamics(p["Q"], ir.DT, p0)
    ir.compare(case, with_p0, got, ref=ir.parameter_reference(case, with_p0, rows), tag="parameter rows ")
    for q in ir.FIELDS:                                          # row 0 holds the system's own values
        assert np.array_equal(getattr(got, q)[0], getattr(plain, q)[0]), q
    assert np.abs(got.rho[1:]).max() > 1e-6
    info = mvi.kernel_info()
    assert info["par_generic_launch_mask"] == 1 << INVERSE_BIT and info["par_generic_launches"] == 1 and info["par_spec_launches"] == 0
    assert info["generic_launch_mask"] == 1 << INVERSE_BIT and info["generic_launches"] == 1
    mvi.clear_parameters()
    _same(plain, mvi.inverse_dynamics(p["Q"], ir.DT, p0))


# ---- 5. status, refusals, and the state of the batch ----------------------------------------------------------------------------
def test_statuses_arrive_per_step(monkeypatch):
    case = [c for c in ir.CASES if c.name == "scissor4" and c.pattern == "uniform"][0]
    p = ir.case_paths(case)
    mvi = _batch(monkeypatch, case.name, case.B)
    good = mvi.inverse_dynamics(p["Q"], ir.DT, p["p0"])
    Q = p["Q"].copy()
    b, k = 2, 6
    Q[b, k, 1] = np.nan
    got = mvi.inverse_dynamics(Q, ir.DT, p["p0"])
    hit = np.zeros(got.status.shape, dtype=bool)
    hit[b, k - 1:k + 2] = True
    assert (got.status[hit] == ir.SINGULAR).all() and (got.status[~hit] == ir.OK).all()
    for q in ("U", "lam", "rho"):
        assert not getattr(got, q)[hit].any(), q
        assert np.array_equal(getattr(got, q)[~hit], getattr(good, q)[~hit]), q
    assert np.isnan(got.P[b, k]).any() and np.isnan(got.h[b, k - 1]).any()


def test_refusals_make_no_launch(monkeypatch):
    L = _lib.lib()
    mvi = _batch(monkeypatch, "mixed_loop", 2)
    N = 3
    Q = np.zeros((2, N + 1, mvi.nq))
    q = Q.ctypes.data

    def host(n_steps, dt, Qp, ridge):
        return L.tg_batch_inverse_dynamics(mvi._h, n_steps, dt, Qp, None, ridge, None, None, None, None, None, None)

    def device(n_steps, dt, Qp, ridge, stride):
        return L.tg_batch_inverse_dynamics_device(mvi._h, n_steps, dt, Qp, stride, None, ridge, None, None, None, None, None, None)
    assert mvi.nu + mvi.nc > mvi.nd
    for call in (host, lambda *a: device(*a, mvi.nq)):
        assert call(N, ir.DT, q, 0.0) == ERR_INVALID and L.tg_last_error().startswith(b"more unknowns (nu + nc) than dynamic configs")
        assert call(N, ir.DT, q, -1.0) == ERR_INVALID and call(N, ir.DT, q, float("nan")) == ERR_INVALID
        assert call(0, ir.DT, q, 1e-4) == ERR_INVALID and call(N, ir.DT, None, 1e-4) == ERR_INVALID
        assert call(N, 0.0, q, 1e-4) == ERR_INVALID
    assert device(N, ir.DT, q, 1e-4, mvi.nq - 1) == ERR_INVALID and L.tg_last_error() == b"row stride of Q shorter than a configuration"
    mvi.set_step_sizes(np.full(N - 1, ir.DT))
    assert host(N, ir.DT, q, 1e-4) == ERR_INVALID and L.tg_last_error() == b"path longer than the step-size list"
    mvi.set_step_sizes(np.full(2, ir.DT), by_trajectory=True)
    assert host(1, ir.DT, q, 1e-4) == ERR_INVALID and L.tg_last_error() == b"a by-trajectory step-size list takes one-step launches only"
    mvi.set_step_sizes(None)
    with pytest.raises(ValueError):
        mvi.inverse_dynamics(Q, ir.DT)                               # n > nd without a ridge
    with pytest.raises(ValueError):
        mvi.inverse_dynamics(Q[:, :1], ir.DT, ridge=1e-4)            # N = 0
    assert mvi.kernel_info()["generic_launches"] == 0


def test_the_batch_state_is_unchanged_and_a_specialised_library_has_no_say(monkeypatch):
    case = [c for c in ir.CASES if c.name == "scissor4" and c.pattern == "alternating"][0]
    name = case.name
    p = ir.case_paths(case)
    B, N = case.B, 6
    _, d = common.build(name)
    rng = np.random.default_rng(common.tb_seed("inverse state", name))
    S0, S1, U, K = common.starts(name, d, B, N, rng)
    plain = _batch(monkeypatch, name, B).inverse_dynamics(p["Q"], p["dts"], p["p0"])

    def fresh():
        mvi = _batch(monkeypatch, name, B, specialize="auto")
        mvi.initialize_from_configs(0.0, S0, ir.DT, S1)
        return mvi

    X_ref = fresh().rollout(N, ir.DT, U, K)
    mvi = fresh()
    assert mvi.kernel_info()["spec_modes"]                               # build() prepares this system's library
    state = lambda: [getattr(mvi, n).copy() for n in ("q1", "q2", "p1", "p2", "lambda1")] + list(mvi.status()) + [mvi.times()]
    before = state()
    _same(plain, mvi.inverse_dynamics(p["Q"], p["dts"], p["p0"]))
    info = mvi.kernel_info()
    assert (info["generic_launch_mask"] >> INVERSE_BIT) & 1 and not (info["spec_launch_mask"] >> INVERSE_BIT) & 1
    for a, b_ in zip(before, state()):
        assert np.array_equal(a, b_)
    assert np.array_equal(mvi.rollout(N, ir.DT, U, K), X_ref)
    assert (mvi.status()[1] == 0).all()
