"""Batched computed torque on the device (BatchMidpointVI.dynamics_inverse, k_dyn_inverse): the case table of
dynamics_inverse_reference.py at every system's own team size and at every team size of common.TEAM_CELLS against the numpy
specification with the bounds of the CPU tests (z and rho max(1e-10, 64 e_ref) relative to max(1, |z|inf), tau and acc 1e-10); equal
bits for a state repeated in a launch, alone in a launch, and through the host and the device entry points; strided rows; the round
trip dynamics -> dynamics_inverse; the parameter twin against rebuilt systems; status, the launch masks, the refusals and the
untouched integrator state."""
import numpy as np
import pytest

import common
import dynamics_inverse_reference as dr
import inverse_dynamics_reference as ir
from trep_amd import BatchMidpointVI, _lib

pytestmark = pytest.mark.gpu

CASE_IDS = [dr.case_id(c) for c in dr.CASES]
DYN_INVERSE_BIT = 14
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
TEAM_RUNS = [(c, t) for c in dr.CASES if c.name in common.TEAM_CELLS for t in sorted(common.TEAM_CELLS[c.name])]
FULL_RANK = [c for c in dr.CASES if c.ridge == 0.0]


def _batch(monkeypatch, name, B, team=None, specialize=False):
    if team is None:
        monkeypatch.delenv("TREPAMD_TEAM", raising=False)
    else:
        monkeypatch.setenv("TREPAMD_TEAM", str(team))
    mvi = BatchMidpointVI(common.build(name)[0], B, specialize=specialize)
    if team is not None:
        assert mvi.kernel_info()["team"] == team
    return mvi


def _same(a, b, fields=dr.FIELDS):
    for q in fields:
        assert np.array_equal(getattr(a, q), getattr(b, q)), q


def _call(mvi, case, **kw):
    p = dr.case_states(case)
    return mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], case.ridge, **kw)


def _fits(mvi):
    """Does a workgroup of the kernel fit the LDS at this batch's team size (tg_system_dynamics_inverse_lds)?"""
    out = np.zeros(4, dtype=np.int32)
    rc = _lib.lib().tg_system_dynamics_inverse_lds(mvi._sys_h, out.ctypes.data_as(_lib._c_ip))
    assert rc in (0, ERR_UNSUPPORTED) and out[0] == mvi.kernel_info()["team"]
    assert (rc == 0) == (int(out[2]) <= 160 * 1024)
    return rc == 0


# ---- 1. the table on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dr.CASES, ids=CASE_IDS)
def test_the_table_at_the_systems_own_team(monkeypatch, case):
    mvi = _batch(monkeypatch, case.name, case.B)
    got = _call(mvi, case)
    dr.compare(case, got)
    info = mvi.kernel_info()
    assert info["generic_launch_mask"] == 1 << DYN_INVERSE_BIT and info["spec_launch_mask"] == 0 and info["generic_launches"] == 1
    assert info["par_generic_launches"] == 0


@pytest.mark.parametrize("case,team", TEAM_RUNS, ids=["%s_team%d" % (dr.case_id(c), t) for c, t in TEAM_RUNS])
def test_every_team_size(monkeypatch, case, team):
    mvi = _batch(monkeypatch, case.name, case.B, team)
    if not _fits(mvi):
        with pytest.raises(_lib.LibraryError, match="system too large for the LDS-resident computed-torque kernel"):
            _call(mvi, case)
        assert mvi.kernel_info()["generic_launches"] == 0
        return
    dr.compare(case, _call(mvi, case), tag="team %d " % team)


def test_both_sides_of_the_lds_limit_are_run(monkeypatch):
    seen = set()
    for case, team in TEAM_RUNS:
        seen.add(_fits(_batch(monkeypatch, case.name, 1, team)))
    assert seen == {True, False}


# ---- 2. equal bits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("scissor4", "wrench_arm", "puppet40"))
def test_a_state_does_not_depend_on_its_launch(monkeypatch, name):
    """Trajectories repeated in one launch, a state repeated within a trajectory, and one state alone in a 1 x 1 launch: the same bits."""
    case = dr.case_by_name(name)
    p = dr.case_states(case)
    Q, dQ, ddQ = p["Q"], p["dQ"], p["ddQ"]
    whole = _call(_batch(monkeypatch, name, case.B), case)
    pick = np.array([2, 0, 2, 1, 2, 2, 0])
    again = _batch(monkeypatch, name, len(pick)).dynamics_inverse(Q[pick], dQ[pick], ddQ[pick], case.ridge)
    for q in dr.FIELDS:
        assert np.array_equal(getattr(again, q), getattr(whole, q)[pick]), q
    b, s = 2, 3
    cols = np.array([s, 0, s, s, 1, s])
    within = _batch(monkeypatch, name, 1).dynamics_inverse(Q[b:b + 1, cols], dQ[b:b + 1, cols], ddQ[b:b + 1, cols], case.ridge)
    one = _batch(monkeypatch, name, 1).dynamics_inverse(Q[b:b + 1, s:s + 1], dQ[b:b + 1, s:s + 1], ddQ[b:b + 1, s:s + 1], case.ridge)
    flat = _batch(monkeypatch, name, 1).dynamics_inverse(Q[b:b + 1, s], dQ[b:b + 1, s], ddQ[b:b + 1, s], case.ridge)
    for q in dr.FIELDS:
        assert np.array_equal(getattr(within, q)[0], getattr(whole, q)[b, cols]), q
        assert np.array_equal(getattr(one, q)[0, 0], getattr(whole, q)[b, s]), q
        assert np.array_equal(getattr(flat, q)[0], getattr(whole, q)[b, s]), q
    assert flat.U.shape == (1, int(p["d"].n_inputs)) and flat.status.shape == (1,)


def _device_call(mvi, M, arrays, strides=(None, None, None), ridge=0.0, want=dr.FIELDS):
    """dynamics_inverse_device with the outputs asked for, downloaded (the others None)."""
    L = _lib.lib()
    B, nd, nu, nc = mvi._batch, mvi.nd, mvi.nu, mvi.nc
    Q_dev, dQ_dev, ddQ_dev = (mvi.device_array(a) for a in arrays)
    size = {"U": nu, "lam": nc, "rho": nd, "tau": nd, "acc": nc}
    dev = {q: (mvi.device_empty(B * M * size[q]) if q in want and size[q] else None) for q in size}
    words = L.tg_device_alloc(0, 4 * B * M)
    assert words
    try:
        mvi.dynamics_inverse_device(M, Q_dev, dQ_dev, ddQ_dev, strides[0], strides[1], strides[2], ridge, dev["U"], dev["lam"], dev["rho"],
                                    dev["tau"], dev["acc"], words if "status" in want else None)
        mvi.synchronize()
        status = np.zeros((B, M), dtype=np.int32)
        _lib.check(L.tg_memcpy_d2h(0, status.ctypes.data, words, 4 * B * M))
    finally:
        L.tg_device_free(0, words)
    get = lambda q: (mvi.download(dev[q], (B, M, size[q])) if dev[q] else np.zeros((B, M, 0))) if q in want else None
    return dr.Result(get("U"), get("lam"), get("rho"), get("tau"), get("acc"), status if "status" in want else None, None, None, None, None, None)


def test_host_and_device_variants_give_the_same_bits(monkeypatch):
    case = dr.case_by_name("mixed_loop")
    p = dr.case_states(case)
    host = _call(_batch(monkeypatch, case.name, case.B), case)
    mvi = _batch(monkeypatch, case.name, case.B)
    stream = _lib.lib().tg_dopt_lane_stream(0, 1)
    assert stream
    mvi.set_stream(stream)
    try:
        arrays = (p["Q"], p["dQ"], p["ddQ"])
        _same(host, _device_call(mvi, case.M, arrays, ridge=case.ridge))
        # strided rows, each array with a stride of its own
        nq = mvi.nq
        widths = (mvi.nX, nq + 3, nq + 1)
        wide = []
        for a, w in zip(arrays, widths):
            x = np.full((case.B, case.M, w), np.nan)
            x[:, :, :nq] = a
            wide.append(x)
        _same(host, _device_call(mvi, case.M, wide, widths, case.ridge))
        # one output alone: the same bits; no output at all: still a launch, nothing written
        alone = _device_call(mvi, case.M, arrays, ridge=case.ridge, want=("tau",))
        assert np.array_equal(alone.tau, host.tau)
        _device_call(mvi, case.M, arrays, ridge=case.ridge, want=())
        assert mvi.kernel_info()["generic_launches"] == 4
    finally:
        mvi.close()


# ---- 3. dynamics and back -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FULL_RANK, ids=[dr.case_id(c) for c in FULL_RANK])
def test_round_trip_through_the_forward_kernel(monkeypatch, case):
    """ddq_d = dynamics(q, dq, u, ddq_k) on the device, then dynamics_inverse of (q, dq, (ddq_d | ddq_k)): u and lambda come back, rho
    and acc vanish -- as far as the forward kernel's answer solves its own equations.  With the oracle's A and r0 at the very states
    the inverse kernel is given, e = r0 + A z_applied, z_applied = (u, lambda of the forward kernel), is the forward answer's residual.
    The least-squares z has |rho|_2 <= |e|_2, so |A (z - z_applied)|_2 <= 2 |e|_2 and, state by state,
    |z - z_applied| <= 2 |e|_2 / sigma_min(A) and |rho| <= |e|_2, each plus the table's bound for the inverse kernel's own error;
    acc is held to the specification's acc of the same states (the forward answer's constraint residual) within the table's 1e-10."""
    p = dr.case_states(case)
    d = p["d"]
    nq, nd, nu, nc = int(d.n_configs), int(d.n_dyn), int(d.n_inputs), int(d.n_constraints)
    rows = case.B * case.M
    rng = np.random.default_rng(common.tb_seed("dynamics inverse round trip", case.name))
    U = rng.standard_normal((rows, nu))
    Q, dQ, ddQ = (p[k].reshape(rows, nq).copy() for k in ("Q", "dQ", "ddQ"))
    mvi = _batch(monkeypatch, case.name, rows)
    ddq, lam, status = mvi.dynamics(Q, dQ, U, ddQ[:, nd:])
    assert (status == 0).all()
    ddQ[:, :nd] = ddq
    got = mvi.dynamics_inverse(Q, dQ, ddQ)
    assert got.U.shape == (rows, nu) and got.status.shape == (rows,) and (got.status == dr.OK).all()
    ref = dr.dynamics_inverse(d, Q[:, None], dQ[:, None], ddQ[:, None])
    applied = dr.unknowns(U, lam)
    scale, bd = dr.floors(ref)["scale"], dr.bound(ref)
    z = dr.unknowns(got.U, got.lam)
    worst = {"e": 0.0, "z": 0.0, "share": 0.0, "rho": 0.0}
    for r in range(rows):
        A, r0 = ref.A[r, 0], ref.r0[r, 0]
        e = float(np.linalg.norm(r0 + A.dot(applied[r])))
        smin = float(np.linalg.svd(A, compute_uv=False).min()) if nu + nc else np.inf
        miss, allowed = float(np.abs(z[r] - applied[r]).max(initial=0.0)), 2 * e / smin + bd * scale
        rho = float(np.abs(got.rho[r]).max())
        worst = {"e": max(worst["e"], e), "z": max(worst["z"], miss), "share": max(worst["share"], miss / allowed), "rho": max(worst["rho"], rho)}
        assert miss <= allowed, (r, miss, allowed, e, smin)
        assert rho <= e + bd * scale, (r, rho, e)
    e_acc = float(np.abs(got.acc - ref.acc[:, 0]).max(initial=0.0)) / max(1.0, float(np.abs(ref.acc).max(initial=0.0)))
    print(dr.case_id(case), "round trip: forward residual |e| %.3e, |z - z_applied| %.3e (largest share of its bound %.3f), |rho| %.3e, acc against the specification %.3e, |acc| %.3e" % (
        worst["e"], worst["z"], worst["share"], worst["rho"], e_acc, float(np.abs(got.acc).max(initial=0.0))))
    assert e_acc <= dr.TOL_DIRECT
    info = mvi.kernel_info()
    assert info["generic_launch_mask"] == (1 << DYN_INVERSE_BIT) | (1 << 5) and info["generic_launches"] == 2


# ---- 4. the parameter table ---------------------------------------------------------------------------------------------------------
def test_parameter_rows_match_rebuilt_systems(monkeypatch):
    case = dr.case_by_name("puppet40")
    rows = ir.parameter_rows(case.name, case.B)
    mvi = _batch(monkeypatch, case.name, case.B)
    plain = _call(mvi, case)
    mvi.set_parameters(inertia=rows["inertia"], gravity=rows["gravity"], group=1)
    got = _call(mvi, case)
    dr.compare(case, got, ref=dr.parameter_reference(case, rows), tag="parameter rows ")
    for q in dr.FIELDS:                                          # row 0 holds the system's own values
        assert np.array_equal(getattr(got, q)[0], getattr(plain, q)[0]), q
    assert np.abs(got.tau[1:] - plain.tau[1:]).max() > 1e-3
    info = mvi.kernel_info()
    assert info["par_generic_launch_mask"] == 1 << DYN_INVERSE_BIT and info["par_generic_launches"] == 1 and info["par_spec_launches"] == 0
    assert info["generic_launch_mask"] == 1 << DYN_INVERSE_BIT and info["generic_launches"] == 1
    mvi.clear_parameters()
    _same(plain, _call(mvi, case))


# ---- 5. status, refusals, and the state of the batch --------------------------------------------------------------------------------
def test_statuses_arrive_per_state(monkeypatch):
    case = dr.case_by_name("scissor4")
    p = dr.case_states(case)
    mvi = _batch(monkeypatch, case.name, case.B)
    good = _call(mvi, case)
    ddQ = p["ddQ"].copy()
    b, s = 2, 6
    ddQ[b, s, 1] = np.nan
    got = mvi.dynamics_inverse(p["Q"], p["dQ"], ddQ)
    hit = np.zeros(got.status.shape, dtype=bool)
    hit[b, s] = True
    assert (got.status[hit] == dr.SINGULAR).all() and (got.status[~hit] == dr.OK).all()
    for q in ("U", "lam", "rho"):
        assert not getattr(got, q)[hit].any(), q
    for q in dr.FIELDS:
        assert np.array_equal(getattr(got, q)[~hit], getattr(good, q)[~hit]), q
    assert np.isnan(got.tau[b, s]).any() and np.isnan(got.acc[b, s]).any()


def test_refusals_make_no_launch(monkeypatch):
    L = _lib.lib()
    mvi = _batch(monkeypatch, "mixed_loop", 2)
    M = 3
    Q = np.zeros((2, M, mvi.nq))
    q = Q.ctypes.data

    def host(n_states, Qp, dQp, ddQp, ridge):
        return L.tg_batch_dynamics_inverse(mvi._h, n_states, Qp, dQp, ddQp, ridge, None, None, None, None, None, None)

    def device(n_states, Qp, dQp, ddQp, ridge, strides=None):
        s = strides or (mvi.nq,) * 3
        return L.tg_batch_dynamics_inverse_device(mvi._h, n_states, Qp, s[0], dQp, s[1], ddQp, s[2], ridge, None, None, None, None, None, None)
    assert mvi.nu + mvi.nc > mvi.nd
    for call in (host, device):
        assert call(M, q, q, q, 0.0) == ERR_INVALID and L.tg_last_error().startswith(b"more unknowns (nu + nc) than dynamic configs")
        assert call(M, q, q, q, -1.0) == ERR_INVALID and call(M, q, q, q, float("nan")) == ERR_INVALID
        assert call(0, q, q, q, 1e-4) == ERR_INVALID
        assert call(M, None, q, q, 1e-4) == ERR_INVALID and call(M, q, None, q, 1e-4) == ERR_INVALID and call(M, q, q, None, 1e-4) == ERR_INVALID
    nq = mvi.nq
    for strides, message in (((nq - 1, nq, nq), b"row stride of Q shorter than a configuration"),
                             ((nq, nq - 1, nq), b"row stride of dQ shorter than a configuration"),
                             ((nq, nq, nq - 1), b"row stride of ddQ shorter than a configuration")):
        assert device(M, q, q, q, 1e-4, strides) == ERR_INVALID and L.tg_last_error() == message
    with pytest.raises(ValueError, match="more unknowns"):
        mvi.dynamics_inverse(Q, Q, Q)                                # n > nd without a ridge
    with pytest.raises(ValueError, match="ridge"):
        mvi.dynamics_inverse(Q, Q, Q, ridge=-1.0)
    with pytest.raises(ValueError):
        mvi.dynamics_inverse(Q[:, :0], Q[:, :0], Q[:, :0], ridge=1e-4)   # M = 0
    with pytest.raises(ValueError):
        mvi.dynamics_inverse(Q, Q[:, :2], Q, ridge=1e-4)             # shapes that differ
    with pytest.raises(ValueError):
        mvi.dynamics_inverse(Q, None, Q, ridge=1e-4)
    with pytest.raises(ValueError, match="null dQ"):
        mvi.dynamics_inverse_device(M, 1, None, 1, ridge=1e-4)
    assert mvi.kernel_info()["generic_launches"] == 0


def test_the_batch_state_is_unchanged_and_a_specialised_library_has_no_say(monkeypatch):
    case = dr.case_by_name("scissor4")
    name = case.name
    B, N = case.B, 6
    _, d = common.build(name)
    rng = np.random.default_rng(common.tb_seed("dynamics inverse state", name))
    S0, S1, U, K = common.starts(name, d, B, N, rng)
    plain = _call(_batch(monkeypatch, name, B), case)

    def fresh():
        mvi = _batch(monkeypatch, name, B, specialize="auto")
        mvi.initialize_from_configs(0.0, S0, ir.DT, S1)
        return mvi

    X_ref = fresh().rollout(N, ir.DT, U, K)
    mvi = fresh()
    assert mvi.kernel_info()["spec_modes"]                               # build() prepares this system's library
    state = lambda: [getattr(mvi, n).copy() for n in ("q1", "q2", "p1", "p2", "lambda1")] + list(mvi.status()) + [mvi.times()]
    before = state()
    _same(plain, _call(mvi, case))
    info = mvi.kernel_info()
    assert (info["generic_launch_mask"] >> DYN_INVERSE_BIT) & 1 and not (info["spec_launch_mask"] >> DYN_INVERSE_BIT) & 1
    for a, b_ in zip(before, state()):
        assert np.array_equal(a, b_)
    assert np.array_equal(mvi.rollout(N, ir.DT, U, K), X_ref)
    assert (mvi.status()[1] == 0).all()
