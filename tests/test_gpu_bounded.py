"""Bounded inverse dynamics on the device (BatchMidpointVI.dynamics_inverse / inverse_dynamics with bounds=, the BND instantiations
of k_dyn_inverse / k_inverse, csrc/bvls_solve.hpp): both tables of bounded_reference.py at the system's own team size and at every
team size of common.TEAM_CELLS against the certified specification (z and rho max(1e-10, 64 e_ref) relative to max(1, |z|inf), the
direct quantities as their siblings, `active` equal); equal bits through the host and the device entry points, for repeated states
and across the four team sizes; all-infinite bounds to the bits of the rcond= kernels; the round trip from dynamics(); the status
rows beside untouched neighbours; the refusals; and the solver alone (tg_batch_debug_bvls_solve) on crafted problems at teams 1, 4, 16
and 64, 65 problems per launch whose numbers of solves are interleaved -- the one place where teams that finish at different times
share a wavefront and a workgroup.  Every test runs a handful of launches on tables of at most 65 states."""
import numpy as np
import pytest

import bounded_reference as br
import common
import dynamics_inverse_reference as cref
import inverse_dynamics_reference as dref
import min_norm_reference as mr
from trep_amd import BatchMidpointVI, _lib

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -3
DYN_INVERSE_BIT, INVERSE_BIT = 14, 11
OK_C = [c for c in br.CONTINUOUS if c.expect == "ok"]


def _teams(name):
    return sorted(common.TEAM_CELLS[name]) if name in common.TEAM_CELLS else [None]


CT_RUNS = [(c, t) for c in OK_C for t in _teams(c.name)]
ID_RUNS = [(c, t) for c in br.DISCRETE for t in _teams(c.name)]
_tid = lambda t: "own" if t is None else "team%d" % t


def _batch(monkeypatch, name, B, team=None):
    if team is None:
        monkeypatch.delenv("TREPAMD_TEAM", raising=False)
    else:
        monkeypatch.setenv("TREPAMD_TEAM", str(team))
    mvi = BatchMidpointVI(common.build(name)[0], B, specialize=False)
    if team is not None:
        assert mvi.kernel_info()["team"] == team
    return mvi


def _fits(mvi, fn):
    out = np.zeros(4, dtype=np.int32)
    rc = fn(mvi._sys_h, out.ctypes.data_as(_lib._c_ip))
    assert rc in (0, ERR_UNSUPPORTED) and out[0] == mvi.kernel_info()["team"] and (rc == 0) == (int(out[2]) <= 160 * 1024)
    return rc == 0


def _same(a, b):
    for q in a._fields:
        assert np.array_equal(getattr(a, q), getattr(b, q)), q


def _ct(mvi, t):
    p = t.inputs
    return mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], t.case.ridge, bounds=(t.lo, t.hi))


def _dt(t):
    return t.inputs["dts"] if t.case.pattern != "uniform" else dref.DT


# ---- 1. both tables on the device ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,team", CT_RUNS, ids=["%s_%s" % (br.ccase_id(c), _tid(t)) for c, t in CT_RUNS])
def test_computed_torque_table(monkeypatch, case, team):
    t = br.continuous_table(case)
    mvi = _batch(monkeypatch, case.name, case.B, team)
    if not _fits(mvi, _lib.lib().tg_system_dynamics_inverse_bounded_lds):
        with pytest.raises(_lib.LibraryError, match="system too large for the LDS-resident computed-torque kernel"):
            _ct(mvi, t)
        return
    got = _ct(mvi, t)
    assert got._fields[-3:] == ("rank", "active", "solves") and got.active.shape == t.active.shape and got.active.dtype == np.int32
    br.compare_continuous(t, got, "%s " % _tid(team))
    info = mvi.kernel_info()
    assert info["generic_launch_mask"] == 1 << DYN_INVERSE_BIT and info["spec_launch_mask"] == 0 and info["generic_launches"] == 1


@pytest.mark.parametrize("case,team", ID_RUNS, ids=["%s_%s" % (br.dcase_id(c), _tid(t)) for c, t in ID_RUNS])
def test_discrete_table(monkeypatch, case, team):
    mvi = _batch(monkeypatch, case.name, case.B, team)
    fits = _fits(mvi, _lib.lib().tg_system_inverse_dynamics_bounded_lds)
    for with_p0 in (True, False):
        t = br.discrete_table(case, with_p0)
        p = t.inputs
        call = lambda: mvi.inverse_dynamics(p["Q"], _dt(t), p["p0"] if with_p0 else None, case.ridge, bounds=(t.lo, t.hi))
        if not fits:
            with pytest.raises(_lib.LibraryError, match="system too large for the LDS-resident inverse-dynamics kernel"):
                call()
            return
        got = call()
        assert got._fields[-3:] == ("rank", "active", "solves")
        br.compare_discrete(t, got, "%s " % _tid(team))
        if not with_p0:
            for q in ("U", "lam", "rho", "rank", "active", "solves"):
                assert not getattr(got, q)[:, 0].any(), q
    assert mvi.kernel_info()["generic_launch_mask"] == 1 << INVERSE_BIT and getattr(mvi, "_step_sizes", None) is None


def test_parameter_twin_matches_rebuilt_systems(monkeypatch):
    c = br.CONTINUOUS[0]
    t = br.continuous_table(c)
    rows = dref.parameter_rows(c.name, c.B)
    ref = cref.parameter_reference(t.base, rows)
    solved = np.ones((c.B, c.M), dtype=bool)
    z, z_aug, rho, rho_aug, active, g, margins = br._solve_table(ref.A, ref.r0, c.ridge, lambda b, s: t.lo, lambda b, s: t.hi, solved)
    twin = t._replace(ref=ref, z=z, z_aug=z_aug, rho=rho, rho_aug=rho_aug, active=active, g=g, margins=margins)
    mvi = _batch(monkeypatch, c.name, c.B)
    mvi.set_parameters(inertia=rows["inertia"], gravity=rows["gravity"], group=1)
    br.compare_continuous(twin, _ct(mvi, t), "parameter rows ")
    info = mvi.kernel_info()
    assert info["par_generic_launches"] == 1 and info["generic_launches"] == 0


def test_tension_bounds_helper(monkeypatch):
    mvi = _batch(monkeypatch, "puppet40", 1)
    for call in ("dynamics_inverse", "inverse_dynamics"):
        lo, hi = mvi.tension_bounds(call)
        want = br.tension_bounds("puppet40", mvi.nu, mvi.nc, call)
        assert np.array_equal(lo, want[0]) and np.array_equal(hi, want[1])
    with pytest.raises(ValueError, match="call must be"):
        mvi.tension_bounds("rollout")
    arm = _batch(monkeypatch, "wrench_arm", 1)
    lo, hi = arm.tension_bounds()
    assert np.all(lo == -np.inf) and np.all(hi == np.inf)


# ---- 2. equal bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("scissor4", "wrench_arm"))
def test_the_four_team_sizes_give_the_same_bits(monkeypatch, name):
    c = [c for c in OK_C if c.name == name][0]
    t = br.continuous_table(c)
    d = [d for d in br.DISCRETE if d.name == name][0]
    td = br.discrete_table(d, True)
    first, ran = None, []
    for team in (1, 4, 16, 64):
        mvi = _batch(monkeypatch, name, c.B, team)
        if not (_fits(mvi, _lib.lib().tg_system_dynamics_inverse_bounded_lds) and _fits(mvi, _lib.lib().tg_system_inverse_dynamics_bounded_lds)):
            continue      # (scissor4 at teams 1 and 4 -- 64 and 16 teams to a workgroup -- exceeds its LDS: refused, as test_computed_torque_table shows)
        ran.append(team)
        got = (_ct(mvi, t), mvi.inverse_dynamics(td.inputs["Q"], _dt(td), td.inputs["p0"], d.ridge, bounds=(td.lo, td.hi)))
        if first is None:
            first = got
        else:
            _same(first[0], got[0])
            _same(first[1], got[1])
    assert ran == [16, 64] if name == "scissor4" else len(ran) >= 3, ran


def test_a_state_does_not_depend_on_its_launch(monkeypatch):
    c = [c for c in OK_C if c.name == "scissor4"][0]
    t = br.continuous_table(c)
    p = t.inputs
    whole = _ct(_batch(monkeypatch, c.name, c.B), t)
    pick = np.array([2, 0, 2, 1, 2, 2, 0])
    again = _batch(monkeypatch, c.name, len(pick)).dynamics_inverse(p["Q"][pick], p["dQ"][pick], p["ddQ"][pick], c.ridge, bounds=(t.lo, t.hi))
    for q in whole._fields:
        assert np.array_equal(getattr(again, q), getattr(whole, q)[pick]), q
    b, s = 2, 3
    flat = _batch(monkeypatch, c.name, 1).dynamics_inverse(p["Q"][b:b + 1, s], p["dQ"][b:b + 1, s], p["ddQ"][b:b + 1, s], c.ridge, bounds=(t.lo, t.hi))
    for q in whole._fields:
        assert np.array_equal(getattr(flat, q)[0], getattr(whole, q)[b, s]), q
    assert flat.active.shape == (1, t.z.shape[-1]) and flat.solves.shape == (1,)


def _words(count):
    w = _lib.lib().tg_device_alloc(0, 4 * count)
    assert w
    return w


def _download_words(w, shape):
    out = np.zeros(shape, dtype=np.int32)
    _lib.check(_lib.lib().tg_memcpy_d2h(0, out.ctypes.data, w, 4 * out.size))
    return out


def test_host_and_device_entry_points_give_the_same_bits(monkeypatch):
    """Both questions on wrench_arm (the per-trajectory box in the discrete one), strided rows, then null outputs."""
    L = _lib.lib()
    c = [c for c in OK_C if c.name == "wrench_arm"][0]
    t = br.continuous_table(c)
    p = t.inputs
    mvi = _batch(monkeypatch, c.name, c.B)
    host = _ct(mvi, t)
    B, M, nd, nu, nc, nq = c.B, c.M, mvi.nd, mvi.nu, mvi.nc, mvi.nq
    n = nu + nc
    widths = (mvi.nX, nq + 3, nq + 1)
    wide = []
    for a, w in zip((p["Q"], p["dQ"], p["ddQ"]), widths):
        x = np.full((B, M, w), np.nan)
        x[:, :, :nq] = a
        wide.append(mvi.device_array(x))
    size = {"U": nu, "lam": nc, "rho": nd, "tau": nd, "acc": nc}
    dev = {q: mvi.device_empty(B * M * k) for q, k in size.items()}
    words = {q: _words(B * M * k) for q, k in (("status", 1), ("rank", 1), ("solves", 1), ("active", n))}
    box = (mvi.device_array(t.lo[None]), mvi.device_array(t.hi[None]), 1)
    try:
        mvi.dynamics_inverse_device(M, wide[0], wide[1], wide[2], widths[0], widths[1], widths[2], c.ridge, dev["U"], dev["lam"], dev["rho"], dev["tau"],
                                    dev["acc"], words["status"], rank_dev=words["rank"], bounds_dev=box, active_dev=words["active"], solves_dev=words["solves"])
        mvi.synchronize()
        for q, k in size.items():
            assert np.array_equal(mvi.download(dev[q], (B, M, k)), getattr(host, q)), q
        for q in ("status", "rank", "solves"):
            assert np.array_equal(_download_words(words[q], (B, M)), getattr(host, q)), q
        assert np.array_equal(_download_words(words["active"], (B, M, n)), host.active)
        mvi.dynamics_inverse_device(M, wide[0], wide[1], wide[2], widths[0], widths[1], widths[2], c.ridge, bounds_dev=box)      # null outputs: still a launch
        mvi.synchronize()
        assert mvi.kernel_info()["generic_launches"] == 3
        with pytest.raises(ValueError, match="need bounds_dev"):
            mvi.dynamics_inverse_device(M, wide[0], wide[1], wide[2], solves_dev=words["solves"])
        # the discrete question, one box per trajectory
        d = [d for d in br.DISCRETE if d.per_trajectory][0]
        td = br.discrete_table(d, True)
        q_ = td.inputs
        N = d.N
        mvd = _batch(monkeypatch, d.name, d.B)
        hostd = mvd.inverse_dynamics(q_["Q"], _dt(td), q_["p0"], d.ridge, bounds=(td.lo, td.hi))
        U, lam, P, rho, h = (mvd.device_empty(B * N * nu), mvd.device_empty(B * N * nc), mvd.device_empty(B * (N + 1) * nd), mvd.device_empty(B * N * nd),
                             mvd.device_empty(B * N * nc))
        mvd.set_step_sizes(q_["dts"])
        mvd.inverse_dynamics_device(N, float(q_["dts"][0]), mvd.device_array(q_["Q"]), None, mvd.device_array(q_["p0"]), d.ridge, U, lam, P, rho, h,
                                    words["status"], rank_dev=words["rank"], bounds_dev=(mvd.device_array(td.lo), mvd.device_array(td.hi), d.B),
                                    active_dev=words["active"], solves_dev=words["solves"])
        mvd.synchronize()
        got = type(hostd)(mvd.download(U, (B, N, nu)), mvd.download(lam, (B, N, nc)), mvd.download(P, (B, N + 1, nd)), mvd.download(rho, (B, N, nd)),
                          mvd.download(h, (B, N, nc)), _download_words(words["status"], (B, N)), _download_words(words["rank"], (B, N)),
                          _download_words(words["active"], (B, N, n)), _download_words(words["solves"], (B, N)))
        _same(hostd, got)
    finally:
        for w in words.values():
            L.tg_device_free(0, w)


@pytest.mark.parametrize("name", ("puppet40", "wrench_arm", "scissor4", "puppet_forces"))
def test_infinite_bounds_give_the_bits_of_the_rcond_kernels(monkeypatch, name):
    ridge = 1e-4 if name == "puppet_forces" else 0.0
    Q, dQ, ddQ = cref.draw_states(name, 3, 5, 0)
    mvi = _batch(monkeypatch, name, 3)
    old = mvi.dynamics_inverse(Q, dQ, ddQ, ridge, rcond=br.RCOND)
    new = mvi.dynamics_inverse(Q, dQ, ddQ, ridge, bounds=(None, None))
    for q in old._fields:
        assert np.array_equal(getattr(old, q), getattr(new, q)), q
    assert (new.solves == 1).all() and not new.active.any()
    base = [c for c in dref.CASES if c.name == name][0]
    p = dref.case_paths(base)
    mvd = _batch(monkeypatch, name, base.B)
    for p0 in (p["p0"], None):
        old = mvd.inverse_dynamics(p["Q"], dref.DT, p0, ridge, rcond=br.RCOND)
        new = mvd.inverse_dynamics(p["Q"], dref.DT, p0, ridge, bounds=(-np.inf, np.inf))
        for q in old._fields:
            assert np.array_equal(getattr(old, q), getattr(new, q)), q


def test_without_bounds_nothing_changes(monkeypatch):
    c = [c for c in OK_C if c.name == "wrench_arm"][0]
    p = br.continuous_table(c).inputs
    mvi = _batch(monkeypatch, c.name, c.B)
    assert mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"])._fields == ("U", "lam", "rho", "tau", "acc", "status")
    assert mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], rcond=1e-9)._fields[-1] == "rank"


# ---- 3. the round trip --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("wrench_arm", "scissor4", "puppet40"))
def test_round_trip_from_dynamics_with_a_box_that_contains_the_answer(monkeypatch, name):
    """dynamics() -> bounded dynamics_inverse returns the forward u and lambda when the box contains them: with e = r0 + A z_forward
    (the residual of the forward answer in the inverse problem's own terms), |z - z_forward|_2 <= 2 |e|_2 / sigma_min(A), the derived
    bound tests/test_gpu_dynamics_inverse.py uses.  The box is one-sided at distance 1 from the forward answer on alternating sides,
    so every variable has a finite bound and none is active."""
    d = common.build(name)[1]
    B = 4
    mvi = _batch(monkeypatch, name, B)
    rng = np.random.default_rng(common.tb_seed("bounded round trip", name))
    poses = cref.recorded_poses(name)
    Q = poses[rng.integers(len(poses), size=B)]
    dQ = 0.3 * rng.standard_normal(Q.shape)
    U = rng.standard_normal((B, mvi.nu))
    ddQk = rng.standard_normal((B, mvi.nk))
    ddq, lam, status = mvi.dynamics(Q, dQ, U, ddQk)
    assert (status == 0).all()
    zf = np.concatenate([U, lam], axis=1)
    side = np.arange(zf.shape[1]) % 2 == 0
    lo, hi = np.where(side, zf - 1.0, -np.inf), np.where(side, np.inf, zf + 1.0)
    ddQ = np.concatenate([ddq, ddQk], axis=1)
    got = mvi.dynamics_inverse(Q, dQ, ddQ, bounds=(lo, hi))
    assert (got.status == 0).all() and not got.active.any() and (got.solves == 1).all()
    ref = cref.dynamics_inverse(d, Q[:, None], dQ[:, None], ddQ[:, None])
    for b in range(B):
        A, r0 = ref.A[b, 0], ref.r0[b, 0]
        e = r0 + A.dot(zf[b])
        smin = np.linalg.svd(A, compute_uv=False).min()
        miss = np.linalg.norm(np.concatenate([got.U[b], got.lam[b]]) - zf[b])
        bound = 2.0 * np.linalg.norm(e) / smin + 1e-12 * max(1.0, np.abs(zf[b]).max())
        print("%s state %d: |z - z_forward| %.3e, 2 |e| / sigma_min %.3e" % (name, b, miss, bound))
        assert miss <= bound


# ---- 4. status rows and refusals --------------------------------------------------------------------------------------------------------------
def test_singular_and_non_finite_rows_beside_untouched_neighbours(monkeypatch):
    c = [c for c in br.CONTINUOUS if c.expect == "singular"][0]
    p = cref.case_states(cref.Case(c.name, c.B, c.M, c.ridge, 0, "bounded"))
    mvi = _batch(monkeypatch, c.name, c.B)
    lo, hi = mvi.tension_bounds("dynamics_inverse")
    got = mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], 0.0, bounds=(lo, hi))
    assert (got.status == br.SINGULAR).all() and (got.rank == 16).all() and (got.solves == 1).all()
    assert not got.U.any() and not got.lam.any() and not got.rho.any() and not got.active.any() and np.abs(got.tau).min() > 0.0
    # with the ridge the same states have answers; one state that is not a number among them
    t = br.continuous_table(br.CONTINUOUS[1])
    q = t.inputs
    good = _ct(mvi, t)
    assert (good.status == br.OK).all()
    Q = q["Q"].copy()
    Q[1, 2, :] = np.nan
    bad = mvi.dynamics_inverse(Q, q["dQ"], q["ddQ"], t.case.ridge, bounds=(t.lo, t.hi))
    hit = np.zeros(bad.status.shape, dtype=bool)
    hit[1, 2] = True
    assert (bad.status[hit] == br.SINGULAR).all() and (bad.status[~hit] == br.OK).all()
    for f in ("U", "lam", "rho", "rank", "active"):
        assert not getattr(bad, f)[hit].any(), f
    for f in bad._fields:
        if f not in ("tau", "acc"):
            assert np.array_equal(getattr(bad, f)[~hit], getattr(good, f)[~hit]), f


def test_refusals(monkeypatch):
    c = [c for c in br.CONTINUOUS if c.expect == "refused"][0]
    p = cref.case_states(cref.Case(c.name, c.B, c.M, 0.0, 0, "bounded"))
    mvi = _batch(monkeypatch, c.name, c.B)
    n = mvi.nu + mvi.nc
    with pytest.raises(ValueError, match="not strictly convex without a ridge"):
        mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], 0.0, bounds=(-1.0, 1.0))
    path = np.repeat(p["Q"][:, :1], 3, axis=1)
    with pytest.raises(ValueError, match="not strictly convex without a ridge"):
        mvi.inverse_dynamics(path, 0.01, None, 0.0, bounds=(-1.0, 1.0))
    ridge = 1e-4
    assert (mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], ridge, bounds=(-1.0, 1.0)).status == br.OK).all()
    nan = np.zeros(n)
    nan[1] = np.nan
    for bounds, message in (((nan, 1.0), "a bound is not a number"), ((-1.0, nan), "a bound is not a number"),
                            ((1.0, -1.0), "a lower bound above its upper bound"), ((np.inf, np.inf), "a bound that no finite value meets"),
                            ((-np.inf, -np.inf), "a bound that no finite value meets")):
        with pytest.raises(ValueError, match=message):
            mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], ridge, bounds=bounds)
        with pytest.raises(ValueError, match=message):
            mvi.inverse_dynamics(path, 0.01, None, ridge, bounds=bounds)
    with pytest.raises(ValueError, match="expected bounds of shape"):
        mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], ridge, bounds=(np.zeros(n + 1), 1.0))
    with pytest.raises(ValueError, match="rcond must be finite, not negative and below 1"):
        mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], ridge, rcond=1.0, bounds=(-1.0, 1.0))
    L = _lib.lib()
    z = np.zeros(2 * n)
    Q = mvi.device_array(p["Q"])
    args = lambda rows, lo, hi: (mvi._h, c.M, Q, mvi.nq, Q, mvi.nq, Q, mvi.nq, ridge, 1e-9, lo, hi, rows) + (None,) * 9
    assert L.tg_batch_dynamics_inverse_bounded_device(*args(2, Q, Q)) == ERR_INVALID and L.tg_last_error() == b"bound_rows must be 1 or the batch size"
    assert L.tg_batch_dynamics_inverse_bounded_device(*args(1, None, Q)) == ERR_INVALID and L.tg_last_error() == b"null lo or hi"
    assert L.tg_batch_dynamics_inverse_bounded(mvi._h, c.M, p["Q"].ctypes.data, p["Q"].ctypes.data, p["Q"].ctypes.data, ridge, 1e-9, z.ctypes.data, None, 1,
                                               *(None,) * 9) == ERR_INVALID and L.tg_last_error() == b"null lo or hi"
    assert mvi.kernel_info()["generic_launches"] == 1


# ---- 5. the solver alone: teams that need different numbers of solves in one wavefront -------------------------------------------------------
def _hook(mvi, team, A, c, lo, hi, max_solves=0):
    count, rows, cols = A.shape
    A, c, lo, hi = (np.ascontiguousarray(a, dtype=float) for a in (A, c, lo, hi))
    z = np.full((count, cols), np.nan)
    active = np.full((count, cols), -9, dtype=np.int32)
    solves, rank, status = (np.full(count, -1, dtype=np.int32) for _ in range(3))
    _lib.check(_lib.lib().tg_batch_debug_bvls_solve(mvi._h, team, count, rows, cols, A.ctypes.data, c.ctypes.data, lo.ctypes.data, hi.ctypes.data,
                                                    br.RCOND, max_solves, z.ctypes.data, active.ctypes.data, solves.ctypes.data, rank.ctypes.data,
                                                    status.ctypes.data))
    return z, active, solves, rank, status


@pytest.fixture(scope="module")
def hook_batch():
    mvi = BatchMidpointVI(common.build("pendulum1")[0], 1, specialize=False)
    yield mvi
    mvi.close()


def _sixty_five(rows, cols):
    """65 crafted problems of one shape, kinds cycling so that neighbours in a wavefront need different numbers of solves."""
    probs = [br.crafted(rows, cols, br.KINDS[i % len(br.KINDS)], i // len(br.KINDS)) for i in range(65)]
    if (rows, cols) == (4, 3):
        probs[7] = br.refree_problem()
    return tuple(np.array([p[k] for p in probs]) for k in range(4))


SHAPES = [s for s in mr.SHAPES if s[0] >= s[1]] + [(4, 3)]


@pytest.mark.parametrize("rows,cols", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_solver_on_crafted_problems_at_every_team_size(hook_batch, rows, cols):
    A, c, lo, hi = _sixty_five(rows, cols)
    refs = [br.solve_box(A[p], -c[p], 0.0, lo[p], hi[p]) for p in range(65)]
    certs = [br.certificate(A[p], -c[p], 0.0, lo[p], hi[p], refs[p].z, refs[p].active) for p in range(65)]
    first = None
    for team in (1, 4, 16, 64):
        z, active, solves, rank, status = _hook(hook_batch, team, A, c, lo, hi)
        assert (status == br.OK).all(), (team, status)
        worst = 0.0
        for p in range(65):
            scale = max(1.0, float(np.abs(refs[p].z).max()))
            bd = max(br.TOL, br.MARGIN * float(np.abs(refs[p].z - refs[p].z_aug).max()) / scale)
            err = float(np.abs(z[p] - refs[p].z).max()) / scale
            worst = max(worst, err / bd)
            assert err <= bd, (team, p, err, bd)
            assert np.all(z[p] >= lo[p]) and np.all(z[p] <= hi[p])
            if certs[p]["margin_z"] >= br.MARGIN_Z and certs[p]["margin_g"] >= br.MARGIN_G:
                assert np.array_equal(active[p], refs[p].active), (team, p)
        assert np.array_equal(rank, (lo < hi).sum(-1))
        assert solves.min() == 1 and (cols == 1 or len(np.unique(solves)) >= 3) and solves.max() <= 3 * cols + 3
        assert (np.diff(solves) != 0).sum() >= (0 if cols == 1 else 20)      # neighbours finish at different times
        print("%dx%d team %d: worst share of the bound %.3e, solves %s" % (rows, cols, team, worst, np.bincount(solves).tolist()))
        if first is None:
            first = (z, active, solves)
        else:
            assert np.array_equal(z, first[0]) and np.array_equal(active, first[1]) and np.array_equal(solves, first[2]), team
    if (rows, cols) == (4, 3):
        assert first[2][7] - 1 > int((first[1][7] != 0).sum())      # bound, then freed again


def test_solver_hook_status_rows_beside_untouched_neighbours(hook_batch):
    """TG_NOT_CONVERGED through a cap below a problem's need (the honest way to reach it), TG_SINGULAR for a rank-deficient first solve
    (with its rank) and for entries that are not finite (rank 0), each among problems that keep their bits."""
    A, c, lo, hi = _sixty_five(6, 5)
    for team in (4, 64):
        z, active, solves, rank, status = _hook(hook_batch, team, A, c, lo, hi)
        cap = int(np.sort(np.unique(solves))[1])       # the second smallest need: some problems finish, the others are cut
        zc, ac, sc, rc, stc = _hook(hook_batch, team, A, c, lo, hi, max_solves=cap)
        cut = solves > cap
        assert cut.any() and (~cut).any()
        assert (stc[cut] == br.NOT_CONVERGED).all() and (sc[cut] == cap).all() and (stc[~cut] == br.OK).all()
        assert np.all(zc >= lo) and np.all(zc <= hi)
        assert np.array_equal(zc[~cut], z[~cut]) and np.array_equal(ac[~cut], active[~cut]) and np.array_equal(sc[~cut], solves[~cut])
        A2, c2 = A.copy(), c.copy()
        A2[10, :, 4] = A2[10, :, 0] - A2[10, :, 1]      # rank 4 of 5
        A2[20, 3, 2] = np.nan
        c2[30, 1] = np.inf
        lo2, hi2 = lo.copy(), hi.copy()
        lo2[40, 1] = hi2[40, 1] = 0.5
        A2[40, 0, 1] = np.nan                           # in a column that starts bound
        zs, as_, ss, rs, sts = _hook(hook_batch, team, A2, c2, lo2, hi2)
        hit = np.zeros(65, dtype=bool)
        hit[[10, 20, 30, 40]] = True
        assert (sts[hit] == br.SINGULAR).all() and (sts[~hit] == br.OK).all()
        assert rs[10] == 4 and not rs[[20, 30, 40]].any() and not zs[hit].any() and not as_[hit].any()
        assert np.array_equal(zs[~hit], z[~hit]) and np.array_equal(as_[~hit], active[~hit]) and np.array_equal(ss[~hit], solves[~hit])
