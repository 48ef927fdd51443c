"""Rank-revealing least squares on the device (BatchMidpointVI.dynamics_inverse / inverse_dynamics with rcond=, the LSQ
instantiations of k_dyn_inverse / k_inverse, csrc/lsq_solve.hpp): both tables of min_norm_reference.py at the system's own team size
and at every team size of common.TEAM_CELLS against the numpy specification with the bounds of the CPU tests (z and rho
max(1e-10, 64 e_ref) relative to max(1, |z|inf), the direct quantities 1e-10, the ranks equal); equal bits through the host and the
device entry points and for a state repeated in a launch or alone in it; the parameter twin; the refusals; and the solver alone
(tg_batch_debug_lsq_solve) on crafted problems at teams 1, 4, 16 and 64, 65 problems of interleaved rank per launch -- the smallest
setting in which control flow around a TG_SYNC that differed between the teams of a wavefront would show."""
import numpy as np
import pytest

import common
import dynamics_inverse_reference as dr
import inverse_dynamics_reference as ir
import min_norm_reference as mr
from trep_amd import BatchMidpointVI, _lib

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -3
DYN_INVERSE_BIT, INVERSE_BIT = 14, 11


def _teams(name):
    return sorted(common.TEAM_CELLS[name]) if name in common.TEAM_CELLS else [None]


CT_RUNS = [(c, t) for c in mr.CT_CASES for t in _teams(c.name)]
ID_RUNS = [(c, t) for c in mr.ID_CASES for t in (_teams(c.base.name) if c.base.pattern == "uniform" else [None])]
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


def _ct(mvi, case):
    p = dr.case_states(mr.ct_base(case))
    return mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], case.ridge, rcond=mr.RCOND)


def _dt(c):
    return ir.step_sizes(c) if c.pattern != "uniform" else ir.DT


# ---- 1. both tables on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,team", CT_RUNS, ids=["%s_%s" % (mr.ct_id(c), _tid(t)) for c, t in CT_RUNS])
def test_computed_torque_table(monkeypatch, case, team):
    base = mr.ct_base(case)
    mvi = _batch(monkeypatch, case.name, base.B, team)
    if not _fits(mvi, _lib.lib().tg_system_dynamics_inverse_lsq_lds):
        with pytest.raises(_lib.LibraryError, match="system too large for the LDS-resident computed-torque kernel"):
            _ct(mvi, case)
        return
    got = _ct(mvi, case)
    assert got._fields[-1] == "rank" and got.rank.shape == (base.B, base.M) and got.rank.dtype == np.int32
    mr.compare_ct(case, got, tag="%s " % _tid(team))
    info = mvi.kernel_info()
    assert info["generic_launch_mask"] == 1 << DYN_INVERSE_BIT and info["spec_launch_mask"] == 0 and info["generic_launches"] == 1


@pytest.mark.parametrize("case,team", ID_RUNS, ids=["%s_%s" % (mr.id_id(c), _tid(t)) for c, t in ID_RUNS])
def test_discrete_table(monkeypatch, case, team):
    p = ir.case_paths(case.base)
    mvi = _batch(monkeypatch, case.base.name, case.base.B, team)
    if not _fits(mvi, _lib.lib().tg_system_inverse_dynamics_lsq_lds):
        with pytest.raises(_lib.LibraryError, match="system too large for the LDS-resident inverse-dynamics kernel"):
            mvi.inverse_dynamics(p["Q"], _dt(case.base), p["p0"], case.ridge, rcond=mr.RCOND)
        return
    for with_p0 in (True, False):
        got = mvi.inverse_dynamics(p["Q"], _dt(case.base), p["p0"] if with_p0 else None, case.ridge, rcond=mr.RCOND)
        assert got._fields[-1] == "rank"
        mr.compare_id(case, with_p0, got, tag="%s " % _tid(team))
        if not with_p0:
            for q in ("U", "lam", "rho", "rank"):
                assert not getattr(got, q)[:, 0].any(), q
    assert mvi.kernel_info()["generic_launch_mask"] == 1 << INVERSE_BIT and getattr(mvi, "_step_sizes", None) is None


def test_rcond_none_is_the_existing_path(monkeypatch):
    """rcond=None: today's namedtuple and today's refusal of n > nd without a ridge; a float accepts it."""
    case = dr.case_by_name("mixed_loop")
    p = dr.case_states(case)
    mvi = _batch(monkeypatch, case.name, case.B)
    old = mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], case.ridge)
    assert old._fields == ("U", "lam", "rho", "tau", "acc", "status")
    with pytest.raises(ValueError, match="more unknowns"):
        mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], 0.0)
    new = mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], 0.0, rcond=mr.RCOND)
    assert (new.rank == 5).all() and (new.status == mr.OK).all()
    assert np.array_equal(new.tau, old.tau) and np.array_equal(new.acc, old.acc)          # the evaluation is the same code


# ---- 2. equal bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("puppet_forces", "mixed_loop"))
def test_a_state_does_not_depend_on_its_launch(monkeypatch, name):
    case = [c for c in mr.CT_CASES if c.name == name and not c.ridge][0]
    base = mr.ct_base(case)
    p = dr.case_states(base)
    Q, dQ, ddQ = p["Q"], p["dQ"], p["ddQ"]
    whole = _ct(_batch(monkeypatch, name, base.B), case)
    pick = np.array([2, 0, 2, 1, 2, 2, 0])
    again = _batch(monkeypatch, name, len(pick)).dynamics_inverse(Q[pick], dQ[pick], ddQ[pick], case.ridge, rcond=mr.RCOND)
    for q in whole._fields:
        assert np.array_equal(getattr(again, q), getattr(whole, q)[pick]), q
    b, s = 2, 3
    one = _batch(monkeypatch, name, 1).dynamics_inverse(Q[b:b + 1, s:s + 1], dQ[b:b + 1, s:s + 1], ddQ[b:b + 1, s:s + 1], case.ridge, rcond=mr.RCOND)
    flat = _batch(monkeypatch, name, 1).dynamics_inverse(Q[b:b + 1, s], dQ[b:b + 1, s], ddQ[b:b + 1, s], case.ridge, rcond=mr.RCOND)
    for q in whole._fields:
        assert np.array_equal(getattr(one, q)[0, 0], getattr(whole, q)[b, s]), q
        assert np.array_equal(getattr(flat, q)[0], getattr(whole, q)[b, s]), q
    assert flat.rank.shape == (1,)


def test_a_step_does_not_depend_on_its_launch(monkeypatch):
    case = [c for c in mr.ID_CASES if c.base.name == "mixed_loop" and not c.ridge][0]
    p = ir.case_paths(case.base)
    Q, p0 = p["Q"], p["p0"]
    whole = _batch(monkeypatch, case.base.name, case.base.B).inverse_dynamics(Q, ir.DT, p0, 0.0, rcond=mr.RCOND)
    pick = np.array([3, 0, 3, 1, 3, 2, 4])
    again = _batch(monkeypatch, case.base.name, len(pick)).inverse_dynamics(Q[pick], ir.DT, p0[pick], 0.0, rcond=mr.RCOND)
    _same(again, type(whole)(*[getattr(whole, q)[pick] for q in whole._fields]))
    b, k = 3, 7
    one = _batch(monkeypatch, case.base.name, 1).inverse_dynamics(Q[b:b + 1, k:k + 2], ir.DT, whole.P[b:b + 1, k], 0.0, rcond=mr.RCOND)
    for q in ("U", "lam", "rho", "h", "status", "rank"):
        assert np.array_equal(getattr(one, q)[0, 0], getattr(whole, q)[b, k]), q


def _words(mvi, count):
    L = _lib.lib()
    w = L.tg_device_alloc(0, 4 * count)
    assert w
    return w


def _download_words(mvi, w, shape):
    out = np.zeros(shape, dtype=np.int32)
    _lib.check(_lib.lib().tg_memcpy_d2h(0, out.ctypes.data, w, 4 * out.size))
    return out


def test_host_and_device_computed_torque_give_the_same_bits(monkeypatch):
    case = mr.CT_CASES[1]                 # mixed_loop, n > nd, no ridge
    base = mr.ct_base(case)
    p = dr.case_states(base)
    host = _ct(_batch(monkeypatch, case.name, base.B), case)
    mvi = _batch(monkeypatch, case.name, base.B)
    L = _lib.lib()
    B, M, nd, nu, nc, nq = base.B, base.M, mvi.nd, mvi.nu, mvi.nc, mvi.nq
    widths = (mvi.nX, nq + 3, nq + 1)              # strided rows, each array with a stride of its own
    wide = []
    for a, w in zip((p["Q"], p["dQ"], p["ddQ"]), widths):
        x = np.full((B, M, w), np.nan)
        x[:, :, :nq] = a
        wide.append(mvi.device_array(x))
    size = {"U": nu, "lam": nc, "rho": nd, "tau": nd, "acc": nc}
    dev = {q: mvi.device_empty(B * M * n) for q, n in size.items()}
    status_dev, rank_dev = _words(mvi, B * M), _words(mvi, B * M)
    try:
        mvi.dynamics_inverse_device(M, wide[0], wide[1], wide[2], widths[0], widths[1], widths[2], case.ridge, dev["U"], dev["lam"], dev["rho"],
                                    dev["tau"], dev["acc"], status_dev, rcond=mr.RCOND, rank_dev=rank_dev)
        mvi.synchronize()
        for q, n in size.items():
            assert np.array_equal(mvi.download(dev[q], (B, M, n)), getattr(host, q)), q
        assert np.array_equal(_download_words(mvi, status_dev, (B, M)), host.status)
        assert np.array_equal(_download_words(mvi, rank_dev, (B, M)), host.rank)
        # null outputs, the rank among them: still a launch
        mvi.dynamics_inverse_device(M, wide[0], wide[1], wide[2], widths[0], widths[1], widths[2], case.ridge, rcond=mr.RCOND)
        mvi.synchronize()
        assert mvi.kernel_info()["generic_launches"] == 2
        with pytest.raises(ValueError, match="rank_dev needs rcond"):
            mvi.dynamics_inverse_device(M, wide[0], wide[1], wide[2], rank_dev=rank_dev)
    finally:
        L.tg_device_free(0, status_dev)
        L.tg_device_free(0, rank_dev)


def test_host_and_device_inverse_dynamics_give_the_same_bits(monkeypatch):
    case = [c for c in mr.ID_CASES if c.base.name == "mixed_loop" and not c.ridge][0]
    p = ir.case_paths(case.base)
    B, N = case.base.B, case.base.N
    host = _batch(monkeypatch, case.base.name, B).inverse_dynamics(p["Q"], ir.DT, p["p0"], 0.0, rcond=mr.RCOND)
    mvi = _batch(monkeypatch, case.base.name, B)
    L = _lib.lib()
    nd, nu, nc = mvi.nd, mvi.nu, mvi.nc
    U, lam, P, rho, h = (mvi.device_empty(B * N * nu), mvi.device_empty(B * N * nc), mvi.device_empty(B * (N + 1) * nd),
                         mvi.device_empty(B * N * nd), mvi.device_empty(B * N * nc))
    status_dev, rank_dev = _words(mvi, B * N), _words(mvi, B * N)
    try:
        mvi.inverse_dynamics_device(N, ir.DT, mvi.device_array(p["Q"]), None, mvi.device_array(p["p0"]), 0.0, U, lam, P, rho, h, status_dev,
                                    rcond=mr.RCOND, rank_dev=rank_dev)
        mvi.synchronize()
        got = type(host)(mvi.download(U, (B, N, nu)), mvi.download(lam, (B, N, nc)), mvi.download(P, (B, N + 1, nd)), mvi.download(rho, (B, N, nd)),
                         mvi.download(h, (B, N, nc)), _download_words(mvi, status_dev, (B, N)), _download_words(mvi, rank_dev, (B, N)))
        _same(host, got)
    finally:
        L.tg_device_free(0, status_dev)
        L.tg_device_free(0, rank_dev)


def test_parameter_twin_matches_rebuilt_systems(monkeypatch):
    case = dr.case_by_name("puppet40")
    p = dr.case_states(case)
    rows = ir.parameter_rows(case.name, case.B)
    mvi = _batch(monkeypatch, case.name, case.B)
    mvi.set_parameters(inertia=rows["inertia"], gravity=rows["gravity"], group=1)
    got = mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], 0.0, rcond=mr.RCOND)
    dr.compare(case, got, ref=dr.parameter_reference(case, rows), tag="parameter rows (lsq) ")
    assert (got.rank == 6).all()
    info = mvi.kernel_info()
    assert info["par_generic_launches"] == 1 and info["generic_launches"] == 0


# ---- 3. status and refusals --------------------------------------------------------------------------------------------------------------
def test_status_of_a_non_finite_state(monkeypatch):
    case = mr.CT_CASES[0]
    base = mr.ct_base(case)
    p = dr.case_states(base)
    mvi = _batch(monkeypatch, case.name, base.B)
    good = _ct(mvi, case)
    ddQ = p["ddQ"].copy()
    b, s = 1, 2
    ddQ[b, s, 1] = np.nan
    got = mvi.dynamics_inverse(p["Q"], p["dQ"], ddQ, case.ridge, rcond=mr.RCOND)
    hit = np.zeros(got.status.shape, dtype=bool)
    hit[b, s] = True
    assert (got.status[hit] == mr.SINGULAR).all() and (got.status[~hit] == mr.OK).all()
    for q in ("U", "lam", "rho", "rank"):
        assert not getattr(got, q)[hit].any(), q
    for q in got._fields:
        assert np.array_equal(getattr(got, q)[~hit], getattr(good, q)[~hit]), q


@pytest.mark.parametrize("name", ("scissor4", "puppet40", "puppet_forces"))
def test_status_of_a_state_that_is_not_a_number(monkeypatch, name):
    """A whole row of Q not a number (a diverged rollout read in place): TG_SINGULAR with U, lam, rho zero and rank 0, as the augmented
    kernel answers -- not TG_OK with rank 0 and a rho that is not a number.  The same for dQ and ddQ in the states beside it."""
    base = dr.case_by_name(name)
    p = dr.case_states(base)
    mvi = _batch(monkeypatch, name, base.B)
    good = mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], 0.0, rcond=mr.RCOND)
    Q, dQ, ddQ = p["Q"].copy(), p["dQ"].copy(), p["ddQ"].copy()
    Q[0, 0, :], dQ[1, 1, :], ddQ[2, 2, :] = np.nan, np.nan, np.nan
    got = mvi.dynamics_inverse(Q, dQ, ddQ, 0.0, rcond=mr.RCOND)
    hit = np.zeros(got.status.shape, dtype=bool)
    hit[0, 0] = hit[1, 1] = hit[2, 2] = True
    assert (got.status[hit] == mr.SINGULAR).all() and (got.status[~hit] == mr.OK).all(), got.status
    for q in ("U", "lam", "rho", "rank"):
        assert not getattr(got, q)[hit].any(), q
    for q in got._fields:
        assert np.array_equal(getattr(got, q)[~hit], getattr(good, q)[~hit]), q


def test_status_of_a_path_with_a_configuration_that_is_not_a_number(monkeypatch):
    case = [c for c in mr.ID_CASES if c.base.name == "puppet_forces" and not c.ridge][0]
    p = ir.case_paths(case.base)
    mvi = _batch(monkeypatch, case.base.name, case.base.B)
    good = mvi.inverse_dynamics(p["Q"], ir.DT, p["p0"], 0.0, rcond=mr.RCOND)
    Q = p["Q"].copy()
    k = 6
    Q[1, k, :] = np.nan
    got = mvi.inverse_dynamics(Q, ir.DT, p["p0"], 0.0, rcond=mr.RCOND)
    hit = np.zeros(got.status.shape, dtype=bool)
    hit[1, k - 1:k + 2] = True            # p_k, the pair itself, and the next step's p
    assert (got.status[hit] == mr.SINGULAR).all() and (got.status[~hit] == mr.OK).all(), got.status
    for q in ("U", "lam", "rho", "rank"):
        assert not getattr(got, q)[hit].any(), q
        assert np.array_equal(getattr(got, q)[~hit], getattr(good, q)[~hit]), q


@pytest.mark.parametrize("case", [c for c in mr.CT_CASES if c.ridge > 0], ids=[mr.ct_id(c) for c in mr.CT_CASES if c.ridge > 0])
def test_ridge_rows_agree_with_the_existing_kernel(monkeypatch, case):
    """With a ridge both kernels answer the same question: each is within the bound of its reference, the references within the bound
    of each other (test_min_norm_cpu.py), so the kernels within twice the bound; tau and acc are the same code: equal bits."""
    base = mr.ct_base(case)
    p = dr.case_states(base)
    mvi = _batch(monkeypatch, case.name, base.B)
    old = mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], base.ridge)
    new = _ct(mvi, case)
    ref_new, ref_old = mr.ct_reference(case), dr.case_reference(base)
    scale, bd = max(mr.floor(ref_new)[1], dr.floors(ref_old)["scale"]), max(mr.bound(ref_new), dr.bound(ref_old))
    e_z = float(np.abs(dr.unknowns(new.U, new.lam) - dr.unknowns(old.U, old.lam)).max()) / scale
    e_rho = float(np.abs(new.rho - old.rho).max()) / scale
    print(mr.ct_id(case), "kernels: z %.3e rho %.3e bound %.3e" % (e_z, e_rho, 2 * bd))
    assert e_z <= 2 * bd and e_rho <= 2 * bd
    assert np.array_equal(new.tau, old.tau) and np.array_equal(new.acc, old.acc) and np.array_equal(new.status, old.status)


def test_refusals(monkeypatch):
    case = dr.case_by_name("mixed_loop")
    p = dr.case_states(case)
    mvi = _batch(monkeypatch, case.name, case.B)
    for rcond in (-1e-12, 1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="rcond must be finite, not negative and below 1"):
            mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], 0.0, rcond=rcond)
        q = ir.case_paths(ir.CASES[8])
        with pytest.raises(ValueError, match="rcond must be finite, not negative and below 1"):
            mvi.inverse_dynamics(q["Q"], ir.DT, None, 0.0, rcond=rcond)
    with pytest.raises(ValueError, match="ridge must be finite and not negative"):
        mvi.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], -1.0, rcond=mr.RCOND)
    L = _lib.lib()
    Q = mvi.device_array(p["Q"])
    rc = L.tg_batch_dynamics_inverse_lsq_device(mvi._h, case.M, Q, mvi.nq - 1, Q, mvi.nq, Q, mvi.nq, 0.0, 1e-9, None, None, None, None, None, None, None)
    assert rc == ERR_INVALID and L.tg_last_error() == b"row stride of Q shorter than a configuration"
    assert mvi.kernel_info()["generic_launches"] == 0


# ---- 4. the solver alone: teams of different rank in one wavefront ----------------------------------------------------------------------
def _hook(mvi, team, A, c, rcond):
    count, rows, cols = A.shape
    z = np.full((count, cols), np.nan)
    rank, status = np.full(count, -1, dtype=np.int32), np.full(count, -1, dtype=np.int32)
    _lib.check(_lib.lib().tg_batch_debug_lsq_solve(mvi._h, team, count, rows, cols, A.ctypes.data, c.ctypes.data, rcond, z.ctypes.data,
                                                   rank.ctypes.data, status.ctypes.data))
    return z, rank, status


@pytest.fixture(scope="module")
def hook_batch():
    mvi = BatchMidpointVI(common.build("pendulum1")[0], 1, specialize=False)
    yield mvi
    mvi.close()


@pytest.mark.parametrize("rows,cols", mr.SHAPES, ids=["%dx%d" % s for s in mr.SHAPES])
def test_solver_on_crafted_problems_at_every_team_size(hook_batch, rows, cols):
    """65 problems per launch (one full block of teams plus a ragged one at TEAM = 1; 17 blocks at TEAM = 16), ranks 0, 1, min - 1 and
    full interleaved, zero matrices beside full-rank ones: rank and z against the SVD, per problem within max(1e-10, 64 e_ref)
    relative to max(1, |z|inf); a zero matrix is rank 0 with TG_OK; and the same bits at every team size (the order of every sum is
    the same)."""
    A, c, kinds = mr.crafted(rows, cols)
    assert len(A) == 65
    z_ref, rank_ref, above, below = mr.crafted_reference(A, c)
    bounds = []
    for p in range(len(A)):
        a = mr.solve(A[p], -c[p], 0.0, mr.CRAFT_RCOND)
        scale = max(1.0, float(np.abs(a.z).max()))
        bounds.append((scale, max(mr.TOL, mr.MARGIN * float(np.abs(a.z - a.z2).max()) / scale)))
    first = None
    for team in (1, 4, 16, 64):
        z, rank, status = _hook(hook_batch, team, A, c, mr.CRAFT_RCOND)
        assert (status == mr.OK).all(), (team, status)
        assert np.array_equal(rank, rank_ref), (team, [(k, int(a), int(b)) for k, a, b in zip(kinds, rank, rank_ref) if a != b])
        worst = 0.0
        for p, (scale, bd) in enumerate(bounds):
            err = float(np.abs(z[p] - z_ref[p]).max()) / scale
            worst = max(worst, err / bd)
            assert err <= bd, (team, p, kinds[p], err, bd)
        print("%dx%d team %d: worst share of the bound %.3e" % (rows, cols, team, worst))
        zero = np.array(kinds) == "zero"
        assert not z[zero].any() and not rank[zero].any()
        if first is None:
            first = (z, rank)
        else:
            assert np.array_equal(z, first[0]) and np.array_equal(rank, first[1]), team


def test_solver_hook_reports_a_non_finite_answer_beside_good_ones(hook_batch):
    A, c, _ = mr.crafted(6, 5, count=9)
    good = _hook(hook_batch, 4, A, c, mr.CRAFT_RCOND)
    c2 = c.copy()
    c2[4, 2] = np.nan
    z, rank, status = _hook(hook_batch, 4, A, c2, mr.CRAFT_RCOND)
    hit = np.arange(9) == 4
    assert status[4] == mr.SINGULAR and (status[~hit] == mr.OK).all() and not z[4].any() and rank[4] == 0
    assert np.array_equal(z[~hit], good[0][~hit]) and np.array_equal(rank[~hit], good[1][~hit])


NOT_FINITE = {
    "all_nan": lambda A, c: A.fill(np.nan),
    "nan_and_zero_columns": lambda A, c: (A.fill(0.0), A[:, 0].fill(np.nan)),
    "one_nan_entry": lambda A, c: A.__setitem__((-1, -1), np.nan),
    "one_inf_entry": lambda A, c: A.__setitem__((0, 0), np.inf),
    "nan_in_c": lambda A, c: c.__setitem__(-1, np.nan),
    "nan_in_c_zero_matrix": lambda A, c: (A.fill(0.0), c.__setitem__(0, np.nan)),
}


@pytest.mark.parametrize("rows,cols", ((3, 2), (2, 3), (6, 5)), ids=("3x2", "2x3", "6x5"))
def test_solver_hook_tells_not_finite_from_rank_zero(hook_batch, rows, cols):
    """Every kind of entry that is not finite, each beside a zero matrix (rank 0, TG_OK) and good problems in the same wavefront:
    TG_SINGULAR with z = 0 and rank 0 there, the neighbours' bits untouched, at every team size."""
    kinds = sorted(NOT_FINITE)
    A, c, _ = mr.crafted(rows, cols, count=3 * len(kinds))
    spoiled = np.zeros(len(A), dtype=bool)
    A2, c2 = A.copy(), c.copy()
    for i, kind in enumerate(kinds):
        NOT_FINITE[kind](A2[3 * i + 1], c2[3 * i + 1])
        spoiled[3 * i + 1] = True
    for team in (1, 4, 16, 64):
        good = _hook(hook_batch, team, A, c, mr.CRAFT_RCOND)
        z, rank, status = _hook(hook_batch, team, A2, c2, mr.CRAFT_RCOND)
        assert (status[spoiled] == mr.SINGULAR).all() and (status[~spoiled] == mr.OK).all(), (team, status)
        assert not z[spoiled].any() and not rank[spoiled].any()
        assert np.array_equal(z[~spoiled], good[0][~spoiled]) and np.array_equal(rank[~spoiled], good[1][~spoiled])
