"""Batched equilibrium search on the device (BatchMidpointVI.minimize_potential_energy, k_equilibrium): the case table of
equilibrium_reference.py at every system's own team size, in one full block of teams plus a ragged one, and at every team size on
the smallest system that reaches it, against the numpy reference with the bounds of the CPU tests (test_equilibrium_cpu.py) -- end
points within 64 max(floor, 1e-13), V within the energy parity figure, trial counts and status equal on the rows whose decisions
are firm -- bit-equality, the parameter-table twin against references on rebuilt systems, the recorded equilibrium of the
reference's SLSQP run, the status cases, the untouched batch state and the device-pointer variant."""

import numpy as np
import pytest

import common
import equilibrium_reference as er
from test_equilibrium_cpu import check_parameter_rows, parameter_inputs, parameter_reference, parameter_rows, PAR_SYSTEMS
from trep_amd import BatchMidpointVI, _lib

pytestmark = pytest.mark.gpu

CASE_IDS = [er.case_id(c) for c in er.CASES]
EQUILIBRIUM_BIT = 10
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
# (team, the smallest system of the table whose workgroup fits 160 KiB of LDS at that team size, its mask)
TEAMS = [(1, "dual_pendulums", "all"), (4, "plane_link", "all"), (4, "spring_link", "keep_kinematic"), (16, "plane_link", "all"),
         (16, "scissor4", "constant"), (64, "plane_link", "all"), (64, "puppet_basic", "all")]


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
    return dict(keep_kinematic=mask == "keep_kinematic", constant_q_list=er.CONSTANT[name] if mask == "constant" else None)


def _same(a, b, rows=slice(None)):
    for k in ("Q", "mu", "V", "iterations", "status"):
        assert np.array_equal(getattr(a, k)[rows], getattr(b, k)), k


def _check_rows(case, got, pick):
    """The comparison of er.compare on the table's rows `pick` (any number of them, in any order)."""
    ref = er.case_reference(*case)
    Q0, free = er.case_inputs(*case)
    err = float(np.abs(got.Q - ref.Q[pick]).max())
    mu_err = float(np.abs(got.mu - ref.mu[pick]).max(initial=0.0))
    v_err = float((np.abs(got.V - ref.V[pick]) / np.maximum(1.0, np.abs(ref.V[pick]))).max())
    print(er.case_id(case), "error %.3e mu %.3e bound %.3e V %.3e trials %s reference %s" % (
        err, mu_err, er.case_bound(*case), v_err, got.iterations, ref.iterations[pick]))
    assert np.array_equal(got.status, ref.status[pick]) and (got.status == er.OK).all()
    assert err <= er.case_bound(*case) and mu_err <= er.case_bound(*case) and v_err <= er.V_PARITY
    firm = er.firm_rows(ref)[pick]
    assert np.array_equal(got.iterations[firm], ref.iterations[pick][firm])
    assert np.array_equal(got.Q[:, ~free], Q0[pick][:, ~free])


# ---- 1. the table on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", er.CASES, ids=CASE_IDS)
def test_the_table_at_the_systems_own_team(monkeypatch, case):
    name, mask, _ = case
    Q0, free = er.case_inputs(*case)
    mvi = _batch(monkeypatch, name, len(Q0))
    assert np.array_equal(mvi.free_mask(**_kw(name, mask)) != 0, free)
    got = mvi.minimize_potential_energy(Q0, tolerance=er.TOL, **_kw(name, mask))
    er.compare(case, got)                             # the same checks as the emulation: bounds, firm rows, rest row, repeat, fixed
    assert er.certified(name, got, free).all()
    info = mvi.kernel_info()
    assert info["generic_launch_mask"] == 1 << EQUILIBRIUM_BIT and info["spec_launch_mask"] == 0 and info["generic_launches"] == 1
    assert info["par_generic_launches"] == 0
    # one full block of teams plus a ragged one
    per_block = 64 // info["team"]
    pick = np.arange(per_block + min(3, max(per_block - 1, 1))) % len(Q0)
    ragged = _batch(monkeypatch, name, len(pick)).minimize_potential_energy(Q0[pick], tolerance=er.TOL, **_kw(name, mask))
    _check_rows(case, ragged, pick)
    _same(got, ragged, pick)                          # a pose does not see its neighbours


@pytest.mark.parametrize("team,name,mask", TEAMS)
def test_every_team_size(monkeypatch, team, name, mask):
    case = (name, mask, 0.1)
    Q0, free = er.case_inputs(*case)
    per_block = 64 // team
    pick = np.arange(per_block + (3 if per_block > 1 else 4)) % len(Q0)
    got = _batch(monkeypatch, name, len(pick), team).minimize_potential_energy(Q0[pick], tolerance=er.TOL, **_kw(name, mask))
    _check_rows(case, got, pick)
    own = _batch(monkeypatch, name, len(Q0)).minimize_potential_energy(Q0, tolerance=er.TOL, **_kw(name, mask))
    assert np.array_equal(got.status, own.status[pick]) and np.abs(got.Q - own.Q[pick]).max() <= er.case_bound(*case)


def test_equal_poses_give_equal_bits_and_a_second_call_too(monkeypatch):
    case = ("puppet40", "keep_kinematic", 0.02)
    Q0, free = er.case_inputs(*case)
    mvi = _batch(monkeypatch, case[0], len(Q0))
    got = mvi.minimize_potential_energy(Q0, keep_kinematic=True)
    assert np.array_equal(Q0[er.REPEAT], Q0[0])
    for k in got._fields:
        assert np.array_equal(getattr(got, k)[er.REPEAT], getattr(got, k)[0]), k
    _same(got, mvi.minimize_potential_energy(Q0, keep_kinematic=True))
    assert np.array_equal(got.Q[:, ~free], Q0[:, ~free]) and not np.array_equal(got.Q[:, free], Q0[:, free])


# ---- 2. the parameter table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PAR_SYSTEMS))
def test_parameter_rows_match_rebuilt_systems(monkeypatch, name):
    Q0, free, case = parameter_inputs(name)
    rows = parameter_rows(name)
    mvi = _batch(monkeypatch, name, len(Q0))
    plain = mvi.minimize_potential_energy(Q0, **_kw(name, PAR_SYSTEMS[name]))
    mvi.set_parameters(inertia=rows["inertia"], gravity=rows["gravity"], group=3)
    got = mvi.minimize_potential_energy(Q0, **_kw(name, PAR_SYSTEMS[name]))
    check_parameter_rows(name, got, parameter_reference(name, Q0, free, rows, 3), case)
    for k in ("Q", "mu", "V", "iterations", "status"):           # row 0 holds the system's own values
        assert np.array_equal(getattr(got, k)[:3], getattr(plain, k)[:3]), k
    info = mvi.kernel_info()
    assert info["par_generic_launch_mask"] == 1 << EQUILIBRIUM_BIT and info["par_generic_launches"] == 1 and info["par_spec_launches"] == 0
    assert info["generic_launch_mask"] == 1 << EQUILIBRIUM_BIT and info["generic_launches"] == 1
    mvi.clear_parameters()
    _same(plain, mvi.minimize_potential_energy(Q0, **_kw(name, PAR_SYSTEMS[name])))


# ---- 3. the recorded equilibrium of the reference's own routine -----------------------------------------------------------------
def test_golden_equilibrium_comes_back(monkeypatch):
    """minpot_q of tests/golden/dsystem_extras.npz: the reference's SLSQP equilibrium of spring_link under keep_kinematic, with the
    tolerances of test_minimize_potential_energy_matches_reference."""
    g = common.golden("dsystem_extras")
    name, B = "spring_link", 9
    free = er.free_mask(name, "keep_kinematic")
    rng = np.random.default_rng(common.tb_seed("equilibrium golden", name))
    Q = np.tile(g["minpot_q"], (B, 1))
    Q[1:, free] += 0.02 * rng.standard_normal((B - 1, int(free.sum())))
    Q[-1] = g["minpot_q0"]                             # and the SLSQP run's own start
    got = _batch(monkeypatch, name, B).minimize_potential_energy(Q, keep_kinematic=True)
    print(got.iterations, got.status, got.V[:, 1] - g["minpot_V"][0])
    assert (got.status == er.OK).all()
    for b in range(B):
        assert abs(got.V[b, 1] - g["minpot_V"][0]) < 1e-7
        assert np.allclose(np.cos(got.Q[b] - g["minpot_q"]), 1.0, atol=1e-8) or common.relerr(got.Q[b], g["minpot_q"]) < 1e-4
    assert got.V[-1, 1] <= got.V[-1, 0]                # (the perturbed starts violate the constraint: their V may rise)


# ---- 4. status, and the state of the batch ----------------------------------------------------------------------------------------
def test_statuses_arrive_per_pose(monkeypatch):
    case = ("puppet_basic", "all", 0.1)
    name = case[0]
    Q0, free = er.case_inputs(*case)
    ref = er.case_reference(*case)
    slow = int(np.argmax(ref.iterations))
    rows = np.array([Q0[er.EQUILIBRIUM], Q0[slow], Q0[er.EQUILIBRIUM], Q0[0]])
    got = _batch(monkeypatch, name, 4).minimize_potential_energy(rows, max_iterations=2)
    want = er.minimize(name, rows, free, max_iterations=2)
    assert list(got.status) == [er.OK, er.NOT_CONVERGED, er.OK, er.NOT_CONVERGED] and list(got.iterations) == [0, 2, 0, 2]
    assert np.array_equal(got.status, want.status) and np.abs(got.Q - want.Q).max() <= er.MARGIN * 1e-13
    assert np.array_equal(got.Q[0], rows[0]) and np.array_equal(got.Q[2], rows[2])
    full = _batch(monkeypatch, name, 4).minimize_potential_energy(rows)
    assert (full.status == er.OK).all() and list(full.iterations) == [0, ref.iterations[slow], 0, ref.iterations[0]]
    # nothing free: TG_OK only where the input passes the test already (h alone: g is empty)
    case = ("plane_link", "all", 0.02)
    P0 = er.case_inputs(*case)[0]
    rows = np.array([er.case_reference(*case, 1e-13).Q[0], P0[0]])
    held = _batch(monkeypatch, case[0], 2).minimize_potential_energy(rows, constant_q_list=[c.name for c in common.build(case[0])[0].configs])
    assert list(held.status) == [er.OK, er.SINGULAR] and not held.iterations.any() and np.array_equal(held.Q, rows)


def test_refusals_make_no_launch(monkeypatch):
    L = _lib.lib()
    mvi = _batch(monkeypatch, "scissor4", 2)
    q = np.zeros((2, mvi.nq))
    p = q.ctypes.data
    for tol, its in ((0.0, 100), (1e-10, -1)):
        assert L.tg_batch_minimize_potential(mvi._h, p, None, tol, its, p, None, None, None, None) == ERR_INVALID
    assert L.tg_batch_minimize_potential(mvi._h, None, None, 1e-10, 100, p, None, None, None, None) == ERR_INVALID
    assert mvi.kernel_info()["generic_launches"] == 0
    arm = _batch(monkeypatch, "nonlinear_spring_arm", 2)
    with pytest.raises(_lib.LibraryError):
        arm.minimize_potential_energy(np.zeros((2, arm.nq)))
    assert arm.kernel_info()["generic_launches"] == 0


def test_the_batch_state_is_unchanged(monkeypatch):
    name = "puppet_basic"
    case = (name, "all", 0.02)
    Q0, free = er.case_inputs(*case)
    B, N, DT = len(Q0), 6, 0.01
    system, d = common.build(name)
    rng = np.random.default_rng(common.tb_seed("equilibrium state", name))
    S0, S1, U, K = common.starts(name, d, B, N, rng)
    plain = _batch(monkeypatch, name, B).minimize_potential_energy(Q0)

    def fresh():
        mvi = _batch(monkeypatch, name, B, specialize="auto")
        mvi.initialize_from_configs(0.0, S0, DT, S1)
        return mvi

    X_ref = fresh().rollout(N, DT, U, K)
    mvi = fresh()
    state = lambda: [getattr(mvi, n).copy() for n in ("q1", "q2", "p1", "p2", "lambda1")] + list(mvi.status()) + [mvi.times()]
    before = state()
    _same(plain, mvi.minimize_potential_energy(Q0))             # a specialised library, if one is loaded, has no say
    info = mvi.kernel_info()
    assert (info["generic_launch_mask"] >> EQUILIBRIUM_BIT) & 1 and not (info["spec_launch_mask"] >> EQUILIBRIUM_BIT) & 1
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)
    assert np.array_equal(mvi.rollout(N, DT, U, K), X_ref)
    assert (mvi.status()[1] == 0).all()


# ---- 5. device pointers on a caller's stream ---------------------------------------------------------------------------------------
def test_device_variant_leaves_results_on_the_device(monkeypatch):
    L = _lib.lib()
    case = ("scissor4", "constant", 0.02)
    name, mask, _ = case
    Q0, free = er.case_inputs(*case)
    B = len(Q0)
    host = _batch(monkeypatch, name, B).minimize_potential_energy(Q0, **_kw(name, mask))
    mvi = _batch(monkeypatch, name, B)
    stream = L.tg_dopt_lane_stream(0, 1)
    assert stream
    mvi.set_stream(stream)
    nq, nc = mvi.nq, mvi.nc
    q_dev = mvi.device_array(Q0)
    mask_host = np.ascontiguousarray(free, dtype=np.int32)
    ints = L.tg_device_alloc(0, 4 * (nq + 2 * B))
    assert ints
    try:
        _lib.check(L.tg_memcpy_h2d(0, ints, mask_host.ctypes.data, 4 * nq))
        q_out, mu_out, v_out = mvi.device_empty(B * nq), mvi.device_empty(B * nc), mvi.device_empty(B * 2)
        _lib.check(L.tg_batch_minimize_potential_device(mvi._h, q_dev, ints, er.TOL, 100, q_out, mu_out, v_out, ints + 4 * nq,
                                                        ints + 4 * (nq + B)))
        mvi.synchronize()
        back = np.zeros(2 * B, dtype=np.int32)
        _lib.check(L.tg_memcpy_d2h(0, back.ctypes.data, ints + 4 * nq, 8 * B))
        got = er.Equilibrium(mvi.download(q_out, (B, nq)), mvi.download(mu_out, (B, nc)), mvi.download(v_out, (B, 2)), back[:B], back[B:], None)
        _same(host, got)
    finally:
        L.tg_device_free(0, ints)
        mvi.close()
