"""Batched equilibrium search without a device: the numpy reference (equilibrium_reference.py) on its case table with the certificate
of a minimum that does not depend on the iteration, the failures of the undamped iteration, the mutations the table must catch, and
the kernel itself (mvi_equilibrium.hpp) compiled for the host with TEAM = 1 (emu_pose_harness.py) against the reference --
end points within the per-case bound, V within the energy parity figure, trial counts and status equal on every row whose decisions
are firm -- with its parameter-table twin, the status cases, the refusals of the C entry points and the layout guards.

Per case, floor = max |q_ref(tolerance 1e-10) - q_ref(tolerance 1e-13)| and the bound on |q - q_ref| is 64 max(floor, 1e-13)
(tools/equilibrium_parity.py writes both, with the worst errors, to profiles/equilibrium_parity.json)."""
import ctypes
import json
import os

import numpy as np
import pytest

import common
import emu_pose_harness
import emu_harness
import equilibrium_reference as er
import projection_reference as pr
from test_parameters_cpu import rebuilt
from trep_amd import _lib, descriptor, parameters

CASE_IDS = [er.case_id(c) for c in er.CASES]
ERR_INVALID, ERR_UNSUPPORTED = -1, -3


def _emu(name):
    return emu_pose_harness.EmuEquilibrium(common.build(name)[1])


# ---- 1. the reference reaches certified minima on the table -------------------------------------------------------------------
@pytest.mark.parametrize("case", er.CASES, ids=CASE_IDS)
def test_reference_reaches_certified_minima(case):
    ref = er.case_reference(*case)
    Q0, free = er.case_inputs(*case)
    print(er.case_id(case), "trials", ref.iterations, "smallest margin %.3e" % ref.margin.min())
    assert (ref.status == er.OK).all(), ref.status
    assert er.certified(case[0], ref, free).all()
    assert ref.iterations[er.EQUILIBRIUM] == 0 and np.array_equal(ref.Q[er.EQUILIBRIUM], Q0[er.EQUILIBRIUM])
    assert ref.iterations[:er.EQUILIBRIUM].min() >= 1           # every other row of the table really is off its equilibrium
    assert (~er.firm_rows(ref)).sum() * 8 <= len(Q0)
    assert np.array_equal(ref.Q[:, ~free], Q0[:, ~free])


@pytest.mark.parametrize("case", er.CASES, ids=CASE_IDS)
def test_energy_does_not_rise_from_a_feasible_start(case):
    ref = er.case_reference(*case)
    Q0, free = er.case_inputs(*case)
    ev = er.potential_of(case[0])
    feasible = np.array([np.abs(ev.con(q)[0]).max(initial=0.0) <= er.TOL for q in Q0])
    assert feasible[er.EQUILIBRIUM] and (ev.nc > 0 or feasible.all())
    assert (ref.V[feasible, 1] <= ref.V[feasible, 0]).all()
    assert np.array_equal(ref.V[:, 0], np.array([ev.V(q) for q in Q0]))


# ---- 2. what the safeguards are for -------------------------------------------------------------------------------------------
def test_undamped_iteration_reaches_a_non_minimum_from_golden_poses():
    """The projection's plain Newton on the KKT conditions converges to stationary points that are no minima."""
    seen = 0
    for name, mask in (("plane_link", "all"), ("spring_link", "keep_kinematic")):
        free = er.free_mask(name, mask)
        poses = pr.golden_poses(name)
        Q = poses[np.linspace(0, len(poses) - 1, 24).astype(int)]
        got = er.minimize(name, Q, free, opt=er.UNDAMPED)
        ev = er.potential_of(name)
        for b in np.flatnonzero(got.status == er.OK):
            floor = er.reduced_hessian_floor(ev, got.Q[b], got.mu[b], free)
            print(name, b, "reduced Hessian floor %.3e" % floor)
            seen += floor < 0.0
        safe = er.minimize(name, Q, free)
        ok = safe.status == er.OK
        assert er.certified(name, safe, free)[ok].all()         # the safeguarded iteration: whatever converges is a minimum
    assert seen >= 1


MUTANTS = {"no_definiteness_test": er.SPEC._replace(definiteness=False), "no_mu_curvature": er.SPEC._replace(mu_curvature=False),
           "vq_sign_flipped": er.SPEC._replace(vq_sign=-1.0)}
MUTANT_CASES = {"no_definiteness_test": ("pendulum5", "all", er.GOLDEN_START), "no_mu_curvature": ("plane_link", "all", 0.1),
                "vq_sign_flipped": ("spring_link", "keep_kinematic", 0.02)}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutation_fails_the_table(mutant):
    """A mutant fails the table if, on one of its cases, a row does not end TG_OK at a certified minimum, or the answer misses the
    comparison the emulation and the device have to pass."""
    case = MUTANT_CASES[mutant]
    Q0, free = er.case_inputs(*case)
    got = er.minimize(case[0], Q0, free, opt=MUTANTS[mutant])
    certified = er.certified(case[0], got, free)
    print(mutant, er.case_id(case), "status", got.status, "certified", certified, "trials", got.iterations)
    failed = not certified.all()
    if not failed:
        try:
            er.compare(case, got)
        except AssertionError:
            failed = True
    assert failed


# ---- 3. the emulated kernel over the table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", er.CASES, ids=CASE_IDS)
def test_emulated_kernel_over_the_table(case):
    Q0, free = er.case_inputs(*case)
    got = _emu(case[0]).minimize(Q0, free, tolerance=er.TOL)
    er.compare(case, got)
    assert er.certified(case[0], got, free).all()


def test_emulated_kernel_with_a_null_mask_is_the_all_mask():
    case = ("plane_link", "all", 0.1)
    Q0, free = er.case_inputs(*case)
    emu = _emu(case[0])
    a, b = emu.minimize(Q0, free), emu.minimize(Q0, None)
    for k in a._fields:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


PAR_SYSTEMS = {"plane_link": "all", "spring_link": "keep_kinematic"}


def parameter_rows(name):
    """Four rows: (g, m), (2 g, m), (g, m'), (2 g, m') with m' the masses and inertias scaled body by body."""
    system = common.build(name)[0]
    base = parameters.base_values(system)
    scale = 1.0 + 0.5 * np.arange(1, len(base["inertia"]) + 1)[:, None] / len(base["inertia"])
    inertia = np.array([base["inertia"], base["inertia"], base["inertia"] * scale, base["inertia"] * scale])
    gravity = np.array([base["gravity"], 2 * base["gravity"], base["gravity"], 2 * base["gravity"]])
    return {"inertia": inertia, "gravity": gravity}


def parameter_table(name, rows):
    system = common.build(name)[0]
    nd = len(system.dyn_configs)
    damping = parameters.base_values(system)["damping"]
    damping = np.zeros(nd) if damping is None else damping
    return np.array([np.concatenate([rows["inertia"][r].ravel(), rows["gravity"][r], damping]) for r in range(len(rows["inertia"]))])


def parameter_reference(name, Q0, free, rows, group):
    """Every pose by the reference on a descriptor built with its row's values."""
    out = []
    for r in range(len(rows["inertia"])):
        ev = er.Potential(descriptor.flatten(rebuilt(common.BUILDERS[name], rows, r)))
        out.append(er.minimize(name, Q0[r * group:(r + 1) * group], free, ev=ev))
    return er.Equilibrium(*[np.concatenate([getattr(o, k) for o in out]) for k in er.Equilibrium._fields])


def parameter_inputs(name):
    case = (name, PAR_SYSTEMS[name], 0.02)
    Q0, free = er.case_inputs(*case)
    return np.concatenate([Q0[:3]] * 4), free, case


def check_parameter_rows(name, got, ref, case):
    """Each pose matches the reference of its row; gravity alone moves no equilibrium of a pure-gravity system and moves a spring's."""
    bound = max(er.case_bound(*case), er.MARGIN * 1e-13)
    err = float(np.abs(got.Q - ref.Q).max())
    verr = float((np.abs(got.V - ref.V) / np.maximum(1.0, np.abs(ref.V))).max())
    print(name, "parameter rows: error %.3e bound %.3e V %.3e trials %s reference %s" % (err, bound, verr, got.iterations, ref.iterations))
    assert (ref.status == er.OK).all() and np.array_equal(got.status, ref.status)
    firm = er.firm_rows(ref)
    assert np.array_equal(got.iterations[firm], ref.iterations[firm])
    assert err <= bound and verr <= er.V_PARITY
    moved = float(np.abs(got.Q[3:6] - got.Q[0:3]).max())        # g -> 2 g, the same masses, the same starts
    if name == "plane_link":
        assert moved <= 2 * bound
        assert np.abs(got.V[3:6, 1] - 2 * got.V[0:3, 1]).max() <= er.V_PARITY * np.abs(got.V[3:6, 1]).max() + 1e-12
    else:
        assert moved > 1e-3


@pytest.mark.parametrize("name", sorted(PAR_SYSTEMS))
def test_emulated_parameter_twin_matches_rebuilt_systems(name):
    Q0, free, case = parameter_inputs(name)
    rows = parameter_rows(name)
    got = _emu(name).minimize(Q0, free, rows=parameter_table(name, rows), group=3)
    ref = parameter_reference(name, Q0, free, rows, 3)
    check_parameter_rows(name, got, ref, case)
    base = _emu(name).minimize(Q0[:3], free)
    for k in base._fields:                                       # row 0 holds the system's own values
        assert np.array_equal(getattr(got, k)[:3], getattr(base, k)), k


# ---- 4. status ------------------------------------------------------------------------------------------------------------------
def test_status_not_converged_returns_the_last_accepted_iterate():
    case = ("puppet_basic", "all", 0.1)
    Q0, free = er.case_inputs(*case)
    ref = er.case_reference(*case)
    slow = int(np.argmax(ref.iterations))
    rows = np.array([Q0[er.EQUILIBRIUM], Q0[slow], Q0[er.EQUILIBRIUM]])
    emu = _emu(case[0])
    got = emu.minimize(rows, free, max_iterations=2)
    want = er.minimize(case[0], rows, free, max_iterations=2)
    assert list(got.status) == [er.OK, er.NOT_CONVERGED, er.OK] and list(got.iterations) == [0, 2, 0]
    assert np.array_equal(got.status, want.status) and np.array_equal(got.iterations, want.iterations)
    assert np.abs(got.Q - want.Q).max() <= er.MARGIN * 1e-13
    assert emu.minimize(Q0[slow][None], free, max_iterations=0).status[0] == er.NOT_CONVERGED
    assert np.array_equal(emu.minimize(Q0[slow][None], free, max_iterations=0).Q[0], Q0[slow])


def test_status_empty_free_set():
    case = ("plane_link", "all", 0.02)
    Q0, free = er.case_inputs(*case)
    rest = er.case_reference(*case, 1e-13).Q[0]
    none = np.zeros(len(free), dtype=bool)
    got = _emu(case[0]).minimize(np.array([rest, Q0[0]]), none)
    assert list(got.status) == [er.OK, er.SINGULAR] and not got.iterations.any()      # nothing free: g is empty, the test is h alone
    assert np.array_equal(got.Q, np.array([rest, Q0[0]]))
    d = common.build("pendulum1")[1]
    hang = emu_pose_harness.EmuEquilibrium(d).minimize(np.array([[0.0], [0.3]]), np.zeros(1, dtype=bool))
    assert list(hang.status) == [er.OK, er.OK] and not hang.iterations.any()          # no constraint either: nothing to test
    assert np.array_equal(hang.Q, [[0.0], [0.3]])


def test_status_the_regularisation_runs_out():
    """scissor4 with the slider held, far from the manifold: as many constraints as free configs, every trial is Newton on h
    alone and none lowers the merit -- tau grows to its end, 21 trials, TG_SINGULAR, q unchanged (draw 0 of the case holds such rows)."""
    case = ("scissor4", "constant", 0.1)
    free = er.free_mask(case[0], case[1])
    eq = er.equilibria(case[0], case[1])
    rng = np.random.default_rng(common.tb_seed("equilibrium", *case[:2], 100, 0))
    Q = eq[rng.integers(len(eq), size=24)].copy()
    Q[:, free] += 0.1 * rng.standard_normal((24, int(free.sum())))
    ref = er.minimize(case[0], Q, free)
    assert (ref.status == er.SINGULAR).any() and set(ref.status) <= {er.OK, er.SINGULAR}
    got = _emu(case[0]).minimize(Q, free)
    assert np.array_equal(got.status, ref.status) and np.array_equal(got.iterations, ref.iterations)
    lost = ref.status == er.SINGULAR
    assert np.array_equal(got.Q[lost], Q[lost]) and (got.iterations[lost] == 21).all()


# ---- 5. refusals of the entry points, computed on the host ----------------------------------------------------------------------
def test_null_handles_are_refused():
    L = _lib.lib()
    for name in ("tg_batch_minimize_potential", "tg_batch_minimize_potential_device"):
        assert getattr(L, name)(None, None, None, 1e-10, 100, None, None, None, None, None) == ERR_INVALID
        assert L.tg_last_error() == b"null argument"
    assert L.tg_system_equilibrium_lds(None, None) == ERR_INVALID and L.tg_last_error() == b"null argument"


@pytest.mark.parametrize("entry", ("tg_batch_minimize_potential", "tg_batch_minimize_potential_device"))
def test_bad_scalars_are_refused_before_the_batch_is_looked_at(entry):
    L = _lib.lib()
    fn = getattr(L, entry)
    batch = ctypes.create_string_buffer(1 << 20)
    q = np.zeros(64)
    b, p = ctypes.addressof(batch), q.ctypes.data
    for tol, its, message in ((0.0, 100, b"tolerance must be positive"), (-1e-10, 100, b"tolerance must be positive"),
                              (float("nan"), 100, b"tolerance must be positive"), (1e-10, -1, b"max_iterations must not be negative")):
        assert fn(b, p, None, tol, its, p, None, None, None, None) == ERR_INVALID
        assert L.tg_last_error() == message
    assert fn(b, None, None, 1e-10, 100, p, None, None, None, None) == ERR_INVALID and L.tg_last_error() == b"null argument"
    assert fn(b, p, None, 1e-10, 100, None, None, None, None, None) == ERR_INVALID and L.tg_last_error() == b"null argument"


def test_a_nonlinear_config_spring_is_refused():
    L = _lib.lib()
    d = common.build("nonlinear_spring_arm")[1]
    sys_h = L.tg_system_create(d.byref())
    assert sys_h
    try:
        out = np.zeros(4, dtype=np.int32)
        assert L.tg_system_equilibrium_lds(sys_h, out.ctypes.data_as(_lib._c_ip)) == ERR_UNSUPPORTED
        assert L.tg_last_error().startswith(b"a NonlinearConfigSpring has a force but no potential energy")
        assert out[0] > 0 and out[1] > 0
    finally:
        L.tg_system_destroy(sys_h)


LDS_CELLS = [(n, t) for n in ("pendulum1", "plane_link", "scissor4", "puppet_basic", "puppet40", "pendulum5") for t in (1, 4, 16, 64)]


def lds_doubles(rollout, nq, nc):
    """Per team: the rollout slice, the KKT image [n][n + 1] (n = nq + nc), W and the Cholesky work area [nq][nq] each, q0 [nq], the
    kept pose and multipliers [n], V_q [nq], g [nq], V (2), the solver's row scales [n], the free configs' places (int [nq])."""
    even = lambda x: (x + 1) & ~1
    n = nq + nc
    return even(even(even(rollout) + n * (n + 1) + 2 * nq * nq + nq + n + 2 * nq + 2 + n) + (nq + 1) // 2)


@pytest.mark.parametrize("name,team", LDS_CELLS)
def test_lds_of_a_workgroup_and_its_refusal(monkeypatch, name, team):
    monkeypatch.setenv("TREPAMD_TEAM", str(team))
    L = _lib.lib()
    d = common.build(name)[1]
    slice_, rollout = emu_pose_harness.EmuEquilibrium(d).lds_doubles()
    assert rollout == emu_harness.lds_slices(d)["rollout"]
    assert slice_ == lds_doubles(rollout, int(d.n_configs), int(d.n_constraints))
    sys_h = L.tg_system_create(d.byref())
    assert sys_h
    try:
        out = np.zeros(4, dtype=np.int32)
        rc = L.tg_system_equilibrium_lds(sys_h, out.ctypes.data_as(_lib._c_ip))
        bytes_ = (64 // team) * slice_ * 8
        assert list(out) == [team, slice_, bytes_, 0]
        if bytes_ > 160 * 1024:
            assert rc == ERR_UNSUPPORTED and L.tg_last_error() == b"system too large for the LDS-resident equilibrium kernel"
        else:
            assert rc == 0
    finally:
        L.tg_system_destroy(sys_h)


def test_both_sides_of_the_lds_limit_are_in_the_cells(monkeypatch):
    L = _lib.lib()
    seen = set()
    for name, team in LDS_CELLS:
        monkeypatch.setenv("TREPAMD_TEAM", str(team))
        d = common.build(name)[1]
        sys_h = L.tg_system_create(d.byref())
        out = np.zeros(4, dtype=np.int32)
        seen.add(L.tg_system_equilibrium_lds(sys_h, out.ctypes.data_as(_lib._c_ip)))
        L.tg_system_destroy(sys_h)
    assert seen == {0, ERR_UNSUPPORTED}


# ---- 6. layout guards -----------------------------------------------------------------------------------------------------------
def test_run_args_layout_is_the_emulation_harness_mirror():
    assert ctypes.sizeof(emu_harness.RunArgs) == emu_pose_harness.sizeof_run_args()


def test_the_new_entry_points_are_exported_and_declared():
    names = set(_lib.exported_symbols())
    assert {"tg_batch_minimize_potential", "tg_batch_minimize_potential_device", "tg_system_equilibrium_lds"} <= names
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "trep_amd.h")).read()
    for n in _lib._EQUILIBRIUM_SIGNATURES:
        assert "int %s(" % n in header


def test_parity_profile_covers_the_table():
    """The committed record names every case of the table and is consistent with itself; it recomputes neither a floor nor an
    error.  The parity check proper is test_emulated_kernel_over_the_table."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "equilibrium_parity.json")
    with open(path) as f:
        prof = json.load(f)
    assert sorted(prof["cases"]) == sorted(CASE_IDS)
    for cid, row in prof["cases"].items():
        assert row["bound"] == er.MARGIN * max(row["floor"], 1e-13)
        assert row["emulation_error"] <= row["bound"]
