"""Batched constraint projection without a device: the numpy reference (projection_reference.py) on its case table, the checks of an
answer that do not depend on the iteration, the teeth of those checks, and the kernel itself (mvi_project.hpp) compiled for the host
with TEAM = 1 (emu_pose_harness.py) against the reference -- answers within the per-case bound, step counts within one, the
status cases, the refusals of the C entry points and the layout guards.

Per case, floor = max |q_ref(tolerance 1e-10) - q_ref(tolerance 1e-13)| and the bound on |q - q_ref| is 64 max(floor, 1e-13)
(tools/projection_parity.py writes both, with the worst errors, to profiles/projection_parity.json)."""
import ctypes
import json
import os

import numpy as np
import pytest

import common
import emu_harness
import emu_pose_harness
import projection_reference as pr
from trep_amd import _lib

CASE_IDS = [pr.case_id(c) for c in pr.CASES]
ERR_INVALID, ERR_UNSUPPORTED = -1, -3


def _emu(name):
    return emu_pose_harness.EmuProjection(common.build(name)[1])


# ---- 1. the reference iteration converges on the table ----------------------------------------------------------------------
@pytest.mark.parametrize("case", pr.CASES, ids=CASE_IDS)
def test_reference_converges_within_the_cap(case):
    ref = pr.case_reference(*case)
    assert (ref.status == pr.OK).all(), ref.status
    assert ref.iterations.max() <= pr.STEP_CAP, ref.iterations
    assert ref.iterations[pr.CONSISTENT] == 0
    assert ref.iterations[:pr.CONSISTENT].min() >= 1           # every other row of the table really is off the manifold


# ---- 2. the answer, independent of the iteration ------------------------------------------------------------------------------
def _assert_answer(case, got):
    name = case[0]
    Q0, dQ0, free = pr.case_inputs(*case)
    res = pr.residuals(name, Q0, dQ0, free, got)
    print(pr.case_id(case), dict((k, float(v.max())) for k, v in res.items()))
    assert res["fixed"].all()
    for k in ("h", "normal", "stationary", "tangent", "row_space"):
        assert res[k].max() <= 1.0, (k, res[k])


@pytest.mark.parametrize("case", pr.CASES, ids=CASE_IDS)
def test_reference_answer(case):
    _assert_answer(case, pr.case_reference(*case))


# ---- 3 / 4. the emulated kernel over the table --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pr.CASES, ids=CASE_IDS)
def test_emulated_kernel_over_the_table(case):
    name = case[0]
    Q0, dQ0, free = pr.case_inputs(*case)
    ref = pr.case_reference(*case)
    got = _emu(name).project(Q0, dQ0, free, tolerance=pr.TOL)
    bound = pr.case_bound(*case)
    err = float(np.abs(got.Q - ref.Q).max())
    print(pr.case_id(case), "floor %.3e bound %.3e error %.3e steps %s reference %s" % (pr.case_floor(*case), bound, err, got.iterations, ref.iterations))
    assert (got.status == pr.OK).all(), got.status
    assert err <= bound
    # the curvature term: without it the iteration is a sequential linearisation with 13-26 steps on puppet40 under keep_kinematic
    assert (got.iterations <= ref.iterations + 1).all(), (got.iterations, ref.iterations)
    assert got.iterations[pr.CONSISTENT] == 0 and np.array_equal(got.Q[pr.CONSISTENT], Q0[pr.CONSISTENT])
    assert np.array_equal(got.Q[pr.REPEAT], got.Q[0]) and np.array_equal(got.dQ[pr.REPEAT], got.dQ[0]) and np.array_equal(got.mu[pr.REPEAT], got.mu[0])
    _assert_answer(case, got)


def test_emulated_kernel_without_velocities_and_multipliers():
    case = ("puppet_basic", "constant", 0.02)
    Q0, dQ0, free = pr.case_inputs(*case)
    emu = _emu(case[0])
    full, bare = emu.project(Q0, dQ0, free), emu.project(Q0, None, free)
    assert bare.dQ is None
    assert np.array_equal(full.Q, bare.Q) and np.array_equal(full.mu, bare.mu) and np.array_equal(full.iterations, bare.iterations)


def test_parity_profile_covers_the_table():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "projection_parity.json")
    with open(path) as f:
        prof = json.load(f)
    assert sorted(prof["cases"]) == sorted(CASE_IDS)
    for cid, row in prof["cases"].items():
        assert row["bound"] == pr.MARGIN * max(row["floor"], 1e-13)
        assert row["emulation_error"] <= row["bound"]


# ---- 5. teeth of (2), on the reference alone ----------------------------------------------------------------------------------
SHIFTED = [(n, "constant") for n in pr.SYSTEMS] + [("puppet40", "keep_kinematic")]


@pytest.mark.parametrize("name,mask", SHIFTED)
def test_teeth_mask_shifted_by_one(name, mask):
    Q0, dQ0, free = pr.case_inputs(name, mask, 0.02)
    wrong = np.roll(free, 1)
    assert not np.array_equal(wrong, free)
    got = pr.project(name, Q0, dQ0, wrong)
    res = pr.residuals(name, Q0, dQ0, free, got)
    print(name, mask, pr.worst(res))
    assert not res["fixed"][:pr.CONSISTENT].any()
    assert pr.worst(res) >= 100.0


@pytest.mark.parametrize("name", pr.SYSTEMS)
def test_teeth_dropped_hessian_pair(name):
    """The curvature changes the rate, not the fixed point: the mutant gets the reference's own step count on every row."""
    case = (name, "all", 0.1)
    Q0, dQ0, free = pr.case_inputs(*case)
    ref = pr.case_reference(*case)
    ev = pr.constraints_of(name)
    rows = [pr.project_one(ev, Q0[b], free, dQ0[b], max_iterations=int(ref.iterations[b]), drop="largest") for b in range(len(Q0))]
    got = pr.Projection(np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows]).reshape(len(Q0), ev.nc), None, None)
    res = pr.residuals(name, Q0, dQ0, free, got)
    worst = max(float(res[k].max()) for k in ("h", "normal", "stationary"))
    print(name, worst)
    assert worst >= 100.0


@pytest.mark.parametrize("noise", (0.02, 0.1))
def test_teeth_length_config_column_left_out(noise):
    """Reaches the systems whose distance constraints have a length config, where that config is free: puppet40, mask "all"."""
    name = "puppet40"
    ev = pr.Constraints(common.build(name)[1])
    assert (np.asarray(ev.d.constraint_config[:ev.nc]) >= 0).any()
    ev.drop_length_column = True
    Q0, dQ0, free = pr.case_inputs(name, "all", noise)
    got = pr.project(name, Q0, dQ0, free, ev=ev)
    res = pr.residuals(name, Q0, dQ0, free, got)
    print(name, noise, pr.worst(res))
    assert pr.worst(res) >= 100.0


# ---- 6. status ------------------------------------------------------------------------------------------------------------
def _status_rows(name="puppet40"):
    """(perturbed pose, three consistent poses)."""
    Q0 = pr.case_inputs(name, "all", 0.02)[0]
    good = pr.case_reference(name, "all", 0.02, 1e-13).Q[2:5]
    return Q0[0], good


def test_status_not_converged_returns_the_first_iterate():
    name = "puppet40"
    bad, good = _status_rows(name)
    emu = _emu(name)
    with_bad = emu.project(np.array([good[0], bad, good[1], good[2]]), max_iterations=1)
    without = emu.project(good, max_iterations=1)
    assert list(with_bad.status) == [pr.OK, pr.NOT_CONVERGED, pr.OK, pr.OK] and list(with_bad.iterations) == [0, 1, 0, 0]
    first = pr.project_one(pr.constraints_of(name), bad, np.ones(emu.nq, dtype=bool), max_iterations=1)
    assert first[4] == pr.NOT_CONVERGED and np.abs(with_bad.Q[1] - first[0]).max() <= pr.MARGIN * 1e-13
    assert np.abs(with_bad.Q[1] - bad).max() > 1e-4
    for k in ("Q", "mu", "iterations", "status"):
        assert np.array_equal(getattr(with_bad, k)[[0, 2, 3]], getattr(without, k)), k
    assert emu.project(bad[None], max_iterations=0).status[0] == pr.NOT_CONVERGED


def test_status_empty_free_set():
    name = "puppet40"
    bad, good = _status_rows(name)
    emu = _emu(name)
    none = np.zeros(emu.nq, dtype=bool)
    dq = np.ones((4, emu.nq))
    with_bad = emu.project(np.array([good[0], bad, good[1], good[2]]), dq, free=none)
    without = emu.project(good, dq[:3], free=none)
    assert list(with_bad.status) == [pr.OK, pr.SINGULAR, pr.OK, pr.OK] and not with_bad.iterations.any()
    assert np.array_equal(with_bad.Q[1], bad) and np.array_equal(with_bad.Q[0], good[0])        # q unchanged, consistent or not
    assert np.array_equal(with_bad.dQ, dq)                                                       # nothing free: the rates stay
    for k in ("Q", "dQ", "mu", "iterations", "status"):
        assert np.array_equal(getattr(with_bad, k)[[0, 2, 3]], getattr(without, k)), k


def test_status_without_constraints():
    d = common.build("pendulum1")[1]
    emu = emu_pose_harness.EmuProjection(d)
    Q = np.array([[0.3], [-1.2], [4.0]])
    dQ = np.array([[1.0], [2.0], [3.0]])
    got = emu.project(Q, dQ)
    assert np.array_equal(got.Q, Q) and np.array_equal(got.dQ, dQ) and not got.status.any() and not got.iterations.any()
    assert got.mu.shape == (3, 0)


# ---- 7. refusals of the entry points, computed on the host -----------------------------------------------------------------------
def test_null_handles_are_refused():
    L = _lib.lib()
    for name in ("tg_batch_project_constraints", "tg_batch_project_constraints_device"):
        assert getattr(L, name)(None, None, None, None, 1e-10, 50, None, None, None, None, None) == ERR_INVALID
        assert L.tg_last_error() == b"null argument"
    assert L.tg_system_projection_lds(None, None) == ERR_INVALID and L.tg_last_error() == b"null argument"


@pytest.mark.parametrize("entry", ("tg_batch_project_constraints", "tg_batch_project_constraints_device"))
def test_bad_scalars_are_refused_before_the_batch_is_looked_at(entry):
    """The argument checks come before anything of the batch is read: a block of zeros stands in for it (were one read after all, its
    null system would be refused as well)."""
    L = _lib.lib()
    fn = getattr(L, entry)
    batch = ctypes.create_string_buffer(1 << 20)
    q = np.zeros(64)
    b, p = ctypes.addressof(batch), q.ctypes.data
    for tol, its, dq, dq_out, message in ((0.0, 50, None, None, b"tolerance must be positive"),
                                          (-1e-10, 50, None, None, b"tolerance must be positive"),
                                          (float("nan"), 50, None, None, b"tolerance must be positive"),
                                          (1e-10, -1, None, None, b"max_iterations must not be negative"),
                                          (1e-10, 50, None, p, b"dq_out without dq")):
        assert fn(b, p, dq, None, tol, its, p, dq_out, None, None, None) == ERR_INVALID
        assert L.tg_last_error() == message
    assert fn(b, None, None, None, 1e-10, 50, p, None, None, None, None) == ERR_INVALID and L.tg_last_error() == b"null argument"
    assert fn(b, p, None, None, 1e-10, 50, None, None, None, None, None) == ERR_INVALID and L.tg_last_error() == b"null argument"


LDS_CELLS = [(n, t) for n in ("pendulum1", "plane_link", "scissor4", "puppet_basic", "puppet40", "pendulum5") for t in (1, 4, 16, 64)]


@pytest.mark.parametrize("name,team", LDS_CELLS)
def test_lds_of_a_workgroup_and_its_refusal(monkeypatch, name, team):
    """Per team: the rollout slice, the KKT image [n][n + 1] (n = nq + nc), q0 [nq], the solver's row scales [n] and the free configs'
    places (int [nq]); 64 / team teams per workgroup; refused above 160 KiB."""
    monkeypatch.setenv("TREPAMD_TEAM", str(team))
    L = _lib.lib()
    d = common.build(name)[1]
    nq, nc = int(d.n_configs), int(d.n_constraints)
    n = nq + nc
    slice_, rollout = emu_pose_harness.EmuProjection(d).lds_doubles()
    assert rollout == emu_harness.lds_slices(d)["rollout"]
    even = lambda x: (x + 1) & ~1
    assert slice_ == even(even(even(rollout) + n * (n + 1) + nq + n) + (nq + 1) // 2)
    sys_h = L.tg_system_create(d.byref())
    assert sys_h
    try:
        out = np.zeros(4, dtype=np.int32)
        rc = L.tg_system_projection_lds(sys_h, out.ctypes.data_as(_lib._c_ip))
        bytes_ = (64 // team) * slice_ * 8
        assert list(out) == [team, slice_, bytes_, 0]
        if bytes_ > 160 * 1024:
            assert rc == ERR_UNSUPPORTED and L.tg_last_error() == b"system too large for the LDS-resident projection kernel"
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
        seen.add(L.tg_system_projection_lds(sys_h, out.ctypes.data_as(_lib._c_ip)))
        L.tg_system_destroy(sys_h)
    assert seen == {0, ERR_UNSUPPORTED}


# ---- 8. layout guards -------------------------------------------------------------------------------------------------------
def test_run_args_layout_is_the_emulation_harness_mirror():
    assert ctypes.sizeof(emu_harness.RunArgs) == emu_pose_harness.sizeof_run_args()


def test_the_new_entry_points_are_exported_and_declared():
    names = set(_lib.exported_symbols())
    assert {"tg_batch_project_constraints", "tg_batch_project_constraints_device", "tg_system_projection_lds"} <= names
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "trep_amd.h")).read()
    for n in _lib._PROJECTION_SIGNATURES:
        assert "int %s(" % n in header
