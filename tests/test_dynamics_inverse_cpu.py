"""Batched computed torque without a device: the numpy specification (dynamics_inverse_reference.py) against the reference project's own
records (tests/golden/dynamics.npz), the conditions of the case table, the mutations the table must catch, the kernel itself
(mvi_dyn_inverse.hpp) compiled for the host with TEAM = 1 (emu_dyn_inverse_harness.py) over the whole table, its parameter-table twin, the
strided read, null outputs, a [B][nq] call, the status cases, and the refusals and LDS geometry of the C entry points.

Measured here (tools/dynamics_inverse_parity.py writes the per-case floors and errors to profiles/dynamics_inverse_parity.json):
  on the recorded states of dynamics.npz (21 systems, 4 states each; only mixed_loop, n > nd, is not of full column rank), worst over
  the systems: u recovered to 8.4e-14 (wrench_arm), lambda to 8.7e-15 (ladder_point), |rho| 2.8e-14 (pendulum5) and |acc| 1.4e-14
  (ladder_mixed), relative to max(1, |want|inf), max(1, |tau|inf) and max(1, |Ad ddq_d|inf);
  the emulated kernel over the table stays under 1.4e-2 of its bound for z and rho (wrench_arm: 3.0e-12 against a floor of 3.5e-12)
  and under 2e-4 of 1e-10 for tau and acc (scissor4: 1.9e-14);
  the mutated specifications miss by 1.7e9 bounds at the least (the kinematic accelerations ignored, on spatial_loop)."""
import ctypes
import os

import numpy as np
import pytest

import common
import dynamics_inverse_reference as dr
import emu_dyn_inverse_harness
import emu_harness
from oracle.oracle import OracleMVI
from trep_amd import _lib

CASE_IDS = [dr.case_id(c) for c in dr.CASES]
ERR_INVALID, ERR_UNSUPPORTED = -1, -3


def _emu(name):
    return emu_dyn_inverse_harness.EmuDynInverse(common.build(name)[1])


def _run(case, **kw):
    p = dr.case_states(case)
    return _emu(case.name).dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], case.ridge, **kw)


def _same(a, b, fields=dr.FIELDS):
    for q in fields:
        assert np.array_equal(getattr(a, q), getattr(b, q)), q


# ---- 1. the specification against the reference project's records ---------------------------------------------------------------------
GOLDEN = dict(np.load(os.path.join(common.GOLDEN, "dynamics.npz")))
GOLDEN_SYSTEMS = sorted(k[:-len("_ddqk")] for k in GOLDEN if k.endswith("_ddqk"))


@pytest.mark.parametrize("name", GOLDEN_SYSTEMS)
def test_specification_returns_the_recorded_inputs_and_multipliers(name):
    """ddq = (the recorded f | the recorded ddqk): the recorded (u, lam) is an exact solution, so rho = 0 and acc = 0 on every system,
    and where A has full column rank (sigma_min >= SIGMA_MIN) least squares returns the recorded u and lam themselves."""
    assert name in common.BUILDERS
    _, d = common.build(name)
    o = OracleMVI(d)
    nd, nu = int(d.n_dyn), int(d.n_inputs)
    g = lambda k: GOLDEN["%s_%s" % (name, k)]
    for s in range(len(g("q"))):
        q, dq, u, ddqk, f, lam = g("q")[s], g("dq")[s], g("u")[s], g("ddqk")[s], g("f")[s], g("lam")[s]
        Ad, F_du, Mm, D0, ddq0, _ = dr.ingredients(o, q, dq, ddqk)
        A = np.concatenate([F_du, Ad.T], axis=1)
        r0 = D0 - Mm.dot(f)
        z = np.linalg.lstsq(A, -r0, rcond=None)[0] if A.shape[1] else np.zeros(0)
        rho, acc = r0 + A.dot(z), Ad.dot(f - ddq0)
        smin = np.linalg.svd(A, compute_uv=False).min() if A.shape[1] else np.inf
        full = A.shape[1] <= nd and smin >= dr.SIGMA_MIN
        scale_t = max(1.0, float(np.abs(r0).max(initial=0.0)))
        e_rho, e_acc = float(np.abs(rho).max(initial=0.0)) / scale_t, float(np.abs(acc).max(initial=0.0)) / max(1.0, float(np.abs(Ad.dot(f)).max(initial=0.0)))
        e_u = common.relerr(z[:nu], u) if full else None
        e_l = common.relerr(z[nu:], lam) if full else None
        print(name, s, "sigma_min %.3e full rank %s: u %s lam %s rho %.3e acc %.3e" % (
            smin, full, "-" if e_u is None else "%.3e" % e_u, "-" if e_l is None else "%.3e" % e_l, e_rho, e_acc))
        assert e_rho <= dr.TOL and e_acc <= dr.TOL
        if full:
            assert e_u <= dr.TOL and e_l <= dr.TOL


# ---- 2. the conditions of the table --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dr.CASES, ids=CASE_IDS)
def test_the_table_meets_its_conditions(case):
    """dynamics() is non-singular at every state (case_reference raises otherwise), the continuous equations are affine within
    AFFINITY (asserted inside the specification), and a ridge-free case with unknowns has sigma_min(A) >= SIGMA_MIN."""
    ref = dr.case_reference(case)
    p = dr.case_states(case)
    d = p["d"]
    nd, n = int(d.n_dyn), int(d.n_inputs + d.n_constraints)
    assert p["Q"].shape == (case.B, case.M, int(d.n_configs))
    assert (ref.status == dr.OK).all() and np.isfinite(ref.z).all() and np.isfinite(ref.tau).all()
    smin = dr.sigma_min(ref)
    print(dr.case_id(case), "n %d nd %d sigma_min %.3e |rho|inf %.3e |acc|inf %.3e" % (n, nd, smin, np.abs(ref.rho).max(initial=0.0), np.abs(ref.acc).max(initial=0.0)))
    if case.ridge == 0.0 and n > 0:
        assert n <= nd and smin >= dr.SIGMA_MIN
    if case.name == "mixed_loop":
        assert n > nd and case.ridge > 0
    if case.name == "puppet_forces":
        assert smin < 1e-10 and case.ridge > 0         # rank deficient
    if case.name == "damper_link":
        assert n == 0
    if case.name == "pend_on_cart":
        assert np.abs(ref.rho).max() > 1e-3            # underactuated: the residual is the point of the case


# ---- 3. mutated specifications -----------------------------------------------------------------------------------------------------
# mutant -> the table rows that reach its ingredient and must miss by at least 1e3 bounds
MUTANT_ROWS = {
    "ignore_ddqk": ("wrench_arm", "spatial_loop", "puppet40"),           # the kinematic accelerations left out: rows with kinematic configs
    "discrete_sign": ("scissor4", "spatial_loop", "puppet40"),           # -Ad' as in the discrete kernel: rows with constraints
    "input_dt": ("pend_on_cart", "wrench_arm", "wrench_torque"),         # dt F_du in place of F_du: rows with inputs
}


@pytest.mark.parametrize("mutant", sorted(MUTANT_ROWS))
def test_mutation_misses_the_table(mutant):
    for name in MUTANT_ROWS[mutant]:
        c = dr.case_by_name(name)
        p = dr.case_states(c)
        ref = dr.case_reference(c)
        got = dr.dynamics_inverse(p["d"], p["Q"], p["dQ"], p["ddQ"], c.ridge, spec=dict(dr.SPEC, **{mutant: True}))
        e = dr.errors(ref, got)
        margin = max(max(e["z"], e["rho"]) / dr.bound(ref), max(e["tau"], e["acc"]) / dr.TOL_DIRECT)
        print(mutant, dr.case_id(c), "misses by %.3e bounds" % margin, e)
        assert margin >= 1e3, (mutant, name, e)


# ---- 4. the emulated kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dr.CASES, ids=CASE_IDS)
def test_emulated_kernel_over_the_table(case):
    got = _run(case)
    dr.compare(case, got)
    assert (got.status == dr.OK).all()


def test_emulated_kernel_does_not_depend_on_what_the_scratch_held():
    case = dr.case_by_name("wrench_arm")
    _same(_run(case, poison=True), _run(case, poison=False))


def test_emulated_state_does_not_depend_on_its_launch():
    """A state alone in a B = 1, M = 1 call, and a trajectory twice in one call: the same bits."""
    case = dr.case_by_name("scissor4")
    p = dr.case_states(case)
    emu = _emu(case.name)
    Q, dQ, ddQ = p["Q"], p["dQ"], p["ddQ"]
    whole = emu.dynamics_inverse(Q, dQ, ddQ)
    b, s = 3, 7
    one = emu.dynamics_inverse(Q[b:b + 1, s:s + 1], dQ[b:b + 1, s:s + 1], ddQ[b:b + 1, s:s + 1])
    twice = emu.dynamics_inverse(Q[[b, b]], dQ[[b, b]], ddQ[[b, b]])
    for q in dr.FIELDS:
        assert np.array_equal(getattr(one, q)[0, 0], getattr(whole, q)[b, s]), q
        assert np.array_equal(getattr(twice, q)[0], getattr(whole, q)[b]) and np.array_equal(getattr(twice, q)[1], getattr(whole, q)[b]), q


def test_emulated_kernel_reads_strided_rows():
    """Q taken from X [B][M][nX] with the row stride nX, as the device variant reads a rollout's X; dQ and ddQ with strides of their own."""
    case = dr.case_by_name("wrench_arm")
    p = dr.case_states(case)
    d = p["d"]
    nq = int(d.n_configs)
    packed = _run(case)
    widths = (int(d.n_configs + d.n_dyn + d.n_kin), nq + 3, nq + 1)
    wide = []
    for a, w in zip((p["Q"], p["dQ"], p["ddQ"]), widths):
        x = np.full((case.B, case.M, w), np.nan)
        x[:, :, :nq] = a
        wide.append(x)
    _same(packed, _emu(case.name).dynamics_inverse(*wide, ridge=case.ridge, strides=widths))


def test_emulated_kernel_writes_only_what_is_asked_for():
    """Every output alone, the others null: the same bits as in the call with all of them."""
    case = dr.case_by_name("spatial_loop")
    full = _run(case)
    for q in dr.FIELDS:
        alone = _run(case, want=(q,))
        assert np.array_equal(getattr(alone, q), getattr(full, q)), q
        assert all(getattr(alone, o) is None for o in dr.FIELDS if o != q)
    nothing = _run(case, want=())
    assert all(v is None for v in nothing)


def test_emulated_kernel_on_one_state_per_trajectory():
    """Q [B][nq], i.e. n_states = 1: every trajectory's single state, the same bits as the states have inside the table's launch."""
    case = dr.case_by_name("mixed_loop")
    p = dr.case_states(case)
    emu = _emu(case.name)
    whole = emu.dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], case.ridge)
    s = 4
    flat = emu.dynamics_inverse(p["Q"][:, s:s + 1], p["dQ"][:, s:s + 1], p["ddQ"][:, s:s + 1], case.ridge)
    for q in dr.FIELDS:
        assert np.array_equal(getattr(flat, q)[:, 0], getattr(whole, q)[:, s]), q


def test_status_singular_image_zeroes_the_answer_and_keeps_tau_and_acc():
    """An acceleration that is not a number makes that state's image unsolvable: TG_SINGULAR there, with U, lam and rho zero and tau
    and acc still written; every other state of the call keeps its bits."""
    case = dr.case_by_name("scissor4")
    p = dr.case_states(case)
    good = _run(case)
    ddQ = p["ddQ"].copy()
    b, s = 2, 6
    ddQ[b, s, 1] = np.nan
    got = _emu(case.name).dynamics_inverse(p["Q"], p["dQ"], ddQ)
    hit = np.zeros(got.status.shape, dtype=bool)
    hit[b, s] = True
    assert (got.status[hit] == dr.SINGULAR).all() and (got.status[~hit] == dr.OK).all()
    for q in ("U", "lam", "rho"):
        assert not getattr(got, q)[hit].any(), q
    for q in dr.FIELDS:
        assert np.array_equal(getattr(got, q)[~hit], getattr(good, q)[~hit]), q
    assert np.isnan(got.tau[b, s]).any() and np.isnan(got.acc[b, s]).any()


def test_nothing_to_solve_returns_the_residual():
    """nu + nc == 0: rho = r0 = -tau, TG_OK, and nothing else is written."""
    for name in ("pendulum5", "damper_link"):
        _, d = common.build(name)
        assert d.n_inputs + d.n_constraints == 0
        Q, dQ, ddQ = dr.draw_states(name, 2, 3, 0)
        ref = dr.dynamics_inverse(d, Q, dQ, ddQ)
        got = emu_dyn_inverse_harness.EmuDynInverse(d).dynamics_inverse(Q, dQ, ddQ)
        assert (got.status == dr.OK).all()
        assert np.array_equal(got.rho, -got.tau)
        assert np.abs(got.rho - ref.rho).max() <= dr.TOL_DIRECT * max(1.0, np.abs(ref.rho).max())
        assert np.abs(ref.rho).min() > 1e-6
        assert got.U.size == 0 and got.lam.size == 0 and got.acc.size == 0


def test_accelerations_that_dynamics_returned_are_consistent():
    """ddq = dynamics(q, dq, u, ddq_k) of the oracle: the kernel returns that u and lambda, rho = 0 and acc = 0 (the round trip the
    device test makes through the forward kernel)."""
    case = dr.case_by_name("wrench_torque")
    p = dr.case_states(case)
    d = p["d"]
    nd, nu = int(d.n_dyn), int(d.n_inputs)
    o = OracleMVI(d)
    rng = np.random.default_rng(common.tb_seed("dynamics inverse round trip", case.name))
    U = rng.standard_normal((case.B, case.M, nu))
    ddQ, LAM = p["ddQ"].copy(), np.zeros((case.B, case.M, int(d.n_constraints)))
    for b in range(case.B):
        for s in range(case.M):
            ddQ[b, s, :nd], LAM[b, s] = o.dynamics(p["Q"][b, s], p["dQ"][b, s], U[b, s], ddQ[b, s, nd:])
    got = _emu(case.name).dynamics_inverse(p["Q"], p["dQ"], ddQ)
    ref = dr.dynamics_inverse(d, p["Q"], p["dQ"], ddQ)
    bd = dr.bound(ref)
    e_u, e_l = common.relerr(got.U, U), common.relerr(got.lam, LAM)
    e_rho, e_acc = float(np.abs(got.rho).max()) / max(1.0, np.abs(ref.tau).max()), float(np.abs(got.acc).max(initial=0.0))
    print("round trip: u %.3e lam %.3e rho %.3e acc %.3e bound %.3e sigma_min %.3e" % (e_u, e_l, e_rho, e_acc, bd, dr.sigma_min(ref)))
    assert max(e_u, e_l, e_rho) <= bd and e_acc <= dr.TOL_DIRECT


PAR_CASE = dr.case_by_name("puppet40")


def test_emulated_parameter_twin_matches_rebuilt_systems():
    import inverse_dynamics_reference as ir
    p = dr.case_states(PAR_CASE)
    rows = ir.parameter_rows(PAR_CASE.name, PAR_CASE.B)
    got = _emu(PAR_CASE.name).dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], rows=ir.parameter_table(PAR_CASE.name, rows), group=1)
    dr.compare(PAR_CASE, got, ref=dr.parameter_reference(PAR_CASE, rows), tag="parameter rows ")
    base = _run(PAR_CASE)
    for q in dr.FIELDS:                                         # row 0 holds the system's own values
        assert np.array_equal(getattr(got, q)[0], getattr(base, q)[0]), q
    assert np.abs(got.tau[1:] - base.tau[1:]).max() > 1e-3     # the other rows' masses ask for other forces
    assert np.array_equal(got.acc, base.acc)                    # constraints know no masses


# ---- 5. the C entry points without a device -------------------------------------------------------------------------------------------
def _host(L, b, n_states, Q, dQ, ddQ, ridge):
    return L.tg_batch_dynamics_inverse(b, n_states, Q, dQ, ddQ, ridge, None, None, None, None, None, None)


def _device(L, b, n_states, Q, dQ, ddQ, ridge, stride=8):
    return L.tg_batch_dynamics_inverse_device(b, n_states, Q, stride, dQ, stride, ddQ, stride, ridge, None, None, None, None, None, None)


def test_null_handles_are_refused():
    L = _lib.lib()
    p = np.zeros(64).ctypes.data
    assert _host(L, None, 1, p, p, p, 0.0) == ERR_INVALID and L.tg_last_error() == b"null argument"
    assert _device(L, None, 1, p, p, p, 0.0) == ERR_INVALID and L.tg_last_error() == b"null argument"
    assert L.tg_system_dynamics_inverse_lds(None, None) == ERR_INVALID and L.tg_last_error() == b"null argument"


@pytest.mark.parametrize("call", (_host, _device), ids=("host", "device"))
def test_bad_arguments_are_refused_before_a_device_is_touched(call):
    """Every refusal the arguments alone show is decided before the batch is looked at (n > nd without a ridge and the short strides
    need a batch on a device: test_gpu_dynamics_inverse.py)."""
    L = _lib.lib()
    batch = ctypes.create_string_buffer(1 << 20)
    q = np.zeros(64)
    b, p = ctypes.addressof(batch), q.ctypes.data
    for n_states, Q, dQ, ddQ, ridge, message in (
            (1, p, p, p, -1e-6, b"ridge must be finite and not negative"),
            (1, p, p, p, float("nan"), b"ridge must be finite and not negative"),
            (1, p, p, p, float("inf"), b"ridge must be finite and not negative"),
            (0, p, p, p, 0.0, b"n_states must be at least 1"),
            (-3, p, p, p, 0.0, b"n_states must be at least 1"),
            (1, None, p, p, 0.0, b"null Q"),
            (1, p, None, p, 0.0, b"null dQ"),
            (1, p, p, None, 0.0, b"null ddQ")):
        assert call(L, b, n_states, Q, dQ, ddQ, ridge) == ERR_INVALID
        assert L.tg_last_error() == message


LDS_CELLS = [(n, t) for n in ("pendulum1", "pend_on_cart", "wrench_arm", "scissor4", "puppet_forces", "puppet40") for t in (1, 4, 16, 64)]


def lds_doubles(rollout, nq, nd, nu, nc):
    """Per team: the rollout slice, the image [m][m + 1] (m = nd + nu + nc), the accelerations [nq] and the solver's row scales [m]."""
    even = lambda x: (x + 1) & ~1
    m = nd + nu + nc
    return even(even(rollout) + m * (m + 1) + nq + m)


@pytest.mark.parametrize("name,team", LDS_CELLS)
def test_lds_of_a_workgroup_and_its_refusal(monkeypatch, name, team):
    monkeypatch.setenv("TREPAMD_TEAM", str(team))
    L = _lib.lib()
    d = common.build(name)[1]
    nq, nd, nu, nc = int(d.n_configs), int(d.n_dyn), int(d.n_inputs), int(d.n_constraints)
    slice_, rollout, o_kkt, o_ddq, o_scal = emu_dyn_inverse_harness.EmuDynInverse(d).lds_doubles()
    assert rollout == emu_harness.lds_slices(d)["rollout"]
    assert slice_ == lds_doubles(rollout, nq, nd, nu, nc)
    m = nd + nu + nc
    assert o_kkt >= rollout and o_ddq == o_kkt + m * (m + 1) and o_scal == o_ddq + nq and o_scal + m <= slice_
    sys_h = L.tg_system_create(d.byref())
    assert sys_h
    try:
        out = np.zeros(4, dtype=np.int32)
        rc = L.tg_system_dynamics_inverse_lds(sys_h, out.ctypes.data_as(_lib._c_ip))
        bytes_ = (64 // team) * slice_ * 8
        assert list(out) == [team, slice_, bytes_, 0]
        if bytes_ > 160 * 1024:
            assert rc == ERR_UNSUPPORTED and L.tg_last_error() == b"system too large for the LDS-resident computed-torque kernel"
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
        seen.add(L.tg_system_dynamics_inverse_lds(sys_h, out.ctypes.data_as(_lib._c_ip)))
        L.tg_system_destroy(sys_h)
    assert seen == {0, ERR_UNSUPPORTED}


def test_the_new_entry_points_are_exported_and_declared():
    names = set(_lib.exported_symbols())
    assert {"tg_batch_dynamics_inverse", "tg_batch_dynamics_inverse_device", "tg_system_dynamics_inverse_lds"} <= names
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "trep_amd.h")).read()
    L = _lib.lib()
    for n in _lib._DYN_INVERSE_SIGNATURES:
        assert "int %s(" % n in header
        assert getattr(L, n)


def test_the_python_call_is_there():
    from trep_amd import BatchMidpointVI
    from trep_amd.midpointvi import DynamicsInverse
    assert DynamicsInverse._fields == ("U", "lam", "rho", "tau", "acc", "status")
    assert callable(BatchMidpointVI.dynamics_inverse) and callable(BatchMidpointVI.dynamics_inverse_device)


def test_parity_profile_covers_the_table():
    """The committed record names every case of the table and is consistent with itself; it recomputes neither a floor nor an error.
    The parity check proper is test_emulated_kernel_over_the_table."""
    import json
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dynamics_inverse_parity.json")
    with open(path) as f:
        prof = json.load(f)
    assert sorted(prof["cases"]) == sorted(CASE_IDS)
    for cid, row in prof["cases"].items():
        assert row["bound"] == max(dr.TOL, dr.MARGIN * max(row["floor_z"], row["floor_rho"])) and row["bound_direct"] == dr.TOL_DIRECT
        for errors in (row["emulation_error"], row["device_error"]):
            if errors is not None:
                assert max(errors["z"], errors["rho"]) <= row["bound"] and max(errors["tau"], errors["acc"]) <= row["bound_direct"]
