"""Batched inverse dynamics without a device: the numpy specification (inverse_dynamics_reference.py) against what the oracle's own
rollouts applied, the round trip through the oracle, the mutations the table must catch, the kernel itself (mvi_inverse.hpp)
compiled for the host with TEAM = 1 (emu_invdyn_harness.py) over the whole table, its parameter-table twin, the strided read, the
status cases, and the refusals and LDS geometry of the C entry points.

Measured here (tools/inverse_dynamics_parity.py writes the per-case floors and errors to profiles/inverse_dynamics_parity.json):
  recovery of the applied impulses on clean oracle rollouts, over the ridge-free table: worst |z - z_applied| 9.5e-11, at most
  0.47 of the derived per-step bound 2 tolerance / sigma_min(A~) (pend_on_cart); |rho| <= 3.7e-11 (scissor4);
  round trip Q -> (P_0, U) -> oracle rollout -> Q, worst over the table: 1.0e-11 over 13 steps (spatial_loop), 6.4e-13 on scissor4,
  1.5e-12 on pend_on_cart.  Its bound, 2.3e-9, is 64 x the largest figure measured when the method was first tried (3.6e-11 over 24
  steps): a margin for other seeds and horizons;
  the mutated specifications miss by 5.9e6 bounds at the least (Dh at Q_{k+1} on puppet40), 1e9 and more elsewhere."""
import ctypes
import os

import numpy as np
import pytest

import common
import emu_harness
import emu_invdyn_harness
import inverse_dynamics_reference as ir
from oracle.oracle import OracleMVI
from trep_amd import _lib

CASE_IDS = [ir.case_id(c) for c in ir.CASES]
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
FEASIBLE = [c for c in ir.CASES if c.ridge == 0.0]
ROUND_TRIP_BOUND = 2.3e-9


def _emu(name):
    return emu_invdyn_harness.EmuInverse(common.build(name)[1])


def _dt(c):
    return ir.step_sizes(c) if c.pattern != "uniform" else ir.DT


def _clean_reference(c, with_p0):
    p = ir.case_paths(c)
    return ir.inverse_dynamics(p["d"], p["Q_clean"], p["dts"], p["p0"] if with_p0 else None, c.ridge)


# ---- 1. the specification recovers what the oracle's rollouts applied ---------------------------------------------------------
@pytest.mark.parametrize("case", FEASIBLE, ids=[ir.case_id(c) for c in FEASIBLE])
def test_reference_recovers_applied_inputs_and_multipliers(case):
    """The oracle accepts a step when |f|_2 <= tolerance, f = r0 + A~ z_applied.  The least-squares z has |rho|_2 <= |f|_2, so
    |A~ (z - z_applied)|_2 <= 2 tolerance and |z - z_applied| <= 2 tolerance / sigma_min(A~), step by step; and |rho| <= tolerance."""
    p = ir.case_paths(case)
    nu = int(p["d"].n_inputs)
    ref = _clean_reference(case, True)
    applied = ir.impulses(nu, p["U"], p["lam"], p["dts"])
    worst = margin = 0.0
    for b in range(case.B):
        for k in range(case.N):
            if applied.shape[2] == 0:
                continue
            smin = np.linalg.svd(ref.A[b, k], compute_uv=False).min()
            miss = float(np.linalg.norm(ref.z[b, k] - applied[b, k]))
            worst, margin = max(worst, miss), max(margin, miss / (2 * ir.TOL / smin))
            assert miss <= 2 * ir.TOL / smin, (b, k, miss, smin)
    rho = float(np.abs(ref.rho).max())
    print(ir.case_id(case), "worst |z - z_applied| %.3e, largest share of its bound %.3f, |rho|inf %.3e" % (worst, margin, rho))
    assert rho <= 1e-9


# ---- 2. round trip through the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FEASIBLE, ids=[ir.case_id(c) for c in FEASIBLE])
def test_round_trip_through_the_oracle_retraces_the_path(case):
    """Without p0: initialize_from_state(t_0, Q_0, P_0), then steps with the recovered U and the path's own kinematic configs."""
    p = ir.case_paths(case)
    d, Q, dts = p["d"], p["Q_clean"], p["dts"]
    nd = int(d.n_dyn)
    ref = _clean_reference(case, False)
    worst = 0.0
    for b in range(case.B):
        o = OracleMVI(d)
        o.initialize_from_state(0.0, Q[b, 0], ref.P[b, 0])
        for k in range(case.N):
            o.step(o.times()[1] + dts[k], ref.U[b, k], Q[b, k + 1, nd:])
            worst = max(worst, float(np.abs(o.q2 - Q[b, k + 1]).max()))
    print(ir.case_id(case), "round trip: worst |Q - Q_again| %.3e over %d steps" % (worst, case.N))
    assert worst <= ROUND_TRIP_BOUND


# ---- 3. mutated references ----------------------------------------------------------------------------------------------------
# mutant -> the table rows that reach its ingredient and must miss by more than 100 bounds
MUTANT_ROWS = {
    "dh_at_next": ("scissor4_5x13", "spatial_loop_5x13", "puppet40_3x5"),          # Dh(Q_{k+1}) in place of Dh(Q_k): rows with constraints
    "p_from_same_pair": ("pend_on_cart_5x13", "wrench_arm_5x13", "scissor4_5x13_alternating"),     # p_k from pair k: any row
    "dt_twice": ("pend_on_cart_5x13", "wrench_arm_5x13", "wrench_torque_5x13"),    # dt F_du in place of F_du: rows with inputs
}


@pytest.mark.parametrize("mutant", sorted(MUTANT_ROWS))
def test_mutation_misses_the_table(mutant):
    by_id = dict((ir.case_id(c), c) for c in ir.CASES)
    for cid in MUTANT_ROWS[mutant]:
        c = by_id[cid]
        p = ir.case_paths(c)
        ref = ir.case_reference(c, True)
        got = ir.inverse_dynamics(p["d"], p["Q"], p["dts"], p["p0"], c.ridge, spec=dict(ir.SPEC, **{mutant: True}))
        e = ir.errors(c, ref, got)
        worst = max(e.values())
        print(mutant, cid, "misses by %.3e = %.0f bounds" % (worst, worst / ir.bound(ref)))
        assert worst > 100 * ir.bound(ref), (mutant, cid, e)


# ---- 4. the emulated kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_p0", (True, False), ids=("p0", "no_p0"))
@pytest.mark.parametrize("case", ir.CASES, ids=CASE_IDS)
def test_emulated_kernel_over_the_table(case, with_p0):
    p = ir.case_paths(case)
    got = _emu(case.name).inverse_dynamics(p["Q"], _dt(case), p["p0"] if with_p0 else None, case.ridge)
    ir.compare(case, with_p0, got)
    if not with_p0:
        for q in ("U", "lam", "rho"):
            assert not getattr(got, q)[:, 0].any(), q
        assert (got.status == ir.OK).all()


def test_emulated_kernel_does_not_depend_on_what_the_scratch_held():
    case = ir.CASES[1]
    p = ir.case_paths(case)
    emu = _emu(case.name)
    a, b = emu.inverse_dynamics(p["Q"], ir.DT, p["p0"], poison=True), emu.inverse_dynamics(p["Q"], ir.DT, p["p0"], poison=False)
    for q in ir.FIELDS:
        assert np.array_equal(getattr(a, q), getattr(b, q)), q


def test_emulated_step_does_not_depend_on_its_launch():
    """(b, k) alone in a B = 1, N = 1 call, and twice in one call: the same bits."""
    case = [c for c in ir.CASES if c.name == "scissor4" and c.pattern == "alternating"][0]
    p = ir.case_paths(case)
    emu = _emu(case.name)
    Q, dts = p["Q"], p["dts"]
    whole = emu.inverse_dynamics(Q, dts, p["p0"])
    b, k = 3, 7
    one = emu.inverse_dynamics(Q[b:b + 1, k:k + 2], dts[k:k + 1], whole.P[b:b + 1, k])
    twice = emu.inverse_dynamics(np.array([Q[b], Q[b]]), dts, np.array([p["p0"][b], p["p0"][b]]))
    for q in ("U", "lam", "rho", "h"):
        assert np.array_equal(getattr(one, q)[0, 0], getattr(whole, q)[b, k]), q
        assert np.array_equal(getattr(twice, q)[0], getattr(whole, q)[b]) and np.array_equal(getattr(twice, q)[1], getattr(whole, q)[b]), q
    assert np.array_equal(one.P[0, 1], whole.P[b, k + 1])


def test_emulated_kernel_reads_a_strided_state_trajectory():
    """Q taken from X [B][N+1][nX] = [Q; P; v] with the row stride nX, as the device variant reads a rollout's X."""
    case = ir.CASES[1]
    p = ir.case_paths(case)
    d = p["d"]
    emu = _emu(case.name)
    packed = emu.inverse_dynamics(p["Q"], ir.DT, p["p0"])
    nX = int(d.n_configs + d.n_dyn + d.n_kin)
    X = np.full((case.B, case.N + 1, nX), np.nan)
    X[:, :, :int(d.n_configs)] = p["Q"]
    strided = emu.inverse_dynamics(X, ir.DT, p["p0"], stride=nX)
    for q in ir.FIELDS:
        assert np.array_equal(getattr(packed, q), getattr(strided, q)), q


def test_status_singular_image_zeroes_the_step_and_keeps_p_and_h():
    """A configuration that is not a number makes the images of the three steps that read it (through Q_k, Q_{k+1} or p_k) unsolvable:
    TG_SINGULAR there, with U, lam and rho zero and P and h still written; every other step of the call keeps its bits.  (An image
    that is singular by its shape alone, n > nd without a ridge, is not rejected reliably -- rounding leaves pivots over the guard --
    which is why the C entry points refuse that call.)"""
    case = [c for c in ir.CASES if c.name == "scissor4" and c.pattern == "uniform"][0]
    p = ir.case_paths(case)
    emu = _emu(case.name)
    good = emu.inverse_dynamics(p["Q"], ir.DT, p["p0"])
    Q = p["Q"].copy()
    b, k = 2, 6
    Q[b, k, 1] = np.nan
    got = emu.inverse_dynamics(Q, ir.DT, p["p0"])
    hit = np.zeros(got.status.shape, dtype=bool)
    hit[b, k - 1:k + 2] = True
    assert (got.status[hit] == ir.SINGULAR).all() and (got.status[~hit] == ir.OK).all()
    for q in ("U", "lam", "rho"):
        assert not getattr(got, q)[hit].any(), q
        assert np.array_equal(getattr(got, q)[~hit], getattr(good, q)[~hit]), q
    assert np.isnan(got.P[b, k]).any() and np.isnan(got.h[b, k - 1]).any()
    assert np.array_equal(got.h[~hit], good.h[~hit])


def test_nothing_to_solve_returns_the_residual():
    """nu + nc == 0: rho = r0, TG_OK; without p0 step 0 is force-free by the choice of P_0."""
    _, d = common.build("pendulum5")
    assert d.n_inputs + d.n_constraints == 0
    rng = np.random.default_rng(11)
    Q = np.cumsum(0.02 * rng.standard_normal((2, 4, int(d.n_configs))), axis=1)
    p0 = rng.standard_normal((2, int(d.n_dyn)))
    emu = emu_invdyn_harness.EmuInverse(d)
    for given in (p0, None):
        ref = ir.inverse_dynamics(d, Q, np.full(3, ir.DT), given)
        got = emu.inverse_dynamics(Q, ir.DT, given)
        assert (got.status == ir.OK).all()
        assert np.abs(got.rho - ref.rho).max() <= 1e-12 and np.abs(got.P - ref.P).max() <= 1e-12
        assert np.abs(ref.rho[:, 1:]).min() > 1e-6
    assert not got.rho[:, 0].any()


PAR_CASE = [c for c in ir.CASES if c.name == "puppet40"][0]


@pytest.mark.parametrize("with_p0", (True, False), ids=("p0", "no_p0"))
def test_emulated_parameter_twin_matches_rebuilt_systems(with_p0):
    p = ir.case_paths(PAR_CASE)
    rows = ir.parameter_rows(PAR_CASE.name, PAR_CASE.B)
    got = _emu(PAR_CASE.name).inverse_dynamics(p["Q"], ir.DT, p["p0"] if with_p0 else None, rows=ir.parameter_table(PAR_CASE.name, rows), group=1)
    ref = ir.parameter_reference(PAR_CASE, with_p0, rows)
    ir.compare(PAR_CASE, with_p0, got, ref=ref, tag="parameter rows ")
    base = _emu(PAR_CASE.name).inverse_dynamics(p["Q"], ir.DT, p["p0"] if with_p0 else None)
    for q in ir.FIELDS:                                         # row 0 holds the system's own values
        assert np.array_equal(getattr(got, q)[0], getattr(base, q)[0]), q
    assert np.abs(got.rho[1:]).max() > 1e-6                     # the path belongs to row 0's masses: the other rows cannot follow it


# ---- 5. the C entry points without a device -------------------------------------------------------------------------------------
def test_null_handles_are_refused():
    L = _lib.lib()
    assert L.tg_batch_inverse_dynamics(None, 1, 0.01, None, None, 0.0, None, None, None, None, None, None) == ERR_INVALID
    assert L.tg_last_error() == b"null argument"
    assert L.tg_batch_inverse_dynamics_device(None, 1, 0.01, None, 0, None, 0.0, None, None, None, None, None, None) == ERR_INVALID
    assert L.tg_last_error() == b"null argument"
    assert L.tg_system_inverse_dynamics_lds(None, None) == ERR_INVALID and L.tg_last_error() == b"null argument"


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_bad_scalars_are_refused_before_anything_is_staged(device):
    """Every refusal that needs no step-size list and no system: decided on the host from the arguments alone (the by-trajectory
    list, the short list and n > nd need a batch on a device: test_gpu_inverse_dynamics.py)."""
    L = _lib.lib()
    batch = ctypes.create_string_buffer(1 << 20)
    q = np.zeros(64)
    b, p = ctypes.addressof(batch), q.ctypes.data

    def call(n_steps, dt, Q, ridge):
        if device:
            return L.tg_batch_inverse_dynamics_device(b, n_steps, dt, Q, 8, None, ridge, None, None, None, None, None, None)
        return L.tg_batch_inverse_dynamics(b, n_steps, dt, Q, None, ridge, None, None, None, None, None, None)
    for n_steps, dt, Q, ridge, message in (
            (1, 0.01, None, 0.0, b"null argument"),
            (1, 0.01, p, -1e-6, b"ridge must be finite and not negative"),
            (1, 0.01, p, float("nan"), b"ridge must be finite and not negative"),
            (1, 0.01, p, float("inf"), b"ridge must be finite and not negative"),
            (0, 0.01, p, 0.0, b"n_steps must be at least 1"),
            (-3, 0.01, p, 0.0, b"n_steps must be at least 1"),
            (1, 0.0, p, 0.0, b"step size must be finite and not zero"),
            (1, float("nan"), p, 0.0, b"step size must be finite and not zero")):
        assert call(n_steps, dt, Q, ridge) == ERR_INVALID
        assert L.tg_last_error() == message


LDS_CELLS = [(n, t) for n in ("pendulum1", "pend_on_cart", "wrench_arm", "scissor4", "puppet_forces", "puppet40") for t in (1, 4, 16, 64)]


def lds_doubles(rollout, nd, nu, nc):
    """Per team: the rollout slice, the image [m][m + 1] (m = nd + nu + nc), p_k [nd] and the solver's row scales [m]."""
    even = lambda x: (x + 1) & ~1
    m = nd + nu + nc
    return even(even(rollout) + m * (m + 1) + nd + m)


@pytest.mark.parametrize("name,team", LDS_CELLS)
def test_lds_of_a_workgroup_and_its_refusal(monkeypatch, name, team):
    monkeypatch.setenv("TREPAMD_TEAM", str(team))
    L = _lib.lib()
    d = common.build(name)[1]
    slice_, rollout = emu_invdyn_harness.EmuInverse(d).lds_doubles()
    assert rollout == emu_harness.lds_slices(d)["rollout"]
    assert slice_ == lds_doubles(rollout, int(d.n_dyn), int(d.n_inputs), int(d.n_constraints))
    sys_h = L.tg_system_create(d.byref())
    assert sys_h
    try:
        out = np.zeros(4, dtype=np.int32)
        rc = L.tg_system_inverse_dynamics_lds(sys_h, out.ctypes.data_as(_lib._c_ip))
        bytes_ = (64 // team) * slice_ * 8
        assert list(out) == [team, slice_, bytes_, 0]
        if bytes_ > 160 * 1024:
            assert rc == ERR_UNSUPPORTED and L.tg_last_error() == b"system too large for the LDS-resident inverse-dynamics kernel"
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
        seen.add(L.tg_system_inverse_dynamics_lds(sys_h, out.ctypes.data_as(_lib._c_ip)))
        L.tg_system_destroy(sys_h)
    assert seen == {0, ERR_UNSUPPORTED}


def test_the_new_entry_points_are_exported_and_declared():
    names = set(_lib.exported_symbols())
    assert {"tg_batch_inverse_dynamics", "tg_batch_inverse_dynamics_device", "tg_system_inverse_dynamics_lds"} <= names
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "trep_amd.h")).read()
    for n in _lib._INVERSE_SIGNATURES:
        assert "int %s(" % n in header


def test_parity_profile_covers_the_table():
    """The committed record names every case of the table, with and without p0, and is consistent with itself; it recomputes
    neither a floor nor an error.  The parity check proper is test_emulated_kernel_over_the_table."""
    import json
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "inverse_dynamics_parity.json")
    with open(path) as f:
        prof = json.load(f)
    assert sorted(prof["cases"]) == sorted("%s_%s" % (cid, tag) for cid in CASE_IDS for tag in ("p0", "no_p0"))
    for cid, row in prof["cases"].items():
        assert row["bound"] == max(ir.TOL, ir.MARGIN * max(row["floor_z"], row["floor_rho"]))
        assert max(row["emulation_error"].values()) <= row["bound"]
        if row["device_error"] is not None:
            assert max(row["device_error"].values()) <= row["bound"]
