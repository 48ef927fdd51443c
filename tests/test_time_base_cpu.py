"""The non-uniform time base (tg_batch_set_step_sizes) without a GPU: conditions on the case table of common.py that keep the device
tests (test_gpu_time_base.py) honest -- checked with the oracle alone -- and the generic kernel source under emulation (TEAM = 1) over
the same table.

The conditions are no measurements of any kernel: a wrong time base must be far from the right one in the reference itself
(otherwise a device test that passes says nothing), one unit in the last place of the start must stay below the tolerances (otherwise
a device test fails for no fault of the kernel), and the closed loops' feedback must do something without blowing up."""
import numpy as np
import pytest

from common import (D1, TB_CASES, TB_CLOSED_LOOP, TB_DT, TB_GROUP, TB_HORIZON, TB_N, TB_PREDICTOR_SYSTEMS, TB_PREDICTOR_TOL, TB_SECOND_TERM, TB_SYSTEMS, TB_TOL, build, relerr,
                    tb_batch, tb_bound, tb_case, tb_closed_loop_inputs, tb_closed_loop_reference, tb_e_ref, tb_horizon,
                    tb_oracle_rollout, tb_predictor_reference, tb_reference, tb_step_sizes, tb_wrong_step_sizes)
from emu_harness import EmuBatch

LOOP_CASES = [(n, p) for n, p in TB_CASES if n in TB_CLOSED_LOOP]
HORIZON_SYSTEMS = ("pend_on_cart", "scissor4", "spring_arm", "puppet40")
EMU_TOL = 1e-10                        # the emulation tests' tolerance (test_kernel_emulation.py)
EMU_B = 3                              # trajectories the emulation runs of a case
SLOW = ("puppet40", "puppet_basic", "puppet_forces")


def test_table_teams_are_the_librarys():
    """The team in TB_SYSTEMS (it sets the batch size: one full block and a ragged one) is the one the library picks."""
    from trep_amd import _lib
    L = _lib.lib()
    for name, (team, _, _) in TB_SYSTEMS.items():
        _, d = build(name)
        h = L.tg_system_create(d.byref())
        assert h
        out = np.zeros(8, dtype=np.int32)
        _lib.check(L.tg_system_info(h, out.ctypes.data_as(_lib._c_ip)))
        L.tg_system_destroy(h)
        assert int(out[0]) == team, (name, int(out[0]))
        assert tb_batch(name) == max(2 * (64 // team) + 1, 5)


@pytest.mark.parametrize("pattern", ["alternating", "random"])
def test_step_size_patterns(pattern):
    dts = tb_step_sizes(pattern, TB_N, "x")
    assert dts.shape == (TB_N,) and dts.min() >= 0.6 * TB_DT and dts.max() <= 1.5 * TB_DT
    assert np.array_equal(dts, tb_step_sizes(pattern, TB_N, "x"))
    if pattern == "alternating":
        assert np.allclose(dts[::2], 0.6 * TB_DT) and np.allclose(dts[1::2], 1.5 * TB_DT)
    for wrong in tb_wrong_step_sizes(dts).values():
        assert np.abs(wrong - dts).max() > 0.1 * TB_DT


@pytest.mark.parametrize("name,pattern", TB_CASES)
def test_wrong_time_bases_are_told_apart(name, pattern):
    """The oracle on a uniform grid of the mean step, on the list shifted one step forward and one step back is at least 1e-4 from
    the oracle on the right list, for every trajectory: six decades above the tolerance a device run is held to."""
    c = tb_case(name, pattern)
    ref = tb_reference(name, pattern)
    for kind, dts in tb_wrong_step_sizes(c["dts"]).items():
        for b in range(c["B"]):
            wrong = tb_oracle_rollout(c["d"], c["Q0"][b], c["Q1"][b], dts, c["U"][b], c["K"][b])
            assert relerr(wrong["X"], ref[b]["X"]) >= 1e-4, (name, pattern, kind, b)


def _check_floor(name, pattern, e_ref):
    for q, e in e_ref.items():
        print("%s %s e_ref(%s) = %.2e, bound %.2e" % (name, pattern, q, e, tb_bound(q, e_ref)))
        if (name, q) in TB_SECOND_TERM:
            assert 64.0 * e < 10.0 * TB_TOL[q], (name, pattern, q, e)       # the second term, but no blank cheque
        else:
            assert 64.0 * e <= TB_TOL[q], (name, pattern, q, e)             # the bound is the project's tolerance itself


@pytest.mark.parametrize("name,pattern", TB_CASES)
def test_one_ulp_of_the_start_stays_under_the_tolerances(name, pattern):
    """Conditioning: with (q0, q1) one unit in the last place off, the oracle's X, p1, p2, lambda1 and the derivatives of its last step stay
    within e_ref; 64 e_ref is below the project's tolerance for every quantity but the ones in TB_SECOND_TERM."""
    _check_floor(name, pattern, tb_e_ref(name, pattern))


@pytest.mark.parametrize("name,pattern", LOOP_CASES)
def test_closed_loop_inputs(name, pattern):
    """Shapes; row 0 of bX exact and the others moved; every oracle step of the loop converges (tb_oracle_rollout raises otherwise); the
    feedback moves X by 1e-6 .. 1e-2 against the gain-free run; U inherits X's tolerance (gain rows below one); conditioning."""
    c = tb_case(name, pattern)
    d, B, N = c["d"], c["B"], c["N"]
    nX, nU = d.n_configs + d.n_dyn + d.n_kin, d.n_inputs + d.n_kin
    Kp, bX, bU = tb_closed_loop_inputs(name, pattern)
    assert Kp.shape == ((B + TB_GROUP - 1) // TB_GROUP, N, nU, nX) and bX.shape == (B, N + 1, nX) and bU.shape == (B, N, nU)
    assert np.abs(Kp).sum(axis=-1).max() <= 1.0 + 2 * TB_DT
    open_loop = tb_reference(name, pattern)
    loop = tb_closed_loop_reference(name, pattern)
    for b in range(B):
        assert np.array_equal(bX[b, 0], open_loop[b]["X"][0]) and np.array_equal(loop[b]["X"][0], bX[b, 0])
        assert np.abs(bX[b, 1:] - open_loop[b]["X"][1:]).min() > 0.0
        assert np.array_equal(loop[b]["U"][0], bU[b, 0])                                   # no correction at k = 0
        moved = relerr(loop[b]["X"], open_loop[b]["X"])
        assert 1e-6 <= moved <= 1e-2, (name, pattern, b, moved)
    _check_floor(name, pattern, tb_e_ref(name, pattern, closed_loop=True))


# ---- the generic kernel source under emulation over the same table ---------------------------------------------------------------------
def _emu_shape(name):
    """(steps, trajectories): the puppets' emulation is slow, they run a shorter horizon (a case of its own, with its own reference)."""
    return (8 if name in SLOW else TB_N), EMU_B


def _emu_start(c, B):
    e = EmuBatch(c["d"], B)
    e.initialize_from_configs(0.0, c["Q0"][:B], TB_DT, c["Q1"][:B])
    return e


@pytest.mark.parametrize("name,pattern", TB_CASES)
def test_emulated_rollout_and_derivatives_on_the_table(name, pattern):
    """Open loop by step, then the non-rollout modes on the times the rollout left (t2 - t1 = the last step's size): X with its v rows,
    p1, p2, lambda1, iteration totals, deriv1, A / B with the -+1/dt entries of the v rows, deriv2z."""
    N, B = _emu_shape(name)
    c = tb_case(name, pattern, N, B)
    ref = tb_reference(name, pattern, N, B)
    d, dts = c["d"], c["dts"]
    nq, nd, nk, nu = d.n_configs, d.n_dyn, d.n_kin, d.n_inputs
    e = _emu_start(c, B)
    X = e.rollout(N, dts[0], c["U"] if nu else None, c["K"] if nk else None, dts=dts)
    assert (e.status == 0).all()
    t = tp = TB_DT
    for k in range(N):
        tp, t = t, t + dts[k]
    assert (e.t1, e.t2) == (tp, t)
    from common import tb_contraction
    Z, ZL = tb_contraction(name, B)
    d1 = e.deriv1()
    A, Bm = e.linearize()
    HZ = e.deriv2z(Z, ZL if d.n_constraints else None)
    for b in range(B):
        r = ref[b]
        assert relerr(X[b], r["X"]) < EMU_TOL, (name, pattern, b, relerr(X[b], r["X"]))
        assert relerr(e.p1[b], r["p1"]) < EMU_TOL and relerr(e.p2[b], r["p2"]) < EMU_TOL
        assert abs(int(e.iters[b]) - r["iterations"]) <= 1
        if int(e.iters[b]) == r["iterations"]:
            assert relerr(e.lam[b], r["lambda1"]) < tb_bound("lambda1", tb_e_ref(name, pattern, N, B)), (name, pattern, b)
        for n in D1:
            assert relerr(d1[n][b], r["d1"][n]) < 1e-9, (name, pattern, b, n)
        assert relerr(A[b], r["A"]) < 1e-9 and relerr(Bm[b], r["B"]) < 1e-9, (name, pattern, b)
        if nk:      # the v rows explicitly: -1/dt on Qk in A, +1/dt on rho in B, with the LAST step's size
            v = slice(nq + nd, nq + nd + nk)
            assert np.allclose(A[b][v, nd:nq], -np.eye(nk) / dts[N - 1], rtol=1e-12, atol=0.0)
            assert np.allclose(Bm[b][v, nu:], np.eye(nk) / dts[N - 1], rtol=1e-12, atol=0.0)
        assert relerr(HZ[b], r["hz"]) < 1e-8, (name, pattern, b)


@pytest.mark.parametrize("pattern", ["alternating", "random"])
@pytest.mark.parametrize("name", TB_PREDICTOR_SYSTEMS)
def test_emulated_extrapolating_predictor_follows_the_step_ratio(name, pattern):
    """Constant velocity on a non-uniform grid is q2 + (q2 - q1) dt_k / dt_{k-1}.  Without the ratio the warm start is off by a factor
    0.4 or 2.5 on the alternating list and saves nothing there; with it no trajectory takes more iterations than the plain run and the
    batch takes fewer.  Both runs against the oracle at X's tolerance, all three at the solver tolerance TB_PREDICTOR_TOL (common.py
    says why)."""
    N, B = _emu_shape(name)
    c = tb_case(name, pattern, N, B)
    ref = tb_predictor_reference(name, pattern, N, B)        # (converges on every step, or this raises)
    d = c["d"]
    runs = {}
    for predictor in (0, 1):
        e = EmuBatch(d, B, tolerance=TB_PREDICTOR_TOL)
        e.initialize_from_configs(0.0, c["Q0"][:B], TB_DT, c["Q1"][:B])
        e.predictor = predictor
        X = e.rollout(N, c["dts"][0], c["U"] if d.n_inputs else None, c["K"] if d.n_kin else None, dts=c["dts"])
        assert (e.status == 0).all()
        for b in range(B):
            assert relerr(X[b], ref[b]["X"]) < EMU_TOL, (name, pattern, predictor, b, relerr(X[b], ref[b]["X"]))
        runs[predictor] = e.iters.copy()
    for b in range(B):
        assert abs(int(runs[0][b]) - ref[b]["iterations"]) <= 1
    assert (runs[1] <= runs[0]).all(), (name, pattern, runs[1], runs[0])
    assert runs[1].sum() < runs[0].sum(), (name, pattern, runs[1], runs[0])


def test_feedback_paths_of_the_closed_loop_systems():
    """The closed-loop cases are there for both feedback paths of the rollout kernel: the puppets (team 64) must meet the condition of
    the wave-spread path, the small-team systems must not.  A schedule change that moves a case to the other path fails here."""
    from common import tb_wave_spread_feedback
    from trep_amd import _lib
    L = _lib.lib()
    want = {"puppet40": True, "puppet_forces": True, "pend_on_cart": False, "wrench_arm": False, "spring_arm": False}
    assert set(want) == set(TB_CLOSED_LOOP)
    for name, spread in want.items():
        _, d = build(name)
        h = L.tg_system_create(d.byref())
        out = np.zeros(8, dtype=np.int32)
        _lib.check(L.tg_system_info(h, out.ctypes.data_as(_lib._c_ip)))
        L.tg_system_destroy(h)
        assert int(out[0]) == TB_SYSTEMS[name][0]
        assert tb_wave_spread_feedback(d, int(out[0]), int(out[5])) == spread, (name, out)


@pytest.mark.parametrize("name,pattern", LOOP_CASES)
def test_emulated_closed_loop_on_the_table(name, pattern):
    """rollout_closed_loop(dts=): the per-row feedback path (the wave-spread one is device code) with v = (k2 - k1) / dt_{k-1}."""
    N, B = _emu_shape(name)
    c = tb_case(name, pattern, N, B)
    Kp, bX, bU = tb_closed_loop_inputs(name, pattern, N, B)
    ref = tb_closed_loop_reference(name, pattern, N, B)
    e = _emu_start(c, B)
    X, U = e.rollout_closed_loop(N, c["dts"][0], Kp, bX, bU, group_size=TB_GROUP, dts=c["dts"])
    assert (e.status == 0).all()
    for b in range(B):
        assert relerr(X[b], ref[b]["X"]) < EMU_TOL, (name, pattern, b, relerr(X[b], ref[b]["X"]))
        assert relerr(U[b], ref[b]["U"]) < EMU_TOL, (name, pattern, b)


@pytest.mark.parametrize("name", HORIZON_SYSTEMS)
@pytest.mark.parametrize("pattern", ["alternating", "random"])
def test_emulated_one_step_per_trajectory(name, pattern):
    """RunArgs.dt_period: trajectory (s, k) of a horizon batch steps by dts[k], and deriv1 / linearize / deriv2z carry that size."""
    h = tb_horizon(name, pattern)
    S, H = TB_HORIZON
    d, X, U, dts, refs = h["d"], h["X"], h["U"], h["dts"], h["refs"]
    nq, nd, nk, nu = d.n_configs, d.n_dyn, d.n_kin, d.n_inputs
    B = S * H
    e = EmuBatch(d, B)
    x0 = X[:, :H].reshape(B, -1)
    e.q1[:], e.q2[:], e.p1[:], e.p2[:] = x0[:, :nq], x0[:, :nq], x0[:, nq:nq + nd], x0[:, nq:nq + nd]
    u = U.reshape(B, 1, -1)
    e.set_step_sizes(dts)
    hint = np.ascontiguousarray(X[:, 1:, :nd].reshape(B, nd))
    e.rollout(1, 0.5 * TB_DT, np.ascontiguousarray(u[:, :, :nu]) if nu else None, np.ascontiguousarray(u[:, :, nu:]) if nk else None,
              want_X=False, q2_hint=hint)                                # (a scalar dt that is nobody's: the list must win)
    assert (e.status == 0).all()
    e.t1, e.t2 = 0.0, 0.5 * TB_DT
    d1 = e.deriv1()
    A, Bm = e.linearize()
    HZ = e.deriv2z(h["Z"])
    for t, r in enumerate(refs):
        assert relerr(e.q2[t], r["q2"]) < EMU_TOL and relerr(e.p2[t], r["p2"]) < EMU_TOL, (name, pattern, t)
        for n in D1:
            assert relerr(d1[n][t], r["d1"][n]) < 1e-9, (name, pattern, t, n)
        assert relerr(A[t], r["A"]) < 1e-9 and relerr(Bm[t], r["B"]) < 1e-9, (name, pattern, t)
        if nk:
            v = slice(nq + nd, nq + nd + nk)
            assert np.allclose(A[t][v, nd:nq], -np.eye(nk) / dts[t % H], rtol=1e-12, atol=0.0)
            assert np.allclose(Bm[t][v, nu:], np.eye(nk) / dts[t % H], rtol=1e-12, atol=0.0)
        assert relerr(HZ[t], r["hz"]) < 1e-8, (name, pattern, t)
