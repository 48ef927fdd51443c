"""The non-uniform time base (tg_batch_set_step_sizes) of every kernel against the oracle, on the case table of common.py.

Almost every kernel mode reads the step size (run_trajectory, csrc/mvi_core.hpp): the rollout loop per step (core.dt / core.inv_dt,
dt_prev for the feedback's v, the v rows of X), calc_p2, calc_f, deriv1 with the 1/dt entries of A_k / B_k, deriv2z.  By step: step k
of a rollout uses dt[k]; by trajectory: trajectory t of a one-step batch uses dt[t % count].  The reference is OracleMVI stepped with
o.step(o.times()[1] + dts[k], ...) (common.tb_oracle_rollout); the step-size patterns put the largest ratio the table allows between
neighbours, and test_time_base_cpu.py shows that a list that is off by one step, or its mean, is at least 1e-4 away in the reference
itself.  Bounds: the project's tolerances (common.TB_TOL), raised only through max(tolerance, 64 e_ref) with e_ref the reference's own
response to one ulp of the start (common.tb_e_ref) -- never through anything a kernel produced.  Nothing is compiled here: the
specialised kernels are the libraries build() made."""
import ctypes

import numpy as np
import pytest

from common import (BUILDERS, D1, TB_CLOSED_LOOP, TB_DT, TB_EXTRA, TB_GROUP, TB_HORIZON, TB_KINDS, TB_N, TB_PATTERNS, TB_PREDICTOR_SYSTEMS,
                    TB_PREDICTOR_TOL, TB_SYSTEMS, TB_TOL, build,
                    relerr, tb_AB, tb_batch, tb_bound, tb_case, tb_closed_loop_inputs, tb_closed_loop_reference, tb_contraction,
                    tb_e_ref, tb_horizon, tb_oracle_derivs, tb_oracle_rollout, tb_predictor_reference, tb_reference, tb_step_sizes)
from oracle.oracle import OracleMVI
from test_gpu_parity import _assert_kernels
from test_parameters_cpu import random_rows, rebuilt
from trep_amd import BatchMidpointVI, _lib, descriptor
from trep_amd._lib import LibraryError

pytestmark = pytest.mark.gpu

DT = TB_DT
EXTRA = TB_EXTRA                # steps of the second rollout; the list is that much longer than the first one
SPEC_MODES = ("rollout", "deriv1", "deriv2z")
KIND_IDS = ["%s-%s" % (n, "spec" if s else "generic") for n, s in TB_KINDS]


def _batch(monkeypatch, name, B, spec, system=None):
    """A batch on the generic kernels, or on the system's prebuilt specialised library ("auto" loads a cached library and never builds)."""
    monkeypatch.delenv("TREPAMD_TEAM", raising=False)
    monkeypatch.delenv("TREPAMD_NO_SPECIALIZE", raising=False)
    monkeypatch.delenv("TREPAMD_SPEC_OVERRIDE", raising=False)
    if system is None:
        system, _ = build(name)
    mvi = BatchMidpointVI(system, B, specialize="auto" if spec else False)
    info = mvi.kernel_info()
    assert info["team"] == TB_SYSTEMS[name][0], (name, info)
    assert (info["spec_library"] is not None) == bool(spec), (name, spec, info)
    return mvi


def _assert_kind(mvi, spec, modes):
    """The intended kind of kernel ran, and only it (per-trajectory parameter kernels: _assert_par)."""
    info = mvi.kernel_info()
    assert info["par_spec_launches"] == 0 and info["par_generic_launches"] == 0, info
    if spec:
        core = [m for m in modes if m in SPEC_MODES]
        _assert_kernels(info, True, core)
        assert not set(info["generic_launched"]) & set(info["spec_modes"]), info
    else:
        _assert_kernels(info, False, modes)
        assert info["spec_launches"] == 0 and not info["spec_launched"], info


def _summed(t2, dts):
    """(t1, t2) after stepping through dts from t2, summed in the library's order (advance_times)."""
    t = tp = t2
    for x in dts:
        tp, t = t, t + float(x)
    return tp, t


def _force(mvi, refs, key="o"):
    """Put the batch at exactly the oracles' last step (the times are the launch's own): the residual and the derivatives are then
    taken at the same point, as in test_gpu_team_sizes.py."""
    os_ = [r[key] for r in refs]
    mvi.q1, mvi.q2 = np.array([o.q1 for o in os_]), np.array([o.q2 for o in os_])
    mvi.p1, mvi.p2 = np.array([o.p1 for o in os_]), np.array([o.p2 for o in os_])
    if mvi.nu:
        mvi.u1 = np.array([o.u1 for o in os_])
    if mvi.nc:
        mvi.lambda1 = np.array([o.lambda1 for o in os_])


def _continued(d, r, dts, U, K):
    """The oracle of a cached reference run continued on a copy (the cached one stays as it is for the tests that share it)."""
    o, o2 = r["o"], OracleMVI(d)
    o2.set_times(*o.times())
    o2.q1, o2.q2, o2.p1, o2.p2, o2.u1, o2.lambda1 = o.q1, o.q2, o.p1, o.p2, o.u1, o.lambda1
    return tb_oracle_rollout(d, None, None, dts, U, K, o=o2)


def _in(c, key, n0, n1):
    a = c[key][:, n0:n1]
    return np.ascontiguousarray(a) if a.shape[2] else None


def _check_open_loop(tag, c, ref, e_ref, X, mvi, N, iters_ref=None):
    """X (with its v rows), status, iteration totals, p1 / p2 / lambda1 after the launch."""
    iters, status = mvi.status()
    assert (status == 0).all(), (tag, status)
    p1, p2, lam = mvi.p1, mvi.p2, mvi.lambda1
    worst = dict(X=0.0, p1=0.0, p2=0.0, lambda1=0.0)
    for b, r in enumerate(ref):
        for q, got in (("X", X[b]), ("p1", p1[b]), ("p2", p2[b])):
            e = relerr(got, r[q])
            worst[q] = max(worst[q], e)
            assert e < tb_bound(q, e_ref), (tag, q, b, e)
        want = r["iterations"] if iters_ref is None else iters_ref[b]
        assert abs(int(iters[b]) - want) <= 1, (tag, b, int(iters[b]), want)
        if mvi.nc and int(iters[b]) == want:
            e = relerr(lam[b], r["lambda1"])
            worst["lambda1"] = max(worst["lambda1"], e)
            assert e < tb_bound("lambda1", e_ref), (tag, "lambda1", b, e)
    print(tag, " ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    return worst


def run_open_loop(monkeypatch, name, spec, pattern, record=None):
    c = tb_case(name, pattern)
    d, B, N, dts = c["d"], c["B"], TB_N, c["dts_all"]
    nq, nd, nk, nc = d.n_configs, d.n_dyn, d.n_kin, d.n_constraints
    Z, ZL = tb_contraction(name, B)
    ref = tb_reference(name, pattern)
    e_ref = tb_e_ref(name, pattern)
    tag = "%s %s %s" % (name, "spec" if spec else "generic", pattern)
    mvi = _batch(monkeypatch, name, B, spec)
    # 1. a list longer than the rollout, set on the batch; the rollout itself is asked for with a scalar that is nobody's step
    mvi.set_step_sizes(dts)
    mvi.initialize_from_configs(0.0, c["Q0"], DT, c["Q1"])
    X = mvi.rollout(N, 0.77 * DT, _in(c, "U", 0, N), _in(c, "K", 0, N))
    worst = _check_open_loop(tag, c, ref, e_ref, X, mvi, N)
    assert mvi.times() == _summed(DT, dts[:N]), (tag, mvi.times())
    # the v rows explicitly: (k2 - k1) / dt_k with the step's own size
    if nk:
        for b in range(B):
            v = (X[b, 1:, nd:nq] - X[b, :-1, nd:nq]) / dts[:N, None]
            assert relerr(X[b, 1:, nq + nd:], v) < TB_TOL["X"], (tag, b)
    # 2. the residual of the device's own final state vanishes to the solver tolerance.  The residual the rollout held to it is its own
    # last Newton evaluation; calc_f evaluates the same state along another path, and each of the two is held to the f tolerance
    # against the oracle: that, twice, is all the slack there is
    f = mvi.calc_f()
    assert np.abs(f).max() < mvi.tolerance + 2.0 * TB_TOL["f"], (tag, np.abs(f).max())
    # 3. the non-rollout modes on the times the launch left: t2 - t1 is the last step's size (advance_times)
    _force(mvi, ref)
    f = mvi.calc_f()
    mvi.calc_p2()
    p2 = mvi.p2
    _force(mvi, ref)
    mvi.calc_deriv1()
    d1 = dict((n, mvi.deriv1(n)) for n in D1)
    HZ = mvi.deriv2_contract(Z, ZL if nc else None)
    for b, r in enumerate(ref):
        worst["f"] = max(worst.get("f", 0.0), relerr(f[b], r["f"]))
        assert relerr(f[b], r["f"]) < TB_TOL["f"], (tag, b)
        worst["calc_p2"] = max(worst.get("calc_p2", 0.0), relerr(p2[b], r["calc_p2"]))
        assert relerr(p2[b], r["calc_p2"]) < TB_TOL["calc_p2"], (tag, b, relerr(p2[b], r["calc_p2"]))
        e1 = max(relerr(d1[n][b], r["d1"][n]) for n in D1)
        worst["d1"] = max(worst.get("d1", 0.0), e1)
        assert e1 < tb_bound("d1", e_ref), (tag, b, e1)
        A, Bm = tb_AB(d, dict((n, d1[n][b]) for n in D1), mvi.times()[1] - mvi.times()[0])
        eab = max(relerr(A, r["A"]), relerr(Bm, r["B"]))
        worst["AB"] = max(worst.get("AB", 0.0), eab)
        assert eab < tb_bound("AB", e_ref), (tag, b, eab)
        eh = relerr(HZ[b], r["hz"])
        worst["hz"] = max(worst.get("hz", 0.0), eh)
        assert eh < tb_bound("hz", e_ref), (tag, b, eh)
    # 4. the sugar rollout(N, dts, ...) from the same start: the same launch, bit for bit, and the batch's own list is back afterwards
    mvi.initialize_from_configs(0.0, c["Q0"], DT, c["Q1"])
    X2 = mvi.rollout(N, dts[:N], _in(c, "U", 0, N), _in(c, "K", 0, N))
    assert np.array_equal(X2, X), tag
    assert mvi.times() == _summed(DT, dts[:N])
    # 5. a second rollout of the same batch starts again at dts[0]; so does the oracle
    X3 = mvi.rollout(EXTRA, 0.77 * DT, _in(c, "U_all", N, N + EXTRA), _in(c, "K_all", N, N + EXTRA))
    t_before = _summed(DT, dts[:N])[1]
    assert mvi.times() == _summed(t_before, dts[:EXTRA]), tag
    ref2 = [_continued(d, r, dts[:EXTRA], c["U_all"][b, N:], c["K_all"][b, N:]) for b, r in enumerate(ref)]
    _check_open_loop(tag + " second", c, ref2, e_ref, X3, mvi, EXTRA)
    _assert_kind(mvi, spec, ["rollout", "calc_p2", "calc_f", "deriv1", "deriv2z"])
    mvi.close()
    if record is not None:
        record(worst)
    return worst


@pytest.mark.parametrize("pattern", TB_PATTERNS)
@pytest.mark.parametrize("name,spec", TB_KINDS, ids=KIND_IDS)
def test_open_loop_rollout_by_step(monkeypatch, name, spec, pattern):
    """set_step_sizes(list longer than the rollout) + device rollout, the sugar rollout(N, dts, U, K), a second rollout of the same
    batch; X with its v rows, status, iteration totals, times(), p1 / p2 / lambda1, calc_f, calc_p2, deriv1, A / B, deriv2z."""
    run_open_loop(monkeypatch, name, spec, pattern)


PREDICTOR_KINDS = [(n, False) for n in TB_PREDICTOR_SYSTEMS] + [("puppet40", True)]


@pytest.mark.parametrize("pattern", TB_PATTERNS)
@pytest.mark.parametrize("name,spec", PREDICTOR_KINDS, ids=["%s-%s" % (n, "spec" if s else "generic") for n, s in PREDICTOR_KINDS])
def test_extrapolating_predictor_by_step(monkeypatch, name, spec, pattern):
    """predictor = "extrapolate" on a non-uniform grid (the warm start q2 + (q2 - q1) dt_k / dt_{k-1}): the same trajectory to X's
    tolerance, iteration totals not above the plain run's; unconstrained systems and a constrained one.  Plain run, extrapolated run
    and oracle all solve to TB_PREDICTOR_TOL: a warm start inside the tolerance ball is accepted as it is, so either run -- and the
    oracle -- is the exact trajectory only to the solver tolerance (common.py has the oracle's own figures at 1e-10)."""
    c = tb_case(name, pattern)
    ref = tb_predictor_reference(name, pattern)
    N = TB_N
    mvi = _batch(monkeypatch, name, c["B"], spec)
    mvi.tolerance = TB_PREDICTOR_TOL
    mvi.set_step_sizes(c["dts"])
    runs = {}
    for mode in ("reference", "extrapolate"):
        mvi.predictor = mode
        mvi.initialize_from_configs(0.0, c["Q0"], DT, c["Q1"])
        X = mvi.rollout(N, 0.77 * DT, _in(c, "U", 0, N), _in(c, "K", 0, N))
        iters, status = mvi.status()
        assert (status == 0).all(), (name, mode)
        errs = [relerr(X[b], r["X"]) for b, r in enumerate(ref)]
        print(name, pattern, mode, "X against the oracle %.2e" % max(errs), "iterations", iters.sum())
        assert max(errs) < TB_TOL["X"], (name, pattern, mode, errs)
        runs[mode] = iters
    for b, r in enumerate(ref):
        assert abs(int(runs["reference"][b]) - r["iterations"]) <= 1, (name, b)
    assert (runs["extrapolate"] <= runs["reference"]).all(), (name, runs["extrapolate"], runs["reference"])
    _assert_kind(mvi, spec, ["rollout", "calc_p2"])
    mvi.close()


# ---- closed loop, by step ---------------------------------------------------------------------------------------------------------------
# Which feedback path a case runs follows from the condition in run_trajectory: TEAM == 64 && 2 (nu + nk) <= 64 && nX <= 32 parts &&
# nX + 4 (nu + nk) <= 6 n_items spreads the gain rows over the wavefront (v from dt_prev in its dx pass).  puppet40 (nU = 18, nX = 80,
# parts = 3) and puppet_forces (nU = 18, nX = 44) have a team of 64 and meet it, generic and specialised; pend_on_cart (team 4),
# wrench_arm and spring_arm (team 16) fail TEAM == 64 and run the per-row loop (v from dtp = dt_prev).
# test_time_base_cpu.py::test_feedback_paths_of_the_closed_loop_systems holds the systems to this.
LOOP_KINDS = [(n, False) for n in TB_CLOSED_LOOP] + [("puppet40", True)]


def _device_ints(mvi, values):
    a = np.ascontiguousarray(values, dtype=np.int32)
    p = mvi.device_empty((a.nbytes + 7) // 8)
    _lib.check(_lib.lib().tg_memcpy_h2d(mvi.device, p, a.ctypes.data, a.nbytes))
    return p


def run_closed_loop(monkeypatch, name, spec, pattern, record=None):
    c = tb_case(name, pattern)
    d, B, N, dts = c["d"], c["B"], c["N"], c["dts"]
    nX, nU = d.n_configs + d.n_dyn + d.n_kin, d.n_inputs + d.n_kin
    Kp, bX, bU = tb_closed_loop_inputs(name, pattern)
    ref = tb_closed_loop_reference(name, pattern)
    e_ref = tb_e_ref(name, pattern, closed_loop=True)
    tag = "%s %s %s loop" % (name, "spec" if spec else "generic", pattern)
    mvi = _batch(monkeypatch, name, B, spec)
    mvi.set_step_sizes(dts)
    mvi.initialize_from_configs(0.0, c["Q0"], DT, c["Q1"])
    X, U = mvi.rollout_closed_loop(N, 0.77 * DT, Kp, bX, bU, group_size=TB_GROUP)
    iters, status = mvi.status()
    assert (status == 0).all(), (tag, status)
    assert mvi.times() == _summed(DT, dts), tag
    worst = dict(X=0.0, U=0.0)
    for b, r in enumerate(ref):
        ex, eu = relerr(X[b], r["X"]), relerr(U[b], r["U"])
        worst["X"], worst["U"] = max(worst["X"], ex), max(worst["U"], eu)
        assert ex < tb_bound("X", e_ref), (tag, b, ex)
        assert eu < tb_bound("U", e_ref), (tag, b, eu)
        assert abs(int(iters[b]) - r["iterations"]) <= 1, (tag, b)
    print(tag, "X %.2e U %.2e" % (worst["X"], worst["U"]))
    # the subset launch: the first n trajectories of the batch, gains through a group map that is no prefix of the groups -- launch slot
    # t holds trajectory perm[t] of the case (the last group may have one member: its slot mate is a copy)
    groups = Kp.shape[0]
    select = [groups - 1, 0] if groups < 4 else [groups - 1, 0, 2]
    perm = np.array([min(TB_GROUP * g + j, B - 1) for g in select for j in range(TB_GROUP)])
    n = len(perm)
    assert n < B
    fill = lambda a: np.concatenate([a[perm], a[n:]])
    mvi.initialize_from_configs(0.0, fill(c["Q0"]), DT, fill(c["Q1"]))
    dev = [mvi.device_array(a) for a in (Kp, fill(bX), fill(bU))]
    Xd, Ud = mvi.device_array(np.full((B, N + 1, nX), 7.0)), mvi.device_array(np.full((B, N, nU), 7.0))
    _lib.check(_lib.lib().tg_batch_rollout_closed_loop_subset(mvi._h, n, N, 0.77 * DT, dev[0], TB_GROUP, _device_ints(mvi, select), dev[1],
                                                              dev[2], Xd, Ud, 200))
    mvi.synchronize()
    Xs, Us = mvi.download(Xd, (B, N + 1, nX)), mvi.download(Ud, (B, N, nU))
    its, sts = mvi.status()
    assert (sts[:n] == 0).all(), (tag, sts)
    for t, b in enumerate(perm):
        assert relerr(Xs[t], ref[b]["X"]) < tb_bound("X", e_ref), (tag, "subset", t, b, relerr(Xs[t], ref[b]["X"]))
        assert relerr(Us[t], ref[b]["U"]) < tb_bound("U", e_ref), (tag, "subset", t, b)
        assert np.array_equal(Xs[t], X[b]) and np.array_equal(Us[t], U[b]), (tag, "subset", t, b)      # the same arithmetic as the full launch
    # (the rows behind the n trajectories of a subset launch are rows of the trajectory-major buffers: untouched)
    assert (Xs[n:] == 7.0).all() and (Us[n:] == 7.0).all(), tag
    _assert_kind(mvi, spec, ["rollout", "calc_p2"])
    mvi.close()
    if record is not None:
        record(worst)
    return worst


@pytest.mark.parametrize("pattern", TB_PATTERNS)
@pytest.mark.parametrize("name,spec", LOOP_KINDS, ids=["%s-%s" % (n, "spec" if s else "generic") for n, s in LOOP_KINDS])
def test_closed_loop_rollout_by_step(monkeypatch, name, spec, pattern):
    """rollout_closed_loop and tg_batch_rollout_closed_loop_subset against the numpy loop over oracle steps, U_k = bU_k - K_k (X_k - bX_k),
    X_k = [q2; p2; (k2 - k1) / dt_{k-1}]: X and Uout."""
    run_closed_loop(monkeypatch, name, spec, pattern)


# ---- one step per trajectory ------------------------------------------------------------------------------------------------------------
HORIZON_KINDS = [(n, False) for n in ("pend_on_cart", "scissor4", "spring_arm", "puppet40")] + \
                [(n, True) for n in ("pend_on_cart", "scissor4", "puppet40")]


def _check_horizon(tag, mvi, h, refs, spec, par=False):
    """The checks of a horizon batch built the way BatchDOptimizer does; refs[t] is trajectory t's oracle step."""
    L = _lib.lib()
    S, H = TB_HORIZON
    d, dts = h["d"], h["dts"]
    nq, nd, nk, nu = d.n_configs, d.n_dyn, d.n_kin, d.n_inputs
    nX, nU, R = nq + nd + nk, nu + nk, nq + nd + nu + nk
    B = S * H
    mvi.set_step_sizes(dts, by_trajectory=True)
    Xd, Ud = mvi.device_array(h["X"]), mvi.device_array(h["U"])
    # (the scalar is nobody's step: every trajectory must take its own from the list)
    _lib.check(L.tg_batch_set_from_trajectories(mvi._h, S, H, 0.0, 0.77 * DT, Xd, Ud, 200))
    Ad, Bd = mvi.device_array(np.full((B, nX, nX), np.nan)), mvi.device_array(np.full((B, nX, nU), np.nan))
    _lib.check(L.tg_batch_linearize(mvi._h, Ad, Bd))
    zd = mvi.device_array(h["Z"])
    full, part = mvi.device_array(np.full((B, R, R), np.nan)), mvi.device_array(np.full((B, R, R), 7.0))
    _lib.check(L.tg_batch_deriv2_contract_device(mvi._h, zd, full))
    k0, k1 = 1, 4
    _lib.check(L.tg_batch_deriv2_contract_device_range(mvi._h, zd, part, H, k0, k1))
    mvi.synchronize()
    iters, status = mvi.status()
    assert (status == 0).all(), (tag, status)
    q2, p2 = mvi.q2, mvi.p2
    A, Bm = mvi.download(Ad, (B, nX, nX)), mvi.download(Bd, (B, nX, nU))
    F, P = mvi.download(full, (B, R, R)), mvi.download(part, (B, R, R))
    mvi.calc_deriv1()
    d1 = dict((n, mvi.deriv1(n)) for n in D1)
    rows = np.array([s * H + k for s in range(S) for k in range(k0, k1)])
    rest = np.setdiff1d(np.arange(B), rows)
    assert (P[rest] == 7.0).all(), tag                         # the range launch leaves every other row untouched
    worst = dict(q2=0.0, p2=0.0, d1=0.0, AB=0.0, hz=0.0)
    for t, r in enumerate(refs):
        dt = dts[t % H]
        e = dict(q2=relerr(q2[t], r["q2"]), p2=relerr(p2[t], r["p2"]), d1=max(relerr(d1[n][t], r["d1"][n]) for n in D1),
                 AB=max(relerr(A[t], r["A"]), relerr(Bm[t], r["B"])), hz=relerr(F[t], r["hz"]))
        for q in e:
            worst[q] = max(worst[q], e[q])
        assert e["q2"] < TB_TOL["X"] and e["p2"] < TB_TOL["X"], (tag, t, e)
        assert abs(int(iters[t]) - r["iterations"]) <= 1, (tag, t)
        assert e["d1"] < TB_TOL["d1"] and e["AB"] < TB_TOL["AB"] and e["hz"] < TB_TOL["hz"], (tag, t, e)
        # A / B rebuilt in numpy from the device's own blocks with this trajectory's dt: the kernel's A / B output path
        Ar, Br = tb_AB(d, dict((n, d1[n][t]) for n in D1), dt)
        assert relerr(A[t], Ar) < 1e-12 and relerr(Bm[t], Br) < 1e-12, (tag, t)
        if nk:      # the -+1/dt_k entries of the v rows explicitly
            v = slice(nq + nd, nX)
            assert np.allclose(A[t][v, nd:nq], -np.eye(nk) / dt, rtol=1e-13, atol=0.0), (tag, t)
            assert np.allclose(Bm[t][v, nu:], np.eye(nk) / dt, rtol=1e-13, atol=0.0), (tag, t)
        if t in rows:
            assert relerr(P[t], r["hz"]) < TB_TOL["hz"], (tag, t, relerr(P[t], r["hz"]))
            assert np.array_equal(P[t], F[t]), (tag, t)
    print(tag, " ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    info = mvi.kernel_info()
    if par:
        assert {"rollout", "deriv1", "deriv2z"} <= set(info["par_generic_launched"]) and not info["par_spec_launched"], info
        assert info["generic_launches"] == 0 and info["spec_launches"] == 0, info
    else:
        _assert_kind(mvi, spec, ["rollout", "deriv1", "deriv2z"])
    return worst


def run_horizon(monkeypatch, name, spec, pattern, record=None):
    h = tb_horizon(name, pattern)
    S, H = TB_HORIZON
    mvi = _batch(monkeypatch, name, S * H, spec)
    worst = _check_horizon("%s %s %s horizon" % (name, "spec" if spec else "generic", pattern), mvi, h, h["refs"], spec)
    mvi.close()
    if record is not None:
        record(worst)
    return worst


@pytest.mark.parametrize("pattern", TB_PATTERNS)
@pytest.mark.parametrize("name,spec", HORIZON_KINDS, ids=["%s-%s" % (n, "spec" if s else "generic") for n, s in HORIZON_KINDS])
def test_one_step_per_trajectory(monkeypatch, name, spec, pattern):
    """A horizon batch of 2 seeds x 5 steps with a by-trajectory list of 5 (t % count wraps once): tg_batch_set_from_trajectories,
    tg_batch_linearize, tg_batch_deriv2_contract_device and its range launch (horizon 5, steps 1..3: a remapped launch whose slot index
    differs from its trajectory index).  Trajectory (s, k) equals an oracle set to X[s][k] and stepped by t[k+1] - t[k]."""
    run_horizon(monkeypatch, name, spec, pattern)


def test_one_step_per_trajectory_with_parameter_rows(monkeypatch):
    """The same with a per-trajectory parameter table (one row of masses per seed, group = horizon): the reference is the system rebuilt
    with the seed's row, as in test_gpu_parameters.py."""
    name, pattern = "scissor4", "alternating"
    S, H = TB_HORIZON
    make = BUILDERS[name]
    system = make()
    rows = dict((k, v) for k, v in random_rows(system, S, seed=77).items() if k == "inertia")
    assert rows
    h = tb_horizon(name, pattern)
    d, X, U, dts = h["d"], h["X"], h["U"], h["dts"]
    nq, nd, nu = d.n_configs, d.n_dyn, d.n_inputs
    refs = []
    for s in range(S):
        ds = descriptor.flatten(rebuilt(make, rows, s))
        for k in range(H):
            o = OracleMVI(ds)
            o.initialize_from_state(0.0, X[s, k, :nq], X[s, k, nq:nq + nd])
            it = o.step(dts[k], U[s, k, :nu], U[s, k, nu:], q2_hint=X[s, k + 1, :nd])
            r = dict(q2=o.q2, p2=o.p2, iterations=it)
            r.update(tb_oracle_derivs(o, ds, dts[k], h["Z"][s * H + k], h["ZL"][s * H + k]))
            refs.append(r)
    # the rows change the answer by far more than the tolerance (otherwise the base system would pass as well)
    assert max(relerr(r["A"], b["A"]) for r, b in zip(refs, h["refs"])) > 1e-4
    mvi = _batch(monkeypatch, name, S * H, False, system=system)
    mvi.set_parameters(group=H, **rows)
    _check_horizon("%s parameter rows horizon" % name, mvi, h, refs, False, par=True)
    mvi.close()


@pytest.mark.parametrize("name,spec", [("pend_on_cart", False), ("scissor4", True), ("spring_arm", False)])
def test_step_with_a_by_trajectory_list(monkeypatch, name, spec):
    """tg_batch_step on a plain batch of 7 with a list of 3: trajectory t takes dt[t % 3], whatever t2 the call names."""
    B = 7
    c = tb_case(name, "random", 2, B)
    d = c["d"]
    dts = DT * np.array([0.6, 1.5, 1.0])
    mvi = _batch(monkeypatch, name, B, spec)
    mvi.initialize_from_configs(0.0, c["Q0"], DT, c["Q1"])
    # (set after the start: while a by-trajectory list is set EVERY mode takes the trajectory's size for t2 - t1, the calc_p2 of
    # initialize_from_configs included)
    mvi.set_step_sizes(dts, by_trajectory=True)
    it, st = mvi.step(DT + 0.77 * DT, _in(c, "U", 0, 1)[:, 0] if d.n_inputs else None, _in(c, "K", 0, 1)[:, 0] if d.n_kin else None)
    assert (st == 0).all()
    q2, p2 = mvi.q2, mvi.p2
    mvi.calc_deriv1()
    d1 = mvi.deriv1("p2_dq1")
    for b in range(B):
        r = tb_oracle_rollout(d, c["Q0"][b], c["Q1"][b], dts[[b % 3]], c["U"][b, :1], c["K"][b, :1])
        assert relerr(q2[b], r["o"].q2) < TB_TOL["X"] and relerr(p2[b], r["p2"]) < TB_TOL["X"], (name, b)
        assert abs(int(it[b]) - r["iterations"]) <= 1
        r["o"].calc_deriv1()
        assert relerr(d1[b], r["o"].deriv1("p2_dq1")) < TB_TOL["d1"], (name, b)
    _assert_kind(mvi, spec, ["rollout", "calc_p2", "deriv1"])
    mvi.close()


# ---- host behaviour ---------------------------------------------------------------------------------------------------------------------
def _small(monkeypatch, name="pend_on_cart", pattern="alternating", N=8, B=5):
    c = tb_case(name, pattern, N, B)
    ref = [tb_oracle_rollout(c["d"], c["Q0"][b], c["Q1"][b], c["dts"], c["U"][b], c["K"][b]) for b in range(B)]
    return c, ref, _batch(monkeypatch, name, B, False)


def _follows(mvi, c, ref, N):
    mvi.initialize_from_configs(0.0, c["Q0"], DT, c["Q1"])
    X = mvi.rollout(N, 0.77 * DT, _in(c, "U", 0, N), _in(c, "K", 0, N))
    assert (mvi.status()[1] == 0).all()
    for b, r in enumerate(ref):
        assert relerr(X[b], r["X"]) < TB_TOL["X"], (b, relerr(X[b], r["X"]))
    return X


@pytest.mark.parametrize("name", ["pend_on_cart", "scissor4"])
def test_refused_list_changes_nothing(monkeypatch, name):
    """A list with a zero or a non-finite entry is refused (return code, tg_last_error) and the list set before stays: the next
    rollout still follows it, and the Python object's copy agrees with the library's."""
    c, ref, mvi = _small(monkeypatch, name)
    L = _lib.lib()
    mvi.set_step_sizes(c["dts"])
    launches = mvi.kernel_info()["generic_launches"]
    for bad, word in ((0.0, "zero"), (np.nan, "finite"), (np.inf, "finite"), (-np.inf, "finite")):
        lst = c["dts"].copy()
        lst[3] = bad
        for by_trajectory in (0, 1):
            rc = L.tg_batch_set_step_sizes(mvi._h, len(lst), lst.ctypes.data, by_trajectory)
            assert rc == _lib.ERR_INVALID, (bad, rc)
            assert word in L.tg_last_error().decode(), (bad, L.tg_last_error())
        with pytest.raises(LibraryError, match=word):
            mvi.set_step_sizes(lst)
        assert np.array_equal(mvi._step_sizes[0], c["dts"]) and mvi._step_sizes[1] is False
    assert L.tg_batch_set_step_sizes(mvi._h, 3, None, 0) == _lib.ERR_INVALID
    assert mvi.kernel_info()["generic_launches"] == launches
    _follows(mvi, c, ref, c["N"])
    assert mvi.times() == _summed(DT, c["dts"])
    mvi.close()


@pytest.mark.parametrize("name,spec", [("pend_on_cart", False), ("scissor4", True), ("puppet40", False)])
def test_one_step_calls_take_the_callers_size_under_a_by_step_list(monkeypatch, name, spec):
    """With a by-step list set, step(t2 + h) with h != dts[0] is an oracle step by h (the list belongs to the rollouts), and so is
    tg_batch_set_from_trajectories with its dt; the times and the derivative modes agree."""
    B = 3
    c = tb_case(name, "alternating", 2, B)
    d = c["d"]
    nq, nd, nu = d.n_configs, d.n_dyn, d.n_inputs
    h = 1.23 * DT
    assert abs(h - c["dts"][0]) > 0.2 * DT
    mvi = _batch(monkeypatch, name, B, spec)
    mvi.set_step_sizes(c["dts"])
    mvi.initialize_from_configs(0.0, c["Q0"], DT, c["Q1"])
    it, st = mvi.step(DT + h, _in(c, "U", 0, 1)[:, 0] if nu else None, _in(c, "K", 0, 1)[:, 0] if d.n_kin else None)
    assert (st == 0).all() and mvi.times() == (DT, DT + h)
    q2, p2 = mvi.q2, mvi.p2
    mvi.calc_deriv1()
    d1 = mvi.deriv1("q2_dp1")
    refs = [tb_oracle_rollout(d, c["Q0"][b], c["Q1"][b], np.array([h]), c["U"][b, :1], c["K"][b, :1]) for b in range(B)]
    for b, r in enumerate(refs):
        assert relerr(q2[b], r["o"].q2) < TB_TOL["X"] and relerr(p2[b], r["p2"]) < TB_TOL["X"], (name, b, relerr(q2[b], r["o"].q2))
        assert abs(int(it[b]) - r["iterations"]) <= 1
        r["o"].calc_deriv1()
        assert relerr(d1[b], r["o"].deriv1("q2_dp1")) < TB_TOL["d1"], (name, b)
    # tg_batch_set_from_trajectories (batch = 3 seeds x 1 step) from the states just reached
    X = np.zeros((B, 2, mvi.nX))
    X[:, 0] = np.array([r["X"][1] for r in refs])
    X[:, 1] = X[:, 0]
    U = np.array([np.concatenate([c["U"][b, 1], c["K"][b, 1]]) for b in range(B)])[:, None]
    _lib.check(_lib.lib().tg_batch_set_from_trajectories(mvi._h, B, 1, 0.0, h, mvi.device_array(X), mvi.device_array(U), 200))
    mvi.synchronize()
    assert (mvi.status()[1] == 0).all() and mvi.times() == (0.0, h)
    q2 = mvi.q2
    for b, r in enumerate(refs):
        o = OracleMVI(d)
        o.initialize_from_state(0.0, X[b, 0, :nq], X[b, 0, nq:nq + nd])
        o.step(h, U[b, 0, :nu], U[b, 0, nu:], q2_hint=X[b, 1, :nd])
        assert relerr(q2[b], o.q2) < TB_TOL["X"], (name, b, relerr(q2[b], o.q2))
    _assert_kind(mvi, spec, ["rollout", "calc_p2", "deriv1"])
    mvi.close()


def test_by_trajectory_list_refuses_longer_rollouts(monkeypatch):
    """Every step of a longer rollout would take the trajectory's size while the times advance by the scalar: TG_ERR_INVALID before any
    launch, for the three rollout entry points; one step is what the list is for."""
    c, ref, mvi = _small(monkeypatch)
    B, N = c["B"], c["N"]
    mvi.initialize_from_configs(0.0, c["Q0"], DT, c["Q1"])
    mvi.set_step_sizes(c["dts"][:3], by_trajectory=True)
    state = (mvi.times(), mvi.q2, mvi.p2)
    launches = mvi.kernel_info()["generic_launches"]
    nX, nU = mvi.nX, mvi.nU
    Kp, bX, bU = np.zeros((B, N, nU, nX)), np.zeros((B, N + 1, nX)), np.zeros((B, N, nU))
    with pytest.raises(LibraryError, match="by-trajectory"):
        mvi.rollout(N, DT, _in(c, "U", 0, N), _in(c, "K", 0, N))
    with pytest.raises(LibraryError, match="by-trajectory"):
        mvi.rollout_closed_loop(N, DT, Kp, bX, bU)
    dev = [mvi.device_array(a) for a in (Kp, bX, bU, bX, bU)]
    rc = _lib.lib().tg_batch_rollout_closed_loop_subset(mvi._h, 2, N, DT, dev[0], 1, None, dev[1], dev[2], dev[3], dev[4], 200)
    assert rc == _lib.ERR_INVALID and "by-trajectory" in _lib.lib().tg_last_error().decode()
    assert mvi.kernel_info()["generic_launches"] == launches
    assert mvi.times() == state[0] and np.array_equal(mvi.q2, state[1]) and np.array_equal(mvi.p2, state[2])
    X = mvi.rollout(1, DT, _in(c, "U", 0, 1), _in(c, "K", 0, 1))          # one step: trajectory t by dts[t % 3]
    for b in range(B):
        r = tb_oracle_rollout(c["d"], c["Q0"][b], c["Q1"][b], c["dts"][[b % 3]], c["U"][b, :1], c["K"][b, :1])
        assert relerr(X[b], r["X"]) < TB_TOL["X"], b
    mvi.close()


def test_rollouts_refuse_a_list_shorter_than_the_rollout(monkeypatch):
    """A by-step list shorter than the rollout is refused before the launch by all three rollout entry points (the kernel would read
    past the list's end): return code, message, no launch, state and times untouched."""
    c, ref, mvi = _small(monkeypatch)
    B, N = c["B"], c["N"]
    L = _lib.lib()
    mvi.set_step_sizes(c["dts"][:N - 1])
    mvi.initialize_from_configs(0.0, c["Q0"], DT, c["Q1"])
    state = (mvi.times(), mvi.q2, mvi.p2)
    launches = mvi.kernel_info()["generic_launches"]
    nX, nU = mvi.nX, mvi.nU
    dev = [mvi.device_array(a) for a in (np.zeros((B, N, nU, nX)), np.zeros((B, N + 1, nX)), np.zeros((B, N, nU)))]
    Xd, Ud = mvi.device_empty(B * (N + 1) * nX), mvi.device_empty(B * N * nU)
    Uo, Ko = mvi.device_array(c["U"]), mvi.device_array(c["K"])
    calls = [lambda: L.tg_batch_rollout(mvi._h, N, DT, Uo, Ko, Xd, 200),
             lambda: L.tg_batch_rollout_closed_loop(mvi._h, N, DT, dev[0], 1, dev[1], dev[2], Xd, Ud, 200),
             lambda: L.tg_batch_rollout_closed_loop_subset(mvi._h, 2, N, DT, dev[0], 1, None, dev[1], dev[2], Xd, Ud, 200)]
    for call in calls:
        assert call() == _lib.ERR_INVALID
        assert "longer than the step-size list" in L.tg_last_error().decode()
    assert mvi.kernel_info()["generic_launches"] == launches
    assert mvi.times() == state[0] and np.array_equal(mvi.q2, state[1]) and np.array_equal(mvi.p2, state[2])
    assert L.tg_batch_rollout_closed_loop(mvi._h, N - 1, DT, dev[0], 1, dev[1], dev[2], Xd, Ud, 200) == 0     # as long as the list: fine
    mvi.synchronize()
    assert mvi.times() == _summed(DT, c["dts"][:N - 1])
    mvi.close()


def test_refresh_keeps_the_list(monkeypatch):
    """A parameter write rebuilds the device schedule (refresh()); the batch's list is carried over, by step and by trajectory."""
    name = "pend_on_cart"
    c = tb_case(name, "alternating", 8, 5)
    system = BUILDERS[name]()
    mvi = _batch(monkeypatch, name, c["B"], False, system=system)
    mvi.set_step_sizes(c["dts"])
    mvi.initialize_from_configs(0.0, c["Q0"], DT, c["Q1"])
    system.masses[0].set_mass(2.5)                           # the next call rebuilds the schedule
    d2 = descriptor.flatten(system)
    ref = [tb_oracle_rollout(d2, c["Q0"][b], c["Q1"][b], c["dts"], c["U"][b], c["K"][b]) for b in range(c["B"])]
    c2 = dict(c, d=d2)
    _follows(mvi, c2, ref, c["N"])
    assert mvi.times() == _summed(DT, c["dts"])
    # by trajectory: the rebuild happens inside step(), which carries the state (momenta of the old masses included) and the list over
    mvi.set_step_sizes(None)
    mvi.initialize_from_configs(0.0, c["Q0"], DT, c["Q1"])
    p2 = mvi.p2
    mvi.set_step_sizes(c["dts"][:3], by_trajectory=True)
    system.masses[0].set_mass(1.5)
    d3 = descriptor.flatten(system)
    it, st = mvi.step(DT + 0.77 * DT, c["U"][:, 0], None)
    assert (st == 0).all() and mvi._step_sizes[1] is True
    q2 = mvi.q2
    for b in range(c["B"]):
        o = OracleMVI(d3)
        o.set_times(0.0, DT)
        o.q1, o.q2, o.p2 = c["Q0"][b], c["Q1"][b], p2[b]
        o.step(DT + c["dts"][b % 3], c["U"][b, 0], c["K"][b, 0])
        assert relerr(q2[b], o.q2) < TB_TOL["X"], (b, relerr(q2[b], o.q2))
    mvi.close()


def test_rollout_with_an_array_restores_the_list_set_before(monkeypatch):
    c, ref, mvi = _small(monkeypatch)
    N = c["N"]
    other = tb_step_sizes("random", N, "another list")
    mvi.set_step_sizes(other)
    mvi.initialize_from_configs(0.0, c["Q0"], DT, c["Q1"])
    X = mvi.rollout(N, c["dts"], _in(c, "U", 0, N), _in(c, "K", 0, N))         # the sugar: this call's own list
    for b, r in enumerate(ref):
        assert relerr(X[b], r["X"]) < TB_TOL["X"], b
    assert np.array_equal(mvi._step_sizes[0], other)
    ref2 = [tb_oracle_rollout(c["d"], c["Q0"][b], c["Q1"][b], other, c["U"][b], c["K"][b]) for b in range(c["B"])]
    _follows(mvi, c, ref2, N)                                                    # ... and the batch's list is in force again
    # the closed-loop sugar likewise
    nX, nU = mvi.nX, mvi.nU
    Kp, bX = np.zeros((c["B"], N, nU, nX)), np.array([r["X"] for r in ref])
    mvi.initialize_from_configs(0.0, c["Q0"], DT, c["Q1"])
    Xc, _ = mvi.rollout_closed_loop(N, c["dts"], Kp, bX, np.array([r["U"] for r in ref]))
    for b, r in enumerate(ref):
        assert relerr(Xc[b], r["X"]) < TB_TOL["X"], b
    _follows(mvi, c, ref2, N)
    mvi.close()


@pytest.mark.parametrize("name,spec", [("pend_on_cart", False), ("puppet40", True)])
def test_snapshot_restore_reproduce_a_non_uniform_rollout(monkeypatch, name, spec):
    c = tb_case(name, "random", 8, 5)
    N = c["N"]
    mvi = _batch(monkeypatch, name, c["B"], spec)
    mvi.set_step_sizes(c["dts"])
    mvi.initialize_from_configs(0.0, c["Q0"], DT, c["Q1"])
    mvi.snapshot()
    runs = []
    for _ in range(2):
        X = mvi.rollout(N, DT, _in(c, "U", 0, N), _in(c, "K", 0, N))
        runs.append((X, mvi.q1, mvi.q2, mvi.p1, mvi.p2, mvi.lambda1, mvi.status()[0], mvi.times()))
        mvi.restore()
        assert mvi.times() == (0.0, DT)
    for a, b in zip(runs[0][:-1], runs[1][:-1]):
        assert np.array_equal(a, b), name
    assert runs[0][-1] == runs[1][-1] == _summed(DT, c["dts"])
    ref = tb_oracle_rollout(c["d"], c["Q0"][0], c["Q1"][0], c["dts"], c["U"][0], c["K"][0])
    assert relerr(runs[0][0][0], ref["X"]) < TB_TOL["X"]
    mvi.close()


def test_dsystem_on_a_non_uniform_grid_matches_the_oracle_built_linearisation(monkeypatch):
    """DSystem.linearize_trajectory and BatchDSystem.set / linearize on a non-uniform t for the scissor lift (8 constraints) against A, B
    built in numpy from the oracle's blocks."""
    import trep_amd
    from trep_amd.discopt.dsystem import BatchDSystem, DSystem
    monkeypatch.delenv("TREPAMD_TEAM", raising=False)
    name, pattern = "scissor4", "random"
    S, H = TB_HORIZON
    h = tb_horizon(name, pattern)
    t = np.concatenate([[0.0], np.cumsum(h["dts"])])
    system = BUILDERS[name]()
    dsys = DSystem(trep_amd.MidpointVI(system), t)
    assert dsys.nX == h["X"].shape[2] and dsys.nU == h["U"].shape[2]
    for s in range(S):
        lt = dsys.linearize_trajectory(h["X"][s], h["U"][s])
        for k in range(H):
            r = h["refs"][s * H + k]
            assert relerr(lt.A[k], r["A"]) < TB_TOL["AB"] and relerr(lt.B[k], r["B"]) < TB_TOL["AB"], (s, k)
    bd = BatchDSystem(system, t, S)
    for k in range(H):
        _, status = bd.set(h["X"][:, k], h["U"][:, k], k, Xk_hint=h["X"][:, k + 1])
        assert (status == 0).all()
        lin = bd.linearize()
        f = bd.f()
        for s in range(S):
            r = h["refs"][s * H + k]
            assert relerr(lin.A[s], r["A"]) < TB_TOL["AB"] and relerr(lin.B[s], r["B"]) < TB_TOL["AB"], (s, k)
            assert relerr(f[s, :len(r["q2"])], r["q2"]) < TB_TOL["X"], (s, k)
