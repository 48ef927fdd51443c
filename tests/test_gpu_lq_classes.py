"""tg_tv_lq over every size class and solver branch of its three kernels (k_tv_lq, k_tv_lq_mfma, k_tv_lq_ds), against the long-double
sweep of tests/lq_reference.py.

Every launch first asks tg_tv_lq_plan which kernel it is about to run and holds that against what the case is there for
(common.LQ_CASES; test_lq_plan_cpu.py shows that the table covers the dispatch).  Bounds: an output may be max(64 e_ref, 1e-13) away
from the reference, e_ref being the distance of the fp64 host sweep (dlqr.py) from the reference on the same problem -- 2.3e-15 at
most over the table, so the bound is 1e-13 .. 1.5e-13 everywhere (test_lq_reference_cpu.py).  The gains are also compared entry by
entry against the size of their own row.  What must be bit for bit (a sweep in chunks = the whole sweep) is asserted bit for bit."""
import ctypes

import numpy as np
import pytest

from common import (LQ_CASES, LQ_KERNELS, LQ_MODES, LQ_SPECIAL_SIZES, LqOutputs, device_pool, lq_case_id, lq_case_nxh, lq_case_problem,
                    lq_case_reference, lq_check_seed, lq_indefinite_problem, lq_plan, lq_singular_problem, lq_special_problem,
                    lq_special_reference, lq_struct, lq_zero_pivot_problem)

pytestmark = pytest.mark.gpu
OK, SINGULAR = 0, 2


def _launch(L, p, kernel=None):
    from trep_amd import _lib
    rc, plan, _, _ = lq_plan(p)
    assert rc == 0 and (kernel is None or plan[0] == kernel), (plan, kernel)
    _lib.check(L.tg_tv_lq(0, ctypes.byref(p)))
    return plan


def _sweep(L, pool, make, S, N, nX, nU, chunks=None, kernel=None, outputs=None, after_chunk=None):
    """Run a problem (make() -> a fresh tg_lq_problem without outputs) whole, or chunk by chunk (list of (k0, k1), last steps first) with the
    (P, b) carried from launch to launch; returns (K, C, P, b at the first swept step, status), b_next rows."""
    out = outputs or LqOutputs(pool, S, N, nX, nU)
    if chunks is None:
        _launch(L, out.bind(make()), kernel)
        return out.get(), out.Z.get()
    carry = [(pool.upload(np.full((S, nX, nX), np.nan)), pool.upload(np.full((S, nX), np.nan))) for _ in range(2)]
    for c, (k0, k1) in enumerate(chunks):
        p = out.bind(make(), carry=carry[c % 2])
        p.k_begin, p.k_end = k0, k1
        if c > 0:
            p.Pt_dev, p.bt_dev = carry[(c - 1) % 2][0].ptr, carry[(c - 1) % 2][1].ptr
        _launch(L, p, kernel)
        if after_chunk is not None:
            after_chunk(c, carry[c % 2])
    last = carry[(len(chunks) - 1) % 2]
    K, C, _, _, st = out.get()
    return (K, C, last[0].get(), last[1].get(), st), out.Z.get()


@pytest.mark.parametrize("case", LQ_CASES, ids=lq_case_id)
def test_size_class(case, monkeypatch):
    """LQR, affine LQ and the Newton model of one table case, different data per seed; with `select` the launch skips a seed, whose
    outputs stay as they were."""
    from trep_amd import _lib
    L = _lib.lib()
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    S, N, nX, nU, nxh = case.S, case.N, case.nX, case.nU, lq_case_nxh(case)
    A, B, Q, Qf, R, q, r, hz = lq_case_problem(case)
    pool = device_pool()
    try:
        dev = dict((k, pool.upload(v)) for k, v in dict(A=A, B=B, Q=Q, Qf=Qf, R=R, q=q, r=r, hz=hz).items())
        seeds = list(case.select) if case.select else list(range(S))
        sel = pool.upload(np.array(seeds, dtype=np.int32), np.int32) if case.select else None
        for mode in LQ_MODES:
            p = lq_struct(len(seeds), N, nX, nU, dev, affine=mode != "lqr", hz=(nxh + nU, nxh) if mode == "newton" else None, ds=case.ds)
            if sel is not None:
                p.select_dev = sel.ptr
            out = LqOutputs(pool, S, N, nX, nU)
            plan = _launch(L, out.bind(p))
            assert plan == case.plan, (plan, case.plan)
            K, C, P0, b0, st = out.get()
            for s in range(S):
                if s not in seeds:
                    assert np.isnan(K[s]).all() and np.isnan(C[s]).all() and np.isnan(P0[s]).all() and np.isnan(b0[s]).all() and st[s] == -9
                    continue
                assert st[s] == OK, (mode, s, st)
                want, floors, bounds = lq_case_reference(case, mode, s)
                assert np.isfinite(K[s]).all() and np.isfinite(P0[s]).all()
                if mode == "lqr":
                    assert np.isnan(b0[s]).all()          # no affine part: not written
                lq_check_seed((K[s], C[s], P0[s], b0[s]), want, tuple(1.0 if b is None else b for b in bounds), "%s %s seed %d" % (lq_case_id(case), mode, s))
                if case.ds:
                    assert not K[s][:, :, nX - case.ds[1]:].any()                   # the v columns of a DSystem's gains are exactly zero
    finally:
        pool.close()


def _special(kernel, monkeypatch):
    env, want = LQ_KERNELS[kernel]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return want


def _check_all(pr, got, tag, seeds=None):
    K, C, P0, b0, st = got
    for s in (range(pr["S"]) if seeds is None else seeds):
        want, floors, bounds, _ = lq_special_reference(pr, s)
        lq_check_seed((K[s], C[s], P0[s], b0[s]), want, bounds, "%s seed %d" % (tag, s))


@pytest.mark.parametrize("ds", LQ_SPECIAL_SIZES, ids=str)
@pytest.mark.parametrize("kernel", list(LQ_KERNELS))
def test_weights_with_strides(kernel, ds, monkeypatch):
    """Q [S][N][nX][nX], R [S][N][nU][nU], Qf [S][nX][nX], all different, with their strides; then a seed stride alone and a step stride alone.
    Against the reference, and bit for bit against S x N one-step launches that each get their step's weights as shared ones (strides 0)."""
    from trep_amd import _lib
    L = _lib.lib()
    want_kernel = _special(kernel, monkeypatch)
    N, S = 5, 2
    pr = lq_special_problem(ds, N, S, "strides")
    nX, nU, nxh, rng = pr["nX"], pr["nU"], pr["nxh"], pr["rng"]

    def spd(n, *lead):
        M = rng.standard_normal(lead + (n, n))
        return np.matmul(M, np.swapaxes(M, -1, -2)) / n + np.eye(n) * (1.0 + rng.random(lead + (1, 1)))
    Qfull, Rfull, Qf = spd(nX, S, N), spd(nU, S, N), 2.0 * spd(nX, S)
    pool = device_pool()
    try:
        base = dict((k, pool.upload(pr[k])) for k in ("A", "B", "q", "r", "hz"))
        for variant in ("seed and step", "seed", "step"):
            if variant == "seed and step":
                Qv, Rv, strides = Qfull, Rfull, dict(Q=(N * nX * nX, nX * nX), Qf=nX * nX, R=(N * nU * nU, nU * nU))
                pick = lambda M, s, k: M[s, k]
            elif variant == "seed":
                Qv, Rv, strides = Qfull[:, 1].copy(), Rfull[:, 2].copy(), dict(Q=(nX * nX, 0), Qf=nX * nX, R=(nU * nU, 0))
                pick = lambda M, s, k: M[s]
            else:
                Qv, Rv, strides = Qfull[1].copy(), Rfull[0].copy(), dict(Q=(0, nX * nX), Qf=0, R=(0, nU * nU))
                pick = lambda M, s, k: M[k]
            Qfv = Qf if variant != "step" else Qf[1]
            dev = dict(base, Q=pool.upload(Qv), R=pool.upload(Rv), Qf=pool.upload(Qfv))
            make = lambda: lq_struct(S, N, nX, nU, dev, hz=(nxh + nU, nxh), ds=ds, strides=strides)
            got, Z = _sweep(L, pool, make, S, N, nX, nU, kernel=want_kernel)
            assert (got[4] == OK).all()
            for s in range(S):
                one = dict(pr, Q=np.array([pick(Qv, s, k) for k in range(N)]), R=np.array([pick(Rv, s, k) for k in range(N)]),
                           Qf=Qfv[s] if variant != "step" else Qfv)
                want, floors, bounds, _ = lq_special_reference(one, s)
                lq_check_seed((got[0][s], got[1][s], got[2][s], got[3][s]), want, bounds, "%s %s strides: %s, seed %d" % (kernel, ds, variant, s))
            # the same sweep as S x N launches of one seed and one step, each pointed at its own weights
            out = LqOutputs(pool, S, N, nX, nU)
            carry = [(pool.upload(np.full((S, nX, nX), np.nan)), pool.upload(np.full((S, nX), np.nan))) for _ in range(2)]
            for s in range(S):
                sel = pool.upload(np.array([s], dtype=np.int32), np.int32)
                for c, k in enumerate(range(N - 1, -1, -1)):
                    qoff = {"seed and step": (s * N + k), "seed": s, "step": k}[variant]
                    dev1 = dict(dev, Q=dev["Q"].ptr + 8 * nX * nX * qoff, R=dev["R"].ptr + 8 * nU * nU * qoff,
                                Qf=dev["Qf"].ptr + (8 * nX * nX * s if variant != "step" else 0))
                    p = out.bind(lq_struct(1, N, nX, nU, dev1, hz=(nxh + nU, nxh), ds=ds), carry=carry[c % 2])
                    p.select_dev, p.k_begin, p.k_end = sel.ptr, k, k + 1
                    if c > 0:
                        p.Pt_dev, p.bt_dev = carry[(c - 1) % 2][0].ptr, carry[(c - 1) % 2][1].ptr
                    _launch(L, p, want_kernel)
                last = carry[(N - 1) % 2]
                assert np.array_equal(last[0].get()[s], got[2][s]) and np.array_equal(last[1].get()[s], got[3][s]), (variant, s)
            K1, C1, _, _, st1 = out.get()
            assert np.array_equal(K1, got[0]) and np.array_equal(C1, got[1]) and np.array_equal(out.Z.get(), Z) and (st1 == OK).all(), variant
    finally:
        pool.close()


@pytest.mark.parametrize("ds", LQ_SPECIAL_SIZES, ids=str)
@pytest.mark.parametrize("kernel", list(LQ_KERNELS))
def test_curvature_layouts(kernel, ds, monkeypatch):
    """HZ wider than its blocks (hz_R = hz_nx + nU + 3, the rest filled with 1e300: never read), without a state part (hz_nx = 0: only
    R_k changes) and over all states (hz_nx = nX: S_k has v rows, which the structured kernel does not compute -- the dispatch hands the
    problem to the dense kernel)."""
    from trep_amd import _lib
    L = _lib.lib()
    want_kernel = _special(kernel, monkeypatch)
    N, S = 6, 2
    pr = lq_special_problem(ds, N, S, "curvature")
    nX, nU, nxh, rng = pr["nX"], pr["nU"], pr["nxh"], pr["rng"]
    pool = device_pool()
    try:
        dev = dict((k, pool.upload(pr[k])) for k in ("A", "B", "Q", "Qf", "R", "q", "r"))
        for name, nx in (("wide", nxh), ("no state part", 0), ("all states", nX)):
            R_ = nx + nU + (3 if name == "wide" else 0)
            core = 0.05 * rng.standard_normal((S, N, nx + nU, nx + nU))
            core = core + np.swapaxes(core, 2, 3)
            hz = np.full((S, N, R_, R_), 1e300)
            hz[:, :, :nx + nU, :nx + nU] = core
            dev["hz"] = pool.upload(hz)
            expect = 1 if (kernel == "structured" and nx > nxh) else want_kernel
            got, _ = _sweep(L, pool, lambda: lq_struct(S, N, nX, nU, dev, hz=(R_, nx), ds=ds), S, N, nX, nU, kernel=expect)
            assert (got[4] == OK).all()
            _check_all(dict(pr, hz=hz, nxh=nx), got, "%s %s curvature: %s" % (kernel, ds, name))
    finally:
        pool.close()


@pytest.mark.parametrize("ds", LQ_SPECIAL_SIZES, ids=str)
@pytest.mark.parametrize("kernel", list(LQ_KERNELS))
def test_indefinite_gamma(kernel, ds, monkeypatch):
    """gamma_k indefinite at every step (half of the inputs with curvature below -(R + B'PB), cond < 1e3: test_lq_reference_cpu.py): whichever
    factorisation the guards of a kernel choose, the gains are the reference's."""
    from trep_amd import _lib
    L = _lib.lib()
    want_kernel = _special(kernel, monkeypatch)
    pr = lq_indefinite_problem(ds)
    S, N, nX, nU, nxh = pr["S"], pr["N"], pr["nX"], pr["nU"], pr["nxh"]
    pool = device_pool()
    try:
        dev = dict((k, pool.upload(pr[k])) for k in ("A", "B", "Q", "Qf", "R", "q", "r", "hz"))
        got, _ = _sweep(L, pool, lambda: lq_struct(S, N, nX, nU, dev, hz=(nxh + nU, nxh), ds=ds), S, N, nX, nU, kernel=want_kernel)
        assert (got[4] == OK).all()
        _check_all(pr, got, "%s %s indefinite" % (kernel, ds))
    finally:
        pool.close()


@pytest.mark.parametrize("ds", LQ_SPECIAL_SIZES, ids=str)
@pytest.mark.parametrize("kernel", list(LQ_KERNELS))
def test_zero_leading_pivot(kernel, ds, monkeypatch):
    """gamma[0][0] = 0 to rounding at the first swept step (P = Qf there, so the test can place it), cond(gamma) < 1e3: an elimination in index
    order must notice (the structured kernel's guard fails, its pivoted fallback takes over), and the gains are the reference's."""
    from trep_amd import _lib
    L = _lib.lib()
    want_kernel = _special(kernel, monkeypatch)
    N, S = 6, 2
    pr = lq_zero_pivot_problem(ds, N, S, N - 1)
    nX, nU, nxh = pr["nX"], pr["nU"], pr["nxh"]
    pool = device_pool()
    try:
        dev = dict((k, pool.upload(pr[k])) for k in ("A", "B", "Q", "Qf", "R", "q", "r", "hz"))
        got, _ = _sweep(L, pool, lambda: lq_struct(S, N, nX, nU, dev, hz=(nxh + nU, nxh), ds=ds), S, N, nX, nU, kernel=want_kernel)
        assert (got[4] == OK).all()
        _check_all(pr, got, "%s %s zero pivot at the first swept step" % (kernel, ds))
    finally:
        pool.close()


@pytest.mark.parametrize("ds", LQ_SPECIAL_SIZES, ids=str)
@pytest.mark.parametrize("kernel", list(LQ_KERNELS))
def test_zero_pivot_in_the_middle_chunk(kernel, ds, monkeypatch):
    """The same zero pivot at a step of the middle chunk of a three-chunk sweep (P there from the reference): the chunked sweep is the whole
    sweep bit for bit -- through the fallback and back to the unpivoted factorisation --, and both are the reference's."""
    from trep_amd import _lib
    L = _lib.lib()
    want_kernel = _special(kernel, monkeypatch)
    N, S, k_star = 9, 2, 4
    pr = lq_zero_pivot_problem(ds, N, S, k_star)
    nX, nU, nxh = pr["nX"], pr["nU"], pr["nxh"]
    pool = device_pool()
    try:
        dev = dict((k, pool.upload(pr[k])) for k in ("A", "B", "Q", "Qf", "R", "q", "r", "hz"))
        make = lambda: lq_struct(S, N, nX, nU, dev, hz=(nxh + nU, nxh), ds=ds)
        whole, Zw = _sweep(L, pool, make, S, N, nX, nU, kernel=want_kernel)
        parts, Zp = _sweep(L, pool, make, S, N, nX, nU, chunks=[(6, 9), (3, 6), (0, 3)], kernel=want_kernel)
        for a, b in zip(whole + (Zw,), parts + (Zp,)):
            assert np.array_equal(a, b)
        assert (whole[4] == OK).all()
        _check_all(pr, whole, "%s %s zero pivot in the middle chunk" % (kernel, ds))
    finally:
        pool.close()


@pytest.mark.parametrize("ds", LQ_SPECIAL_SIZES, ids=str)
@pytest.mark.parametrize("kernel", list(LQ_KERNELS))
def test_singular_gamma_is_a_status(kernel, ds, monkeypatch):
    """One input of the middle seed neither acts nor costs: row u of its gamma is exactly zero, the seed reports TG_SINGULAR (nothing is
    asserted about its numbers), the seeds around it TG_OK with the reference's results.  In a three-chunk sweep where only the first
    launched chunk (the last steps) is singular, the later chunks keep that verdict -- on their own account they would not: the (P, b)
    the singular chunk leaves for that seed (not finite, which would fail every later pivot search as well) is replaced by a finite
    one before the next chunk starts, so the later chunks of that seed are regular sweeps that inherit nothing but the status."""
    from trep_amd import _lib
    L = _lib.lib()
    want_kernel = _special(kernel, monkeypatch)
    N, S, bad, u = 9, 3, 1, 2
    chunks = [(6, 9), (3, 6), (0, 3)]
    for steps, chunked in ((range(N), False), (range(6, 9), True)):
        pr = lq_singular_problem(ds, N, S, bad, u, steps)
        nX, nU, nxh = pr["nX"], pr["nU"], pr["nxh"]
        pool = device_pool()
        try:
            dev = dict((k, pool.upload(pr[k])) for k in ("A", "B", "Q", "Qf", "q", "r", "hz"))
            dev["R"] = pool.upload(pr["R_sk"])
            make = lambda: lq_struct(S, N, nX, nU, dev, hz=(nxh + nU, nxh), ds=ds, strides=dict(R=(N * nU * nU, nU * nU)))

            def finite_carry(c, carry, pr=pr):
                if c == 0:
                    P, b = carry[0].get(), carry[1].get()
                    P[bad], b[bad] = pr["Qf"], pr["q"][bad][chunks[0][0]]
                    carry[0].set(P); carry[1].set(b)
            got, _ = _sweep(L, pool, make, S, N, nX, nU, chunks=chunks if chunked else None, kernel=want_kernel, after_chunk=finite_carry)
            if chunked:
                assert np.isfinite(got[0][bad][:chunks[0][0]]).all() and np.isfinite(got[2][bad]).all()      # the later chunks were regular
            assert list(got[4]) == [OK, SINGULAR, OK], (chunked, got[4])
            good = dict(pr, R=pr["R"])           # the other seeds' R_k is the shared R at every step
            _check_all(good, got, "%s %s beside a singular seed%s" % (kernel, ds, " (chunked)" if chunked else ""), seeds=(0, 2))
        finally:
            pool.close()


def test_misaligned_structured_problem_runs_the_dense_kernel():
    """A and B of a structured problem uploaded 8 bytes into a larger buffer: the plan says dense (the structured kernel's 16-byte loads need
    a 16-byte boundary), and the results are the reference's."""
    from trep_amd import _lib
    L = _lib.lib()
    ds, N, S = (9, 4, 5), 6, 2
    pr = lq_special_problem(ds, N, S, "misaligned")
    nX, nU, nxh = pr["nX"], pr["nU"], pr["nxh"]
    pool = device_pool()
    try:
        dev = dict((k, pool.upload(pr[k])) for k in ("Q", "Qf", "R", "q", "r", "hz"))
        for name in ("A", "B"):
            buf = pool.upload(np.concatenate([[np.nan], pr[name].ravel(), [np.nan]]))
            assert buf.ptr % 16 == 0
            dev[name] = buf.ptr + 8
        make = lambda: lq_struct(S, N, nX, nU, dev, hz=(nxh + nU, nxh), ds=ds)
        out = LqOutputs(pool, S, N, nX, nU)
        assert lq_plan(out.bind(make()))[1] == (1, 2, 20)
        got, _ = _sweep(L, pool, make, S, N, nX, nU, kernel=1, outputs=out)
        assert (got[4] == OK).all()
        _check_all(pr, got, "misaligned structured problem")
    finally:
        pool.close()
