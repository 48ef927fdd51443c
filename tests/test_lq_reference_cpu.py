"""The long-double reference of the discopt sweeps (tests/lq_reference.py) pinned to the host implementation it restates (dlqr.py,
DCost, the formulas of doptimizer.py), the floors e_ref = relerr(fp64 host sweep, long double) of every case the GPU tests run --
their bounds are max(64 e_ref, 1e-13) --, and the conditioning of the problems that steer the LQ kernels through their solver
branches (indefinite gamma, a zero leading pivot): the reference alone must pass them comfortably.  No GPU."""
import numpy as np
import pytest

import lq_reference as ref
from common import (LQ_CASES, LQ_MODES, LQ_SPECIAL_SIZES, host_lq, lq_case_id, lq_case_reference, lq_indefinite_problem,
                    lq_special_reference, lq_zero_pivot_problem, random_lq_problem, relerr)


def test_long_double_is_wider_than_fp64():
    """80-bit x87 long double (eps 1.08e-19).  Where long double is fp64 (eps 2.2e-16) every comparison of this suite would hold fp64
    against fp64: fail loudly instead."""
    assert np.finfo(np.longdouble).eps < 2e-19
    x = ref.ld(1) + ref.ld(2) ** -60
    assert x != 1 and (x.dot(x) if x.ndim else x * x) != 1            # ... and numpy computes in it
    a = ref.ld(np.ones((3, 3))) * (1 + ref.ld(2) ** -60)
    assert (a.dot(a) != 3).all()


def test_gauss_jordan_solves():
    rng = np.random.default_rng(3)
    for n in (1, 2, 9, 32, 64):
        G = rng.standard_normal((n, n))
        if n > 1:
            G[0, 0] = 0.0                               # needs the pivot search
        rhs = rng.standard_normal((n, 5))
        x = ref.gauss_jordan(G, rhs)
        assert x.dtype == np.longdouble
        assert float(np.abs(ref.ld(G).dot(x) - rhs).max()) < 1e-15 * np.linalg.cond(G)
        assert relerr(np.asarray(x, dtype=float), np.linalg.solve(G, rhs)) < 1e-13 * np.linalg.cond(G)
    with pytest.raises(np.linalg.LinAlgError):
        ref.gauss_jordan(np.zeros((2, 2)), np.ones(2))


@pytest.mark.parametrize("nX,nU,nxh,N", [(4, 1, 4, 40), (18, 3, 12, 25), (33, 9, 20, 12), (80, 18, 62, 8)])
def test_sweeps_are_dlqr(nX, nU, nxh, N):
    rng = np.random.default_rng(nX)
    A, B, Q, Qf, R, q, r, hz = random_lq_problem(rng, 1, N, nX, nU, nxh)
    for mode in LQ_MODES:
        affine, newton = mode != "lqr", mode == "newton"
        host = host_lq(A[0], B[0], Q, Qf, R, q[0] if affine else None, r[0] if affine else None, hz[0] if newton else None, nxh)
        w = ref.Weights(Q, Qf, R, hz[0] if newton else None, nxh)
        K, C, P, b, _ = ref.solve_tv_lq(A[0], B[0], q[0] if affine else None, r[0] if affine else None, w)
        assert K.dtype == P.dtype == np.longdouble
        for h, x in zip(host, (K, C, P, b)):
            assert (h is None) == (x is None)
            if x is not None:
                assert ref.relerr(h, x) < 1e-13, mode
        # swept in chunks from the carried (P, b): the same operations, the same numbers
        cuts = [N, N - N // 3, N // 4, 0]
        term, Kc = None, np.zeros_like(K)
        for k1, k0 in zip(cuts[:-1], cuts[1:]):
            Kp, Cp, Pp, bp, kept = ref.solve_tv_lq(A[0], B[0], q[0] if affine else None, r[0] if affine else None, w, k_begin=k0, k_end=k1,
                                                   terminal=term, keep=(k0,))
            Kc[k0:k1] = Kp[k0:k1]
            term = (Pp, bp)
            assert kept[k0][2].shape == (nU, nU)
        assert np.array_equal(Kc, K) and np.array_equal(Pp, P) and (b is None or np.array_equal(bp, b))


def test_weights_with_step_axis_and_wide_curvature():
    rng = np.random.default_rng(11)
    N, nX, nU, nxh = 5, 7, 3, 4
    A, B, Q, Qf, R, q, r, hz = random_lq_problem(rng, 1, N, nX, nU, nxh)
    Qs = Q[None] * (1 + 0.1 * np.arange(N))[:, None, None]
    Rs = R[None] * (2 - 0.1 * np.arange(N))[:, None, None]
    wide = np.full((N, nxh + nU + 3, nxh + nU + 3), 1e300)
    wide[:, :nxh + nU, :nxh + nU] = hz[0]
    w = ref.Weights(Qs, Qf, Rs, wide, nxh)
    from trep_amd.discopt import dlqr

    def Qk(k):
        M = Qs[k].copy() if k < N else Qf
        if k < N:
            M[:nxh, :nxh] += hz[0][k][:nxh, :nxh]
        return M

    def Sk(k):
        M = np.zeros((nX, nU))
        M[:nxh] = hz[0][k][:nxh, nxh:]
        return M
    Kh, Ch, Ph, bh = dlqr.solve_tv_lq(A[0], B[0], q[0], r[0], Qk, Sk, lambda k: Rs[k] + hz[0][k][nxh:, nxh:])
    K, C, P, b, _ = ref.solve_tv_lq(A[0], B[0], q[0], r[0], w)
    assert ref.relerr(np.array(Kh), K) < 1e-13 and ref.relerr(Ph, P) < 1e-13 and ref.relerr(bh, b) < 1e-13 and np.abs(P).max() < 1e3


def test_adjoint_tangent_and_cost_are_the_host_formulas():
    from trep_amd.discopt import DCost
    rng = np.random.default_rng(5)
    N, nX, nU = 9, 11, 4
    A = rng.standard_normal((N, nX, nX)) / np.sqrt(nX); B = rng.standard_normal((N, nX, nU))
    K = 0.1 * rng.standard_normal((N, nU, nX)); C = rng.standard_normal((N, nU))
    q = rng.standard_normal((N + 1, nX)); r = rng.standard_normal((N, nU))
    Z = ref.adjoint(A, B, K, q, r)
    z = q[-1]
    for k in range(N - 1, -1, -1):
        assert ref.relerr(z, Z[k]) < 1e-14
        z = q[k] - r[k].dot(K[k]) + z.dot(A[k] - B[k].dot(K[k]))
    dX, dU, dc = ref.tangent(A, B, K, C, q, r)
    x, acc = np.zeros(nX), 0.0
    for k in range(N):
        u = -K[k].dot(x) - C[k]
        assert ref.relerr(x, dX[k]) < 1e-14 and ref.relerr(u, dU[k]) < 1e-14
        acc += q[k].dot(x) + r[k].dot(u)
        x = A[k].dot(x) + B[k].dot(u)
    assert abs(acc + q[N].dot(x) - float(dc)) < 1e-13 * max(1.0, abs(acc))
    X, U, Xd, Ud = rng.standard_normal((N + 1, nX)), rng.standard_normal((N, nU)), rng.standard_normal((N + 1, nX)), rng.standard_normal((N, nU))
    Q = rng.standard_normal((nX, nX)); Q = Q + Q.T; R = rng.standard_normal((nU, nU)); R = R + R.T; Qf = 2 * Q
    c = DCost(Xd, Ud, Q, R, Qf)
    assert abs(float(ref.cost(X, U, Xd, Ud, Q, R, Qf)) - c.total(X, U)) < 1e-13 * abs(c.total(X, U))
    gq, gr = ref.cost_gradients(X, U, Xd, Ud, Q, R, Qf)
    hq, hr = c.gradients(X, U)
    assert ref.relerr(hq, gq) < 1e-14 and ref.relerr(hr, gr) < 1e-14
    # a weight that is not symmetric: row vector times matrix, (x - xd)' Q
    Qn = rng.standard_normal((nX, nX))
    gq, _ = ref.cost_gradients(X, U, Xd, Ud, Qn, R, Qf)
    assert ref.relerr((X - Xd)[:-1].dot(Qn), gq[:-1]) < 1e-14 and ref.relerr(Qn.dot((X - Xd)[3]), gq[3]) > 1e-3


def test_entry_metric_sees_a_small_column():
    K = np.ones((2, 3, 4)); K[0, 1] = 1e-6
    bad = K.copy(); bad[0, 1, 2] = 2e-6
    assert ref.relerr(bad, K) < 1e-5 and ref.entry_relerr(bad, K) > 0.3
    assert ref.entry_relerr(K, K) == 0.0 and ref.entry_relerr(np.ones(3), np.zeros(3)) == float("inf")
    assert ref.bound(1e-15) == 1e-13 and ref.bound(1e-14) == 64e-14


@pytest.mark.parametrize("case", LQ_CASES, ids=lq_case_id)
def test_floor_of_every_case(case):
    """e_ref per output and mode, worst seed: what a correct fp64 sweep (LAPACK's, in another summation order than the kernels') is away
    from the long-double one.  A floor near 1e-13 would say the problem, not the arithmetic, limits the comparison: the cases stay
    below 2e-14, so no bound of the GPU tests is above 1.3e-12."""
    for mode in LQ_MODES:
        worst = [0.0] * 4
        for s in range(case.S):
            want, floors, bounds = lq_case_reference(case, mode, s)
            for i, e in enumerate(floors):
                assert (e is None) == (want[i] is None) == (mode == "lqr" and i in (1, 3))
                if e is not None:
                    worst[i] = max(worst[i], e)
                    assert bounds[i] == max(64 * e, 1e-13)
        print("%s %s: e_ref K %.2e C %.2e P0 %.2e b0 %.2e" % ((lq_case_id(case), mode) + tuple(worst)))
        assert max(worst) < 2e-14, (mode, worst)


@pytest.mark.parametrize("ds", LQ_SPECIAL_SIZES, ids=str)
def test_indefinite_problem_is_well_posed(ds):
    pr = lq_indefinite_problem(ds)
    h = pr["nU"] // 2
    for s in range(pr["S"]):
        want, floors, bounds, kept = lq_special_reference(pr, s, keep=range(pr["N"]))
        assert sorted(kept) == list(range(pr["N"]))
        for k, (_, _, gamma) in kept.items():
            g = np.asarray(gamma, dtype=np.float64)
            ev = np.linalg.eigvalsh((g + g.T) / 2)
            assert np.linalg.cond(g) < 1e3, (s, k, np.linalg.cond(g))
            assert (ev <= -1.0 + 1e-9).sum() >= h and (ev > 0).any(), (s, k, ev)       # indefinite, the negative part of size O(1)
            assert np.abs(ev).min() > 0.1 and np.abs(ev).max() < 100
        print(ds, s, "e_ref", floors)
        assert max(floors) < 2e-14


@pytest.mark.parametrize("ds", LQ_SPECIAL_SIZES, ids=str)
@pytest.mark.parametrize("N,k_star", [(6, 5), (9, 4)])
def test_zero_pivot_problem_is_well_posed(ds, N, k_star):
    pr = lq_zero_pivot_problem(ds, N, 2, k_star)
    for s in range(pr["S"]):
        want, floors, bounds, kept = lq_special_reference(pr, s, keep=(k_star,))
        g = np.asarray(kept[k_star][2], dtype=np.float64)
        assert np.linalg.cond(g) < 1e3
        # the guard of the unpivoted factorisation is |pivot| > 2^-20 of the row's largest entry: missed by six decades
        assert abs(g[0, 0]) < 2.0 ** -20 * np.abs(g[0]).max() * 1e-6, g[0, 0]
        print(ds, k_star, s, "gamma00 %.2e cond %.1f e_ref" % (g[0, 0], np.linalg.cond(g)), floors)
        assert max(floors) < 2e-14
