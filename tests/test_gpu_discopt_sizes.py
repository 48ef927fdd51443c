"""The smaller discopt kernels over their sizes: tg_adjoint_sweep, tg_quadratic_cost (matrix-core kernel and the VALU kernel behind
TREPAMD_COST_LEGACY=1), tg_quadratic_cost_gradients, tg_armijo_candidates, tg_copy_rows and tg_tangent_rollout on pointers that are
not 16-byte aligned -- against the long-double formulas of tests/lq_reference.py.  Bounds by the rule of test_gpu_lq_classes.py:
max(64 e_ref, 1e-13), e_ref being the distance of the fp64 numpy evaluation of the same formula from the long-double one."""
import numpy as np
import pytest

import lq_reference as ref
from common import device_pool

pytestmark = pytest.mark.gpu
ERR_UNSUPPORTED = -3
# nX over {1, 5, 16, 17, 48, 64, 65, 96}, nU over {1, 4, 17, 32, 33, 64}, N over {1, 15, 16, 17, 33}: horizons shorter than, equal to and
# just over one and two 16-step tile rows, nU > nX once
SIZES = [(1, 1, 1), (5, 4, 15), (16, 17, 16), (17, 32, 17), (48, 33, 33), (48, 64, 15), (64, 33, 1), (64, 64, 16), (65, 4, 17), (96, 1, 33),
         (96, 32, 15), (96, 64, 1)]


def _ids(v):
    return "x".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def _held(got, want, host, tag):
    e_ref, e = ref.relerr(host, want), ref.relerr(got, want)
    print("%s: relerr %.3e, floor %.3e, bound %.3e" % (tag, e, e_ref, ref.bound(e_ref)))
    assert e < ref.bound(e_ref), (tag, e, e_ref)
    return e


@pytest.mark.parametrize("size", SIZES, ids=_ids)
def test_adjoint_sweep_sizes(size):
    from trep_amd import _lib
    L = _lib.lib()
    nX, nU, N = size
    S = 3
    rng = np.random.default_rng(1000 * nX + nU)
    A = rng.standard_normal((S, N, nX, nX)) * (0.9 / np.sqrt(nX)); B = rng.standard_normal((S, N, nX, nU)) * 0.3
    K = rng.standard_normal((S, N, nU, nX)) * 0.1
    q = rng.standard_normal((S, N + 1, nX)); r = rng.standard_normal((S, N, nU))
    sel = [2, 0]
    pool = device_pool()
    try:
        d = dict((k, pool.upload(v)) for k, v in dict(A=A, B=B, K=K, q=q, r=r).items())
        dZ, dsel = pool.upload(np.full((S, N, nX), np.nan)), pool.upload(np.array(sel, dtype=np.int32), np.int32)
        rc = L.tg_adjoint_sweep(0, len(sel), N, nX, nU, dsel.ptr, d["A"].ptr, d["B"].ptr, d["K"].ptr, d["q"].ptr, d["r"].ptr, dZ.ptr)
        lds = 8 * (nX * (nX | 1) + 2 * nX * nU + 2 * nX + nU)
        if nX * nU > 12 * 256 or lds > 160 * 1024 - 64:      # refused on the host, before a launch
            assert rc == ERR_UNSUPPORTED
            return
        _lib.check(rc)
        Z = dZ.get()
        assert np.isnan(Z[1]).all()
        for s in sel:
            host = np.zeros((N, nX))
            z = q[s, -1]
            for k in range(N - 1, -1, -1):
                host[k] = z
                z = q[s, k] - r[s, k].dot(K[s, k]) + z.dot(A[s, k] - B[s, k].dot(K[s, k]))
            _held(Z[s], ref.adjoint(A[s], B[s], K[s], q[s], r[s]), host, "adjoint %s seed %d" % (size, s))
    finally:
        pool.close()


@pytest.mark.parametrize("legacy", [False, True], ids=["mfma", "legacy"])
@pytest.mark.parametrize("group", [1, 3, 8])
@pytest.mark.parametrize("size", SIZES, ids=_ids)
def test_quadratic_cost_sizes(size, group, legacy, monkeypatch):
    """cost[t] of `group` consecutive trajectories per seed, the seeds picked by a selection list, both kernels."""
    from trep_amd import _lib
    from trep_amd.discopt import DCost
    L = _lib.lib()
    if legacy:
        monkeypatch.setenv("TREPAMD_COST_LEGACY", "1")
    nX, nU, N = size
    S, sel = 3, [2, 0]
    T = len(sel) * group
    rng = np.random.default_rng(77 * nX + nU + group)
    X, U = rng.standard_normal((T, N + 1, nX)), rng.standard_normal((T, N, nU))
    Xd, Ud = rng.standard_normal((S, N + 1, nX)), rng.standard_normal((S, N, nU))
    Q = rng.standard_normal((nX, nX)); Q = Q.dot(Q.T) / nX + np.eye(nX)
    R = rng.standard_normal((nU, nU)); R = R.dot(R.T) / nU + np.eye(nU)
    Qf = 2.0 * Q + np.eye(nX)
    pool = device_pool()
    try:
        d = dict((k, pool.upload(v)) for k, v in dict(X=X, U=U, Xd=Xd, Ud=Ud, Q=Q, R=R, Qf=Qf).items())
        dc, dsel = pool.upload(np.full((T + 1,), np.nan)), pool.upload(np.array(sel, dtype=np.int32), np.int32)
        rc = L.tg_quadratic_cost(0, T, group, dsel.ptr, N, nX, nU, d["X"].ptr, d["U"].ptr, d["Xd"].ptr, d["Ud"].ptr, d["Q"].ptr, d["R"].ptr,
                                 d["Qf"].ptr, dc.ptr)
        if legacy and 8 * (2 * nX * nX + nU * nU + 4 * (nX + nU) + 256) > 160 * 1024 - 64:
            assert rc == ERR_UNSUPPORTED
            return
        _lib.check(rc)
        cost = dc.get()
        assert np.isnan(cost[T])
        for t in range(T):
            s = sel[t // group]
            want = ref.cost(X[t], U[t], Xd[s], Ud[s], Q, R, Qf)
            host = DCost(Xd[s], Ud[s], Q, R, Qf).total(X[t], U[t])
            e_ref, e = abs(float(host - want) / float(want)), abs(float(cost[t] - want) / float(want))
            print("cost %s group %d trajectory %d: %.3e (floor %.3e)" % (size, group, t, e, e_ref))
            assert e < ref.bound(e_ref), (t, e, e_ref)
    finally:
        pool.close()


@pytest.mark.parametrize("size", SIZES, ids=_ids)
def test_cost_gradients_sizes(size):
    """q_k = (x_k - xd_k)' Q with a Q that is NOT symmetric (the transposed product would be another vector), r_k likewise."""
    from trep_amd import _lib
    L = _lib.lib()
    nX, nU, N = size
    S, sel = 3, [2, 0]
    rng = np.random.default_rng(5 * nX + nU)
    X, U = rng.standard_normal((S, N + 1, nX)), rng.standard_normal((S, N, nU))
    Xd, Ud = rng.standard_normal((S, N + 1, nX)), rng.standard_normal((S, N, nU))
    Q, R, Qf = rng.standard_normal((nX, nX)), rng.standard_normal((nU, nU)), rng.standard_normal((nX, nX))
    pool = device_pool()
    try:
        d = dict((k, pool.upload(v)) for k, v in dict(X=X, U=U, Xd=Xd, Ud=Ud, Q=Q, R=R, Qf=Qf).items())
        dq, dr = pool.upload(np.full((S, N + 1, nX), np.nan)), pool.upload(np.full((S, N, nU), np.nan))
        dsel = pool.upload(np.array(sel, dtype=np.int32), np.int32)
        _lib.check(L.tg_quadratic_cost_gradients(0, len(sel), N, nX, nU, dsel.ptr, d["X"].ptr, d["U"].ptr, d["Xd"].ptr, d["Ud"].ptr,
                                                 d["Q"].ptr, d["R"].ptr, d["Qf"].ptr, dq.ptr, dr.ptr))
        gq, gr = dq.get(), dr.get()
        assert np.isnan(gq[1]).all() and np.isnan(gr[1]).all()
        for s in sel:
            wq, wr = ref.cost_gradients(X[s], U[s], Xd[s], Ud[s], Q, R, Qf)
            hq = (X[s] - Xd[s]).dot(Q); hq[-1] = (X[s][-1] - Xd[s][-1]).dot(Qf)
            _held(gq[s], wq, hq, "gradient q %s seed %d" % (size, s))
            _held(gr[s], wr, (U[s] - Ud[s]).dot(R), "gradient r %s seed %d" % (size, s))
    finally:
        pool.close()


@pytest.mark.parametrize("size", SIZES[:6] + SIZES[-1:], ids=_ids)
def test_armijo_candidates_sizes(size):
    from trep_amd import _lib
    L = _lib.lib()
    nX, nU, N = size
    S, sel, M = 3, [2, 0], 5
    rng = np.random.default_rng(9 * nX + nU)
    X, U, dX, dU = (rng.standard_normal(sh) for sh in ((S, N + 1, nX), (S, N, nU), (S, N + 1, nX), (S, N, nU)))
    lam = 0.7 ** np.arange(M)
    pool = device_pool()
    try:
        d = dict((k, pool.upload(v)) for k, v in dict(X=X, U=U, dX=dX, dU=dU, lam=lam).items())
        dbX, dbU = pool.upload(np.full((len(sel) * M + 1, N + 1, nX), np.nan)), pool.upload(np.full((len(sel) * M + 1, N, nU), np.nan))
        dsel = pool.upload(np.array(sel, dtype=np.int32), np.int32)
        _lib.check(L.tg_armijo_candidates(0, len(sel), M, N, nX, nU, dsel.ptr, d["lam"].ptr, d["X"].ptr, d["U"].ptr, d["dX"].ptr, d["dU"].ptr,
                                          dbX.ptr, dbU.ptr))
        bX, bU = dbX.get(), dbU.get()
        assert np.isnan(bX[-1]).all() and np.isnan(bU[-1]).all()
        for i, s in enumerate(sel):
            wX = ref.ld(X[s])[None] + ref.ld(lam)[:, None, None] * ref.ld(dX[s])[None]
            wU = ref.ld(U[s])[None] + ref.ld(lam)[:, None, None] * ref.ld(dU[s])[None]
            _held(bX[i * M:(i + 1) * M], wX, X[s][None] + lam[:, None, None] * dX[s][None], "candidates X %s seed %d" % (size, s))
            _held(bU[i * M:(i + 1) * M], wU, U[s][None] + lam[:, None, None] * dU[s][None], "candidates U %s seed %d" % (size, s))
    finally:
        pool.close()


def test_copy_rows_beyond_the_grid_limit():
    """More rows than a grid has blocks in y (65 535): the kernel's row loop covers the rest; rows of one double, of 300 (two blocks in x
    at the last one's edge) and an identity index."""
    from trep_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(3)
    pool = device_pool()
    try:
        for n, width, total in ((70001, 1, 70010), (65536, 1, 65536), (7, 300, 9)):
            src = rng.standard_normal((total, width))
            src_rows = rng.permutation(total)[:n].astype(np.int32)
            dst_rows = rng.permutation(total)[:n].astype(np.int32)
            dsrc, ddst = pool.upload(src), pool.upload(np.full((total, width), np.nan))
            _lib.check(L.tg_copy_rows(0, n, width, pool.upload(dst_rows, np.int32).ptr, pool.upload(src_rows, np.int32).ptr, dsrc.ptr, ddst.ptr))
            want = np.full((total, width), np.nan)
            want[dst_rows] = src[src_rows]
            assert np.array_equal(ddst.get(), want, equal_nan=True), (n, width)
            ddst2 = pool.upload(np.full((total, width), np.nan))
            _lib.check(L.tg_copy_rows(0, n, width, None, None, dsrc.ptr, ddst2.ptr))
            want = np.full((total, width), np.nan)
            want[:n] = src[:n]
            assert np.array_equal(ddst2.get(), want, equal_nan=True), (n, width)
    finally:
        pool.close()


@pytest.mark.parametrize("nX,nU", [(80, 18), (32, 16), (96, 32), (6, 2)])
def test_tangent_rollout_on_misaligned_pointers(nX, nU):
    """A, B, K uploaded 8 bytes into a larger buffer: the plan says one column per thread (the paired variant loads 16 bytes at a time),
    and the results are those of the aligned, paired run to 1e-12 and the reference's."""
    from trep_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(10 * nX + nU)
    S, N = 3, 17
    A = rng.standard_normal((S, N, nX, nX)) * (0.9 / np.sqrt(nX)); B = rng.standard_normal((S, N, nX, nU)) * 0.3
    K = rng.standard_normal((S, N, nU, nX)) * 0.1; C = rng.standard_normal((S, N, nU))
    q = rng.standard_normal((S, N + 1, nX)); r = rng.standard_normal((S, N, nU))
    pool = device_pool()
    try:
        d = dict((k, pool.upload(v)) for k, v in dict(A=A, B=B, K=K, C=C, q=q, r=r).items())
        shifted = {}
        for k, v in dict(A=A, B=B, K=K).items():
            buf = pool.upload(np.concatenate([[np.nan], v.ravel(), [np.nan]]))
            assert buf.ptr % 16 == 0
            shifted[k] = buf.ptr + 8
        out = {}
        for name, ptrs, pair in (("aligned", dict((k, d[k].ptr) for k in "ABK"), 1), ("shifted", shifted, 0)):
            plan = np.zeros(6, dtype=np.int32)
            assert L.tg_tangent_rollout_plan(nX, nU, ptrs["A"], ptrs["B"], ptrs["K"], plan.ctypes.data_as(_lib._c_ip)) == 0
            assert plan[0] == 1 and plan[4] == pair, (name, plan)
            ddX, ddU, ddc = pool.upload(np.full((S, N + 1, nX), np.nan)), pool.upload(np.full((S, N, nU), np.nan)), pool.upload(np.full((S,), np.nan))
            _lib.check(L.tg_tangent_rollout(0, S, N, nX, nU, None, ptrs["A"], ptrs["B"], ptrs["K"], d["C"].ptr, d["q"].ptr, d["r"].ptr,
                                            ddX.ptr, ddU.ptr, ddc.ptr))
            out[name] = (ddX.get(), ddU.get(), ddc.get())
        for a, b in zip(out["aligned"], out["shifted"]):
            assert ref.relerr(b, a) < 1e-12
        for s in range(S):
            wX, wU, wc = ref.tangent(A[s], B[s], K[s], C[s], q[s], r[s])
            hX, hU = np.zeros((N + 1, nX)), np.zeros((N, nU))
            for k in range(N):
                hU[k] = -K[s, k].dot(hX[k]) - C[s, k]
                hX[k + 1] = A[s, k].dot(hX[k]) + B[s, k].dot(hU[k])
            hc = float(np.sum(q[s] * hX) + np.sum(r[s] * hU))
            for name in ("aligned", "shifted"):
                _held(out[name][0][s], wX, hX, "tangent dX %dx%d %s seed %d" % (nX, nU, name, s))
                _held(out[name][1][s], wU, hU, "tangent dU %dx%d %s seed %d" % (nX, nU, name, s))
                _held(np.array([out[name][2][s]]), np.array([wc]), np.array([hc]), "tangent dcost %dx%d %s seed %d" % (nX, nU, name, s))
    finally:
        pool.close()
