"""Extended-precision reference of the discopt sweeps, for the tests only.

The recursions of trep_amd.discopt.dlqr (solve_tv_lqr / solve_tv_lq) with the Newton-model weights assembled like
tg_lq_problem describes them, the adjoint, the tangent rollout with its directional derivative and the quadratic cost with
its gradients -- all in np.longdouble (80-bit x87: 64-bit mantissa, eps = 1.08e-19) with numpy's products and an own Gauss-Jordan with partial pivoting for gamma (numpy's LAPACK bindings do not take long double).  A fp64 sweep, on
the host or on the GPU, is judged by its distance from this one; test_lq_reference_cpu.py pins it to dlqr.py and fails on a
platform whose long double is not wider than fp64.
"""
import numpy as np

LD = np.longdouble


def ld(a):
    return None if a is None else np.asarray(a, dtype=LD)


def gauss_jordan(G, rhs):
    """Solve G X = rhs with Gauss-Jordan elimination and partial pivoting (largest magnitude in the column), in long double."""
    G = np.array(G, dtype=LD)
    n = G.shape[0]
    M = np.concatenate([G, np.array(rhs, dtype=LD).reshape(n, -1)], axis=1)
    for c in range(n):
        piv = c + int(np.argmax(np.abs(M[c:, c])))
        if M[piv, c] == 0:
            raise np.linalg.LinAlgError("singular matrix")
        if piv != c:
            M[[c, piv]] = M[[piv, c]]
        M[c] = M[c] / M[c, c]
        f = M[:, c].copy()
        f[c] = 0
        M -= f[:, None] * M[c][None, :]
    return M[:, n:]


class Weights(object):
    """Q_k, S_k, R_k of tg_lq_problem for one seed: Q [nX][nX] or [N][nX][nX] (a step stride), R likewise, terminal Qf, and
    optionally HZ [N][hz_R][hz_R] with the state part in its first nxh rows / columns and the input part in the nU after them:
    Q_k += HZ[:nxh, :nxh], S_k = HZ[:nxh, nxh:nxh + nU] (zero rows below), R_k += HZ[nxh:nxh + nU, nxh:nxh + nU]."""

    def __init__(self, Q, Qf, R, hz=None, nxh=0, dtype=LD):
        self.dtype = dtype
        self.Q, self.Qf, self.R = (np.asarray(x, dtype=dtype) for x in (Q, Qf, R))
        self.hz = None if hz is None else np.asarray(hz, dtype=dtype)
        self.nxh = nxh
        self.nX, self.nU = self.Qf.shape[0], self.R.shape[-1]

    def Qk(self, k):
        M = (self.Q[k] if self.Q.ndim == 3 else self.Q).copy()
        if self.hz is not None:
            M[:self.nxh, :self.nxh] += self.hz[k][:self.nxh, :self.nxh]
        return M

    def Sk(self, k):
        M = np.zeros((self.nX, self.nU), dtype=self.dtype)
        if self.hz is not None:
            M[:self.nxh, :] = self.hz[k][:self.nxh, self.nxh:self.nxh + self.nU]
        return M

    def Rk(self, k):
        M = (self.R[k] if self.R.ndim == 3 else self.R).copy()
        if self.hz is not None:
            M += self.hz[k][self.nxh:self.nxh + self.nU, self.nxh:self.nxh + self.nU]
        return M


def gamma_at(A_k, B_k, P, w, k):
    """gamma_k = R_k + B_k' P B_k in long double."""
    B_k = ld(B_k)
    return w.Rk(k) + B_k.T.dot(ld(P)).dot(B_k)


def solve_tv_lq(A, B, q, r, w, k_begin=0, k_end=None, terminal=None, keep=()):
    """The backward sweep over the steps k_end - 1 ... k_begin (default: the whole horizon) of one seed.  q = r = None: the
    LQR recursion (no affine terms; C and b come back as None).  terminal = (P, b) at step k_end (default Qf, q_N).
    Returns K [N][nU][nX], C [N][nU], P, b at step k_begin (rows of steps outside the range are zero), and a dict
    {k: (P_k, b_k, gamma_k)} for the steps listed in `keep` (P_k, b_k: the values ENTERING step k - 1, i.e. at step k;
    gamma_k: the matrix step k inverts)."""
    A, B = ld(A), ld(B)
    N, nX, nU = A.shape[0], A.shape[1], B.shape[2]
    affine = q is not None
    q, r = ld(q), ld(r)
    k_end = N if k_end is None or k_end == 0 else k_end
    if terminal is not None:
        P, b = ld(terminal[0]), (ld(terminal[1]) if affine else None)
    else:
        assert k_end == N
        P, b = w.Qf.astype(LD), (q[N] if affine else None)
    K = np.zeros((N, nU, nX), dtype=LD)
    C = np.zeros((N, nU), dtype=LD) if affine else None
    kept = {}
    for k in range(k_end - 1, k_begin - 1, -1):
        BtP = B[k].T.dot(P)
        gamma = w.Rk(k) + BtP.dot(B[k])
        if k in keep:
            kept[k] = (P.copy(), None if b is None else b.copy(), gamma.copy())
        K_part = BtP.dot(A[k]) + w.Sk(k).T
        if affine:
            sol = gauss_jordan(gamma, np.column_stack([B[k].T.dot(b) + r[k], K_part]))
            C[k], K[k] = sol[:, 0], sol[:, 1:]
            b = q[k] - K[k].T.dot(r[k]) + (A[k].T - K[k].T.dot(B[k].T)).dot(b)
        else:
            K[k] = gauss_jordan(gamma, K_part)
        P = w.Qk(k) + A[k].T.dot(P).dot(A[k]) - K_part.T.dot(K[k])
        P = (P + P.T) / 2
    return K, C, P, b, kept


def adjoint(A, B, K, q, r):
    """Z[k] = z_{k+1}; z_k = q_k - K_k' r_k + (A_k - B_k K_k)' z_{k+1}, z_N = q_N."""
    A, B, K, q, r = (ld(x) for x in (A, B, K, q, r))
    N = A.shape[0]
    Z = np.zeros((N, A.shape[1]), dtype=LD)
    z = q[N]
    for k in range(N - 1, -1, -1):
        Z[k] = z
        z = q[k] - K[k].T.dot(r[k]) + (A[k] - B[k].dot(K[k])).T.dot(z)
    return Z


def tangent(A, B, K, C, q, r):
    """dU_k = -K_k dX_k - C_k, dX_{k+1} = A_k dX_k + B_k dU_k, dX_0 = 0; dcost = sum_k q_k.dX_k + r_k.dU_k."""
    A, B, K, C, q, r = (ld(x) for x in (A, B, K, C, q, r))
    N, nX, nU = A.shape[0], A.shape[1], B.shape[2]
    dX, dU = np.zeros((N + 1, nX), dtype=LD), np.zeros((N, nU), dtype=LD)
    for k in range(N):
        dU[k] = -K[k].dot(dX[k]) - C[k]
        dX[k + 1] = A[k].dot(dX[k]) + B[k].dot(dU[k])
    return dX, dU, (q * dX).sum() + (r * dU).sum()


def cost(X, U, Xd, Ud, Q, R, Qf):
    """sum_k 1/2 (x - xd)' Q (x - xd) + 1/2 (u - ud)' R (u - ud) + 1/2 (x_N - xd_N)' Qf (x_N - xd_N)."""
    X, U, Xd, Ud, Q, R, Qf = (ld(x) for x in (X, U, Xd, Ud, Q, R, Qf))
    dx, du = X - Xd, U - Ud
    N = U.shape[0]
    c = LD(0)
    for k in range(N):
        c += dx[k].dot(Q).dot(dx[k]) / 2 + du[k].dot(R).dot(du[k]) / 2
    return c + dx[N].dot(Qf).dot(dx[N]) / 2


def cost_gradients(X, U, Xd, Ud, Q, R, Qf):
    """q_k = (x_k - xd_k)' Q (row N with Qf), r_k = (u_k - ud_k)' R -- row vector times matrix: Q need not be symmetric."""
    X, U, Xd, Ud, Q, R, Qf = (ld(x) for x in (X, U, Xd, Ud, Q, R, Qf))
    dx, du = X - Xd, U - Ud
    gq = dx.dot(Q)
    gq[-1] = dx[-1].dot(Qf)
    return gq, du.dot(R)


def relerr(a, ref):
    """max |a - ref| / max(1, max |ref|) like common.relerr, evaluated in long double."""
    a, ref = ld(a), ld(ref)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - ref).max() / max(LD(1), np.abs(ref).max()))


def entry_relerr(a, ref):
    """max over the entries of |a - ref| / (|ref| + rowmax |ref|), rows along the last axis: an entry is held to the size of its own
    row (one input's gains), so a wrong small entry is not hidden by a large row elsewhere in the array."""
    a, ref = ld(a), ld(ref)
    if a.size == 0:
        return 0.0
    rowmax = np.abs(ref).max(axis=-1, keepdims=True)
    den = np.abs(ref) + rowmax
    err = np.abs(a - ref)
    ok = den > 0
    if (err[~ok] != 0).any():
        return float("inf")
    return float((err[ok] / den[ok]).max()) if ok.any() else 0.0


def bound(e_ref):
    """The bound of a fp64 kernel's output whose fp64 host sweep sits e_ref from long double: max(64 e_ref, 1e-13)."""
    return max(64.0 * float(e_ref), 1e-13)
