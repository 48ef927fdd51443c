"""Reference for the batched normal modes (BatchMidpointVI.normal_modes): the algorithm of include/trep_amd.h in numpy on the oracle
-- V_q, V_qq and M from lagrangian(q, 0), h and Dh as the projection's reference reads them, the multipliers' curvature from a
Richardson ladder on the oracle's Dh (common.fw_ladder: h = 4e-3 halved three times; a single central difference is not accurate
enough here) -- with the invariants that need no reference, the bounds, and the case table the CPU and the GPU tests share.  This
file is the specification: the kernel (csrc/mvi_modes.hpp, csrc/sym_eig.hpp) mirrors it decision for decision."""
import collections
import functools

import numpy as np

import common
import projection_reference as pr
from oracle.oracle import OracleMVI

OK, NOT_CONVERGED, SINGULAR = 0, 1, 2
RCOND, MAX_SWEEPS = 1e-9, 30
MARGIN = pr.MARGIN
TOL = pr.F_PARITY                     # the project's parity figure for first-order quantities of a pose, relative
INVARIANT_MIN = 1e-13
EPS = float(np.finfo(float).eps)
SKIP = 0.0625                         # a pair with |a_pq| <= SKIP eps scale is not rotated (sym_eig.hpp: kJacobiSkip)
GAP = 1e-3                            # a mode is compared as a vector if both neighbours are at least this far, relative to the scale
LADDER_H, LADDER_LEVELS = 4e-3, 2

Options = collections.namedtuple("Options", "mu_curvature vqq_sign mass_all z_first rival")
SPEC = Options(True, 1.0, False, False, False)
Modes = collections.namedtuple("Modes", "omega2 modes count rank mu residual sweeps status")


class Pose(object):
    """Everything the algorithm reads at a pose, from the oracle."""

    def __init__(self, d):
        self.d = d
        self.con = pr.Constraints(d)
        self.o = OracleMVI(d)
        self.nq, self.nd, self.nc = self.con.nq, self.con.nd, self.con.nc
        self.zero = np.zeros(self.nq)
        self._curv = {}

    def derivatives(self, q):
        """V_q, V_qq, M."""
        L = self.o.lagrangian(q, self.zero)
        return -L[0].copy(), -L[2].copy(), L[4].copy()

    def curvature(self, q, mu, F):
        """(sum_c mu_c h_c,qq over F x F by the ladder, the same from the ladder's rival): their difference is the floor."""
        key = (np.asarray(q).tobytes(), tuple(F))
        if key not in self._curv:
            T = np.zeros((2, len(F), self.nc, len(F)), dtype=np.longdouble)
            for j, k in enumerate(F):
                fun = lambda x: self.con(x)[1][:, F].astype(np.longdouble)
                T[0, j], T[1, j] = common.fw_ladder(fun, np.array(q, dtype=float), k, LADDER_H, LADDER_LEVELS)
            self._curv[key] = T
        T = self._curv[key]
        out = []
        for v in (0, 1):
            H = np.array([[float(np.dot(T[v, j, :, i], mu)) for j in range(len(F))] for i in range(len(F))]).reshape(len(F), len(F))
            out.append(0.5 * (H + H.T))
        return out


@functools.lru_cache(maxsize=None)
def pose_of(name):
    return Pose(common.build(name)[1])


def pivoted_qr(A, rcond):
    """Businger-Golub as csrc/lsq_solve.hpp does it: (Q [rows][rows], rank).  Norms summed from scratch, the smaller index wins a tie,
    the factorisation stops when the pivot norm is zero or <= rcond times the first."""
    R = np.array(A, dtype=float)
    rows, cols = R.shape
    Q = np.eye(rows)
    rank, nrm0 = 0, 0.0
    for k in range(min(rows, cols)):
        norms = (R[k:, k:] ** 2).sum(axis=0)
        j = k + int(np.argmax(norms))
        nrm = float(np.sqrt(norms[j - k]))
        if k == 0:
            nrm0 = nrm
        if not (nrm > 0.0 and nrm > rcond * nrm0):
            break
        rank = k + 1
        R[:, [k, j]] = R[:, [j, k]]
        alpha = R[k, k]
        beta = -np.copysign(nrm, alpha)
        v = R[k:, k] / (alpha - beta)
        v[0] = 1.0
        tau = (beta - alpha) / beta
        R[k:, :] -= tau * np.outer(v, v.dot(R[k:, :]))
        Q[:, k:] -= tau * np.outer(Q[:, k:].dot(v), v)
    return Q, rank


def pairs(m, n, s):
    """The pairs of set s in the round-robin ordering of m (even) players, those that hold an index >= n left out."""
    out = []
    for k in range(m // 2):
        a, b = (m - 1, s) if k == 0 else ((s + k) % (m - 1), (s - k) % (m - 1))
        p, q = min(a, b), max(a, b)
        if q < n:
            out.append((p, q))
    return out


def jacobi(C, max_sweeps=MAX_SWEEPS):
    """(eigenvalues in place order, Y, sweeps, converged): cyclic Jacobi, csrc/sym_eig.hpp."""
    A = np.array(C, dtype=float)
    n = len(A)
    Y = np.eye(n)
    m = (n + 1) & ~1
    sweeps = 0
    while True:
        big = float(np.abs(A).max(initial=0.0))
        off = float(np.abs(A - np.diag(np.diag(A))).max(initial=0.0))
        if off <= EPS * big:
            return np.diag(A).copy(), Y, sweeps, True
        if sweeps >= max_sweeps:
            return np.diag(A).copy(), Y, sweeps, False
        sweeps += 1
        cut = SKIP * EPS * big
        for s in range(m - 1):
            rot = []
            for p, q in pairs(m, n, s):
                c, sn = 1.0, 0.0
                if abs(A[p, q]) > cut:
                    theta = (A[q, q] - A[p, p]) / (2.0 * A[p, q])
                    t = np.copysign(1.0, theta) / (abs(theta) + np.hypot(theta, 1.0))
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    sn = t * c
                rot.append((p, q, c, sn))
            for p, q, c, sn in rot:
                x, y = A[p].copy(), A[q].copy()
                A[p], A[q] = c * x - sn * y, sn * x + c * y
            for p, q, c, sn in rot:
                for X in (A, Y):
                    x, y = X[:, p].copy(), X[:, q].copy()
                    X[:, p], X[:, q] = c * x - sn * y, sn * x + c * y
                if sn != 0.0:             # the entry the rotation was made for: exactly zero, not the rounding noise computed there
                    A[p, q] = A[q, p] = 0.0


def cholesky(M):
    """Unpivoted, right-looking; None where a pivot is not > 0 (a NaN fails it)."""
    A = np.array(M, dtype=float)
    n = len(A)
    for k in range(n):
        if not (A[k, k] > 0.0):
            return None
        A[k:, k] /= np.sqrt(A[k, k])
        for j in range(k + 1, n):
            A[j:, j] -= A[j:, k] * A[j, k]
    return np.tril(A)


def sym(A):
    return 0.5 * (A + A.T)


def default_free(ev):
    f = np.zeros(ev.nq, dtype=bool)
    f[:ev.nd] = True
    return f


def assemble(ev, q, free, mu=None, rcond=RCOND, opt=SPEC):
    """Steps 1-5: dict with F, D, M, K (over F), mu, residual, Z, rank, L, C -- or None where the pose is TG_SINGULAR."""
    F = np.flatnonzero(free)
    nF = len(F)
    if not np.isfinite(q).all():
        return None
    h, Dh = ev.con(q)
    Vq, Vqq, Mfull = ev.derivatives(q)
    D = Dh[:, F]
    M = Mfull[np.ix_(F, F)]
    if mu is None:
        mu = np.linalg.lstsq(D.T, -Vq[F], rcond=rcond)[0] if ev.nc and nF else np.zeros(ev.nc)
    mu = np.array(mu, dtype=float)
    residual = float(np.abs(Vq[F] + D.T.dot(mu)).max(initial=0.0))
    K = opt.vqq_sign * Vqq[np.ix_(F, F)]
    if opt.mu_curvature and ev.nc and np.any(mu):
        K = K + ev.curvature(q, mu, F)[1 if opt.rival else 0]
    if ev.nc and nF:
        Qf, r = pivoted_qr(D.T, rcond)
        Z = Qf[:, :nF - r] if opt.z_first else Qf[:, r:]
    else:
        Z, r = np.eye(nF), 0
    Mz = M
    if opt.mass_all:                  # mutation: M over every config, the held ones' columns folded onto the first free ones
        Mz = Mfull[:nF, :nF]
    Mr, Kr = sym(Z.T.dot(Mz).dot(Z)), sym(Z.T.dot(K).dot(Z))
    L = cholesky(Mr)
    if L is None:
        return None
    X = np.linalg.solve(L, Kr) if len(L) else Kr
    C = sym(np.linalg.solve(L, X.T).T) if len(L) else Kr
    if not np.isfinite(C).all() or not np.isfinite(mu).all():
        return None
    return dict(F=F, D=D, M=M, K=K, mu=mu, residual=residual, Z=Z, rank=r, L=L, C=C)


def finish(ev, parts, lam, Y):
    """Step 7 from eigenvalues and vectors of C: (omega2 [nF], modes [nF][nq])."""
    F, nF, nm = parts["F"], len(parts["F"]), len(lam)
    order = np.argsort(lam, kind="stable")
    Phi = parts["Z"].dot(np.linalg.solve(parts["L"].T, Y[:, order])) if nm else np.zeros((nF, 0))
    omega2, modes = np.zeros(nF), np.zeros((nF, ev.nq))
    omega2[:nm] = lam[order]
    for j in range(nm):
        v = Phi[:, j]
        modes[j, F] = v if v[int(np.argmax(np.abs(v)))] >= 0.0 else -v
    return omega2, modes


def modes_one(ev, q, free, mu=None, rcond=RCOND, max_sweeps=MAX_SWEEPS, opt=SPEC, lapack=False):
    nF = int(np.sum(free))
    parts = assemble(ev, np.array(q, dtype=float), free, mu, rcond, opt)
    if parts is None:
        return np.zeros(nF), np.zeros((nF, ev.nq)), 0, 0, np.zeros(ev.nc), 0.0, 0, SINGULAR
    if lapack:
        lam, Y = np.linalg.eigh(parts["C"])
        sweeps, conv = 0, True
    else:
        lam, Y, sweeps, conv = jacobi(parts["C"], max_sweeps)
    omega2, modes = finish(ev, parts, lam, Y)
    return omega2, modes, len(lam), parts["rank"], parts["mu"], parts["residual"], sweeps, OK if conv else NOT_CONVERGED


def normal_modes(name, Q, free=None, mu=None, rcond=RCOND, max_sweeps=MAX_SWEEPS, opt=SPEC, lapack=False, ev=None):
    ev = ev or pose_of(name)
    free = default_free(ev) if free is None else np.asarray(free, dtype=bool)
    rows = [modes_one(ev, Q[b], free, None if mu is None else mu[b], rcond, max_sweeps, opt, lapack) for b in range(len(Q))]
    return Modes(np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows], dtype=np.int32),
                 np.array([r[3] for r in rows], dtype=np.int32), np.array([r[4] for r in rows]).reshape(len(Q), ev.nc),
                 np.array([r[5] for r in rows]), np.array([r[6] for r in rows], dtype=np.int32), np.array([r[7] for r in rows], dtype=np.int32))


# ---- the invariants: no reference needed ------------------------------------------------------------------------------------
def invariants(name, Q, free, got, ev=None):
    """The worst over the batch of |Phi'M Phi - I|, |D Phi|, |K Phi - M Phi Lambda| projected off the range of D' relative to
    |K|max |Phi|max, and whether the held configs are zero; K with the multipliers `got` reports."""
    ev = ev or pose_of(name)
    free = default_free(ev) if free is None else np.asarray(free, dtype=bool)
    out = dict(orthonormal=0.0, tangent=0.0, eigen=0.0, held=True)
    for b in range(len(Q)):
        if got.status[b] == SINGULAR:
            continue
        parts = assemble(ev, Q[b], free, got.mu[b])
        nm = int(got.count[b])
        Phi = got.modes[b][:nm][:, parts["F"]].T
        lam = got.omega2[b][:nm]
        out["held"] = out["held"] and not got.modes[b][:, ~free].any() and not got.modes[b][nm:].any() and not got.omega2[b][nm:].any()
        if nm == 0:
            continue
        M, K, D, Z = parts["M"], parts["K"], parts["D"], parts["Z"]
        out["orthonormal"] = max(out["orthonormal"], float(np.abs(Phi.T.dot(M).dot(Phi) - np.eye(nm)).max()))
        out["tangent"] = max(out["tangent"], float(np.abs(D.dot(Phi)).max(initial=0.0)))
        res = Z.T.dot(K.dot(Phi) - M.dot(Phi) * lam)
        out["eigen"] = max(out["eigen"], float(np.abs(res).max() / (np.abs(K).max() * np.abs(Phi).max())))
    return out


# ---- the case table ---------------------------------------------------------------------------------------------------------
SYSTEMS = ("pendulum1", "pendulum5", "scissor4", "spring_arm", "mixed_loop", "spatial_loop", "ladder_mixed", "extensor_tendon", "puppet40")
RAGGED = 5
# Which draw of a case's seed the table uses (0 unless listed).  spatial_loop: its golden trajectories start at q = 0, where the mass
# matrix itself is singular (a zero eigenvalue: TG_SINGULAR in the reference and in the kernel alike); the table's rows are all
# TG_OK -- the statuses have tests of their own -- so a draw without that pose is taken.
DRAW = {"spatial_loop": 1}


def batch_size(name):
    return pr.batch_size(name)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """batch_size golden poses, each its own where there are enough; the last repeats row 0."""
    rng = np.random.default_rng(common.tb_seed("normal_modes", name, DRAW.get(name, 0)))
    poses = pr.golden_poses(name)
    n = batch_size(name)
    Q = poses[rng.choice(len(poses), size=n - 1, replace=len(poses) < n - 1)]
    return np.concatenate([Q, Q[:1]])


REPEAT = -1


@functools.lru_cache(maxsize=None)
def case_reference(name, kind="spec"):
    Q = case_inputs(name)
    if kind == "lapack":
        return normal_modes(name, Q, lapack=True)
    if kind == "rival":
        return normal_modes(name, Q, opt=SPEC._replace(rival=True))
    return normal_modes(name, Q)


def scale_of(ref):
    return np.maximum(1.0, np.abs(ref.omega2).max(axis=1))


def eig_error(got, ref):
    return float((np.abs(got.omega2 - ref.omega2).max(axis=1, initial=0.0) / scale_of(ref)).max())


@functools.lru_cache(maxsize=None)
def case_floors(name):
    """The two floors of the eigenvalue comparison: the change under the curvature ladder's floor, the spec's distance from LAPACK."""
    ref = case_reference(name)
    return dict(ladder=eig_error(case_reference(name, "rival"), ref), lapack=eig_error(case_reference(name, "lapack"), ref))


def eig_bound(name):
    f = case_floors(name)
    return max(TOL, MARGIN * max(f["ladder"], f["lapack"]))


@functools.lru_cache(maxsize=None)
def invariant_bounds(name):
    inv = invariants(name, case_inputs(name), None, case_reference(name))
    return dict((k, MARGIN * max(v, INVARIANT_MIN)) for k, v in inv.items() if k != "held")


def gaps(lam, scale):
    """Per mode the smaller gap to its neighbours, relative to the scale (inf for a single mode)."""
    g = np.full(len(lam), np.inf)
    d = np.diff(lam) / scale
    g[:-1] = np.minimum(g[:-1], d)
    g[1:] = np.minimum(g[1:], d)
    return g


def clusters(sep):
    """Runs of consecutive modes that are not separated: lists of indices."""
    out, cur = [], []
    for j, s in enumerate(sep):
        if s:
            if cur:
                out.append(cur)
            cur = []
        else:
            cur.append(j)
    if cur:
        out.append(cur)
    return out


def shape_errors(name, got, ref, rows=None, ev=None):
    """Per pose and mode the shape error in units of its bound: a separated mode as a vector up to sign, bound max(TOL, MARGIN
    floor) / gap with floor the larger of the spec's distance from LAPACK and its change under the curvature ladder's floor for that mode; the others by the projector of their cluster Phi_c Phi_c' M
    under max(TOL, MARGIN floor) / (the cluster's gap to the rest, at least GAP).  Returns (worst, modes compared by projector, modes)."""
    ev = ev or pose_of(name)
    lap, rival = case_reference(name, "lapack"), case_reference(name, "rival")
    rows = range(len(ref.omega2)) if rows is None else rows
    free = default_free(ev)
    worst, by_projector, total = 0.0, 0, 0
    for i, b in enumerate(rows):
        nm = int(ref.count[b])
        if nm == 0 or ref.status[b] == SINGULAR:
            continue
        total += nm
        lam, scale = ref.omega2[b][:nm], scale_of(ref)[b]
        g = gaps(lam, scale)
        sep = g >= GAP
        M = assemble(ev, case_inputs(name)[b], free, ref.mu[b])["M"]
        F = np.flatnonzero(free)

        def dist(A, B, j):      # relative to the shape's own size (an M-orthonormal shape of a light mode is large)
            size = max(1.0, np.abs(B.modes[b][j]).max())
            return min(np.abs(A.modes[b if A is not got else i][j] - s * B.modes[b][j]).max() for s in (1.0, -1.0)) / size
        for j in np.flatnonzero(sep):
            floor = max(dist(lap, ref, j), dist(rival, ref, j))
            bound = max(TOL, MARGIN * floor) / min(g[j], 1.0)
            worst = max(worst, dist(got, ref, j) / bound)
        for c in clusters(sep):
            by_projector += len(c)
            P = lambda X, row: X.modes[row][c][:, F].T.dot(X.modes[row][c][:, F]).dot(M)
            out_gap = abs(lam[c[0]] - lam[c[0] - 1]) / scale if c[0] > 0 else np.inf
            if c[-1] + 1 < nm:
                out_gap = min(out_gap, abs(lam[c[-1] + 1] - lam[c[-1]]) / scale)
            floor = max(float(np.abs(P(lap, b) - P(ref, b)).max()), float(np.abs(P(rival, b) - P(ref, b)).max()))
            bound = max(TOL, MARGIN * floor) / min(max(out_gap, GAP), 1.0)
            worst = max(worst, float(np.abs(P(got, i) - P(ref, b)).max()) / bound)
    return worst, by_projector, total


def sign_rule_errors(got):
    """Modes whose largest component leads the runner-up by a tenth or more and is not positive."""
    bad = 0
    for b in range(len(got.modes)):
        for j in range(int(got.count[b])):
            v = got.modes[b][j]
            a = np.sort(np.abs(v))
            if len(a) > 1 and a[-1] > 0 and a[-2] <= 0.9 * a[-1] and v[int(np.argmax(np.abs(v)))] <= 0.0:
                bad += 1
            if len(a) == 1 and v[0] < 0.0:
                bad += 1
    return bad


def compare(name, got, rows=None):
    """The checks of an implementation of the same algorithm against the reference, shared by the emulation and the device tests;
    `rows`: the table's rows `got` answers (default: all).  Returns the figures it asserted on."""
    ref = case_reference(name)
    Q = case_inputs(name)
    pick = np.arange(len(Q)) if rows is None else np.asarray(rows)
    sub = Modes(*[getattr(ref, k)[pick] for k in Modes._fields])
    inv = invariants(name, Q[pick], None, got)
    ib = invariant_bounds(name)
    shape, by_projector, total = shape_errors(name, got, ref, list(pick))
    fig = dict(eig_error=eig_error(got, sub), eig_bound=eig_bound(name), floors=case_floors(name), shape_in_bounds=shape,
               by_projector=by_projector, modes=total, sweeps=[int(got.sweeps.max(initial=0)), int(ref.sweeps.max(initial=0))],
               mu_error=float(np.abs(got.mu - sub.mu).max(initial=0.0)), invariants=dict((k, inv[k]) for k in ib), invariant_bounds=ib)
    print(name, fig)
    assert np.array_equal(got.status, sub.status) and (sub.status == OK).all(), (got.status, sub.status)
    assert np.array_equal(got.count, sub.count) and np.array_equal(got.rank, sub.rank)
    assert (np.abs(got.sweeps.astype(int) - sub.sweeps) <= 1).all(), (got.sweeps, sub.sweeps)
    assert 2 * int(ref.sweeps.max(initial=0)) < MAX_SWEEPS
    assert fig["eig_error"] <= fig["eig_bound"]
    assert inv["held"] and all(inv[k] <= ib[k] for k in ib), (inv, ib)
    assert shape <= 1.0
    assert sign_rule_errors(got) == 0
    return fig
