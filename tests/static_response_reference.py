"""Reference for the batched static response (BatchMidpointVI.static_response): the algorithm of include/trep_amd.h in numpy on the
oracle -- V_q and V_qq from lagrangian(q, 0), h and Dh as the projection's reference reads them, the multipliers' curvature over ALL
config pairs from the Richardson ladder of normal_modes_reference (common.fw_ladder, with its rival) -- with the invariants that need
no reference, the bounds, and the case table the CPU and the GPU tests share.  This file is the specification: the kernel
(csrc/mvi_response.hpp) mirrors it decision for decision.

Per pose, F the free configs, H the held ones, E the driven held configs:
  mu supplied or the minimum-norm minimiser of |V_q[F] + D_F' mu| under rcond; W = V_qq + sum_c mu_c h_c,qq;
  D_F' P = Q [T; 0] by column-pivoted Householder QR under rcond, rank r, Q = [Q1 Z]; the pseudo-inverse of D_F' is that of its
  rank-r part Q1 (Q1' D_F'); K_r = Z' W_FF Z symmetrised, Cholesky (none: TG_SINGULAR);
  X_p = -D_F^+ D_H E, X = X_p + Z K_r^-1 Z' (-W_FH E - W_FF X_p), dmu = -(D_F')^+ (W_FF X + W_FH E), defect = |D_F X + D_H E|inf;
  C = Z K_r^-1 Z', R = (D_F')^+ (I - W_FF C)."""
import collections
import functools

import numpy as np

import common
import equilibrium_reference as er
import normal_modes_reference as nr
import projection_reference as pr

OK, NOT_CONVERGED, SINGULAR = 0, 1, 2
RCOND = 1e-9
MARGIN = pr.MARGIN
TOL = pr.F_PARITY
INVARIANT_MIN = 1e-13
ARRAYS = ("dq", "dmu", "compliance", "reaction", "mu", "residual", "defect")

# mutations switch single terms off; rival: the ladder's rival curvature; lapack: pinv / svd / solve in place of QR and Cholesky
Options = collections.namedtuple("Options", "fh_curvature fh_vqq dh_term ff_curvature rival lapack")
SPEC = Options(True, True, True, True, False, False)
Response = collections.namedtuple("Response", "dq dmu compliance reaction rank mu residual defect status")


def pose_of(name):
    return nr.pose_of(name)


def parts_of(ev, q, free, mu=None, rcond=RCOND, opt=SPEC):
    """Steps 1-5: dict with F, H, Dh, mu, residual, W, Z, rank, pinv ((D_F')^+, [nc][nF]), L -- or None where the pose is TG_SINGULAR."""
    free = np.asarray(free, dtype=bool)
    F, H = np.flatnonzero(free), np.flatnonzero(~free)
    nF = len(F)
    if not np.isfinite(q).all():
        return None
    _, Dh = ev.con(q)
    Vq, Vqq, _ = ev.derivatives(q)
    D = Dh[:, F]
    if mu is None:
        mu = np.linalg.lstsq(D.T, -Vq[F], rcond=rcond)[0] if ev.nc and nF else np.zeros(ev.nc)
    mu = np.array(mu, dtype=float)
    if not np.isfinite(mu).all():
        return None
    residual = float(np.abs(Vq[F] + D.T.dot(mu)).max(initial=0.0))
    every = np.arange(ev.nq)
    curv = ev.curvature(q, mu, every)[1 if opt.rival else 0] if ev.nc and np.any(mu) else np.zeros((ev.nq, ev.nq))
    W = nr.sym(Vqq) + curv
    fh = np.ix_(F, H)
    if not opt.fh_curvature:
        W[fh] -= curv[fh]
    if not opt.fh_vqq:
        W[fh] -= nr.sym(Vqq)[fh]
    if not opt.ff_curvature:
        W[np.ix_(F, F)] -= curv[np.ix_(F, F)]
    if ev.nc and nF:
        if opt.lapack:
            U, s, _ = np.linalg.svd(D.T, full_matrices=True)
            r = int((s > rcond * s.max(initial=0.0)).sum()) if len(s) and s.max() > 0.0 else 0
            Z = U[:, r:]
            pinv = np.linalg.pinv(D.T, rcond=rcond) if r else np.zeros((ev.nc, nF))
        else:
            Qf, r = nr.pivoted_qr(D.T, rcond)
            Q1, Z = Qf[:, :r], Qf[:, r:]
            pinv = np.linalg.lstsq(Q1.T.dot(D.T), Q1.T, rcond=None)[0] if r else np.zeros((ev.nc, nF))
    else:
        Z, r, pinv = np.eye(nF), 0, np.zeros((ev.nc, nF))
    Kr = nr.sym(Z.T.dot(W[np.ix_(F, F)]).dot(Z))
    L = nr.cholesky(Kr)
    if L is None:
        return None
    return dict(F=F, H=H, Dh=Dh, mu=mu, residual=residual, W=W, Z=Z, rank=r, pinv=pinv, L=L, Kr=Kr, lapack=opt.lapack)


def reduced_solve(parts, M):
    """K_r^-1 M."""
    if not len(parts["L"]):
        return M
    if parts["lapack"]:
        return np.linalg.solve(parts["Kr"], M)
    return np.linalg.solve(parts["L"].T, np.linalg.solve(parts["L"], M))


def response_one(ev, q, free, drive, mu=None, rcond=RCOND, compliance=True, opt=SPEC):
    """One pose: the nine outputs, arrays in the shapes of the ABI."""
    nq, nc, nD = ev.nq, ev.nc, len(drive)
    zero = (np.zeros((nD, nq)), np.zeros((nD, nc)), np.zeros((nq, nq)) if compliance else None, np.zeros((nq, nc)) if compliance else None,
            0, np.zeros(nc), 0.0, 0.0, SINGULAR)
    parts = parts_of(ev, np.array(q, dtype=float), free, mu, rcond, opt)
    if parts is None:
        return zero
    F, Z, W, pinv, Dh = parts["F"], parts["Z"], parts["W"], parts["pinv"], parts["Dh"]
    nF = len(F)
    D, Wff = Dh[:, F], W[np.ix_(F, F)]
    b = Dh[:, drive] if opt.dh_term else np.zeros((nc, nD))
    wfh = W[np.ix_(F, drive)]
    Xp = -pinv.T.dot(b)
    X = Xp + Z.dot(reduced_solve(parts, Z.T.dot(-wfh - Wff.dot(Xp))))
    y = -pinv.dot(Wff.dot(X) + wfh)
    defect = float(np.abs(D.dot(X) + Dh[:, drive]).max(initial=0.0))
    dq, dmu = np.zeros((nD, nq)), y.T.copy()
    dq[:, F] = X.T
    dq[np.arange(nD), drive] = 1.0
    out = [dq, dmu, None, None, parts["rank"], parts["mu"], parts["residual"], defect, OK]
    if compliance:
        Cf = Z.dot(reduced_solve(parts, Z.T))
        Rf = pinv.dot(np.eye(nF) - Wff.dot(Cf))
        C, R = np.zeros((nq, nq)), np.zeros((nq, nc))
        C[np.ix_(F, F)] = Cf
        R[F] = Rf.T
        out[2], out[3] = C, R
    if not all(np.isfinite(a).all() for a in out[:4] if a is not None):
        return zero
    return tuple(out)


def default_drive(free):
    return np.flatnonzero(~np.asarray(free, dtype=bool))


def static_response(name, Q, free, drive=None, mu=None, rcond=RCOND, compliance=True, opt=SPEC, ev=None):
    ev = ev or pose_of(name)
    free = np.asarray(free, dtype=bool)
    drive = default_drive(free) if drive is None else np.asarray(drive, dtype=int)
    rows = [response_one(ev, Q[b], free, drive, None if mu is None else mu[b], rcond, compliance, opt) for b in range(len(Q))]
    B, nD = len(Q), len(drive)
    col = lambda k: [r[k] for r in rows]
    return Response(np.array(col(0)).reshape(B, nD, ev.nq), np.array(col(1)).reshape(B, nD, ev.nc),
                    np.array(col(2)).reshape(B, ev.nq, ev.nq) if compliance else None, np.array(col(3)).reshape(B, ev.nq, ev.nc) if compliance else None,
                    np.array(col(4), dtype=np.int32), np.array(col(5)).reshape(B, ev.nc), np.array(col(6)), np.array(col(7)), np.array(col(8), dtype=np.int32))


# ---- the invariants: no reference needed ------------------------------------------------------------------------------------
DEFECT_ZERO = 1e-9      # a pose whose reference defect is under this has constraints that follow the drive


def invariants(name, Q, free, got, drive=None, ev=None, rival=False):
    """The worst over the batch of |C - C'|, |D_F C|, |C W_FF C - C|, |D_F X + D_H E| (where the defect is zero),
    |Z'(W_FF X + W_FH E)|, and whether the held rows and columns are exactly as defined; W with the multipliers `got` reports and
    the curvature of the ladder (rival: of its rival -- the evaluator's own W carries the ladder's floor, and the difference of the
    two evaluations of one answer is its measure)."""
    ev = ev or pose_of(name)
    free = np.asarray(free, dtype=bool)
    drive = default_drive(free) if drive is None else np.asarray(drive, dtype=int)
    out = dict(symmetric=0.0, tangent=0.0, projector=0.0, follows=0.0, stationary=0.0, held=True)
    for b in range(len(Q)):
        if got.status[b] == SINGULAR:
            continue
        parts = parts_of(ev, Q[b], free, got.mu[b], opt=SPEC._replace(rival=rival))
        F, H, Z, W, Dh = parts["F"], parts["H"], parts["Z"], parts["W"], parts["Dh"]
        D, Wff, wfh = Dh[:, F], W[np.ix_(F, F)], W[np.ix_(F, drive)]
        X = got.dq[b][:, F].T
        unit = np.zeros((len(drive), ev.nq))
        unit[np.arange(len(drive)), drive] = 1.0
        out["held"] = out["held"] and np.array_equal(got.dq[b][:, H], unit[:, H])
        if got.defect[b] <= DEFECT_ZERO:
            out["follows"] = max(out["follows"], float(np.abs(D.dot(X) + Dh[:, drive]).max(initial=0.0)))
        out["stationary"] = max(out["stationary"], float(np.abs(Z.T.dot(Wff.dot(X) + wfh)).max(initial=0.0)))
        if got.compliance is not None:
            C = got.compliance[b]
            Cf = C[np.ix_(F, F)]
            out["held"] = out["held"] and not C[H].any() and not C[:, H].any() and not got.reaction[b][H].any()
            out["symmetric"] = max(out["symmetric"], float(np.abs(Cf - Cf.T).max(initial=0.0)))
            out["tangent"] = max(out["tangent"], float(np.abs(D.dot(Cf)).max(initial=0.0)))
            out["projector"] = max(out["projector"], float(np.abs(Cf.dot(Wff).dot(Cf) - Cf).max(initial=0.0)))
    return out


# ---- the case table ---------------------------------------------------------------------------------------------------------
# case id -> (system, mask kind, constant_q_list as config places or None).  Mask kinds as minimize_potential_energy's arguments:
# "keep_kinematic", "all", "constant" (everything outside the list).  scissor4_free is the rank-deficient, ill-conditioned row.
CASES = collections.OrderedDict([
    ("spring_link", ("spring_link", "keep_kinematic", None)),
    ("mixed_loop", ("mixed_loop", "keep_kinematic", None)),
    ("spatial_loop", ("spatial_loop", "keep_kinematic", None)),
    ("scissor4_slider", ("scissor4", "constant", "SLIDER")),
    ("scissor4_free", ("scissor4", "keep_kinematic", None)),
    ("pendulum5_joint", ("pendulum5", "constant", 2)),
    ("pendulum1", ("pendulum1", "all", None)),
    ("ladder_mixed", ("ladder_mixed", "keep_kinematic", None)),
    ("puppet40", ("puppet40", "keep_kinematic", None)),
])
REPEAT = -1
RAGGED = 5
MINIMA = 4


def system_of(case):
    return CASES[case][0]


def constant_names(case):
    """The case's constant_q_list as names (None: none)."""
    name, _, const = CASES[case]
    if const is None:
        return None
    return [const if isinstance(const, str) else pr.config_names(name)[const]]


def free_mask(case):
    name, kind, _ = CASES[case]
    d = common.build(name)[1]
    nq = int(d.n_configs)
    if kind == "all":
        return np.ones(nq, dtype=bool)
    if kind == "keep_kinematic":
        return np.asarray(d.config_kinematic[:nq]) == 0
    fixed = constant_names(case)
    return np.array([n not in fixed for n in pr.config_names(name)])


def batch_size(case):
    return pr.batch_size(system_of(case))


@functools.lru_cache(maxsize=None)
def minima(case):
    """Certified minima the reference minimiser finds from the system's golden poses, re-minimised at tolerance 1e-13: up to MINIMA
    distinct ones."""
    name, free = system_of(case), free_mask(case)
    poses = pr.golden_poses(name)
    found = []
    for b in np.linspace(0, len(poses) - 1, 4 * MINIMA).astype(int):
        one = er.minimize(name, poses[b:b + 1], free)
        if not er.certified(name, one, free)[0]:
            continue
        q = er.minimize(name, one.Q, free, tolerance=1e-13).Q[0]
        if all(np.abs(q - p).max() > 1e-6 for p in found):
            found.append(q)
        if len(found) == MINIMA:
            break
    assert found, case
    return np.array(found)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(Q [batch_size][nq], free): rows drawn from the case's minima; the last repeats row 0."""
    rng = np.random.default_rng(common.tb_seed("static_response", case))
    eq = minima(case)
    n = batch_size(case)
    Q = eq[np.concatenate([np.arange(len(eq)), rng.integers(len(eq), size=n)])[:n - 1]]
    return np.concatenate([Q, Q[:1]]), free_mask(case)


@functools.lru_cache(maxsize=None)
def case_reference(case, kind="spec"):
    Q, free = case_inputs(case)
    opt = SPEC._replace(lapack=kind == "lapack", rival=kind == "rival")
    return static_response(system_of(case), Q, free, opt=opt)


def errors(got, ref):
    """Per array the worst over the poses of max |got - ref| / max(1, |ref array of that pose|max)."""
    out = {}
    for k in ARRAYS:
        g, r = getattr(got, k), getattr(ref, k)
        if g is None or r is None:
            continue
        B = len(r)
        g, r = np.asarray(g, dtype=float).reshape(B, -1), np.asarray(r, dtype=float).reshape(B, -1)
        out[k] = float((np.abs(g - r).max(axis=1, initial=0.0) / np.maximum(1.0, np.abs(r).max(axis=1, initial=0.0))).max(initial=0.0))
    return out


@functools.lru_cache(maxsize=None)
def _case_floors(case):
    ref = case_reference(case)
    lap, riv = errors(case_reference(case, "lapack"), ref), errors(case_reference(case, "rival"), ref)
    return dict(lapack=lap, ladder=riv)


def case_floors(case):
    return _case_floors(case)


def case_bounds(case):
    f = case_floors(case)
    return dict((k, max(TOL, MARGIN * max(f["lapack"][k], f["ladder"][k]))) for k in f["lapack"])


@functools.lru_cache(maxsize=None)
def _invariant_bounds(case):
    Q, free = case_inputs(case)
    inv = invariants(system_of(case), Q, free, case_reference(case))
    riv = invariants(system_of(case), Q, free, case_reference(case), rival=True)      # what the reference leaves under the evaluator's floor
    return dict((k, MARGIN * max(v, riv[k], INVARIANT_MIN)) for k, v in inv.items() if k != "held")


def invariant_bounds(case):
    return _invariant_bounds(case)


def subset(ref, rows, drive_places=None):
    """The rows (poses) of a Response, and of the drive axis the given places."""
    out = []
    for k in Response._fields:
        a = getattr(ref, k)
        if a is not None:
            a = a[rows]
            if drive_places is not None and k in ("dq", "dmu"):
                a = a[:, drive_places]
        out.append(a)
    return Response(*out)


def compare(case, got, rows=None, ref=None, bit_repeat=True):
    """The checks of an implementation of the same algorithm against the reference, shared by the emulation and the device tests;
    `rows`: the table's rows `got` answers (default: all).  Returns the figures it asserted on."""
    ref = ref or case_reference(case)
    Q, free = case_inputs(case)
    pick = np.arange(len(Q)) if rows is None else np.asarray(rows)
    sub = subset(ref, pick)
    err, bounds = errors(got, sub), case_bounds(case)
    inv = invariants(system_of(case), Q[pick], free, got)
    ib = invariant_bounds(case)
    fig = dict(errors=err, bounds=bounds, invariants=dict((k, inv[k]) for k in ib), invariant_bounds=ib)
    print(case, fig)
    assert np.array_equal(got.status, sub.status) and (sub.status == OK).all(), (got.status, sub.status)
    assert np.array_equal(got.rank, sub.rank), (got.rank, sub.rank)
    assert all(err[k] <= bounds[k] for k in err), (err, bounds)
    assert inv["held"] and all(inv[k] <= ib[k] for k in ib), (inv, ib)
    if rows is None and bit_repeat:
        for k in Response._fields:
            if getattr(got, k) is not None:
                assert np.array_equal(getattr(got, k)[REPEAT], getattr(got, k)[0]), k
    return fig
