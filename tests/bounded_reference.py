"""Specification of the bounded inverse questions (BatchMidpointVI.dynamics_inverse / inverse_dynamics with bounds=,
csrc/bvls_solve.hpp): numpy and scipy on the arrays A, r0, ridge that dynamics_inverse_reference and inverse_dynamics_reference produce.

Per state or step:  minimise |r0 + A z|^2 + ridge |z|^2  subject to  lo <= z <= hi,  i.e.  |c - W z| with W = [A; sqrt(ridge) I],
c = (-r0; 0).
  Answer: scipy.optimize.lsq_linear(W, c, (lo, hi), method="bvls") supplies an ACTIVE SET; the answer is that set POLISHED: the bound
  variables exactly on their bounds, the free ones from numpy.linalg.lstsq on the free columns (and, for the floor e_ref, from the
  augmented system [[I, A_f], [A_f', -ridge I]] the sibling references use).
  Certificate: the KKT conditions -- feasibility, |g| on the free set at rounding level, g_j >= 0 at a lower bound and <= 0 at an upper
  one, g = W'(W z - c).  The problem is strictly convex where W has full column rank, so a certified answer is THE answer.
  Admissibility (strict complementarity, so that `active` is unambiguous): every free variable at least MARGIN_Z max(1, |z|inf) inside
  each finite bound; every bound variable (lo < hi) with its gradient at least MARGIN_G max(1, |g|inf) on the right side; the first
  solve's sigma_n / sigma_1 at least MARGIN_S.
Bounds of a comparison: z and rho max(1e-10, 64 e_ref) relative to max(1, |z|inf); tau, acc, P, h as the sibling references hold them;
active equal.  In the discrete question the unknowns are the impulses (dt_k u, lambda): a box on u is given in FORCES and scaled by the
step's own dt_k.

The case tables (CONTINUOUS, DISCRETE) are what the emulated kernels (test_bounded_cpu.py), the device (test_gpu_bounded.py) and
tools/bounded_parity.py run; every box is a rule applied to the UNBOUNDED reference answer of the case's states."""
import collections

import numpy as np
from scipy.optimize import lsq_linear

import common
import dynamics_inverse_reference as cref
import inverse_dynamics_reference as dref

OK, NOT_CONVERGED, SINGULAR = 0, 1, 2
TOL, MARGIN = 1e-10, 64.0
MARGIN_Z, MARGIN_G, MARGIN_S = 1e-6, 1e-6, 1e-6
KKT_FREE = 1e-10                 # |g| on the free set, relative to max(1, |W'c|inf)
RCOND = 1e-9
DRAWS = 8                        # seeded draws a case may try for an admissible table

# box: the rule that makes (lo, hi) from the unbounded answer; twin: also run under a parameter table (puppet40)
CCase = collections.namedtuple("CCase", "name B M ridge box expect")
CONTINUOUS = [
    CCase("puppet40", 3, 5, 0.0, "tension", "ok"),
    CCase("puppet_forces", 3, 5, 1e-4, "tension+inputs", "ok"),
    CCase("wrench_arm", 5, 13, 0.0, "inputs+fixed", "ok"),
    CCase("scissor4", 5, 13, 0.0, "one_sided", "ok"),
    CCase("pend_on_cart", 5, 13, 0.0, "inputs", "ok"),
    CCase("spring_link", 5, 13, 0.0, "all", "ok"),
    CCase("damper_link", 5, 13, 0.0, "all", "ok"),
    CCase("puppet_forces", 3, 5, 0.0, "tension", "singular"),      # rank 16 of 18: TG_SINGULAR at every state
    CCase("mixed_loop", 5, 13, 0.0, "all", "refused"),             # n > nd without a ridge
]
# noise: Gaussian noise on the dynamic configs of the path, the sibling table's NOISE (which that table applies to its unconstrained
# systems alone).  A rolled-out marionette path never needs a pushing string (every multiplier of the sibling table's puppet paths is
# positive: the tension bounds bind nowhere); a path 1e-3 off it asks for accelerations of the order of gravity's in both directions.
DCase = collections.namedtuple("DCase", "name B N ridge pattern box per_trajectory noise")
DISCRETE = [
    DCase("puppet40", 3, 5, 0.0, "uniform", "tension", False, dref.NOISE),
    DCase("wrench_arm", 5, 12, 0.0, "alternating", "inputs", True, 0.0),
    DCase("wrench_arm", 5, 12, 0.0, "random", "inputs", False, 0.0),
    DCase("scissor4", 5, 12, 0.0, "uniform", "one_sided", False, 0.0),
]
Answer = collections.namedtuple("Answer", "z z_aug rho rho_aug active g solves_ref")
_cache = {}


def ccase_id(c):
    return "%s_%dx%d%s_%s" % (c.name, c.B, c.M, "_ridge" if c.ridge else "", c.box.replace("+", "_"))


def dcase_id(c):
    return "%s_%dx%d_%s_%s%s%s" % (c.name, c.B, c.N, c.pattern, c.box, "_rows" if c.per_trajectory else "", "_noise" if c.noise else "")


# ---- one problem ---------------------------------------------------------------------------------------------------------------
def stacked(A, r0, ridge):
    nd, n = A.shape
    if ridge > 0:
        return np.vstack([A, np.sqrt(ridge) * np.eye(n)]), np.concatenate([-r0, np.zeros(n)])
    return A, -r0


def polish(A, r0, ridge, lo, hi, active):
    """(z by lstsq on the free columns of the stacked block, z by the augmented system): bound variables exactly on their bounds."""
    nd, n = A.shape
    free = active == 0
    zb = np.where(active < 0, lo, np.where(active > 0, hi, 0.0))
    zb = np.where(free, 0.0, zb)
    r1 = r0 + A.dot(zb)
    z, z_aug = zb.copy(), zb.copy()
    nf = int(free.sum())
    if nf:
        W, c = stacked(A[:, free], r1, ridge)
        z[free] = np.linalg.lstsq(W, c, rcond=None)[0]
        K = np.block([[np.eye(nd), A[:, free]], [A[:, free].T, -ridge * np.eye(nf)]])
        z_aug[free] = np.linalg.solve(K, np.concatenate([-r1, np.zeros(nf)]))[nd:]
    return z, z_aug


def gradient(A, r0, ridge, z):
    return A.T.dot(r0 + A.dot(z)) + ridge * z


def solve_box(A, r0, ridge, lo, hi):
    """The specification on one problem: Answer."""
    nd, n = A.shape
    if n == 0:
        e = np.zeros(0)
        return Answer(e, e, r0.copy(), r0.copy(), np.zeros(0, dtype=np.int32), e, 0)
    W, c = stacked(A, r0, ridge)
    movable = lo < hi      # (scipy refuses lo == hi: those variables are constants of its problem)
    active = np.full(n, -1, dtype=np.int32)
    nit = 0
    if movable.any():
        res = lsq_linear(W[:, movable], c - W[:, ~movable].dot(lo[~movable]), (lo[movable], hi[movable]), method="bvls", tol=1e-14)
        active[movable] = res.active_mask
        nit = int(res.nit)
    z, z_aug = polish(A, r0, ridge, lo, hi, active)
    return Answer(z, z_aug, r0 + A.dot(z), r0 + A.dot(z_aug), active, gradient(A, r0, ridge, z), nit)


def certificate(A, r0, ridge, lo, hi, z, active):
    """The KKT conditions of an answer and its margins: dict(feasible, free_gradient (relative), sign_ok, margin_z, margin_g, sigma)."""
    n = len(z)
    if n == 0:
        return dict(feasible=True, free_gradient=0.0, sign_ok=True, margin_z=np.inf, margin_g=np.inf, sigma=np.inf)
    W, c = stacked(A, r0, ridge)
    g = gradient(A, r0, ridge, z)
    free, movable = active == 0, lo < hi
    gs = max(1.0, float(np.abs(W.T.dot(c)).max()))
    zs, gscale = max(1.0, float(np.abs(z).max())), max(1.0, float(np.abs(g).max()))
    inside = np.minimum(np.where(np.isfinite(lo), z - lo, np.inf), np.where(np.isfinite(hi), hi - z, np.inf))
    toward = np.where(active < 0, g, -g)      # >= 0 at a bound: leaving it raises the objective
    bound_ = ~free & movable
    first = W[:, movable]
    sv = np.linalg.svd(first, compute_uv=False) if first.shape[1] else np.ones(1)
    return dict(feasible=bool(np.all(z >= lo) and np.all(z <= hi) and np.all(z[active < 0] == lo[active < 0]) and np.all(z[active > 0] == hi[active > 0])),
                free_gradient=float(np.abs(g[free]).max(initial=0.0)) / gs,
                sign_ok=bool(np.all(toward[bound_] >= 0.0)),
                margin_z=float((inside[free] / zs).min(initial=np.inf)),
                margin_g=float((toward[bound_] / gscale).min(initial=np.inf)),
                sigma=float(sv.min() / sv.max()) if sv.max() > 0 else 0.0)


# ---- boxes ---------------------------------------------------------------------------------------------------------------------
def tension_bounds(name, nu, nc, call):
    """As BatchMidpointVI.tension_bounds: Distance multipliers confined to the pulling side (<= 0 continuous, >= 0 discrete)."""
    system = common.build(name)[0]
    lo, hi = np.full(nu + nc, -np.inf), np.full(nu + nc, np.inf)
    for j, con in enumerate(system.constraints):
        if type(con).__name__ == "Distance":
            if call == "dynamics_inverse":
                hi[nu + j] = 0.0
            else:
                lo[nu + j] = 0.0
    return lo, hi


def make_box(rule, name, nu, nc, z_free, call, shift=0.0):
    """(lo, hi) [n] from the unbounded answers z_free [states][n] (in the units of the box: forces for u).  Rules:
    tension: tension_bounds; inputs: every input between the 30 % and 70 % quantiles of its unbounded values; +fixed: the last input
    held at its median (lo == hi); tension+inputs: tension and |u_i| <= half the median |u| of the unbounded answer; one_sided:
    multiplier c >= its 27 % quantile (c even) or <= its 73 % quantile (c odd); all: every variable between its 20 % and 80 % quantiles."""
    n = nu + nc
    lo, hi = np.full(n, -np.inf), np.full(n, np.inf)
    q = lambda j, p: float(np.quantile(z_free[:, j], p + shift if p < 0.5 else p - shift))      # (shift: a draw's own quantile levels)
    if "tension" in rule:
        lo, hi = tension_bounds(name, nu, nc, call)
    if rule == "tension+inputs":
        half = 0.5 * float(np.median(np.abs(z_free[:, :nu])))
        lo[:nu], hi[:nu] = -half, half
    if rule.startswith("inputs"):
        for j in range(nu):
            lo[j], hi[j] = q(j, 0.3), q(j, 0.7)
        if rule.endswith("+fixed"):
            lo[nu - 1] = hi[nu - 1] = q(nu - 1, 0.5)
    if rule == "one_sided":
        for j in range(nc):
            if j % 2 == 0:
                lo[nu + j] = q(nu + j, 0.27)
            else:
                hi[nu + j] = q(nu + j, 0.73)
    if rule == "all":
        for j in range(n):
            lo[j], hi[j] = q(j, 0.2), q(j, 0.8)
    return lo, hi


# ---- the tables ----------------------------------------------------------------------------------------------------------------
Table = collections.namedtuple("Table", "case base inputs ref lo hi z z_aug rho rho_aug active g margins draw")


def _solve_table(A, r0, ridge, lo_of, hi_of, solved):
    """Answers over a [B][M] table of problems; lo_of(b, s), hi_of(b, s) the box in the units of z; solved [B][M] bool."""
    Bn, Mn, nd, n = A.shape
    z, z_aug = np.zeros((Bn, Mn, n)), np.zeros((Bn, Mn, n))
    rho, rho_aug, g = np.zeros((Bn, Mn, nd)), np.zeros((Bn, Mn, nd)), np.zeros((Bn, Mn, n))
    active = np.zeros((Bn, Mn, n), dtype=np.int32)
    margins = []
    for b in range(Bn):
        for s in range(Mn):
            if not solved[b, s]:
                continue
            lo, hi = lo_of(b, s), hi_of(b, s)
            a = solve_box(A[b, s], r0[b, s], ridge, lo, hi)
            z[b, s], z_aug[b, s], rho[b, s], rho_aug[b, s], active[b, s], g[b, s] = a.z, a.z_aug, a.rho, a.rho_aug, a.active, a.g
            cert = certificate(A[b, s], r0[b, s], ridge, lo, hi, a.z, a.active)
            cert["state"] = (b, s)
            margins.append(cert)
    return z, z_aug, rho, rho_aug, active, g, margins


def admissible(margins):
    return all(m["feasible"] and m["sign_ok"] and m["free_gradient"] <= KKT_FREE and m["margin_z"] >= MARGIN_Z and m["margin_g"] >= MARGIN_G
               and m["sigma"] >= MARGIN_S for m in margins)


# puppet_forces with the box the table prescribes (|u_i| <= half the median |u|, eighteen inputs) has no state without an active bound
# in any of the DRAWS draws: an input box that tight always binds.  Its coverage is the other two properties.
NO_FREE_STATE = ("tension+inputs",)


def covered(active, solved, n, rule="", movable=None):
    """Coverage of a table: a state with no active bound (but see NO_FREE_STATE), one with min(2, n) or more (n > 0); of the
    variables with lo < hi (movable [n] bool), since one with lo == hi is bound everywhere."""
    movable = np.ones(n, dtype=bool) if movable is None else movable
    n = int(movable.sum())
    if n == 0:
        return True
    count = (active[..., movable] != 0).sum(axis=-1)[solved]
    return bool(((count == 0).any() or rule in NO_FREE_STATE) and (count >= min(2, n)).any())


def continuous_table(c):
    """Table of a continuous case: the first draw of states whose table is admissible and covered (AssertionError if none of DRAWS)."""
    key = ("ctable", ccase_id(c))
    if key in _cache:
        return _cache[key]
    tried = []
    for draw in range(DRAWS):
        base = cref.Case(c.name, c.B, c.M, c.ridge, draw, "bounded")
        p = cref.case_states(base)
        ref = cref.case_reference(base)
        nu, nc = int(p["d"].n_inputs), int(p["d"].n_constraints)
        n = nu + nc
        lo, hi = make_box(c.box, c.name, nu, nc, ref.z.reshape(c.B * c.M, n), "dynamics_inverse")
        solved = np.ones((c.B, c.M), dtype=bool)
        z, z_aug, rho, rho_aug, active, g, margins = _solve_table(ref.A, ref.r0, c.ridge, lambda b, s: lo, lambda b, s: hi, solved)
        tried.append((draw, admissible(margins), covered(active, solved, n, c.box, lo < hi)))
        if admissible(margins) and covered(active, solved, n, c.box, lo < hi):
            _cache[key] = Table(c, base, p, ref, lo, hi, z, z_aug, rho, rho_aug, active, g, margins, draw)
            return _cache[key]
    raise AssertionError(("no admissible draw", ccase_id(c), tried))


def discrete_table(c, with_p0):
    """Table of a discrete case: the first draw (quantile levels moved inwards by draw / 100; the draw seeds the noise) whose table is
    admissible and covered.  lo, hi are [n] or, per_trajectory, [B][n] (row b widened by 1 + b / 4 about its centre), u in forces."""
    key = ("dtable", dcase_id(c), bool(with_p0))
    if key in _cache:
        return _cache[key]
    base = dref.Case(c.name, c.B, c.N, c.ridge, c.pattern, "bounded")
    p0 = dref.case_paths(base)
    nu, nc, nd = int(p0["d"].n_inputs), int(p0["d"].n_constraints), int(p0["d"].n_dyn)
    n = nu + nc
    dts = np.asarray(p0["dts"], dtype=float)
    solved = np.ones((c.B, c.N), dtype=bool)
    solved[:, 0] = bool(with_p0)
    tried = []
    for draw in range(DRAWS):
        if c.noise:
            rng = np.random.default_rng(common.tb_seed("bounded inverse dynamics", c.name, draw))
            Q = p0["Q"].copy()
            Q[:, :, :nd] += c.noise * rng.standard_normal(Q[:, :, :nd].shape)
            p = dict(p0, Q=Q)
            ref = dref.inverse_dynamics(p["d"], Q, dts, p["p0"] if with_p0 else None, c.ridge)
        else:
            p, ref = p0, dref.case_reference(base, with_p0)
        forces = np.concatenate([ref.U, ref.lam], axis=-1)[solved]
        lo, hi = make_box(c.box, c.name, nu, nc, forces.reshape(-1, n), "inverse_dynamics", 0.01 * draw)
        if c.per_trajectory:
            mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
            finite = np.isfinite(half)
            widen = 1.0 + np.arange(c.B)[:, None] / 4.0
            lo = np.where(finite, mid - widen * half, lo)
            hi = np.where(finite, mid + widen * half, hi)
        scale = lambda k: np.concatenate([np.full(nu, dts[k]), np.ones(nc)])
        row = lambda a, b: a[b] if a.ndim == 2 else a
        z, z_aug, rho, rho_aug, active, g, margins = _solve_table(ref.A, ref.r0, c.ridge, lambda b, k: row(lo, b) * scale(k),
                                                                  lambda b, k: row(hi, b) * scale(k), solved)
        ok = admissible(margins), covered(active, solved, n, c.box)
        tried.append((draw,) + ok)
        if all(ok):
            _cache[key] = Table(c, base, p, ref, lo, hi, z, z_aug, rho, rho_aug, active, g, margins, draw)
            return _cache[key]
    raise AssertionError(("no admissible draw", dcase_id(c), with_p0, tried))


# ---- comparisons ---------------------------------------------------------------------------------------------------------------
def floors(t):
    scale = max(1.0, float(np.abs(t.z).max(initial=0.0)))
    return {"z": float(np.abs(t.z - t.z_aug).max(initial=0.0)) / scale, "rho": float(np.abs(t.rho - t.rho_aug).max(initial=0.0)) / scale, "scale": scale}


def bound(t):
    f = floors(t)
    return max(TOL, MARGIN * max(f["z"], f["rho"]))


def compare_continuous(t, got, tag=""):
    """An answer (U lam rho tau acc status rank active solves) against a continuous table.  Prints the figures first."""
    f, bd = floors(t), bound(t)
    own = lambda w: max(1.0, float(np.abs(w).max(initial=0.0)))
    e = {"z": float(np.abs(cref.unknowns(got.U, got.lam) - t.z).max(initial=0.0)) / f["scale"],
         "rho": float(np.abs(got.rho - t.rho).max(initial=0.0)) / f["scale"],
         "tau": float(np.abs(got.tau - t.ref.tau).max(initial=0.0)) / own(t.ref.tau), "acc": float(np.abs(got.acc - t.ref.acc).max(initial=0.0)) / own(t.ref.acc)}
    print("%s%s: z %.3e rho %.3e (bound %.3e, floors z %.3e rho %.3e) tau %.3e acc %.3e (bound %.1e) |z|inf %.3e solves %s" % (
        tag, ccase_id(t.case), e["z"], e["rho"], bd, f["z"], f["rho"], e["tau"], e["acc"], cref.TOL_DIRECT, f["scale"],
        np.bincount(np.asarray(got.solves).ravel()).tolist()))
    assert np.all(np.asarray(got.status) == OK), got.status
    assert np.array_equal(np.asarray(got.active), t.active), np.argwhere(np.asarray(got.active) != t.active)
    for q in ("z", "rho"):
        assert e[q] <= bd, (ccase_id(t.case), q, e[q], bd)
    for q in ("tau", "acc"):
        assert e[q] <= cref.TOL_DIRECT, (ccase_id(t.case), q, e[q])
    return e


def compare_discrete(t, got, tag=""):
    """An answer (U lam P rho h status rank active solves) against a discrete table.  Prints the figures first."""
    f, bd = floors(t), bound(t)
    nu = int(t.inputs["d"].n_inputs)
    sib = max(dref.TOL, dref.MARGIN * max(dref.floors(t.ref)["z"], dref.floors(t.ref)["rho"]))      # P and h: the sibling's bound and scale
    ss = dref.floors(t.ref)["scale"]
    zg = dref.impulses(nu, got.U, got.lam, t.inputs["dts"])
    e = {"z": float(np.abs(zg - t.z).max(initial=0.0)) / f["scale"], "rho": float(np.abs(got.rho - t.rho).max(initial=0.0)) / f["scale"],
         "P": float(np.abs(got.P - t.ref.P).max(initial=0.0)) / ss, "h": float(np.abs(got.h - t.ref.h).max(initial=0.0)) / ss}
    print("%s%s: z %.3e rho %.3e (bound %.3e, floors z %.3e rho %.3e) P %.3e h %.3e (bound %.3e) |z|inf %.3e solves %s" % (
        tag, dcase_id(t.case), e["z"], e["rho"], bd, f["z"], f["rho"], e["P"], e["h"], sib, f["scale"],
        np.bincount(np.asarray(got.solves).ravel()).tolist()))
    assert np.all(np.asarray(got.status) == OK), got.status
    assert np.array_equal(np.asarray(got.active), t.active), np.argwhere(np.asarray(got.active) != t.active)
    for q in ("z", "rho"):
        assert e[q] <= bd, (dcase_id(t.case), q, e[q], bd)
    for q in ("P", "h"):
        assert e[q] <= sib, (dcase_id(t.case), q, e[q], sib)
    return e


# ---- crafted problems for the solver alone -----------------------------------------------------------------------------------------
def crafted(rows, cols, kind, seed):
    """(A, c, lo, hi) of one crafted problem.  kind: none / some / all_but_one / all (how many variables the box binds, by construction
    from the unconstrained answer), fixed (variable 0 with lo == hi), lower / upper (bounds on one side only)."""
    rng = np.random.default_rng(common.tb_seed("bvls crafted", rows, cols, kind, seed))
    A = rng.standard_normal((rows, cols))
    c = 3.0 * rng.standard_normal(rows)
    z = np.linalg.lstsq(A, c, rcond=None)[0]
    span = 1.0 + np.abs(z)
    lo, hi = z - span, z + span
    if kind == "none":
        pass
    elif kind in ("some", "all_but_one", "all"):
        k = {"some": max(1, cols // 2), "all_but_one": cols - 1, "all": cols}[kind]
        pick = rng.permutation(cols)[:k]
        side = rng.integers(2, size=k)
        for j, s in zip(pick, side):      # the unconstrained answer lies outside the box on these variables
            if s:
                hi[j] = z[j] - 0.5 * span[j]
                lo[j] = hi[j] - span[j]
            else:
                lo[j] = z[j] + 0.5 * span[j]
                hi[j] = lo[j] + span[j]
    elif kind == "fixed":
        lo[0] = hi[0] = z[0] + 0.7 * span[0]
    elif kind == "lower":
        lo, hi = z + 0.3 * span * rng.standard_normal(cols), np.full(cols, np.inf)
    elif kind == "upper":
        lo, hi = np.full(cols, -np.inf), z + 0.3 * span * rng.standard_normal(cols)
    else:
        raise ValueError(kind)
    return A, c, lo, hi


KINDS = ("none", "some", "all_but_one", "all", "fixed", "lower", "upper")


def refree_problem():
    """A 4 x 3 problem on which the active-set loop frees a variable again after it bound it: the emulated solver takes 6 solves and
    ends with ONE variable bound -- without a release, every solve after the first binds at least one variable for good, and 6 solves
    would leave five bound (test_bounded_cpu.py asserts solves - 1 > the number of bound variables)."""
    rng = np.random.default_rng(1)
    A = rng.standard_normal((4, 3))
    c = 3.0 * rng.standard_normal(4)
    lo, hi = -rng.uniform(0.1, 1.0, 3), rng.uniform(0.1, 1.0, 3)
    return A, c, lo, hi
