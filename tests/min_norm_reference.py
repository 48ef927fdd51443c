"""Specification of the rank-revealing least-squares path of the two inverse questions (BatchMidpointVI.dynamics_inverse and
inverse_dynamics with rcond=; csrc/lsq_solve.hpp): numpy and scipy on the arrays of the two existing specifications.

A, r0, the case states and paths, the direct quantities (tau, acc; P, h) and the bound convention are those of
dynamics_inverse_reference.py and inverse_dynamics_reference.py, unchanged.  What is new is the answer of a state or step:
  W = A, c = -r0 (ridge == 0) or W = [A; sqrt(ridge) I], c = (-r0; 0);
  z = numpy.linalg.lstsq(W, c, rcond): the SVD minimum-norm solution -- the answer;
  a second route, scipy.linalg.lstsq(W, c, cond=rcond, lapack_driver="gelsy") (complete orthogonal decomposition); their difference
  is the floor e_ref;
  rank = the number of singular values of W above rcond * sigma_1;  rho = r0 + A z.
Bounds: z and rho max(1e-10, 64 e_ref) relative to max(1, |z|inf); the direct quantities 1e-10 as in the two specifications.
A table row is admissible when at every state the singular values clear the cut by three decades on each side:
sigma_r / sigma_1 >= GAP_ABOVE and sigma_{r+1} / sigma_1 <= GAP_BELOW (test_min_norm_cpu.py asserts it; no state is left out).

CT_CASES (computed torque) and ID_CASES (discrete) are what the emulated kernels (test_min_norm_cpu.py), the device
(test_gpu_min_norm.py) and tools/min_norm_parity.py run; crafted() are the problems the solver alone is given."""
import collections

import numpy as np
import scipy.linalg

import dynamics_inverse_reference as dr
import inverse_dynamics_reference as ir

OK, SINGULAR = 0, 2
RCOND = 1e-9
GAP_ABOVE, GAP_BELOW = 1e-6, 1e-12
TOL, MARGIN, TOL_DIRECT = dr.TOL, dr.MARGIN, dr.TOL_DIRECT

CtCase = collections.namedtuple("CtCase", "name ridge covers")
CT_CASES = [
    CtCase("puppet_forces", 0.0, "rank 16 of 18"),
    CtCase("mixed_loop", 0.0, "A is 5 x 6: n > nd, rank 5"),
    CtCase("wrench_arm", 0.0, "full rank"),
    CtCase("scissor4", 0.0, "nc = 8, no inputs"),
    CtCase("pend_on_cart", 0.0, "rho != 0"),
    CtCase("spring_link", 0.0, "the SPRINGS instantiation"),
    CtCase("damper_link", 0.0, "n = 0"),
    CtCase("puppet40", 0.0, "team 64, the parameter twin"),
    CtCase("puppet_forces", 1e-4, "against the existing case_reference"),
    CtCase("mixed_loop", 1e-4, "against the existing case_reference"),
]
IdCase = collections.namedtuple("IdCase", "base ridge")
# every row of the discrete table at ridge 0 (its rank-deficient and its n > nd row among them, and the non-uniform time bases), and the
# two ridge rows as they stand
ID_CASES = [IdCase(c, 0.0) for c in ir.CASES] + [IdCase(c, c.ridge) for c in ir.CASES if c.ridge > 0]

Answer = collections.namedtuple("Answer", "z z2 rho rank sv")
_cache = {}


def ct_id(c):
    return "%s%s" % (c.name, "_ridge" if c.ridge else "")


def id_id(c):
    return "%s%s%s" % (c.base.name, "_ridge" if c.ridge else "", "" if c.base.pattern == "uniform" else "_" + c.base.pattern)


def stacked(A, r0, ridge):
    """(W, c) of a state."""
    n = A.shape[1]
    if ridge > 0:
        return np.vstack([A, np.sqrt(ridge) * np.eye(n)]), np.concatenate([-r0, np.zeros(n)])
    return A, -r0


def solve(A, r0, ridge, rcond=RCOND):
    """Answer(z by the SVD, z by the complete orthogonal decomposition, rho, rank, singular values of W) of one state."""
    nd, n = A.shape
    if n == 0:
        return Answer(np.zeros(0), np.zeros(0), r0.copy(), 0, np.zeros(0))
    W, c = stacked(A, r0, ridge)
    if W.shape[0] == 0:
        return Answer(np.zeros(n), np.zeros(n), r0.copy(), 0, np.zeros(0))
    z, _, _, sv = np.linalg.lstsq(W, c, rcond=rcond)
    z2 = scipy.linalg.lstsq(W, c, cond=rcond, lapack_driver="gelsy")[0]
    rank = int((sv > rcond * sv[0]).sum()) if sv[0] > 0 else 0
    return Answer(z, z2, r0 + A.dot(z), rank, sv)


# ---- the mutated specifications (test_min_norm_cpu.py): each a plausible wrong answer to a rank-deficient state ----------------------
def solve_basic(A, r0, ridge, rcond=RCOND):
    """The basic solution of column-pivoted QR: zeros on the dependent columns, no second stage."""
    W, c = stacked(A, r0, ridge)
    Q, R, piv = scipy.linalg.qr(W, mode="economic", pivoting=True)
    d = np.abs(np.diag(R))
    r = int((d > rcond * d[0]).sum())
    z = np.zeros(W.shape[1])
    z[piv[:r]] = scipy.linalg.solve_triangular(R[:r, :r], Q.T.dot(c)[:r])
    return z


def solve_rank_shifted(A, r0, ridge, shift, rcond=RCOND):
    """The truncated-SVD answer with `shift` more singular values kept than the rank."""
    W, c = stacked(A, r0, ridge)
    U, s, Vt = np.linalg.svd(W, full_matrices=False)
    r = int((s > rcond * s[0]).sum()) + shift
    with np.errstate(all="ignore"):
        return Vt[:r].T.dot(U[:, :r].T.dot(c) / s[:r])


# ---- the references of the two tables ---------------------------------------------------------------------------------------------------
Reference = collections.namedtuple("Reference", "z z2 rho rank gap_above gap_below A r0 direct status")


def _over_states(A, r0, ridge, live):
    """solve() at every state [..]; live [..]: False where nothing is solved (z = rho = 0, rank 0)."""
    lead = A.shape[:-2]
    n = A.shape[-1]
    z, z2, rho = np.zeros(lead + (n,)), np.zeros(lead + (n,)), np.zeros(lead + (A.shape[-2],))
    rank = np.zeros(lead, dtype=np.int32)
    above, below = np.inf, 0.0
    for idx in np.ndindex(*lead):
        if not live[idx]:
            continue
        a = solve(A[idx], r0[idx], ridge)
        z[idx], z2[idx], rho[idx], rank[idx] = a.z, a.z2, a.rho, a.rank
        if n:
            sv = a.sv / a.sv[0]
            above = min(above, sv[a.rank - 1])
            below = max(below, sv[a.rank] if a.rank < len(sv) else 0.0)
    return z, z2, rho, rank, above, below


def ct_base(c):
    """The row of the existing computed-torque table that supplies the states, A, r0, tau and acc (A and r0 do not depend on the ridge)."""
    return dr.case_by_name(c.name)


def ct_reference(c):
    key = ("ct", ct_id(c))
    if key not in _cache:
        ref = dr.case_reference(ct_base(c))
        live = np.ones(ref.r0.shape[:2], dtype=bool)
        z, z2, rho, rank, above, below = _over_states(ref.A, ref.r0, c.ridge, live)
        _cache[key] = Reference(z, z2, rho, rank, above, below, ref.A, ref.r0, {"tau": ref.tau, "acc": ref.acc}, ref.status)
    return _cache[key]


def id_reference(c, with_p0):
    key = ("id", id_id(c), bool(with_p0))
    if key not in _cache:
        ref = ir.case_reference(c.base, with_p0)
        live = np.ones(ref.r0.shape[:2], dtype=bool)
        if not with_p0:
            live[:, 0] = False            # step 0 is not solved without p0
        z, z2, rho, rank, above, below = _over_states(ref.A, ref.r0, c.ridge, live)
        _cache[key] = Reference(z, z2, rho, rank, above, below, ref.A, ref.r0, {"P": ref.P, "h": ref.h}, ref.status)
    return _cache[key]


def floor(ref):
    """e_ref: the two routes against each other, relative to max(1, |z|inf)."""
    scale = max(1.0, float(np.abs(ref.z).max(initial=0.0)))
    return float(np.abs(ref.z - ref.z2).max(initial=0.0)) / scale, scale


def bound(ref):
    return max(TOL, MARGIN * floor(ref)[0])


def errors(ref, z, rho, direct):
    """Worst errors: z and rho relative to max(1, |z|inf), the direct quantities relative to max(1, |want|inf)."""
    scale = floor(ref)[1]
    e = {"z": float(np.abs(np.asarray(z) - ref.z).max(initial=0.0)) / scale, "rho": float(np.abs(np.asarray(rho) - ref.rho).max(initial=0.0)) / scale}
    for k, want in ref.direct.items():
        e[k] = float(np.abs(np.asarray(direct[k]) - want).max(initial=0.0)) / max(1.0, float(np.abs(want).max(initial=0.0)))
    return e


def compare(tag, ref, z, rho, direct, rank, status):
    """An answer against a reference: status all TG_OK, the ranks equal, every quantity within its bound.  Prints the figures first."""
    e, bd = errors(ref, z, rho, direct), bound(ref)
    print("%s: z %.3e rho %.3e (bound %.3e, floor %.3e, |z|inf %.3e) %s (bound %.1e) rank %d..%d gaps above %.3e below %.3e" % (
        tag, e["z"], e["rho"], bd, floor(ref)[0], floor(ref)[1], " ".join("%s %.3e" % (k, e[k]) for k in ref.direct), TOL_DIRECT,
        ref.rank.min() if ref.rank.size else 0, ref.rank.max() if ref.rank.size else 0, ref.gap_above, ref.gap_below))
    assert np.array_equal(np.asarray(status), ref.status), status
    assert np.array_equal(np.asarray(rank), ref.rank), (rank, ref.rank)
    for q in ("z", "rho"):
        assert e[q] <= bd, (tag, q, e[q], bd)
    for q in ref.direct:
        assert e[q] <= TOL_DIRECT, (tag, q, e[q])
    return e


def compare_ct(c, got, tag=""):
    return compare(tag + ct_id(c), ct_reference(c), dr.unknowns(got.U, got.lam), got.rho, {"tau": got.tau, "acc": got.acc}, got.rank, got.status)


def compare_id(c, with_p0, got, tag=""):
    p = ir.case_paths(c.base)
    z = ir.impulses(int(p["d"].n_inputs), got.U, got.lam, p["dts"])
    return compare("%s%s p0 %s" % (tag, id_id(c), "given" if with_p0 else "absent"), id_reference(c, with_p0), z, got.rho,
                   {"P": got.P, "h": got.h}, got.rank, got.status)


# ---- crafted problems for the solver alone ----------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (3, 1), (1, 3), (5, 6), (6, 5), (22, 18), (40, 18)]
CRAFT_RCOND = 1e-9


def crafted(rows, cols, count=65, seed=0):
    """(A [count][rows][cols], c [count][rows], kinds [count]): problems of one shape with the ranks 0, 1, min - 1 and full interleaved
    (neighbours differ), a duplicated column, a zero column, and columns of scale 1e-6 beside columns of scale 1.  Exact rank comes
    from a product of integer-valued factors scaled to stay exact in fp64, so that the singular values below the cut are rounding
    noise (<= 1e-13 sigma_1) and those above it clear 1e-6 (test_min_norm_cpu.py asserts both on every problem)."""
    rng = np.random.default_rng([rows, cols, seed])
    mn = min(rows, cols)
    kinds = ["zero", "full", "rank1", "deficient", "duplicate", "zero_column", "scaled"]
    A, names = np.zeros((count, rows, cols)), []

    def product(r):
        if r == 0:
            return np.zeros((rows, cols))
        return rng.integers(-3, 4, size=(rows, r)).astype(float).dot(rng.integers(-3, 4, size=(r, cols)).astype(float))
    for p in range(count):
        kind = kinds[p % len(kinds)]
        if kind == "zero":
            a = np.zeros((rows, cols))
        elif kind == "full":
            a = rng.standard_normal((rows, cols))
        elif kind == "rank1":
            a = product(1)
        elif kind == "deficient":
            a = product(max(mn - 1, 0))
        elif kind == "duplicate":
            a = rng.standard_normal((rows, cols))
            if cols > 1:
                a[:, cols - 1] = a[:, 0]
        elif kind == "zero_column":
            a = rng.standard_normal((rows, cols))
            a[:, cols // 2] = 0.0
        else:
            a = rng.standard_normal((rows, cols)) * np.where(np.arange(cols) % 2 == 0, 1.0, 1e-6)[None, :]
        A[p] = a
        names.append(kind)
    c = rng.standard_normal((count, rows))
    return A, c, names


def crafted_reference(A, c, rcond=CRAFT_RCOND):
    """(z, rank, worst gap above, worst gap below) of crafted problems, by the SVD."""
    z, rank = np.zeros(A.shape[:1] + A.shape[2:]), np.zeros(len(A), dtype=np.int32)
    above, below = np.inf, 0.0
    for p in range(len(A)):
        a = solve(A[p], -c[p], 0.0, rcond)
        z[p], rank[p] = a.z, a.rank
        if a.rank:
            sv = a.sv / a.sv[0]
            above = min(above, sv[a.rank - 1])
            below = max(below, sv[a.rank] if a.rank < len(sv) else 0.0)
    return z, rank, above, below
