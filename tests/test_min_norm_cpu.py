"""Rank-revealing least squares for the two inverse questions, without a device: the conditions of the tables of min_norm_reference.py
(every state's singular values clear the cut by three decades on each side; no state is left out), the minimum-norm properties of the
specification that need no second solver, the mutations the tables must catch, the solver itself (csrc/lsq_solve.hpp) and the LSQ
instantiations of the two kernels compiled for the host with TEAM = 1 (emu_lsq_harness.py) over crafted problems and both tables,
strided rows and null outputs, the status cases, and the refusals, LDS geometry and declarations of the C entry points.

Measured here: the emulated kernels stay under 8e-4 of the bound 1e-10 on both tables (scissor4 with the alternating time base:
z 7.3e-14); the floors are 3e-14 at the most, so the second term of the bound is never needed; the least gap above the cut is 8.4e-4
(scissor4, computed torque) and the worst below it 3.4e-17 (puppet_forces, discrete)."""
import ctypes
import os

import numpy as np
import pytest

import common
import dynamics_inverse_reference as dr
import emu_dyn_inverse_harness
import emu_invdyn_harness
import emu_lsq_harness
import inverse_dynamics_reference as ir
import min_norm_reference as mr
from trep_amd import _lib

CT_IDS = [mr.ct_id(c) for c in mr.CT_CASES]
ID_RUNS = [(c, w) for c in mr.ID_CASES for w in (True, False)]
ID_IDS = ["%s_%s" % (mr.id_id(c), "p0" if w else "nop0") for c, w in ID_RUNS]
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _emu(name):
    return emu_lsq_harness.EmuLsq(common.build(name)[1])


def _ct(case, **kw):
    p = dr.case_states(mr.ct_base(case))
    return _emu(case.name).dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], case.ridge, mr.RCOND, **kw)


def _id(case, with_p0, **kw):
    p = ir.case_paths(case.base)
    return _emu(case.base.name).inverse_dynamics(p["Q"], p["dts"], p["p0"] if with_p0 else None, case.ridge, mr.RCOND, **kw)


def _same(a, b):
    for q in a._fields:
        assert np.array_equal(getattr(a, q), getattr(b, q)), q


# ---- 1. the conditions of the tables, on the reference alone --------------------------------------------------------------------------
def _conditions(ref, nd, n, ridge, live_states):
    assert ref.rank.shape == ref.r0.shape[:2] and live_states == ref.rank.size          # no state is left out
    if n == 0:
        assert not ref.rank.any()
        return
    assert ref.gap_above >= mr.GAP_ABOVE and ref.gap_below <= mr.GAP_BELOW, (ref.gap_above, ref.gap_below)
    assert np.isfinite(ref.z).all() and np.isfinite(ref.rho).all()


@pytest.mark.parametrize("case", mr.CT_CASES, ids=CT_IDS)
def test_computed_torque_table_meets_its_conditions(case):
    ref = mr.ct_reference(case)
    d = dr.case_states(mr.ct_base(case))["d"]
    nd, n = int(d.n_dyn), int(d.n_inputs + d.n_constraints)
    print(mr.ct_id(case), "nd %d n %d rank %s gap above %.3e below %.3e floor %.3e |z|inf %.3e" % (
        nd, n, sorted(set(ref.rank.ravel().tolist())), ref.gap_above, ref.gap_below, *mr.floor(ref)))
    _conditions(ref, nd, n, case.ridge, ref.rank.size)
    assert mr.bound(ref) == mr.TOL                                  # the floor never widens the bound on this table
    if case.name == "puppet_forces" and not case.ridge:
        assert n == 18 and (ref.rank == 16).all()
    if case.name == "puppet_forces" and case.ridge:
        assert (ref.rank == 18).all()                              # the rank test runs on the stacked block
    if case.name == "mixed_loop" and not case.ridge:
        assert (nd, n) == (5, 6) and (ref.rank == 5).all()
    if case.name in ("wrench_arm", "scissor4", "pend_on_cart", "spring_link", "puppet40"):
        assert n <= nd and (ref.rank == n).all()
    if case.name == "pend_on_cart":
        assert np.abs(ref.rho).max() > 1e-3
    if case.name == "damper_link":
        assert n == 0


@pytest.mark.parametrize("case,with_p0", ID_RUNS, ids=ID_IDS)
def test_discrete_table_meets_its_conditions(case, with_p0):
    ref = mr.id_reference(case, with_p0)
    d = ir.case_paths(case.base)["d"]
    nd, n = int(d.n_dyn), int(d.n_inputs + d.n_constraints)
    print(mr.id_id(case), with_p0, "nd %d n %d rank %s gap above %.3e below %.3e floor %.3e" % (
        nd, n, sorted(set(ref.rank.ravel().tolist())), ref.gap_above, ref.gap_below, mr.floor(ref)[0]))
    _conditions(ref, nd, n, case.ridge, ref.rank.size)
    solved = ref.rank if with_p0 else ref.rank[:, 1:]
    if not with_p0:
        assert not ref.rank[:, 0].any() and not ref.z[:, 0].any()
    if case.base.name == "puppet_forces" and not case.ridge:
        assert (solved == 16).all() and n == 18
    if case.base.name == "mixed_loop" and not case.ridge:
        assert n > nd and (solved == nd).all()


def test_the_tables_hold_the_rows_the_feature_is_for():
    assert [(c.name, c.ridge) for c in mr.CT_CASES] == [
        ("puppet_forces", 0.0), ("mixed_loop", 0.0), ("wrench_arm", 0.0), ("scissor4", 0.0), ("pend_on_cart", 0.0), ("spring_link", 0.0),
        ("damper_link", 0.0), ("puppet40", 0.0), ("puppet_forces", 1e-4), ("mixed_loop", 1e-4)]
    names = [(c.base.name, c.ridge, c.base.pattern) for c in mr.ID_CASES]
    assert ("puppet_forces", 0.0, "uniform") in names and ("mixed_loop", 0.0, "uniform") in names
    assert any(p != "uniform" for _, _, p in names)
    assert len(mr.ID_CASES) == len(ir.CASES) + 2


# ---- 2. minimum-norm properties that need no second solver ----------------------------------------------------------------------------
DEFICIENT = [c for c in mr.CT_CASES if c.ridge == 0.0 and c.name in ("puppet_forces", "mixed_loop")]


@pytest.mark.parametrize("case", DEFICIENT, ids=[mr.ct_id(c) for c in DEFICIENT])
def test_specification_is_orthogonal_to_the_null_space_and_rho_to_the_range(case):
    """z has no component in the null space of A (N from the SVD) and rho none in its range: |N' z| and |A' rho| vanish relative to
    |z| and |A| |rho| -- and so do the emulated kernel's."""
    ref = mr.ct_reference(case)
    got = _ct(case)
    zs = dr.unknowns(got.U, got.lam)
    worst = {"ref_null": 0.0, "ref_range": 0.0, "emu_null": 0.0, "emu_range": 0.0}
    for idx in np.ndindex(*ref.rank.shape):
        A, r = ref.A[idx], int(ref.rank[idx])
        _, s, Vt = np.linalg.svd(A)
        N = Vt[r:].T
        assert N.shape[1] == A.shape[1] - r and N.shape[1] >= 1
        for tag, z, rho in (("ref", ref.z[idx], ref.rho[idx]), ("emu", zs[idx], got.rho[idx])):
            worst[tag + "_null"] = max(worst[tag + "_null"], float(np.abs(N.T.dot(z)).max()) / max(1.0, float(np.abs(z).max())))
            worst[tag + "_range"] = max(worst[tag + "_range"], float(np.abs(A.T.dot(rho)).max()) / (s[0] * max(1.0, float(np.abs(z).max()))))
    print(mr.ct_id(case), worst)
    assert max(worst.values()) <= mr.TOL


# ---- 3. mutated specifications ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DEFICIENT, ids=[mr.ct_id(c) for c in DEFICIENT])
def test_mutations_miss_the_table(case):
    """The basic solution of pivoted QR, the ridge answer taken for the minimum-norm one, and a rank taken one too high each miss the
    table by at least 1e4 bounds at EVERY state (or are not finite)."""
    ref = mr.ct_reference(case)
    bd, scale = mr.bound(ref), mr.floor(ref)[1]
    ridge_ref = mr.ct_reference(mr.CtCase(case.name, 1e-4, ""))
    least = {"basic": np.inf, "ridge": np.inf, "rank+1": np.inf}
    for idx in np.ndindex(*ref.rank.shape):
        A, r0 = ref.A[idx], ref.r0[idx]
        miss = lambda z: float(np.abs(z - ref.z[idx]).max()) / scale / bd if np.isfinite(z).all() else np.inf
        least["basic"] = min(least["basic"], miss(mr.solve_basic(A, r0, 0.0)))
        least["ridge"] = min(least["ridge"], miss(ridge_ref.z[idx]))
        if ref.rank[idx] < min(A.shape):
            least["rank+1"] = min(least["rank+1"], miss(mr.solve_rank_shifted(A, r0, 0.0, 1)))
    print(mr.ct_id(case), "the mutants miss by at least (bounds):", least)
    assert least["basic"] >= 1e4 and least["ridge"] >= 1e4 and least["rank+1"] >= 1e4
    if case.name == "mixed_loop":
        assert least["rank+1"] == np.inf                 # full row rank: there is no further singular value to take


def test_rank_shifted_specification_with_no_shift_is_the_specification():
    ref = mr.ct_reference(DEFICIENT[0])
    z = mr.solve_rank_shifted(ref.A[0, 0], ref.r0[0, 0], 0.0, 0)
    assert np.abs(z - ref.z[0, 0]).max() <= 1e-12 * max(1.0, np.abs(z).max())


# ---- 4. the emulated solver alone, on crafted problems --------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", mr.SHAPES, ids=["%dx%d" % s for s in mr.SHAPES])
def test_emulated_solver_on_crafted_problems(rows, cols):
    """z and rank against the SVD: per problem max(1e-10, 64 e_ref) relative to max(1, |z|inf), e_ref the two routes of the
    specification against each other on that problem (the columns of scale 1e-6 make conditions of 1e7)."""
    A, c, kinds = mr.crafted(rows, cols)
    assert set(kinds) == {"zero", "full", "rank1", "deficient", "duplicate", "zero_column", "scaled"}
    z_ref, rank_ref, above, below = mr.crafted_reference(A, c)
    # the cut is clear: rounding noise below it, and above it the 1e-6 the scaled columns are made with, a decade and more over rcond
    assert above >= 10 * mr.CRAFT_RCOND and below <= mr.GAP_BELOW, (above, below)
    mn = min(rows, cols)
    assert {0, mn} <= set(rank_ref.tolist()) and (mn < 3 or {1, mn - 1} <= set(rank_ref.tolist()))
    assert (np.diff(rank_ref) != 0).mean() > 0.5 or mn == 1            # neighbours differ in rank
    z, rank, status = emu_lsq_harness.lsq_solve(A, c, mr.CRAFT_RCOND)
    assert (status == mr.OK).all()
    assert np.array_equal(rank, rank_ref), [(k, int(a), int(b)) for k, a, b in zip(kinds, rank, rank_ref) if a != b]
    worst = 0.0
    for p in range(len(A)):
        a = mr.solve(A[p], -c[p], 0.0, mr.CRAFT_RCOND)
        scale = max(1.0, float(np.abs(a.z).max()))
        bd = max(mr.TOL, mr.MARGIN * float(np.abs(a.z - a.z2).max()) / scale)
        err = float(np.abs(z[p] - a.z).max()) / scale
        worst = max(worst, err / bd)
        assert err <= bd, (p, kinds[p], err, bd)
    print("%dx%d: gaps above %.3e below %.3e, worst share of the bound %.3e" % (rows, cols, above, below, worst))
    assert not z[np.array(kinds) == "zero"].any() and not rank[np.array(kinds) == "zero"].any()       # rank 0: z = 0, TG_OK
    _same_arrays = emu_lsq_harness.lsq_solve(A, c, mr.CRAFT_RCOND, poison=False)
    assert np.array_equal(_same_arrays[0], z) and np.array_equal(_same_arrays[1], rank)


def test_emulated_solver_keeps_the_first_of_equal_columns():
    """team_argmax's tie rule: of equal norms the smaller index wins.  Two equal columns: the basic solution would load the first; the
    minimum-norm answer shares the load, and the rank is 1 however the tie falls -- so the rule shows in neither, which is the point:
    the answer does not depend on it."""
    A = np.array([[[1.0, 1.0], [2.0, 2.0], [2.0, 2.0]]])
    c = np.array([[3.0, 6.0, 6.0]])
    z, rank, status = emu_lsq_harness.lsq_solve(A, c, 1e-9)
    assert rank[0] == 1 and status[0] == mr.OK and np.abs(z[0] - 1.5).max() <= 1e-14


NOT_FINITE = {
    "all_nan": lambda A, c: A.fill(np.nan),
    "nan_and_zero_columns": lambda A, c: (A.fill(0.0), A[:, 0].fill(np.nan)),
    "one_nan_entry": lambda A, c: A.__setitem__((-1, -1), np.nan),
    "one_inf_entry": lambda A, c: A.__setitem__((0, 0), np.inf),
    "nan_in_c": lambda A, c: c.__setitem__(-1, np.nan),
    "nan_in_c_zero_matrix": lambda A, c: (A.fill(0.0), c.__setitem__(0, np.nan)),
}


@pytest.mark.parametrize("kind", sorted(NOT_FINITE))
@pytest.mark.parametrize("rows,cols", ((3, 2), (2, 3), (6, 5)), ids=("3x2", "2x3", "6x5"))
def test_emulated_solver_tells_not_finite_from_rank_zero(rows, cols, kind):
    """A matrix or right-hand side with an entry that is not finite is TG_SINGULAR with z = 0 and rank 0 -- never TG_OK with rank 0,
    which is what a zero matrix gets; the problems on either side of it keep their bits."""
    A, c, _ = mr.crafted(rows, cols, count=3)
    good = emu_lsq_harness.lsq_solve(A, c, 1e-9)
    NOT_FINITE[kind](A[1], c[1])
    z, rank, status = emu_lsq_harness.lsq_solve(A, c, 1e-9)
    assert status.tolist() == [mr.OK, mr.SINGULAR, mr.OK] and not z[1].any() and rank[1] == 0
    for i in (0, 2):
        assert np.array_equal(z[i], good[0][i]) and rank[i] == good[1][i]


def test_usable_range_of_the_solver_is_as_documented():
    """lsq_solve.hpp: norms are plain sums of squares.  Inside 1e-140 .. 1e140 the answer is the specification's; a matrix of scale
    1e-170 counts as zero (rank 0, TG_OK) and one of scale 1e160 overflows (TG_SINGULAR)."""
    A, c, kinds = mr.crafted(5, 3, count=2)
    assert kinds[1] == "full"
    for scale in (1e-140, 1e140):
        z, rank, status = emu_lsq_harness.lsq_solve(A * scale, c, 1e-9)
        want = mr.solve(A[1] * scale, -c[1], 0.0, 1e-9)
        assert status[1] == mr.OK and rank[1] == 3 == want.rank
        assert np.abs(z[1] - want.z).max() <= 1e-10 * np.abs(want.z).max()
    z, rank, status = emu_lsq_harness.lsq_solve(A * 1e-170, c, 1e-9)
    assert status[1] == mr.OK and rank[1] == 0 and not z[1].any()
    assert emu_lsq_harness.lsq_solve(A * 1e160, c, 1e-9)[2][1] == mr.SINGULAR


def test_emulated_solver_reports_a_non_finite_answer():
    A, c, _ = mr.crafted(6, 5, count=3)
    c[1, 2] = np.nan
    z, rank, status = emu_lsq_harness.lsq_solve(A, c, 1e-9)
    assert status.tolist() == [mr.OK, mr.SINGULAR, mr.OK] and not z[1].any() and rank[1] == 0
    A[2, 0, 0] = np.inf
    assert emu_lsq_harness.lsq_solve(A, c, 1e-9)[2][2] == mr.SINGULAR


# ---- 5. the emulated kernels over both tables ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mr.CT_CASES, ids=CT_IDS)
def test_emulated_computed_torque_over_the_table(case):
    got = _ct(case)
    mr.compare_ct(case, got)
    assert (got.status == mr.OK).all()


@pytest.mark.parametrize("case,with_p0", ID_RUNS, ids=ID_IDS)
def test_emulated_inverse_dynamics_over_the_table(case, with_p0):
    got = _id(case, with_p0)
    mr.compare_id(case, with_p0, got)
    assert (got.status == mr.OK).all()


@pytest.mark.parametrize("name", ("wrench_arm", "scissor4"))
def test_full_rank_answers_agree_with_the_kernel_already_trusted(name):
    """Where A has full column rank both kernels answer the same question: within the table's bound of each other, and tau and acc --
    the same code -- to the bit."""
    case = dr.case_by_name(name)
    p = dr.case_states(case)
    old = emu_dyn_inverse_harness.EmuDynInverse(p["d"]).dynamics_inverse(p["Q"], p["dQ"], p["ddQ"])
    new = _emu(name).dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], 0.0, mr.RCOND)
    assert np.array_equal(old.tau, new.tau) and np.array_equal(old.acc, new.acc) and np.array_equal(old.status, new.status)
    scale = max(1.0, float(np.abs(dr.unknowns(old.U, old.lam)).max()))
    assert np.abs(dr.unknowns(old.U, old.lam) - dr.unknowns(new.U, new.lam)).max() / scale <= 2 * mr.TOL
    assert np.abs(old.rho - new.rho).max() / scale <= 2 * mr.TOL


def test_existing_discrete_kernel_and_the_new_one_share_their_direct_outputs():
    case = ir.CASES[5]
    p = ir.case_paths(case)
    old = emu_invdyn_harness.EmuInverse(p["d"]).inverse_dynamics(p["Q"], p["dts"], p["p0"])
    new = _emu(case.name).inverse_dynamics(p["Q"], p["dts"], p["p0"], 0.0, mr.RCOND)
    assert np.array_equal(old.P, new.P) and np.array_equal(old.h, new.h) and np.array_equal(old.status, new.status)


def test_emulated_kernels_do_not_depend_on_what_the_scratch_held():
    case = mr.CT_CASES[0]
    _same(_ct(case, poison=True), _ct(case, poison=False))
    idc = [c for c in mr.ID_CASES if c.base.name == "mixed_loop" and not c.ridge][0]
    _same(_id(idc, True, poison=True), _id(idc, True, poison=False))


def test_emulated_state_does_not_depend_on_its_launch():
    case = mr.CT_CASES[1]
    p = dr.case_states(mr.ct_base(case))
    emu = _emu(case.name)
    whole = _ct(case)
    b, s = 3, 7
    cut = lambda a: a[b:b + 1, s:s + 1]
    one = emu.dynamics_inverse(cut(p["Q"]), cut(p["dQ"]), cut(p["ddQ"]), case.ridge, mr.RCOND)
    twice = emu.dynamics_inverse(p["Q"][[b, b]], p["dQ"][[b, b]], p["ddQ"][[b, b]], case.ridge, mr.RCOND)
    for q in whole._fields:
        assert np.array_equal(getattr(one, q)[0, 0], getattr(whole, q)[b, s]), q
        assert np.array_equal(getattr(twice, q)[0], getattr(whole, q)[b]) and np.array_equal(getattr(twice, q)[1], getattr(whole, q)[b]), q


def test_emulated_kernels_read_strided_rows():
    case = mr.CT_CASES[1]
    p = dr.case_states(mr.ct_base(case))
    nq = int(p["d"].n_configs)
    widths = (nq + 5, nq + 3, nq + 1)
    wide = []
    for a, w in zip((p["Q"], p["dQ"], p["ddQ"]), widths):
        x = np.full(a.shape[:2] + (w,), np.nan)
        x[:, :, :nq] = a
        wide.append(x)
    _same(_ct(case), _emu(case.name).dynamics_inverse(*wide, ridge=case.ridge, rcond=mr.RCOND, strides=widths))
    idc = [c for c in mr.ID_CASES if c.base.name == "mixed_loop" and not c.ridge][0]
    q = ir.case_paths(idc.base)
    X = np.full(q["Q"].shape[:2] + (nq + 4,), np.nan)
    X[:, :, :nq] = q["Q"]
    _same(_id(idc, True), _emu(idc.base.name).inverse_dynamics(X, q["dts"], q["p0"], idc.ridge, mr.RCOND, stride=nq + 4))


def test_emulated_kernel_writes_only_what_is_asked_for():
    case = mr.CT_CASES[1]
    full = _ct(case)
    for q in full._fields:
        alone = _ct(case, want=(q,))
        assert np.array_equal(getattr(alone, q), getattr(full, q)), q
        assert all(getattr(alone, o) is None for o in full._fields if o != q)
    assert all(v is None for v in _ct(case, want=()))


def test_status_of_a_non_finite_state():
    """An acceleration that is not a number: TG_SINGULAR there with U, lam, rho zero and rank 0, tau and acc still written; every other
    state keeps its bits."""
    case = mr.CT_CASES[0]
    p = dr.case_states(mr.ct_base(case))
    good = _ct(case)
    ddQ = p["ddQ"].copy()
    b, s = 1, 2
    ddQ[b, s, 1] = np.nan
    got = _emu(case.name).dynamics_inverse(p["Q"], p["dQ"], ddQ, case.ridge, mr.RCOND)
    hit = np.zeros(got.status.shape, dtype=bool)
    hit[b, s] = True
    assert (got.status[hit] == mr.SINGULAR).all() and (got.status[~hit] == mr.OK).all()
    for q in ("U", "lam", "rho", "rank"):
        assert not getattr(got, q)[hit].any(), q
    for q in got._fields:
        assert np.array_equal(getattr(got, q)[~hit], getattr(good, q)[~hit]), q
    assert np.isnan(got.tau[b, s]).any()


@pytest.mark.parametrize("name", ("scissor4", "puppet40", "puppet_forces", "mixed_loop"))
@pytest.mark.parametrize("where", ("Q", "dQ", "ddQ"))
def test_status_of_a_state_that_is_not_a_number(name, where):
    """A whole row of Q, dQ or ddQ not a number (a diverged rollout read in place): A, r0 or both are not finite.  TG_SINGULAR with
    U, lam, rho zero and rank 0, as the augmented kernel answers -- not TG_OK with rank 0 and a rho that is not a number."""
    base = dr.case_by_name(name)
    p = dr.case_states(base)
    arrays = {k: p[k][:2, :3].copy() for k in ("Q", "dQ", "ddQ")}
    emu = _emu(name)
    good = emu.dynamics_inverse(arrays["Q"], arrays["dQ"], arrays["ddQ"], 0.0, mr.RCOND)
    arrays[where][0, 0, :] = np.nan
    got = emu.dynamics_inverse(arrays["Q"], arrays["dQ"], arrays["ddQ"], 0.0, mr.RCOND)
    hit = np.zeros(got.status.shape, dtype=bool)
    hit[0, 0] = True
    assert (got.status[hit] == mr.SINGULAR).all() and (got.status[~hit] == mr.OK).all(), got.status
    for q in ("U", "lam", "rho", "rank"):
        assert not getattr(got, q)[hit].any(), q
    for q in got._fields:
        assert np.array_equal(getattr(got, q)[~hit], getattr(good, q)[~hit]), q
    if base.ridge == 0.0:                                     # where the augmented kernel runs without a ridge: the same status words
        old = emu_dyn_inverse_harness.EmuDynInverse(p["d"]).dynamics_inverse(arrays["Q"], arrays["dQ"], arrays["ddQ"])
        assert np.array_equal(old.status, got.status) and not old.rho[hit].any()


@pytest.mark.parametrize("with_p0", (True, False), ids=("p0", "nop0"))
def test_status_of_a_path_with_a_configuration_that_is_not_a_number(with_p0):
    """Q_k not a number spoils the steps k - 1, k and k + 1 (p_k, the pair, and the next step's p): TG_SINGULAR, zeros and rank 0
    there; the other steps keep their bits."""
    case = [c for c in mr.ID_CASES if c.base.name == "puppet_forces" and not c.ridge][0]
    p = ir.case_paths(case.base)
    Q, p0 = p["Q"][:2].copy(), (p["p0"][:2] if with_p0 else None)
    emu = _emu(case.base.name)
    good = emu.inverse_dynamics(Q, p["dts"], p0, 0.0, mr.RCOND)
    k = 6
    Q[1, k, :] = np.nan
    got = emu.inverse_dynamics(Q, p["dts"], p0, 0.0, mr.RCOND)
    hit = np.zeros(got.status.shape, dtype=bool)
    hit[1, k - 1:k + 2] = True
    assert (got.status[hit] == mr.SINGULAR).all() and (got.status[~hit] == mr.OK).all(), got.status
    for q in ("U", "lam", "rho", "rank"):
        assert not getattr(got, q)[hit].any(), q
        assert np.array_equal(getattr(got, q)[~hit], getattr(good, q)[~hit]), q


@pytest.mark.parametrize("case", [c for c in mr.CT_CASES if c.ridge > 0], ids=[mr.ct_id(c) for c in mr.CT_CASES if c.ridge > 0])
def test_ridge_rows_agree_with_the_existing_reference_and_kernel(case):
    """With a ridge the stacked block has full column rank and both specifications answer the same question: the new reference's z
    and rho against dynamics_inverse_reference.case_reference's (QR on the stacked system) within the bound, and the emulated new
    kernel against the emulated augmented one within twice the bound (each is within one of its reference)."""
    base = mr.ct_base(case)
    assert base.ridge == case.ridge
    new, old = mr.ct_reference(case), dr.case_reference(base)
    scale = max(mr.floor(new)[1], dr.floors(old)["scale"])
    bd = max(mr.bound(new), dr.bound(old))
    e_z, e_rho = float(np.abs(new.z - old.z).max()) / scale, float(np.abs(new.rho - old.rho).max()) / scale
    print(mr.ct_id(case), "references: z %.3e rho %.3e bound %.3e" % (e_z, e_rho, bd))
    assert e_z <= bd and e_rho <= bd
    p = dr.case_states(base)
    k_old = emu_dyn_inverse_harness.EmuDynInverse(p["d"]).dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], base.ridge)
    k_new = _ct(case)
    e_z = float(np.abs(dr.unknowns(k_new.U, k_new.lam) - dr.unknowns(k_old.U, k_old.lam)).max()) / scale
    e_rho = float(np.abs(k_new.rho - k_old.rho).max()) / scale
    print(mr.ct_id(case), "kernels: z %.3e rho %.3e" % (e_z, e_rho))
    assert e_z <= 2 * bd and e_rho <= 2 * bd
    assert np.array_equal(k_new.tau, k_old.tau) and np.array_equal(k_new.acc, k_old.acc)


@pytest.mark.parametrize("with_p0", (True, False), ids=("p0", "nop0"))
@pytest.mark.parametrize("case", [c for c in mr.ID_CASES if c.ridge > 0], ids=[mr.id_id(c) for c in mr.ID_CASES if c.ridge > 0])
def test_discrete_ridge_rows_agree_with_the_existing_reference(case, with_p0):
    new, old = mr.id_reference(case, with_p0), ir.case_reference(case.base, with_p0)
    scale = max(mr.floor(new)[1], ir.floors(old)["scale"])
    bd = max(mr.bound(new), ir.bound(old))
    e_z, e_rho = float(np.abs(new.z - old.z).max()) / scale, float(np.abs(new.rho - old.rho).max()) / scale
    print(mr.id_id(case), with_p0, "references: z %.3e rho %.3e bound %.3e" % (e_z, e_rho, bd))
    assert e_z <= bd and e_rho <= bd


def test_nothing_to_solve_returns_the_residual_and_rank_zero():
    for name in ("pendulum5", "damper_link"):
        _, d = common.build(name)
        Q, dQ, ddQ = dr.draw_states(name, 2, 3, 0)
        got = emu_lsq_harness.EmuLsq(d).dynamics_inverse(Q, dQ, ddQ, 0.0, mr.RCOND)
        old = emu_dyn_inverse_harness.EmuDynInverse(d).dynamics_inverse(Q, dQ, ddQ)
        assert (got.status == mr.OK).all() and not got.rank.any()
        assert np.array_equal(got.rho, -got.tau) and np.array_equal(got.rho, old.rho) and np.abs(got.rho).min() > 1e-6


def test_emulated_parameter_twin_matches_rebuilt_systems():
    """puppet40, every trajectory under its own row of masses, inertias and gravity: full rank there, so the existing parameter
    reference (QR on rebuilt systems) is the answer, within the table's bound."""
    case = dr.case_by_name("puppet40")
    p = dr.case_states(case)
    rows = ir.parameter_rows(case.name, case.B)
    got = _emu(case.name).dynamics_inverse(p["Q"], p["dQ"], p["ddQ"], 0.0, mr.RCOND, rows=ir.parameter_table(case.name, rows), group=1)
    dr.compare(case, got, ref=dr.parameter_reference(case, rows), tag="parameter rows (lsq) ")
    assert (got.rank == 6).all()
    base = _ct(mr.CtCase("puppet40", 0.0, ""))
    for q in got._fields:
        assert np.array_equal(getattr(got, q)[0], getattr(base, q)[0]), q
    assert np.abs(got.tau[1:] - base.tau[1:]).max() > 1e-3


# ---- 6. the C entry points without a device -------------------------------------------------------------------------------------------
def _ct_host(L, b, n_states, Q, dQ, ddQ, ridge, rcond):
    return L.tg_batch_dynamics_inverse_lsq(b, n_states, Q, dQ, ddQ, ridge, rcond, None, None, None, None, None, None, None)


def _ct_device(L, b, n_states, Q, dQ, ddQ, ridge, rcond):
    return L.tg_batch_dynamics_inverse_lsq_device(b, n_states, Q, 8, dQ, 8, ddQ, 8, ridge, rcond, None, None, None, None, None, None, None)


def _id_host(L, b, n_steps, dt, Q, ridge, rcond):
    return L.tg_batch_inverse_dynamics_lsq(b, n_steps, dt, Q, None, ridge, rcond, None, None, None, None, None, None, None)


def _id_device(L, b, n_steps, dt, Q, ridge, rcond):
    return L.tg_batch_inverse_dynamics_lsq_device(b, n_steps, dt, Q, 8, None, ridge, rcond, None, None, None, None, None, None, None)


BAD_RCOND = (-1e-12, 1.0, 2.0, float("nan"), float("inf"))


@pytest.mark.parametrize("call", (_ct_host, _ct_device), ids=("host", "device"))
def test_computed_torque_refusals_before_a_device_is_touched(call):
    L = _lib.lib()
    batch = ctypes.create_string_buffer(1 << 20)
    b, p = ctypes.addressof(batch), np.zeros(64).ctypes.data
    for rcond in BAD_RCOND:
        assert call(L, b, 1, p, p, p, 0.0, rcond) == ERR_INVALID and L.tg_last_error() == b"rcond must be finite, not negative and below 1"
        assert call(L, None, 1, p, p, p, 0.0, rcond) == ERR_INVALID
    for n_states, Q, dQ, ddQ, ridge, message in (
            (1, p, p, p, -1e-6, b"ridge must be finite and not negative"),
            (1, p, p, p, float("nan"), b"ridge must be finite and not negative"),
            (0, p, p, p, 0.0, b"n_states must be at least 1"),
            (1, None, p, p, 0.0, b"null Q"),
            (1, p, None, p, 0.0, b"null dQ"),
            (1, p, p, None, 0.0, b"null ddQ")):
        assert call(L, b, n_states, Q, dQ, ddQ, ridge, 1e-9) == ERR_INVALID
        assert L.tg_last_error() == message
    assert call(L, None, 1, p, p, p, 0.0, 1e-9) == ERR_INVALID and L.tg_last_error() == b"null argument"


@pytest.mark.parametrize("call", (_id_host, _id_device), ids=("host", "device"))
def test_discrete_refusals_before_a_device_is_touched(call):
    L = _lib.lib()
    p = np.zeros(64).ctypes.data
    for rcond in BAD_RCOND:
        assert call(L, None, 1, 0.01, p, 0.0, rcond) == ERR_INVALID and L.tg_last_error() == b"rcond must be finite, not negative and below 1"
    assert call(L, None, 1, 0.01, p, 0.0, 1e-9) == ERR_INVALID and L.tg_last_error() == b"null argument"


def test_solver_hook_refusals():
    L = _lib.lib()
    batch = ctypes.create_string_buffer(1 << 20)
    b, p = ctypes.addressof(batch), np.zeros(64).ctypes.data
    hook = L.tg_batch_debug_lsq_solve
    assert hook(None, 1, 1, 1, 1, p, p, 1e-9, p, p, p) == ERR_INVALID and L.tg_last_error() == b"null argument"
    assert hook(b, 1, 1, 1, 1, None, p, 1e-9, p, p, p) == ERR_INVALID
    assert hook(b, 3, 1, 1, 1, p, p, 1e-9, p, p, p) == ERR_INVALID and L.tg_last_error() == b"team must be 1, 4, 16 or 64"
    assert hook(b, 4, 0, 1, 1, p, p, 1e-9, p, p, p) == ERR_INVALID
    assert hook(b, 4, 1, 0, 1, p, p, 1e-9, p, p, p) == ERR_INVALID
    assert hook(b, 4, 1, 1, 2000, p, p, 1e-9, p, p, p) == ERR_INVALID
    assert hook(b, 4, 1, 1, 1, p, p, 1.0, p, p, p) == ERR_INVALID and L.tg_last_error() == b"rcond must be finite, not negative and below 1"
    assert hook(b, 1, 1, 200, 200, p, p, 1e-9, p, p, p) == ERR_UNSUPPORTED         # 64 teams of 200 x 201 doubles


LDS_CELLS = [(n, t) for n in ("pendulum1", "pend_on_cart", "mixed_loop", "scissor4", "puppet_forces", "puppet40") for t in (1, 4, 16, 64)]


@pytest.mark.parametrize("name,team", LDS_CELLS)
def test_lds_of_a_workgroup_and_its_refusal(monkeypatch, name, team):
    """Per team the rollout slice, the stacked block [nd + n][n + 1], the accelerations [nq] or p_k [nd], and the solver's 4 n doubles:
    never more than 4 n doubles above the layout of the augmented image."""
    monkeypatch.setenv("TREPAMD_TEAM", str(team))
    L = _lib.lib()
    d = common.build(name)[1]
    nq, nd, n = int(d.n_configs), int(d.n_dyn), int(d.n_inputs + d.n_constraints)
    ct, ct_old, inv, inv_old, rollout, o_kkt, o_ddq, o_scal = emu_lsq_harness.EmuLsq(d).lds_doubles()
    even = lambda x: (x + 1) & ~1
    assert ct == even(even(rollout) + (nd + n) * (n + 1) + nq + 4 * n) and inv == even(even(rollout) + (nd + n) * (n + 1) + nd + 4 * n)
    assert ct <= ct_old + 4 * n and inv <= inv_old + 4 * n
    assert o_kkt == even(rollout) and o_ddq == o_kkt + (nd + n) * (n + 1) and o_scal == o_ddq + nq and o_scal + 4 * n <= ct
    sys_h = L.tg_system_create(d.byref())
    assert sys_h
    try:
        for fn, slice_, message in ((L.tg_system_dynamics_inverse_lsq_lds, ct, b"system too large for the LDS-resident computed-torque kernel"),
                                    (L.tg_system_inverse_dynamics_lsq_lds, inv, b"system too large for the LDS-resident inverse-dynamics kernel")):
            out = np.zeros(4, dtype=np.int32)
            rc = fn(sys_h, out.ctypes.data_as(_lib._c_ip))
            bytes_ = (64 // team) * slice_ * 8
            assert list(out) == [team, slice_, bytes_, 0]
            if bytes_ > 160 * 1024:
                assert rc == ERR_UNSUPPORTED and L.tg_last_error() == message
            else:
                assert rc == 0
    finally:
        L.tg_system_destroy(sys_h)
    assert L.tg_system_dynamics_inverse_lsq_lds(None, None) == ERR_INVALID and L.tg_system_inverse_dynamics_lsq_lds(None, None) == ERR_INVALID


def test_the_new_entry_points_are_exported_and_declared():
    names = set(_lib.exported_symbols())
    want = {"tg_batch_dynamics_inverse_lsq", "tg_batch_dynamics_inverse_lsq_device", "tg_system_dynamics_inverse_lsq_lds",
            "tg_batch_inverse_dynamics_lsq", "tg_batch_inverse_dynamics_lsq_device", "tg_system_inverse_dynamics_lsq_lds",
            "tg_batch_debug_lsq_solve"}
    assert want == set(_lib._LSQ_SIGNATURES) and want <= names
    header = open(os.path.join(ROOT, "include", "trep_amd.h")).read()
    L = _lib.lib()
    for n in want:
        assert "int %s(" % n in header
        assert getattr(L, n)
    assert "the rank test runs on the STACKED block" in header


def test_the_python_calls_take_rcond():
    import inspect
    from trep_amd import BatchMidpointVI
    from trep_amd.midpointvi import DynamicsInverse, DynamicsInverseRank, InverseDynamics, InverseDynamicsRank
    assert DynamicsInverseRank._fields == DynamicsInverse._fields + ("rank",)
    assert InverseDynamicsRank._fields == InverseDynamics._fields + ("rank",)
    for f in (BatchMidpointVI.dynamics_inverse, BatchMidpointVI.inverse_dynamics):
        assert inspect.signature(f).parameters["rcond"].default is None
    for f in (BatchMidpointVI.dynamics_inverse_device, BatchMidpointVI.inverse_dynamics_device):
        params = inspect.signature(f).parameters
        assert params["rcond"].default is None and params["rank_dev"].default is None


def test_parity_profile_covers_both_tables():
    """The committed record names every case of both tables and is consistent with itself; it recomputes neither a floor nor an error."""
    import json
    with open(os.path.join(ROOT, "profiles", "min_norm_parity.json")) as f:
        prof = json.load(f)
    want = ["ct_" + i for i in CT_IDS] + ["id_%s_%s" % (mr.id_id(c), "p0" if w else "nop0") for c, w in ID_RUNS]
    assert sorted(prof["cases"]) == sorted(want) and prof["rcond"] == mr.RCOND
    for row in prof["cases"].values():
        assert row["bound"] == max(mr.TOL, mr.MARGIN * row["floor"]) and row["bound_direct"] == mr.TOL_DIRECT
        for errors, equal in ((row["emulation_error"], row["emulation_rank_equal"]), (row["device_error"], row["device_rank_equal"])):
            if errors is not None:
                assert equal and max(errors["z"], errors["rho"]) <= row["bound"]
                assert max(v for q, v in errors.items() if q not in ("z", "rho")) <= row["bound_direct"]
