"""Model branches that only spatial_loop, mixed_loop and the two ladders reach (point components x / y / z, PointToPoint3D, a plane
normal behind a constant rotation, a const_se3 with a rotation, kinematic rotary configs, the world-frame path of the specialised kernel
with point / plane constraints and an odd Newton system), without a GPU:

* the plan cells the device tests rely on, read back from the generated specialisation header: a schedule change that moves a system
  off the path under test fails here instead of silently removing coverage;
* both ladders specialise (hipcc is a child process and needs no GPU): with an odd nf the composite form's image is odd too, and its
  16-byte clear used to refuse to compile;
* honesty of the oracle comparisons, with the oracle alone (the style of test_time_base_cpu.py): a descriptor with one of these
  branches got wrong either does not solve or is at least 1e3 tolerances from the right one in X, lambda or the l1_* derivatives."""
import re

import numpy as np
import pytest

from common import (D1, MB_CLOSED_LOOP, MB_GENERIC, MB_LADDERS, MB_N, MB_SECOND_TERM, MB_TEAM, TB_DT, TB_TOL, build, mb_batch, mb_bound, mb_case,
                    mb_contraction, mb_e_ref, mb_reference, relerr, tb_closed_loop_inputs, tb_closed_loop_reference, trajectories)
from emu_harness import EmuBatch
from oracle.oracle import OracleMVI, OracleError
from trep_amd import descriptor

DT = 0.01
_PUPPET = dict(wev_ok=1, cmp_ok=1, bbd_ok=1, bbd_pk_ok=1, fb_on=1, tr_on=1, dhr_sides=1, dhr_types=1, wev_rc_ident=1, has_plane=0, nf=28)
PLAN = {
    "ladder_point": dict(wev_ok=1, cmp_ok=1, bbd_ok=1, bbd_pk_ok=0, fb_on=0, tr_on=0, dhr_sides=3, dhr_types=2, wev_rc_ident=1, has_plane=0, nf=19),
    "ladder_mixed": dict(wev_ok=1, cmp_ok=1, bbd_ok=1, bbd_pk_ok=0, fb_on=0, tr_on=0, dhr_sides=3, dhr_types=7, wev_rc_ident=0, has_plane=1, nf=20),
    "spatial_loop": dict(wev_ok=0, nf=9),
    "mixed_loop": dict(wev_ok=0, nf=8, has_plane=1),
    "puppet40": _PUPPET,
    "puppet_basic": _PUPPET,
}


def _ints(system):
    from trep_amd import specialize
    text = specialize.header(system)
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"static constexpr int (\w+) = (-?\d+);", text)}, text


@pytest.mark.parametrize("name", sorted(PLAN))
def test_plan_cells(name):
    c, text = _ints(build(name)[0])
    got = dict((k, c[k]) for k in PLAN[name])
    assert got == PLAN[name], (name, got)
    if PLAN[name]["wev_ok"]:
        assert "#define SPEC_TEAM 64\n" in text          # the world-frame path is compiled for a full wavefront only
        assert c["o_Df"] % 2 == 0                         # what the image clear asserts
        assert c["df_ld"] == (c["nf"] + 1) | 1


def test_an_odd_newton_system_has_an_odd_image():
    """The case the fix is for: nf = 19 has the row stride 21, 399 doubles; nf = 20 has 21 as well, 420."""
    c = _ints(build("ladder_point")[0])[0]
    assert (c["nf"] * c["df_ld"]) % 2 == 1
    c = _ints(build("ladder_mixed")[0])[0]
    assert (c["nf"] * c["df_ld"]) % 2 == 0


@pytest.mark.parametrize("name", ["ladder_point", "ladder_mixed"])
def test_ladders_specialise(name):
    import os
    from trep_amd import specialize
    system = build(name)[0]
    path = specialize.build(system)
    assert os.path.exists(path) and specialize.is_built(system)


@pytest.mark.parametrize("name", MB_GENERIC)
def test_small_loops_are_closed_at_zero(name):
    """Closed at q = 0 by construction: the reference's h(0), recorded in the golden, is one rounding of the plane product at most
    (mixed_loop: 6.9e-18), and so is the oracle's."""
    from common import golden
    _, d = build(name)
    assert np.abs(golden(name)["h0"]).max() <= 2.0 ** -56
    o = OracleMVI(d)
    o.set_times(0.0, DT)
    o.q1 = np.zeros(d.n_configs)
    o.q2 = np.zeros(d.n_configs)
    h = o.calc_f()[d.n_dyn:]
    print(name, "oracle h(0)", h)
    assert np.abs(h).max() <= 2.0 ** -56


# ---- honesty: mutated descriptors against the right one, oracle alone --------------------------------------------------------------------
HONESTY_N = 12
MARGIN = 1e3


def _mutant(d, **changes):
    t = dict((k, (v.copy() if isinstance(v, np.ndarray) else v)) for k, v in d.tables.items() if not k.startswith("_pad_"))
    for k, fn in changes.items():
        fn(t[k])
    return descriptor.SystemDesc(t)


def _frame(system, name):
    return [f.name for f in system.frames].index(name)


def _frame_of_config(system, name):
    return [f.config.name if f.config is not None else None for f in system.frames].index(name)


def _set(i, v):
    def fn(a):
        a[i] = v
    return fn


def _swap(i, j):
    def fn(a):
        a[i], a[j] = a[j], a[i]
    return fn


def _transpose_rotation(i):
    def fn(lg):
        m = lg.reshape(-1, 3, 4)
        m[i, :, :3] = m[i, :, :3].T.copy()
    return fn


def _plane_on_parent(system, d):
    """The plane constraint's frame replaced by the parent of its const_se3 frame (same origin, p = 0): the normal stays (0.2, 1, 0.1)
    but is no longer carried through Ry(0.3) Rx(-0.2)."""
    plane = _frame(system, "Plane")
    parent = int(d.frame_parent[plane])
    c = int(np.flatnonzero(d.constraint_type == 2)[0])
    key = "constraint_frame1" if d.constraint_frame1[c] == plane else "constraint_frame2"
    assert d.tables[key][c] == plane
    return {key: _set(c, parent)}


def _mutants(name):
    system, d = build(name)
    RX, RY, RZ = 4, 5, 6          # include/trep_amd.h: TG_RX, TG_RY, TG_RZ
    comp = [int(x) for x in d.constraint_component]
    if name == "spatial_loop":
        assert comp == [0, 1, 2]
        turn = _frame_of_config(system, "turn")
        assert d.frame_transform[turn] == RZ
        return d, [("point x -> y", dict(constraint_component=_set(0, 1))),
                   ("point y -> z", dict(constraint_component=_set(1, 2))),
                   ("point x <-> y", dict(constraint_component=_swap(0, 1))),
                   ("point y <-> z", dict(constraint_component=_swap(1, 2))),
                   ("const_se3 rotation transposed", dict(frame_lg=_transpose_rotation(_frame(system, "Tilt")))),
                   ("kinematic rz -> rx", dict(frame_transform=_set(turn, RX))),
                   ("kinematic rz -> ry", dict(frame_transform=_set(turn, RY)))]
    assert name == "mixed_loop" and comp[:2] == [1, 2]
    knee = _frame_of_config(system, "kr")
    assert d.frame_transform[knee] == RX
    return d, [("point y -> x", dict(constraint_component=_set(0, 0))),
               ("point z -> x", dict(constraint_component=_set(1, 0))),
               ("point y <-> z", dict(constraint_component=_swap(0, 1))),
               ("plane normal not carried through the constant rotation", _plane_on_parent(system, d)),
               ("const_se3 rotation transposed", dict(frame_lg=_transpose_rotation(_frame(system, "Plane")))),
               ("kinematic rx -> ry", dict(frame_transform=_set(knee, RY))),
               ("kinematic rx -> rz", dict(frame_transform=_set(knee, RZ)))]


def _run(d, q0, U, K):
    """Rollout from rest: dict(X [N+1][nq + nd], lam [N][nc], l1 = the l1_* first derivatives of the last step), or None if a step is
    singular or does not converge."""
    o = OracleMVI(d)
    try:
        o.initialize_from_configs(0.0, q0, DT, q0)
        X, lam = [np.concatenate([o.q2, o.p2])], []
        for k in range(HONESTY_N):
            o.step(o.t2 + DT, U[k], K[k])
            X.append(np.concatenate([o.q2, o.p2]))
            lam.append(o.lambda1)
        o.calc_deriv1()
    except OracleError:
        return None
    l1 = np.concatenate([o.deriv1(n).reshape(-1) for n in ("l1_dq1", "l1_dp1", "l1_du1", "l1_dk2")])
    if not all(np.isfinite(a).all() for a in (np.array(X), np.array(lam), l1)):
        return None
    return dict(X=np.array(X), lam=np.array(lam), l1=l1)


@pytest.mark.parametrize("name", ["spatial_loop", "mixed_loop"])
def test_mutated_descriptors_are_told_apart(name):
    """Every mutant ends singular / not converged, or is at least 1e3 tolerances from the right descriptor in X, lambda or l1_*.  lambda and
    l1_* are part of the comparison because a swap inside a point constraint only permutes the multipliers: X alone cannot see it."""
    d, mutants = _mutants(name)
    prefix, q0, U, K = trajectories(name)[0]
    right = _run(d, q0, U, K)
    assert right is not None
    again = _run(_mutant(d), q0, U, K)                       # the copy itself changes nothing
    assert all(np.array_equal(again[k], right[k]) for k in right)
    tol = dict(X=TB_TOL["X"], lam=TB_TOL["lambda1"], l1=TB_TOL["d1"])
    for what, changes in mutants:
        got = _run(_mutant(d, **changes), q0, U, K)
        if got is None:
            print("%s, %s: does not solve" % (name, what))
            continue
        margins = dict((k, relerr(got[k], right[k]) / tol[k]) for k in tol)
        print("%s, %s: %s tolerances" % (name, what, ", ".join("%s %.1e" % kv for kv in margins.items())))
        assert max(margins.values()) >= MARGIN, (name, what, margins)
        if "<->" in what:
            assert max(margins["lam"], margins["l1"]) >= MARGIN, (name, what, margins)


# ---- the case table of the device tests (common.MB_*): conditions on it, and the generic kernel source under emulation over it ----------
@pytest.mark.parametrize("name", MB_GENERIC + MB_LADDERS)
def test_case_teams_are_the_librarys(name):
    from trep_amd import _lib
    L = _lib.lib()
    _, d = build(name)
    h = L.tg_system_create(d.byref())
    assert h
    out = np.zeros(8, dtype=np.int32)
    _lib.check(L.tg_system_info(h, out.ctypes.data_as(_lib._c_ip)))
    L.tg_system_destroy(h)
    assert int(out[0]) == MB_TEAM[name] and mb_batch(name) == max(2 * (64 // MB_TEAM[name]) + 1, 5)
    c = mb_case(name)
    assert c["B"] == mb_batch(name) and c["N"] == MB_N and np.array_equal(c["dts"], np.full(MB_N, TB_DT))


def _check_floor(name, e_ref):
    for q, e in e_ref.items():
        print("%s e_ref(%s) = %.2e, bound %.2e" % (name, q, e, mb_bound(name, q, e_ref)))
        if (name, q) in MB_SECOND_TERM:
            assert TB_TOL[q] < 64.0 * e < 10.0 * TB_TOL[q], (name, q, e)     # needed, and no blank cheque
        else:
            assert 64.0 * e <= TB_TOL[q], (name, q, e)                        # the bound is the project's tolerance itself


@pytest.mark.parametrize("name", MB_GENERIC + MB_LADDERS)
def test_one_ulp_of_the_start_stays_under_the_tolerances(name):
    """Conditioning, from the oracle alone: which quantities need the second term of the bound (common.MB_SECOND_TERM: at most one per
    system) and that every other one is held to the project's tolerance."""
    assert len(set(n for n, _ in MB_SECOND_TERM)) == len(MB_SECOND_TERM)
    _check_floor(name, mb_e_ref(name))


@pytest.mark.parametrize("name", MB_CLOSED_LOOP)
def test_closed_loop_inputs(name):
    """The feedback moves X by 1e-6 .. 1e-2 against the open loop and every oracle step converges; conditioning of the loop."""
    c = mb_case(name)
    Kp, bX, bU = tb_closed_loop_inputs(name, "uniform", MB_N, c["B"])
    open_loop = mb_reference(name)
    loop = tb_closed_loop_reference(name, "uniform", MB_N, c["B"])
    for b in range(c["B"]):
        moved = relerr(loop[b]["X"], open_loop[b]["X"])
        assert 1e-6 <= moved <= 1e-2, (name, b, moved)
    _check_floor(name, mb_e_ref(name, closed_loop=True))


@pytest.mark.parametrize("name", MB_GENERIC + MB_LADDERS)
def test_emulated_generic_kernels_on_the_cases(name):
    """The generic kernel source at TEAM = 1 on three trajectories of the case: rollout, deriv1, deriv2z against the oracle."""
    c, ref, e_ref = mb_case(name), mb_reference(name), mb_e_ref(name)
    d, B = c["d"], 3
    nu, nk, nc = d.n_inputs, d.n_kin, d.n_constraints
    Z, ZL = mb_contraction(name)
    e = EmuBatch(d, B)
    e.initialize_from_configs(0.0, c["Q0"][:B], TB_DT, c["Q1"][:B])
    X = e.rollout(MB_N, TB_DT, c["U"][:B] if nu else None, c["K"][:B] if nk else None)
    assert (e.status == 0).all()
    d1 = e.deriv1()
    HZ = e.deriv2z(Z[:B], ZL[:B] if nc else None)
    for b in range(B):
        r = ref[b]
        errs = dict(X=relerr(X[b], r["X"]), p2=relerr(e.p2[b], r["p2"]), lambda1=relerr(e.lam[b], r["lambda1"]),
                    d1=max(relerr(d1[n][b], r["d1"][n]) for n in D1), hz=relerr(HZ[b], r["hz"]))
        print(name, b, " ".join("%s %.2e" % kv for kv in errs.items()))
        for q, err in errs.items():
            assert err < mb_bound(name, q, e_ref), (name, b, q, err)
        assert int(e.iters[b]) == r["iterations"], (name, b)
