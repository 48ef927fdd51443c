"""CPU tests of the batched normal modes: the numpy specification (normal_modes_reference.py) against LAPACK and a closed form, the
teeth of its checks, the kernel body compiled for the host (emu_modes_harness.py) against the specification over the case table, the
status cases, and the refusals of the C entry points that need no device."""
import ctypes
import os

import numpy as np
import pytest

import common
import emu_harness
import emu_modes_harness
import normal_modes_reference as nr
from trep_amd import _lib, parameters

ERR_INVALID, ERR_UNSUPPORTED = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emulated():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = emu_modes_harness.EmuModes(common.build(name)[1]).normal_modes(nr.case_inputs(name))
        return cache[name]
    return get


# ---- 1. the specification ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nr.SYSTEMS)
def test_specification_against_lapack(name):
    ref, lap = nr.case_reference(name), nr.case_reference(name, "lapack")
    floors = nr.case_floors(name)
    inv = nr.invariants(name, nr.case_inputs(name), None, ref)
    print(name, floors, inv, "sweeps", int(ref.sweeps.max()))
    assert (ref.status == nr.OK).all() and np.array_equal(ref.count, lap.count)
    assert floors["lapack"] <= nr.TOL
    assert 2 * int(ref.sweeps.max()) < nr.MAX_SWEEPS
    assert inv["held"] and max(inv["orthonormal"], inv["tangent"], inv["eigen"]) <= nr.MARGIN * nr.INVARIANT_MIN


def test_facts_about_the_table():
    """What the checks rely on: the mode counts, an unstable pose, an odd order, and that at most a quarter of the table's modes
    fall to the projector comparison."""
    by_projector = total = 0
    for name in nr.SYSTEMS:
        ref = nr.case_reference(name)
        _, p, t = nr.shape_errors(name, ref, ref)
        by_projector, total = by_projector + p, total + t
    assert 4 * by_projector <= total, (by_projector, total)
    assert set(nr.case_reference("puppet40").count) == {16} and set(nr.case_reference("puppet40").rank) == {6}
    assert set(nr.case_reference("scissor4").count) == {1} and set(nr.case_reference("pendulum1").count) == {1}
    assert set(nr.case_reference("pendulum5").count) == {5}
    assert (nr.case_reference("ladder_mixed").omega2.min(axis=1) < 0.0).any()


def test_one_link_pendulum_closed_form():
    """A unit point mass on a unit massless link: omega^2 = +|g| hanging, -|g| inverted."""
    g = float(np.linalg.norm(parameters.base_values(common.build("pendulum1")[0])["gravity"]))
    got = nr.normal_modes("pendulum1", np.array([[0.0], [np.pi]]))
    assert (got.status == nr.OK).all() and list(got.count) == [1, 1]
    assert abs(got.omega2[0, 0] - g) <= 1e-13 * g and abs(got.omega2[1, 0] + g) <= 1e-13 * g
    assert np.abs(got.modes - 1.0).max() <= 1e-14          # M = 1: the M-orthonormal shape is 1, positive by the sign rule


# (mutation, the systems that reach it, the least number of eigenvalue bounds it must miss by: a tenth of the smallest measured)
TEETH = [("mu_curvature", dict(mu_curvature=False), ("scissor4", "mixed_loop", "puppet40")),
         ("vqq_sign", dict(vqq_sign=-1.0), ("pendulum5", "spring_arm", "puppet40")),
         ("z_first", dict(z_first=True), ("mixed_loop", "puppet40"))]


@pytest.mark.parametrize("tag,change,systems", TEETH, ids=[t[0] for t in TEETH])
def test_teeth(tag, change, systems):
    for name in systems:
        Q = nr.case_inputs(name)[:4]
        ref = nr.Modes(*[getattr(nr.case_reference(name), k)[:4] for k in nr.Modes._fields])
        bad = nr.normal_modes(name, Q, opt=nr.SPEC._replace(**change))
        if tag == "z_first":          # the wrong columns span (part of) the range of D': the shapes leave the tangent space
            miss = nr.invariants(name, Q, None, bad)["tangent"] / nr.invariant_bounds(name)["tangent"]
        else:
            miss = nr.eig_error(bad, ref) / nr.eig_bound(name)
        print(tag, name, "misses by %.3g bounds" % miss)
        assert miss >= 1e3, (tag, name, miss)


def test_teeth_mass_over_the_wrong_configs():
    """M indexed over the leading configs instead of F, with a held config that is not the last."""
    ev = nr.pose_of("pendulum5")
    free = nr.default_free(ev)
    free[0] = False
    Q = nr.case_inputs("pendulum5")[:4]
    ref = nr.normal_modes("pendulum5", Q, free)
    bad = nr.normal_modes("pendulum5", Q, free, opt=nr.SPEC._replace(mass_all=True))
    miss = nr.eig_error(bad, ref) / nr.TOL
    print("mass_all misses by %.3g bounds" % miss)
    assert miss >= 1e3


# ---- 2. the emulated kernel over the table ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nr.SYSTEMS)
def test_emulated_kernel_over_the_table(emulated, name):
    got = emulated(name)
    nr.compare(name, got)
    for k in nr.Modes._fields:
        assert np.array_equal(getattr(got, k)[nr.REPEAT], getattr(got, k)[0]), k


def test_emulated_mu_supplied_against_mu_computed(emulated):
    name = "mixed_loop"
    got = emulated(name)
    again = emu_modes_harness.EmuModes(common.build(name)[1]).normal_modes(nr.case_inputs(name), mu=got.mu)
    for k in nr.Modes._fields:
        assert np.array_equal(getattr(got, k), getattr(again, k)), k
    other = emu_modes_harness.EmuModes(common.build(name)[1]).normal_modes(nr.case_inputs(name), mu=np.zeros_like(got.mu))
    want = nr.normal_modes(name, nr.case_inputs(name), mu=np.zeros_like(got.mu))
    assert nr.eig_error(other, want) <= nr.eig_bound(name) and np.abs(other.residual - want.residual).max() <= 1e-10
    assert not other.mu.any()


def test_emulated_constant_q_list():
    name = "pendulum5"
    ev = nr.pose_of(name)
    free = nr.default_free(ev)
    free[1] = False
    Q = nr.case_inputs(name)[:6]
    got = emu_modes_harness.EmuModes(common.build(name)[1]).normal_modes(Q, free=free)
    want = nr.normal_modes(name, Q, free)
    assert list(got.count) == [4] * 6 and got.modes.shape == (6, 4, 5) and not got.modes[:, :, 1].any()
    assert nr.eig_error(got, want) <= nr.TOL
    inv = nr.invariants(name, Q, free, got)
    assert inv["held"] and max(inv["orthonormal"], inv["eigen"]) <= nr.MARGIN * nr.INVARIANT_MIN


# ---- 3. the statuses ----------------------------------------------------------------------------------------------------------------
def test_emulated_statuses():
    name = "pendulum5"
    emu = emu_modes_harness.EmuModes(common.build(name)[1])
    Q = nr.case_inputs(name)[:3].copy()
    one = emu.normal_modes(Q, max_sweeps=1)
    want = nr.normal_modes(name, Q, max_sweeps=1)
    assert list(one.status) == [nr.NOT_CONVERGED] * 3 == list(want.status) and list(one.sweeps) == [1] * 3
    assert one.omega2.any() and (np.diff(one.omega2, axis=1) >= 0.0).all()          # the current answer is still written, in order
    Q[1, 2] = np.nan
    got = emu.normal_modes(Q)
    assert list(got.status) == [nr.OK, nr.SINGULAR, nr.OK]
    for k in ("omega2", "modes", "count", "rank", "mu", "residual", "sweeps"):
        assert not np.asarray(getattr(got, k)[1]).any(), k
    assert list(nr.normal_modes(name, Q).status) == [nr.OK, nr.SINGULAR, nr.OK]


def test_emulated_massless_free_config_is_singular():
    """A parameter row without mass: M_r has no Cholesky factor."""
    name = "pendulum5"
    system = common.build(name)[0]
    base = parameters.base_values(system)
    damping = np.zeros(len(system.dyn_configs)) if base["damping"] is None else base["damping"]
    rows = np.array([np.concatenate([base["inertia"].ravel() * s, base["gravity"], damping]) for s in (1.0, 0.0)])
    Q = nr.case_inputs(name)[:2]
    got = emu_modes_harness.EmuModes(common.build(name)[1]).normal_modes(np.concatenate([Q, Q]), rows=rows, group=2)
    assert list(got.status) == [nr.OK, nr.OK, nr.SINGULAR, nr.SINGULAR]
    assert not got.omega2[2:].any() and not got.modes[2:].any() and not got.count[2:].any()
    assert nr.eig_error(nr.Modes(*[getattr(got, k)[:2] for k in nr.Modes._fields]), nr.normal_modes(name, Q)) <= nr.TOL


# ---- 4. the C entry points without a device -------------------------------------------------------------------------------------------
def lds_doubles(rollout, nq, nc):
    """modes_layout in words: the frame's regions and the kernel's own."""
    n, im = nq + nc, nq * (nq | 1)
    off = (rollout + 1) & ~1
    off += n * (n + 1) + 2 * nq * nq + 4 * im + nq
    off += nq + nq + 2 + (4 * nc + 2) + (nq + 2) + 2 * nq + n
    off = (off + 1) & ~1
    off += (nq + 1) // 2
    return (off + 1) & ~1


@pytest.mark.parametrize("name", ("pendulum1", "mixed_loop", "puppet40"))
def test_lds_of_a_workgroup(name):
    L = _lib.lib()
    d = common.build(name)[1]
    slice_, rollout = emu_modes_harness.EmuModes(d).lds_doubles()
    assert rollout == emu_harness.lds_slices(d)["rollout"]
    assert slice_ == lds_doubles(rollout, int(d.n_configs), int(d.n_constraints))
    sys_h = L.tg_system_create(d.byref())
    try:
        out = np.zeros(4, dtype=np.int32)
        rc = L.tg_system_normal_modes_lds(sys_h, out.ctypes.data_as(_lib._c_ip))
        assert rc == 0 and out[1] == slice_ and out[2] == (64 // out[0]) * slice_ * 8 and out[2] <= 160 * 1024 and out[3] == 0
        assert L.tg_system_normal_modes_lds(None, out.ctypes.data_as(_lib._c_ip)) == ERR_INVALID
    finally:
        L.tg_system_destroy(sys_h)


def test_refusals_without_a_device(monkeypatch):
    L = _lib.lib()
    out = np.zeros(4, dtype=np.int32)
    d = common.build("nonlinear_spring_arm")[1]
    sys_h = L.tg_system_create(d.byref())
    try:
        assert L.tg_system_normal_modes_lds(sys_h, out.ctypes.data_as(_lib._c_ip)) == ERR_UNSUPPORTED
        assert b"NonlinearConfigSpring" in L.tg_last_error()
    finally:
        L.tg_system_destroy(sys_h)
    monkeypatch.setenv("TREPAMD_TEAM", "1")
    d = common.build("puppet40")[1]
    sys_h = L.tg_system_create(d.byref())
    try:
        assert L.tg_system_normal_modes_lds(sys_h, out.ctypes.data_as(_lib._c_ip)) == ERR_UNSUPPORTED
        assert L.tg_last_error() == b"system too large for the LDS-resident normal-modes kernel" and out[0] == 1
    finally:
        L.tg_system_destroy(sys_h)
    z = np.zeros(8)
    for fn in (L.tg_batch_normal_modes, L.tg_batch_normal_modes_device):
        assert fn(None, z.ctypes.data, None, None, 1e-9, 30, z.ctypes.data, z.ctypes.data, None, None, None, None, None, None) == ERR_INVALID


def test_layout_and_declarations():
    assert ctypes.sizeof(emu_harness.RunArgs) == int(emu_modes_harness.lib().emu_sizeof_run_args())
    names = set(_lib.exported_symbols())
    assert set(_lib._MODES_SIGNATURES) <= names
    header = open(os.path.join(ROOT, "include", "trep_amd.h")).read()
    for n in _lib._MODES_SIGNATURES:
        assert "int %s(" % n in header


def test_parity_profile_covers_the_table():
    """The committed record names every system of the table and is consistent with itself; it recomputes nothing."""
    import json
    with open(os.path.join(ROOT, "profiles", "normal_modes_parity.json")) as f:
        prof = json.load(f)
    assert sorted(prof["cases"]) == sorted(nr.SYSTEMS)
    for name, row in prof["cases"].items():
        assert row["eig_bound"] == max(prof["tolerance"], prof["margin"] * max(row["floors"].values()))
        assert 2 * row["reference_sweeps"] < row["max_sweeps"]
        for side in ("emulation", "device"):
            if side in row:
                assert row[side]["eig_error"] <= row["eig_bound"] and row[side]["shape_in_bounds"] <= 1.0
