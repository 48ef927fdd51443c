"""CPU tests of the batched static response: the numpy specification (static_response_reference.py) against central differences of
the reference minimiser and against the modal sum of the normal-modes reference, its invariants, the teeth of its checks, the kernel
body compiled for the host (emu_response_harness.py) against the specification over the case table, the status cases, and the
refusals of the C entry points that need no device."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import common
import emu_harness
import emu_response_harness
import equilibrium_reference as er
import normal_modes_reference as nr
import static_response_reference as sr
from trep_amd import _lib

ERR_INVALID, ERR_UNSUPPORTED = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = tuple(sr.CASES)


@functools.lru_cache(maxsize=None)
def emu_of(name):
    return emu_response_harness.EmuResponse(common.build(name)[1])


@pytest.fixture(scope="module")
def emulated():
    cache = {}

    def get(case):
        if case not in cache:
            Q, free = sr.case_inputs(case)
            cache[case] = emu_of(sr.system_of(case)).static_response(Q, free)
        return cache[case]
    return get


def rel(a, b):
    """max |a - b| / max(1, |b|max)."""
    return float(np.abs(a - b).max(initial=0.0) / max(1.0, np.abs(b).max(initial=0.0)))


# ---- 1. the specification against central differences of the reference minimiser ---------------------------------------------------
def central_differences(case, q, mu, step):
    """(dq [nD][nq], dmu [nD][nc]) of the rest pose along every held config: the reference minimiser at tolerance 1e-13 from the
    pose moved by +-step along the specification's own dq (a predictor start, so that it stays on the branch)."""
    name, free = sr.system_of(case), sr.free_mask(case)
    drive = sr.default_drive(free)
    lin = sr.static_response(name, q[None], free, mu=mu[None], compliance=False)
    dq, dmu = np.zeros((len(drive), len(q))), np.zeros((len(drive), len(mu)))
    for j in range(len(drive)):
        ends = [er.minimize(name, (q + s * step * lin.dq[0, j])[None], free, tolerance=1e-13) for s in (1.0, -1.0)]
        dq[j] = (ends[0].Q[0] - ends[1].Q[0]) / (2 * step)
        dmu[j] = (ends[0].mu[0] - ends[1].mu[0]) / (2 * step)
    return dq, dmu


@pytest.mark.parametrize("case", ("spring_link", "scissor4_slider", "puppet40"))
def test_specification_against_central_differences(case):
    """The bound: MARGIN x the difference between the quotients of steps 1e-5 and 2e-5 (their truncation and cancellation), at least
    the rounding of a quotient whose end points are of order one, eps / step.
    Measured (dq / dmu, error under bound): spring_link 2.1e-12 / 1.4e-18 under 1.4e-9, scissor4 with the slider held 1.1e-9 under
    2.2e-7 / 5.6e-9 under 1.1e-6, puppet40 1.5e-9 under 2.9e-7 / 1.8e-9 under 3.3e-7."""
    name, free = sr.system_of(case), sr.free_mask(case)
    q = sr.case_inputs(case)[0][0]
    rest = er.minimize(name, q[None], free, tolerance=1e-13)
    q, mu = rest.Q[0], rest.mu[0]
    ref = sr.static_response(name, q[None], free, mu=mu[None], compliance=False)
    fine, coarse = central_differences(case, q, mu, 1e-5), central_differences(case, q, mu, 2e-5)
    for k, got, a, b in (("dq", ref.dq[0], fine[0], coarse[0]), ("dmu", ref.dmu[0], fine[1], coarse[1])):
        err, bound = rel(got, a), sr.MARGIN * max(rel(b, a), nr.EPS / 1e-5)
        print(case, k, "error %.3e bound %.3e" % (err, bound))
        assert err <= bound and bound < 1e-4, (case, k, err, bound)


# ---- 2. the compliance against the modal sum ------------------------------------------------------------------------------------------
MODAL = ("spring_link", "mixed_loop", "spatial_loop", "scissor4_free", "pendulum1", "ladder_mixed", "puppet40")      # F = the dynamic configs


def modal_sum(case, ref, **kw):
    name = sr.system_of(case)
    Q, _ = sr.case_inputs(case)
    m = nr.normal_modes(name, Q, mu=ref.mu, **kw)
    assert (m.status == nr.OK).all()
    out = []
    for b in range(len(Q)):
        n = int(m.count[b])
        Phi = m.modes[b][:n]
        out.append(Phi.T.dot(Phi / m.omega2[b][:n, None]))
    return np.array(out)


@pytest.mark.parametrize("case", MODAL)
def test_compliance_is_the_modal_sum(case):
    """C = Phi diag(1 / omega2) Phi' of normal_modes_reference with the same mask and multipliers.  The floor: what either side of the
    identity changes under the rival ladder and under LAPACK in place of its own factorisations; the scissor4 row with every
    dynamic config free (rank 4 of 8 constraints) goes through the same rule.  Measured: at most 2.0e-15 (puppet40, |C|max 13.3,
    bound 2.2e-11); scissor4 3.5e-17 at the one minimum its golden poses lead to."""
    assert np.array_equal(sr.free_mask(case), nr.default_free(nr.pose_of(sr.system_of(case))))
    ref = sr.case_reference(case)
    per_pose = lambda A, B: max(rel(a, b) for a, b in zip(A, B))
    modal = modal_sum(case, ref)
    floors = dict(modal_ladder=per_pose(modal_sum(case, ref, opt=nr.SPEC._replace(rival=True)), modal),
                  modal_lapack=per_pose(modal_sum(case, ref, lapack=True), modal),
                  ladder=per_pose(sr.case_reference(case, "rival").compliance, ref.compliance),
                  lapack=per_pose(sr.case_reference(case, "lapack").compliance, ref.compliance))
    err, bound = per_pose(ref.compliance, modal), max(sr.TOL, sr.MARGIN * max(floors.values()))
    print(case, "difference %.3e bound %.3e |C|max %.3e" % (err, bound, np.abs(ref.compliance).max()), floors)
    assert err <= bound


# ---- 3. the invariants ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_invariants_of_the_specification(case):
    """The LAPACK variant is another computation of the same answer: its invariants stay within what the specification's own leave."""
    Q, free = sr.case_inputs(case)
    name = sr.system_of(case)
    ref, lap = sr.case_reference(case), sr.case_reference(case, "lapack")
    assert (ref.status == sr.OK).all() and np.array_equal(ref.rank, lap.rank)
    ib = sr.invariant_bounds(case)
    for side in (ref, lap):
        inv = sr.invariants(name, Q, free, side)
        print(case, inv, ib)
        assert inv["held"] and all(inv[k] <= ib[k] for k in ib), (inv, ib)
    assert (ref.defect <= sr.DEFECT_ZERO).all()


# ---- 4. teeth -------------------------------------------------------------------------------------------------------------------------
MUTATIONS = dict(no_fh_curvature=dict(fh_curvature=False), no_fh_vqq=dict(fh_vqq=False), no_dh=dict(dh_term=False), no_ff_curvature=dict(ff_curvature=False))


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_mutations_are_far_from_the_specification(mutation):
    case = "mixed_loop"
    Q, free = sr.case_inputs(case)
    ref, bounds = sr.case_reference(case), sr.case_bounds(case)
    bad = sr.static_response(sr.system_of(case), Q, free, opt=sr.SPEC._replace(**MUTATIONS[mutation]))
    err = sr.errors(bad, ref)
    far = max(err[k] / bounds[k] for k in ("dq", "dmu"))
    print(mutation, err, "bounds away: %.3e" % far)
    assert far >= 1e6


# ---- 5. the kernel compiled for the host ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_emulated_kernel_over_the_table(case, emulated):
    sr.compare(case, emulated(case))


@pytest.mark.parametrize("case", ("mixed_loop", "scissor4_slider", "puppet40"))
def test_emulated_drive_subsets_and_no_compliance(case, emulated):
    Q, free = sr.case_inputs(case)
    emu, full = emu_of(sr.system_of(case)), emulated(case)
    every = sr.default_drive(free)
    places = list(range(len(every)))[::-1][::2]      # a subset, out of order
    part = emu.static_response(Q, free, drive=every[places])
    for k in sr.Response._fields:
        if k == "defect":                                 # (the worst over the driven columns: of fewer, no larger)
            assert (part.defect <= full.defect).all()
            continue
        want = getattr(full, k)[:, places] if k in ("dq", "dmu") else getattr(full, k)
        assert np.array_equal(getattr(part, k), want), k
    lean = emu.static_response(Q, free, compliance=False)
    assert lean.compliance is None and lean.reaction is None
    for k in ("dq", "dmu", "rank", "mu", "residual", "defect", "status"):
        assert np.array_equal(getattr(lean, k), getattr(full, k)), k


def test_emulated_mu_supplied(emulated):
    case = "mixed_loop"
    Q, free = sr.case_inputs(case)
    full = emulated(case)
    again = emu_of(sr.system_of(case)).static_response(Q, free, mu=full.mu)
    for k in sr.Response._fields:
        assert np.array_equal(getattr(again, k), getattr(full, k)), k


def test_emulated_statuses():
    """A pose that is not finite and a maximum (the inverted pendulum): TG_SINGULAR, every output zero, in both."""
    case, name = "pendulum5_joint", "pendulum5"
    Q, free = sr.case_inputs(case)
    Q = Q[:3].copy()
    Q[1, 0] = np.nan
    Q[2] = 0.0
    Q[2, 0] = np.pi
    got = emu_of(name).static_response(Q, free)
    want = sr.static_response(name, Q, free)
    assert list(got.status) == list(want.status) == [sr.OK, sr.SINGULAR, sr.SINGULAR]
    for k in sr.Response._fields[:-1]:
        assert not np.asarray(getattr(got, k)[1:]).any() and not np.asarray(getattr(want, k)[1:]).any(), k


# ---- 6. the C entry points without a device ---------------------------------------------------------------------------------------------
def lds_doubles(rollout, nq, nc, nF, nD, loads):
    """response_layout in words: the frame's regions and the kernel's own."""
    n, N, jl = nq + nc, nD + (nF if loads else 0), nF | 1
    off = (rollout + 1) & ~1
    off += n * (n + 1) + nq * nq + nc * max(nF, nD) + nF * jl + max(nF * jl, max(nF, nc) * N) + 2 * nF * max(N, 1)
    off += nq + nq + 2 + (4 * nc + 2) + 2 * ((nq + 1) // 2) + n
    off = (off + 1) & ~1
    off += (nq + 1) // 2
    return (off + 1) & ~1


@pytest.mark.parametrize("case", ("pendulum1", "mixed_loop", "puppet40"))
def test_lds_of_a_workgroup(case):
    L = _lib.lib()
    d = common.build(sr.system_of(case))[1]
    free = sr.free_mask(case)
    nF, nD = int(free.sum()), int((~free).sum())
    sys_h = L.tg_system_create(d.byref())
    try:
        for loads in (1, 0):
            slice_, rollout = emu_of(sr.system_of(case)).lds_doubles(nF, nD, loads)
            assert rollout == emu_harness.lds_slices(d)["rollout"]
            assert slice_ == lds_doubles(rollout, int(d.n_configs), int(d.n_constraints), nF, nD, loads)
            out = np.zeros(4, dtype=np.int32)
            rc = L.tg_system_static_response_lds(sys_h, nF, nD, loads, out.ctypes.data_as(_lib._c_ip))
            assert rc == 0 and out[1] == slice_ and out[2] == (64 // out[0]) * slice_ * 8 and out[2] <= 160 * 1024 and out[3] == 0
        assert L.tg_system_static_response_lds(None, nF, nD, 1, out.ctypes.data_as(_lib._c_ip)) == ERR_INVALID
        assert L.tg_system_static_response_lds(sys_h, nF, nD + 1, 1, out.ctypes.data_as(_lib._c_ip)) == ERR_INVALID
    finally:
        L.tg_system_destroy(sys_h)


def test_refusals_without_a_device(monkeypatch):
    L = _lib.lib()
    out = np.zeros(4, dtype=np.int32)
    d = common.build("nonlinear_spring_arm")[1]
    sys_h = L.tg_system_create(d.byref())
    try:
        assert L.tg_system_static_response_lds(sys_h, 1, 0, 1, out.ctypes.data_as(_lib._c_ip)) == ERR_UNSUPPORTED
        assert b"NonlinearConfigSpring" in L.tg_last_error()
    finally:
        L.tg_system_destroy(sys_h)
    monkeypatch.setenv("TREPAMD_TEAM", "1")
    d = common.build("puppet40")[1]
    sys_h = L.tg_system_create(d.byref())
    try:
        assert L.tg_system_static_response_lds(sys_h, 22, 18, 1, out.ctypes.data_as(_lib._c_ip)) == ERR_UNSUPPORTED
        assert L.tg_last_error() == b"system too large for the LDS-resident static-response kernel" and out[0] == 1
    finally:
        L.tg_system_destroy(sys_h)
    z = np.zeros(8)
    drive = np.zeros(1, dtype=np.int32)
    for fn in (L.tg_batch_static_response, L.tg_batch_static_response_device):
        assert fn(None, z.ctypes.data, None, None, 0, drive.ctypes.data, 1, 1e-9, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data,
                  None, None, None, None, None) == ERR_INVALID


def test_layout_and_declarations():
    assert ctypes.sizeof(emu_harness.RunArgs) == int(emu_response_harness.lib().emu_sizeof_run_args())
    names = set(_lib.exported_symbols())
    assert set(_lib._RESPONSE_SIGNATURES) <= names
    header = open(os.path.join(ROOT, "include", "trep_amd.h")).read()
    for n in _lib._RESPONSE_SIGNATURES:
        assert "int %s(" % n in header
        assert hasattr(_lib.lib(), n)


def test_parity_profile_covers_the_table():
    """The committed record names every case of the table and is consistent with itself; it recomputes nothing."""
    with open(os.path.join(ROOT, "profiles", "static_response_parity.json")) as f:
        prof = json.load(f)
    assert sorted(prof["cases"]) == sorted(sr.CASES)
    for case, row in prof["cases"].items():
        for k, bound in row["bounds"].items():
            assert bound == max(prof["tolerance"], prof["margin"] * max(row["floors"]["lapack"][k], row["floors"]["ladder"][k]))
        for side in ("emulation", "device"):
            if side in row:
                assert all(row[side]["errors"][k] <= row["bounds"][k] for k in row[side]["errors"])
    assert set(prof["throughput"]) >= {"system", "batch", "ms_with_compliance", "ms_without_compliance"}
