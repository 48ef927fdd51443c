"""Batched frame kinematics without a device: the specification (frame_kinematics_reference.py) against the reference project's
recorded frame values, the kernel itself (mvi_frames.hpp) compiled for the host with TEAM = 1 (emu_frames_harness.py) over the case
table and over the selections, the mistakes the table must tell apart, and the LDS geometry and refusals of the C entry points.

Measured here: the closed formulas sit at most 5.4e-4 of a bound from the host accessors and the emulated kernel at most 7.5e-4
(ladder_mixed), over all frames of all seven systems; the planted mistakes miss by 5e10 bounds at the least."""
import ctypes
import os

import numpy as np
import pytest

import common
import emu_harness
import emu_frames_harness
import frame_kinematics_reference as fr
from trep_amd import _lib

ERR_INVALID, ERR_UNSUPPORTED = -1, -3
B, M = 5, 3


def _emu(name):
    return emu_frames_harness.EmuFrames(fr.system_of(name)[1])


# ---- 1. the specification against the reference project's recorded values -------------------------------------------------------------
@pytest.mark.parametrize("name", fr.GOLDEN_SYSTEMS)
def test_reference_module_matches_the_recorded_frames(name):
    g = common.golden("frames")
    system = common.build(name)[0]
    got = fr.reference(system, g[name + "_q"], g[name + "_dq"])
    want_g, want_p, want_vb = g[name + "_g"], g[name + "_p"], g[name + "_vb"]
    assert len(want_g) == len(system.frames)
    bound = lambda tol, w: tol * max(1.0, float(np.abs(w).max()))
    assert np.abs(got.g - want_g[:, :3]).max() <= bound(1e-12, want_g)
    assert np.abs(got.g[:, :, 3] - want_p[:, :3]).max() <= bound(1e-12, want_p)
    want_vb6 = np.array([fr.vec6(m) for m in want_vb])
    assert np.abs(got.vb - want_vb6).max() <= bound(1e-12, want_vb6)
    for m in want_vb:                                    # the recorded matrices are twists: nothing is lost by the 6-vector
        assert np.abs(m[:3, :3] + m[:3, :3].T).max() <= 1e-12 and not m[3].any()
    nonzero = 0
    for c, w in zip(g[name + "_p_dq_cases"], g[name + "_p_dq"]):
        assert np.abs(got.p_dq[c[0], c[1]] - w[:3]).max() <= bound(1e-11, w) and w[3] == 0.0
        nonzero += bool(np.abs(w).max() > 0)
    assert nonzero
    nonzero = 0
    for c, w in zip(g[name + "_vb_ddq_cases"], g[name + "_vb_ddq"]):
        assert np.abs(got.vb_ddq[c[0], c[1]] - fr.vec6(w)).max() <= bound(1e-11, w)
        nonzero += bool(np.abs(w).max() > 0)
    assert nonzero


# ---- 2. the emulated kernel over the table ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fr.SYSTEMS)
def test_emulated_kernel_over_the_table(name):
    system = fr.system_of(name)[0]
    Q, dQ, at = fr.batch_states(name, B, M)
    got = _emu(name).frame_kinematics(Q, dQ)                    # outputs and scratch start as NaN
    fr.compare(got, fr.expected(name, at), tag=name + " ")
    off = fr.off_path(system)
    assert off.any() and not off.all()
    for a in (got.p_dq, got.vb_ddq):                            # off the path: exactly zero, not small
        assert not a[:, :, off].any()
    assert np.array_equal(got.g[:, :, 0], np.broadcast_to(np.eye(4)[:3], (B, M, 3, 4)))      # the world frame


def test_emulated_kernel_does_not_depend_on_what_the_scratch_held():
    Q, dQ, _ = fr.batch_states("mixed_loop", B, M)
    emu = _emu("mixed_loop")
    a, b = emu.frame_kinematics(Q, dQ, poison=True), emu.frame_kinematics(Q, dQ, poison=False)
    for f in fr.FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def test_emulated_kernel_reads_strided_rows_and_needs_no_rates():
    name = "scissor4"
    Q, dQ, at = fr.batch_states(name, B, M)
    emu = _emu(name)
    whole = emu.frame_kinematics(Q, dQ)
    rng = np.random.default_rng(5)
    X = rng.standard_normal((B, M, Q.shape[2] + 7))
    X[:, :, :Q.shape[2]] = Q
    got = emu.frame_kinematics(X, None)
    assert got.vb is None
    for f in ("g", "p_dq", "vb_ddq"):
        assert np.array_equal(getattr(got, f), getattr(whole, f)), f
    alone = emu.frame_kinematics(Q, None, jacobians=False)
    assert alone.p_dq is None and alone.vb_ddq is None and np.array_equal(alone.g, whole.g)
    rates = emu.frame_kinematics(Q, dQ, jacobians=False, want_g=False)
    assert rates.g is None and np.array_equal(rates.vb, whole.vb)


# ---- 3. selections ------------------------------------------------------------------------------------------------------------------
def _selections(system, rng):
    n = len(system.frames)
    fixed = fr.fixed_frames(system)
    assert fixed[0] == 0 and 1 <= len(fixed) <= 5
    some = rng.permutation(n)[:max(2, min(n - 1, 11))]             # more than one pass of the kernel where the system has the frames
    shuffled = np.concatenate([some, some[:1]])
    rng.shuffle(shuffled)
    return {"one": [n - 1], "world": [0], "fixed": [fixed[-1]], "shuffled": list(shuffled)}


@pytest.mark.parametrize("name", fr.SYSTEMS)
def test_emulated_selections(name):
    system = fr.system_of(name)[0]
    Q, dQ, at = fr.batch_states(name, B, M)
    emu = _emu(name)
    whole = emu.frame_kinematics(Q, dQ)
    anchors = emu.anchors()
    assert [f for f in range(len(anchors)) if anchors[f] < 0] == fr.fixed_frames(system)
    for tag, sel in _selections(system, np.random.default_rng(common.tb_seed("frame selections", name))).items():
        got = emu.frame_kinematics(Q, dQ, frames=sel)
        fr.compare(got, fr.expected(name, at, sel), tag="%s %s " % (name, tag))
        for f in fr.FIELDS:                                        # a frame's answer does not depend on the selection around it:
            assert np.array_equal(getattr(got, f), getattr(whole, f)[:, :, sel]), (tag, f)      # equal bits, repeats included
        if tag in ("world", "fixed"):
            assert anchors[sel[0]] < 0 and not got.vb.any() and not got.p_dq.any() and not got.vb_ddq.any()
            assert np.array_equal(got.g, np.broadcast_to(got.g[0, 0], got.g.shape))             # a constant of the system


# ---- 4. the table can tell ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", fr.MUTANTS)
def test_mutation_misses_the_table(mutant):
    reached = 0
    for name in fr.SYSTEMS:
        system = fr.system_of(name)[0]
        q, dq = fr.states(name)
        ref = fr.state_references(name)
        want = fr.Arrays(*[getattr(ref, f)[0] for f in fr.FIELDS])
        clean = fr.worst_ratio(fr.formulas(system, q[0], dq[0]), want)
        assert clean <= 1.0, (name, clean)
        if mutant == "state_off_by_one":
            ratio = fr.worst_ratio(fr.formulas(system, q[1], dq[1]), want)
        elif fr.reaches(system, mutant, q[0]):
            ratio = fr.worst_ratio(fr.formulas(system, q[0], dq[0], mutant=mutant), want)
        else:
            continue
        reached += 1
        print("%s on %s: misses by %.3g bounds (the formulas themselves: %.3g)" % (mutant, name, ratio, clean))
        assert ratio > 1e6, (mutant, name, ratio)
    assert reached >= 1


# ---- 5. the C entry points without a device -------------------------------------------------------------------------------------------
LDS_CELLS = [(n, t) for n in ("pendulum1", "pend_on_cart", "scissor4", "mixed_loop", "puppet40") for t in (1, 4, 16, 64)]


def lds_doubles(rollout):
    """Per team: the rollout slice and eight staged frames, pose [12] and world twist [6] each -- whatever the selection."""
    even = lambda x: (x + 1) & ~1
    return even(even(rollout) + 8 * 12 + 8 * 6)


@pytest.mark.parametrize("name,team", LDS_CELLS)
def test_lds_of_a_workgroup_and_its_refusal(monkeypatch, name, team):
    monkeypatch.setenv("TREPAMD_TEAM", str(team))
    L = _lib.lib()
    d = fr.system_of(name)[1]
    slice_, rollout = _emu(name).lds_doubles()
    assert rollout == emu_harness.lds_slices(d)["rollout"]
    assert slice_ == lds_doubles(rollout)
    sys_h = L.tg_system_create(d.byref())
    assert sys_h
    try:
        out = np.zeros(4, dtype=np.int32)
        rc = L.tg_system_frame_kinematics_lds(sys_h, out.ctypes.data_as(_lib._c_ip))
        bytes_ = (64 // team) * slice_ * 8
        assert list(out) == [team, slice_, bytes_, 0]
        if bytes_ > 160 * 1024:
            assert rc == ERR_UNSUPPORTED and L.tg_last_error() == b"system too large for the LDS-resident frame-kinematics kernel"
        else:
            assert rc == 0
    finally:
        L.tg_system_destroy(sys_h)


def test_both_sides_of_the_lds_limit_are_in_the_cells(monkeypatch):
    L = _lib.lib()
    seen = set()
    for name, team in LDS_CELLS:
        monkeypatch.setenv("TREPAMD_TEAM", str(team))
        sys_h = L.tg_system_create(fr.system_of(name)[1].byref())
        out = np.zeros(4, dtype=np.int32)
        seen.add(L.tg_system_frame_kinematics_lds(sys_h, out.ctypes.data_as(_lib._c_ip)))
        L.tg_system_destroy(sys_h)
    assert seen == {0, ERR_UNSUPPORTED}


def test_null_handles_are_refused():
    L = _lib.lib()
    q = np.zeros(8)
    one = np.zeros(1, dtype=np.int32)
    assert L.tg_batch_frame_kinematics(None, 1, q.ctypes.data, None, 1, one.ctypes.data, q.ctypes.data, None, None, None) == ERR_INVALID
    assert L.tg_last_error() == b"null argument"
    assert L.tg_batch_frame_kinematics_device(None, 1, q.ctypes.data, 8, None, 8, 1, one.ctypes.data, q.ctypes.data, None, None, None) == ERR_INVALID
    assert L.tg_last_error() == b"null argument"
    assert L.tg_system_frame_kinematics_lds(None, None) == ERR_INVALID and L.tg_last_error() == b"null argument"


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_every_refusal_is_decided_without_a_device(device):
    """Each refusal of the entry points returns TG_ERR_INVALID with no device present.  What the arguments alone show is refused with
    its own message whatever the handle; a frame index outside the system and a short row stride need the system, and a handle
    without one (no batch exists without a device) is refused as a null argument there: test_gpu_frame_kinematics.py sees those two
    with their own messages."""
    L = _lib.lib()
    batch = ctypes.create_string_buffer(1 << 20)          # a handle with no system behind it
    q = np.zeros(64)
    sel = np.zeros(2, dtype=np.int32)
    b, p, f = ctypes.addressof(batch), q.ctypes.data, sel.ctypes.data

    def call(n_states, Q, dQ, n_frames, frames, G, VB, JP, JB, stride=8):
        if device:
            return L.tg_batch_frame_kinematics_device(b, n_states, Q, stride, dQ, stride, n_frames, frames, G, VB, JP, JB)
        return L.tg_batch_frame_kinematics(b, n_states, Q, dQ, n_frames, frames, G, VB, JP, JB)
    for args, message in (
            ((0, p, p, 2, f, p, p, p, p), b"n_states must be at least 1"),
            ((-2, p, p, 2, f, p, p, p, p), b"n_states must be at least 1"),
            ((1, None, p, 2, f, p, p, p, p), b"null Q"),
            ((1, p, p, 0, f, p, p, p, p), b"no frames selected"),
            ((1, p, p, 2, None, p, p, p, p), b"no frames selected"),
            ((1, p, None, 2, f, p, p, p, p), b"VB without dQ"),
            ((1, p, p, 2, f, None, None, None, None), b"no output asked for"),
            ((1, p, None, 2, f, None, None, None, None), b"no output asked for")):
        assert call(*args) == ERR_INVALID
        assert L.tg_last_error() == message
    sel[:] = (0, 1 << 20)                                  # a frame outside any system, a stride under any nq
    assert call(1, p, p, 2, f, p, p, p, p) == ERR_INVALID
    assert call(1, p, p, 2, f, p, p, p, p, stride=0) == ERR_INVALID


def test_the_new_entry_points_are_exported_and_declared():
    names = set(_lib.exported_symbols())
    assert {"tg_batch_frame_kinematics", "tg_batch_frame_kinematics_device", "tg_system_frame_kinematics_lds"} <= names
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "trep_amd.h")).read()
    for n in _lib._FRAMES_SIGNATURES:
        assert "int %s(" % n in header
    L = _lib.lib()
    for n in _lib._FRAMES_SIGNATURES:
        assert getattr(L, n)


def test_the_emulator_build_is_ignored_by_git():
    """Like the other emulators' builds: the on-demand .so falls under the `*.so` rule of .gitignore, and no rule takes it out again."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    emu_frames_harness.lib()
    assert os.path.exists(os.path.join(root, "tests", "emu_frames", "libtrepamd_emu_frames.so"))
    rules = [line.strip() for line in open(os.path.join(root, ".gitignore")) if line.strip() and not line.startswith("#")]
    assert "*.so" in rules and not [r for r in rules if r.startswith("!")]
