"""Batched tape measures without a device: the specification (tape_measure_reference.py) against the reference project's recorded
tape, the condition of the case table, the closed formulas and the floors they give, the mistakes the table must tell apart, the
kernel itself (mvi_tape.hpp) compiled for the host with TEAM = 1 (emu_tape_harness.py) over the case table, the selections, the
optional outputs, strided rows, the pass cut and the cached table, and the LDS geometry and refusals of the C entry points.

Measured here: the closed formulas sit at most 1.2e-15 (relative) from the host accessors, so 64 floors stay under every tolerance
and the bounds are the project's own; the emulated kernel stays under 1e-3 of a bound on all seven systems; the planted mistakes miss
by 3.6e10 bounds at the least, except the common ancestors, which only the exact-zero check catches (values within 5e-4 of a bound)."""
import ctypes
import os

import numpy as np
import pytest

import common
import emu_harness
import emu_tape_harness
import tape_measure_reference as tr
from trep_amd import _lib

ERR_INVALID, ERR_UNSUPPORTED = -1, -3
B, M = 5, 3


def _emu(name):
    return emu_tape_harness.EmuTape(tr.system_of(name)[1])


def _ms(name):
    return [list(m) for m in tr.measures(name)]


def _same(a, b):
    for f in tr.FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f
        if x is not None:
            assert np.array_equal(x, y), f


def _exact_zeros(name, got, measure_list=None):
    zq, zqq = tr.structural_zeros(tr.system_of(name)[0], tr.measures(name) if measure_list is None else measure_list)
    ok = True
    for a, z in ((got.length_dq, zq), (got.velocity_dq, zq), (got.length_dqdq, zqq)):
        if a is not None:
            ok = ok and not a[..., z].any()
    return ok


# ---- 1. the specification against the reference project's recorded tape ---------------------------------------------------------------
def test_reference_module_matches_the_recorded_tape():
    g = common.golden("elements")
    system = common.build("extensor_tendon")[0]
    m = tr.measures("extensor_tendon")[0]
    assert [system.frames[f].name for f in m] == [str(n) for n in g["tape_frames"]]
    got = tr.reference(system, g["tape_q"], g["tape_dq"], [m])
    for field, recorded in (("length", "length"), ("velocity", "velocity"), ("length_dq", "length_dq"), ("length_dq", "velocity_ddq"),
                            ("velocity_dq", "velocity_dq"), ("length_dqdq", "length_dqdq"), ("length_dqdq", "velocity_ddqdq")):
        want = g["tape_" + recorded]
        have = getattr(got, field)[0]
        assert have.shape == want.shape, recorded
        assert np.abs(have - want).max() <= 1e-11 * max(1.0, np.abs(want).max()), recorded
    assert np.abs(g["tape_length_dqdq"]).max() > 0.1


# ---- 2. the condition of the table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tr.SYSTEMS)
def test_every_segment_of_the_table_is_long_enough(name):
    lengths = tr.segment_lengths(name)
    print(name, "shortest segment %.3f" % lengths.min())
    assert lengths.min() >= tr.MIN_SEGMENT


def test_the_measures_cover_what_the_issue_lists():
    all_ = {n: tr.measures(n) for n in tr.SYSTEMS}
    assert [len(m) for m in all_["puppet40"]] == [2] * 6 and len(tr.states("puppet40")[0]) == 3
    long_ = [n for n in tr.SYSTEMS if any(len(m) - 1 >= 17 for m in all_[n])]
    assert long_ and "puppet40" not in long_
    constant = 0
    for n in tr.SYSTEMS:
        system = tr.system_of(n)[0]
        zq, _ = tr.structural_zeros(system, all_[n])
        constant += int(zq.all(axis=1).sum())
        assert any(len(m) == 2 for m in all_[n])                               # one segment
    assert constant >= 3                                                        # between frames with no variable ancestor
    assert any(len(set(all_[n])) < len(all_[n]) for n in tr.SYSTEMS)            # a repeated measure
    assert any(tr.exclusive(tr.system_of(n)[0], a, b)[1] for n in tr.SYSTEMS for m in all_[n] for a, b in zip(m[:-1], m[1:]))


# ---- 3. the closed formulas and the floors --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tr.SYSTEMS)
def test_formulas_agree_with_the_reference(name):
    ref, clo, floors = tr.state_references(name), tr.state_formulas(name), tr.floors(name)
    for f in tr.FIELDS:
        print("%s %s: floor %.3e, tolerance %.3e" % (name, f, floors[f], tr.tolerance(name, f)))
        assert tr.tolerance(name, f) == max(tr.TOL[f], 64 * floors[f])
    assert tr.worst_ratio(name, clo, ref) <= 1.0 / 64 + 1e-12
    assert _exact_zeros(name, clo)


# ---- 4. the table can tell ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", tr.MUTANTS)
def test_mutation_misses_the_table(mutant):
    reached = 0
    for name in tr.SYSTEMS:
        system, ms = tr.system_of(name)[0], tr.measures(name)
        q, dq = tr.states(name)
        ref = tr.state_references(name)
        want = tr.Arrays(*[getattr(ref, f)[0] for f in tr.FIELDS])
        clean = tr.formulas(system, q[0], dq[0], ms)
        assert tr.worst_ratio(name, clean, want) <= 1.0 and _exact_zeros(name, clean)
        if mutant == "state_off_by_one":
            got = tr.formulas(system, q[1], dq[1], ms)
        elif tr.reaches(name, mutant):
            got = tr.formulas(system, q[0], dq[0], ms, mutant=mutant)
        else:
            continue
        reached += 1
        ratio, zeros = tr.worst_ratio(name, got, want), _exact_zeros(name, got)
        print("%s on %s: misses by %.3g bounds, exact zeros %s" % (mutant, name, ratio, "kept" if zeros else "lost"))
        assert ratio >= 1e3 or not zeros, (mutant, name, ratio)
        if mutant == "common_not_excluded":
            assert not zeros
    assert reached >= 1


# ---- 5. the emulated kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tr.SYSTEMS)
def test_emulated_kernel_over_the_table(name):
    Q, dQ, at = tr.batch_states(name, B, M)
    got = _emu(name).tape_measures(Q, dQ, _ms(name))                  # outputs and scratch start as NaN
    tr.compare(name, got, tr.expected(name, at), tag=name + " ")
    assert _exact_zeros(name, got)
    assert np.array_equal(got.length_dqdq, np.swapaxes(got.length_dqdq, -1, -2))      # symmetric to the bit


def test_emulated_kernel_does_not_depend_on_what_the_scratch_held():
    Q, dQ, _ = tr.batch_states("mixed_loop", B, M)
    emu = _emu("mixed_loop")
    _same(emu.tape_measures(Q, dQ, _ms("mixed_loop"), poison=True), emu.tape_measures(Q, dQ, _ms("mixed_loop"), poison=False))


@pytest.mark.parametrize("name", tr.SYSTEMS)
def test_emulated_selections(name):
    """A measure's answer does not depend on the selection around it: one alone, reversed order, doubled -- equal bits."""
    Q, dQ, at = tr.batch_states(name, B, M)
    emu, ms = _emu(name), _ms(name)
    whole = emu.tape_measures(Q, dQ, ms)
    T = len(ms)
    for tag, sel in (("last", [T - 1]), ("first", [0]), ("reversed", list(range(T))[::-1]), ("doubled", list(range(T)) + list(range(T)))):
        got = emu.tape_measures(Q, dQ, [ms[t] for t in sel])
        tr.compare(name, got, tr.expected(name, at, sel), tag="%s %s " % (name, tag))
        for f in tr.FIELDS:
            assert np.array_equal(getattr(got, f), getattr(whole, f)[:, :, sel]), (tag, f)


def test_emulated_optional_outputs_and_strided_rows():
    name = "spatial_loop"
    Q, dQ, at = tr.batch_states(name, B, M)
    emu, ms = _emu(name), _ms(name)
    whole = emu.tape_measures(Q, dQ, ms)
    rng = np.random.default_rng(5)
    X = rng.standard_normal((B, M, Q.shape[2] + 7))
    X[:, :, :Q.shape[2]] = Q
    got = emu.tape_measures(X, None, ms)                               # rows 7 doubles further apart, no rates
    assert got.velocity is None and got.velocity_dq is None
    for f in ("length", "length_dq", "length_dqdq"):
        assert np.array_equal(getattr(got, f), getattr(whole, f)), f
    alone = emu.tape_measures(Q, None, ms, gradients=False, hessians=False)
    assert alone.length_dq is None and alone.length_dqdq is None and np.array_equal(alone.length, whole.length)
    rates = emu.tape_measures(Q, dQ, ms, gradients=False, hessians=False, want_length=False)
    assert rates.length is None and np.array_equal(rates.velocity, whole.velocity)
    grads = emu.tape_measures(Q, dQ, ms, hessians=False, want_length=False)
    assert np.array_equal(grads.length_dq, whole.length_dq) and np.array_equal(grads.velocity_dq, whole.velocity_dq)
    hess = emu.tape_measures(Q, None, ms, gradients=False, want_length=False)
    assert hess.length is None and np.array_equal(hess.length_dqdq, whole.length_dqdq)


def test_the_pass_cut_at_16_and_17_segments():
    """A pass holds whole measures, max(16, longest) segments at the most: the cuts, and equal bits whichever pass a measure lands in."""
    name = "pend_on_cart"
    Q, dQ, _ = tr.batch_states(name, B, M)
    emu = _emu(name)
    walk = lambda n: [3 if i % 2 == 0 else 0 for i in range(n + 1)]
    one = [1, 3]
    alone = {n: emu.tape_measures(Q, dQ, [walk(n)]) for n in (8, 15, 16, 17)}
    alone[1] = emu.tape_measures(Q, dQ, [one])
    for sel, sizes, cuts in (([walk(16), one], (16, 1), [0, 1, 2]), ([walk(15), one], (15, 1), [0, 2]), ([walk(17), one], (17, 1), [0, 1, 2]),
                             ([walk(8), walk(8), one], (8, 8, 1), [0, 2, 3]), ([one] * 17, (1,) * 17, [0, 16, 17]),
                             ([one, walk(17), walk(16), one], (1, 17, 16, 1), [0, 1, 2, 4])):
        table = emu.table(sel)
        assert table["cuts"] == cuts and table["longest"] == max(sizes) and table["segments"] == sum(sizes), (sizes, table)
        assert emu.lds_doubles(table["longest"])[0] == lds_doubles(emu.lds_doubles(1)[1], table["longest"])
        got = emu.tape_measures(Q, dQ, sel)
        for t, n in enumerate(sizes):
            for f in tr.FIELDS:
                assert np.array_equal(getattr(got, f)[:, :, t], getattr(alone[n], f)[:, :, 0]), (sizes, t, f)
    # a walk there and back is twice the segment, sixteen or seventeen times over
    assert np.allclose(alone[16].length, 16 * emu.tape_measures(Q, dQ, [[3, 0]]).length, rtol=1e-14)
    assert np.allclose(alone[17].length, 17 * emu.tape_measures(Q, dQ, [[3, 0]]).length, rtol=1e-14)


def test_the_cached_table_and_a_rebuilt_one_give_the_same_bits():
    name = "scissor4"
    Q, dQ, _ = tr.batch_states(name, B, M)
    emu, ms = _emu(name), _ms(name)
    a = emu.tape_measures(Q, dQ, ms, reuse=True)
    assert emu.built
    again = emu.tape_measures(Q, dQ, ms, reuse=True)
    assert not emu.built                                                 # the cached table
    other = emu.tape_measures(Q, dQ, ms[:2], reuse=True)
    assert emu.built
    regrouped = emu.tape_measures(Q, dQ, [ms[0] + ms[1]], reuse=True)    # the same frames, other measure boundaries: not the same selection
    assert emu.built
    back = emu.tape_measures(Q, dQ, ms, reuse=True)
    assert emu.built
    fresh = emu.tape_measures(Q, dQ, ms, reuse=False)
    _same(a, again)
    _same(a, back)
    _same(a, fresh)
    for f in tr.FIELDS:
        assert np.array_equal(getattr(other, f), getattr(a, f)[:, :, :2]), f
    assert regrouped.length.shape == (B, M, 1)


# ---- 6. the C entry points without a device -------------------------------------------------------------------------------------------
LDS_CELLS = [(n, t, longest) for n in ("pend_on_cart", "scissor4", "mixed_loop", "puppet40") for t in (1, 4, 16, 64) for longest in (1, 16, 17, 40)]


def lds_doubles(rollout, longest):
    """Per team: the rollout slice and 14 doubles for each of max(16, longest) staged segments."""
    even = lambda x: (x + 1) & ~1
    return even(even(rollout) + 14 * max(16, longest))


@pytest.mark.parametrize("name,team,longest", LDS_CELLS)
def test_lds_of_a_workgroup_and_its_refusal(monkeypatch, name, team, longest):
    monkeypatch.setenv("TREPAMD_TEAM", str(team))
    L = _lib.lib()
    d = tr.system_of(name)[1]
    slice_, rollout = _emu(name).lds_doubles(longest)
    assert rollout == emu_harness.lds_slices(d)["rollout"]
    assert slice_ == lds_doubles(rollout, longest)
    sys_h = L.tg_system_create(d.byref())
    assert sys_h
    try:
        out = np.zeros(4, dtype=np.int32)
        rc = L.tg_system_tape_measures_lds(sys_h, longest, out.ctypes.data_as(_lib._c_ip))
        bytes_ = (64 // team) * slice_ * 8
        assert list(out) == [team, slice_, bytes_, 0]
        if bytes_ > 160 * 1024:
            assert rc == ERR_UNSUPPORTED and L.tg_last_error() == b"system or measure too large for the LDS-resident tape-measure kernel"
        else:
            assert rc == 0
    finally:
        L.tg_system_destroy(sys_h)


def test_both_sides_of_the_lds_limit_are_in_the_cells(monkeypatch):
    L = _lib.lib()
    seen = set()
    for name, team, longest in LDS_CELLS:
        monkeypatch.setenv("TREPAMD_TEAM", str(team))
        sys_h = L.tg_system_create(tr.system_of(name)[1].byref())
        out = np.zeros(4, dtype=np.int32)
        seen.add(L.tg_system_tape_measures_lds(sys_h, longest, out.ctypes.data_as(_lib._c_ip)))
        L.tg_system_destroy(sys_h)
    assert seen == {0, ERR_UNSUPPORTED}


def test_a_long_measure_alone_is_refused_without_a_device(monkeypatch):
    """The scratch grows with the longest measure only: a small system fits with 17 segments and not with 2000 at four lanes per team."""
    monkeypatch.setenv("TREPAMD_TEAM", "4")
    L = _lib.lib()
    sys_h = L.tg_system_create(tr.system_of("pend_on_cart")[1].byref())
    out = np.zeros(4, dtype=np.int32)
    try:
        assert L.tg_system_tape_measures_lds(sys_h, 17, out.ctypes.data_as(_lib._c_ip)) == 0
        assert L.tg_system_tape_measures_lds(sys_h, 2000, out.ctypes.data_as(_lib._c_ip)) == ERR_UNSUPPORTED
        assert L.tg_system_tape_measures_lds(sys_h, 0, out.ctypes.data_as(_lib._c_ip)) == ERR_INVALID
    finally:
        L.tg_system_destroy(sys_h)


def test_null_handles_are_refused():
    L = _lib.lib()
    q = np.zeros(8)
    start, sel = np.array([0, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    assert L.tg_batch_tape_measures(None, 1, q.ctypes.data, None, 1, start.ctypes.data, sel.ctypes.data, q.ctypes.data, None, None, None, None) == ERR_INVALID
    assert L.tg_last_error() == b"null argument"
    assert L.tg_batch_tape_measures_device(None, 1, q.ctypes.data, 8, None, 8, 1, start.ctypes.data, sel.ctypes.data, q.ctypes.data, None, None, None, None) == ERR_INVALID
    assert L.tg_last_error() == b"null argument"
    assert L.tg_system_tape_measures_lds(None, 1, None) == ERR_INVALID and L.tg_last_error() == b"null argument"


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_every_refusal_is_decided_without_a_device(device):
    """Each refusal of the entry points returns TG_ERR_INVALID with no device present.  What the arguments alone show is refused with
    its own message whatever the handle; a frame index outside the system and a short row stride need the system, and a handle
    without one (no batch exists without a device) is refused as a null argument there: test_gpu_tape_measures.py sees those two
    with their own messages."""
    L = _lib.lib()
    batch = ctypes.create_string_buffer(1 << 20)          # a handle with no system behind it
    q = np.zeros(64)
    start, sel = np.array([0, 2, 5], dtype=np.int32), np.array([0, 1, 1, 2, 1], dtype=np.int32)
    short, twice = np.array([0, 2, 3], dtype=np.int32), np.array([0, 1, 1, 1, 2], dtype=np.int32)
    b, p, s, f = ctypes.addressof(batch), q.ctypes.data, start.ctypes.data, sel.ctypes.data

    def call(n_states, Q, dQ, n_measures, start_, frames, L_, V, LQ, VQ, LQQ, stride=8):
        if device:
            return L.tg_batch_tape_measures_device(b, n_states, Q, stride, dQ, stride, n_measures, start_, frames, L_, V, LQ, VQ, LQQ)
        return L.tg_batch_tape_measures(b, n_states, Q, dQ, n_measures, start_, frames, L_, V, LQ, VQ, LQQ)
    for args, message in (
            ((0, p, p, 2, s, f, p, p, p, p, p), b"n_states must be at least 1"),
            ((-2, p, p, 2, s, f, p, p, p, p, p), b"n_states must be at least 1"),
            ((1, None, p, 2, s, f, p, p, p, p, p), b"null Q"),
            ((1, p, p, 0, s, f, p, p, p, p, p), b"no measures selected"),
            ((1, p, p, 2, None, f, p, p, p, p, p), b"no measures selected"),
            ((1, p, p, 2, s, None, p, p, p, p, p), b"no measures selected"),
            ((1, p, p, 2, short.ctypes.data, f, p, p, p, p, p), b"a measure needs at least two frames"),
            ((1, p, p, 2, s, twice.ctypes.data, p, p, p, p, p), b"two equal consecutive frames in a measure"),
            ((1, p, None, 2, s, f, p, p, p, None, p), b"V or VQ without dQ"),
            ((1, p, None, 2, s, f, p, None, p, p, p), b"V or VQ without dQ"),
            ((1, p, p, 2, s, f, None, None, None, None, None), b"no output asked for"),
            ((1, p, None, 2, s, f, None, None, None, None, None), b"no output asked for")):
        assert call(*args) == ERR_INVALID
        assert L.tg_last_error() == message
    sel[:] = (0, 1 << 20, 1, 2, 1)                         # a frame outside any system, a stride under any nq
    assert call(1, p, p, 2, s, f, p, p, p, p, p) == ERR_INVALID
    sel[:] = (0, 1, 1, 2, 1)
    assert call(1, p, p, 2, s, f, p, p, p, p, p, stride=0) == ERR_INVALID


def test_the_new_entry_points_are_exported_and_declared():
    names = set(_lib.exported_symbols())
    assert {"tg_batch_tape_measures", "tg_batch_tape_measures_device", "tg_system_tape_measures_lds"} <= names
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "trep_amd.h")).read()
    L = _lib.lib()
    for n in _lib._TAPE_SIGNATURES:
        assert "int %s(" % n in header
        assert getattr(L, n)


def test_the_emulator_build_is_ignored_by_git():
    """Like the other emulators' builds: the on-demand .so falls under the `*.so` rule of .gitignore, and no rule takes it out again."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    emu_tape_harness.lib()
    assert os.path.exists(os.path.join(root, "tests", "emu_tape", "libtrepamd_emu_tape.so"))
    rules = [line.strip() for line in open(os.path.join(root, ".gitignore")) if line.strip() and not line.startswith("#")]
    assert "*.so" in rules and not [r for r in rules if r.startswith("!")]


def test_the_host_class_points_to_the_batched_call():
    import trep_amd
    doc = trep_amd.tapemeasure.__doc__
    assert "Nothing here runs on the device" not in doc and "BatchMidpointVI.tape_measures" in doc
