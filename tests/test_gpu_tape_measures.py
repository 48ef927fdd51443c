"""Batched tape measures on the device (BatchMidpointVI.tape_measures, k_tape): the case table of tape_measure_reference.py at every
system's own team size and at every team size of common.TEAM_CELLS, into NaN-poisoned outputs, against the host TapeMeasure accessors
with the bounds of that module; exact zeros where the specification has them; the recorded tape of the reference project; equal bits
for a state repeated in a launch, alone in a launch, through the host and the device entry points, across a re-used, replaced and
grown selection and whatever else is asked for; the device variant reading a rollout's X; the untouched integrator state under a
parameter table and a specialised library; the refusals."""
import numpy as np
import pytest

import common
import tape_measure_reference as tr
from trep_amd import BatchMidpointVI, TapeMeasure, _lib

pytestmark = pytest.mark.gpu

TAPE_BIT = 13
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
M = 3
TEAM_RUNS = [(n, t) for n in tr.SYSTEMS if n in common.TEAM_CELLS for t in sorted(common.TEAM_CELLS[n])]
TOO_LARGE = "system or measure too large for the LDS-resident tape-measure kernel"


def _ms(name, sel=None):
    ms = [list(m) for m in tr.measures(name)]
    return ms if sel is None else [ms[t] for t in sel]


def _longest(measures):
    return max(len(m) - 1 for m in measures)


def _batch(monkeypatch, name, B, team=None, specialize=False):
    if team is None:
        monkeypatch.delenv("TREPAMD_TEAM", raising=False)
    else:
        monkeypatch.setenv("TREPAMD_TEAM", str(team))
    mvi = BatchMidpointVI(tr.system_of(name)[0], B, specialize=specialize)
    if team is not None:
        assert mvi.kernel_info()["team"] == team
    return mvi


def _geometry(mvi, longest):
    """(team size, does a workgroup of the kernel fit the LDS) of this batch (tg_system_tape_measures_lds)."""
    out = np.zeros(4, dtype=np.int32)
    rc = _lib.lib().tg_system_tape_measures_lds(mvi._sys_h, longest, out.ctypes.data_as(_lib._c_ip))
    assert rc in (0, ERR_UNSUPPORTED) and out[0] == mvi.kernel_info()["team"]
    assert (rc == 0) == (int(out[2]) <= 160 * 1024)
    return int(out[0]), rc == 0


def _ragged_batch(team):
    """B with B * M teams = one full block of teams and a ragged one (at one team per block: several blocks)."""
    return (64 // team) // M + 2


def _device_call(mvi, Q, dQ, measures, fields=tr.FIELDS, Q_dev=None, stride=None):
    """tape_measures_device into NaN-filled device arrays, downloaded: what the kernel leaves unwritten shows."""
    B, Mm, nq, T = Q.shape[0], Q.shape[1], mvi.nq, len(measures)
    shapes = {"length": (B, Mm, T), "velocity": (B, Mm, T), "length_dq": (B, Mm, T, nq), "velocity_dq": (B, Mm, T, nq), "length_dqdq": (B, Mm, T, nq, nq)}
    shapes = {f: s if f in fields and (dQ is not None or not f.startswith("velocity")) else None for f, s in shapes.items()}
    dev = {f: None if s is None else mvi.device_array(np.full(s, np.nan)) for f, s in shapes.items()}
    mvi.tape_measures_device(Mm, mvi.device_array(Q) if Q_dev is None else Q_dev, stride, None if dQ is None else mvi.device_array(dQ), None,
                             measures, dev["length"], dev["velocity"], dev["length_dq"], dev["velocity_dq"], dev["length_dqdq"])
    mvi.synchronize()
    return tr.Arrays(*[None if shapes[f] is None else mvi.download(dev[f], shapes[f]) for f in tr.FIELDS])


def _same(a, b, fields=tr.FIELDS):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f
        if x is not None:
            assert np.array_equal(x, y), f


def _take(r, at):
    return tr.Arrays(*[None if getattr(r, f) is None else getattr(r, f)[at] for f in tr.FIELDS])


def _assert_exact_zeros(name, got, measures=None):
    zq, zqq = tr.structural_zeros(tr.system_of(name)[0], tr.measures(name) if measures is None else measures)
    assert zq.any() and not zq.all()
    assert not got.length_dq[:, :, zq].any() and not got.velocity_dq[:, :, zq].any() and not got.length_dqdq[:, :, zqq].any()


# ---- 1. the table on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tr.SYSTEMS)
def test_the_table_at_the_systems_own_team(monkeypatch, name):
    ms = _ms(name)
    team, fits = _geometry(_batch(monkeypatch, name, 1), _longest(ms))
    assert fits
    B = _ragged_batch(team)
    Q, dQ, at = tr.batch_states(name, B, M)
    mvi = _batch(monkeypatch, name, B)
    got = _device_call(mvi, Q, dQ, ms)
    tr.compare(name, got, tr.expected(name, at), tag="%s team %d " % (name, team))
    _assert_exact_zeros(name, got)
    info = mvi.kernel_info()
    assert info["generic_launch_mask"] == 1 << TAPE_BIT and info["generic_launches"] == 1
    assert info["spec_launch_mask"] == 0 and info["spec_launches"] == 0 and info["par_generic_launches"] == 0 and info["par_spec_launches"] == 0


# ---- 2. every team size -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,team", TEAM_RUNS, ids=["%s_team%d" % c for c in TEAM_RUNS])
def test_every_team_size(monkeypatch, name, team):
    ms = _ms(name)
    B = _ragged_batch(team)
    Q, dQ, at = tr.batch_states(name, B, M)
    mvi = _batch(monkeypatch, name, B, team)
    if not _geometry(mvi, _longest(ms))[1]:
        with pytest.raises(_lib.LibraryError, match=TOO_LARGE):
            mvi.tape_measures(Q, dQ, ms, gradients=True, hessians=True)
        assert mvi.kernel_info()["generic_launches"] == 0
        return
    got = _device_call(mvi, Q, dQ, ms)
    tr.compare(name, got, tr.expected(name, at), tag="%s team %d " % (name, team))
    _assert_exact_zeros(name, got)


def test_both_sides_of_the_lds_limit_are_run(monkeypatch):
    seen = set()
    for name, team in TEAM_RUNS:
        seen.add(_geometry(_batch(monkeypatch, name, 1, team), _longest(_ms(name)))[1])
    assert seen == {True, False}


# ---- 3. the reference project's recorded tape ---------------------------------------------------------------------------------------
def test_recorded_tape_on_the_device(monkeypatch):
    g = common.golden("elements")
    monkeypatch.delenv("TREPAMD_TEAM", raising=False)
    system = common.build("extensor_tendon")[0]
    mvi = BatchMidpointVI(system, 1, specialize=False)
    tape = TapeMeasure(system, [str(n) for n in g["tape_frames"]])
    got = mvi.tape_measures(g["tape_q"][None], g["tape_dq"][None], [tape], gradients=True, hessians=True)
    for field, recorded, tol in (("length", "length", 1e-12), ("velocity", "velocity", 1e-12), ("length_dq", "length_dq", 1e-11),
                                 ("length_dq", "velocity_ddq", 1e-11), ("velocity_dq", "velocity_dq", 1e-11),
                                 ("length_dqdq", "length_dqdq", 1e-11), ("length_dqdq", "velocity_ddqdq", 1e-11)):
        want, have = g["tape_" + recorded], getattr(got, field)[0, 0]
        assert have.shape == want.shape, recorded
        err = float(np.abs(have - want).max())
        print(recorded, "%.3e" % err)
        assert err <= tol * max(1.0, float(np.abs(want).max())), recorded


# ---- 4. equal bits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("scissor4", "puppet40"))
def test_a_state_does_not_depend_on_its_launch(monkeypatch, name):
    """A state repeated within a launch, and the same state alone in a B = 1 launch: the same bits."""
    q, dq = tr.states(name)
    ms = _ms(name)
    at = np.array([[1, 0, 1], [2, 1, 1], [1, 2, 0], [0, 1, 2], [1, 1, 1]])
    whole = _device_call(_batch(monkeypatch, name, len(at)), q[at], dq[at], ms)
    first = _take(whole, (0, 0))
    for b, m in zip(*np.nonzero(at == 1)):
        _same(_take(whole, (b, m)), first)
    assert (at == 1).sum() == 9
    alone = _device_call(_batch(monkeypatch, name, 1), q[None, 1:2], dq[None, 1:2], ms)
    _same(_take(alone, (0, 0)), first)


def test_host_and_device_variants_give_the_same_bits(monkeypatch):
    name = "mixed_loop"
    ms = _ms(name)
    Q, dQ, at = tr.batch_states(name, 7, M)
    host = _batch(monkeypatch, name, 7).tape_measures(Q, dQ, ms, gradients=True, hessians=True)
    tr.compare(name, host, tr.expected(name, at), tag="host entry point ")
    mvi = _batch(monkeypatch, name, 7)
    stream = _lib.lib().tg_dopt_lane_stream(0, 1)
    assert stream
    mvi.set_stream(stream)
    try:
        _same(host, _device_call(mvi, Q, dQ, ms))
    finally:
        mvi.close()


def test_a_selection_reused_replaced_and_grown(monkeypatch):
    name = "scissor4"                                                   # its 17-segment measure: two passes and a wider scratch
    Q, dQ, at = tr.batch_states(name, 3, 2)
    first, other = [3, 0, 1, 3], [0]
    everything = [0, 1, 2, 3, 4, 2]
    mvi = _batch(monkeypatch, name, 3)
    a = _device_call(mvi, Q, dQ, _ms(name, first))
    again = _device_call(mvi, Q, dQ, _ms(name, first))                  # the cached table
    b = _device_call(mvi, Q, dQ, _ms(name, other))
    c = _device_call(mvi, Q, dQ, _ms(name, first))                      # rebuilt
    d = _device_call(mvi, Q, dQ, _ms(name, everything))                 # grown
    _same(a, again)
    _same(a, c)
    tr.compare(name, a, tr.expected(name, at, first), tag="first selection ")
    tr.compare(name, b, tr.expected(name, at, other), tag="selection in between ")
    tr.compare(name, d, tr.expected(name, at, everything), tag="grown selection ")
    for f in tr.FIELDS:
        assert np.array_equal(getattr(a, f), getattr(d, f)[:, :, first]), f
        assert np.array_equal(getattr(a, f)[:, :, 0], getattr(a, f)[:, :, 3]), f      # the repeated measure
        assert np.array_equal(getattr(d, f)[:, :, 2], getattr(d, f)[:, :, 5]), f      # the long one, in two different passes
    assert mvi.kernel_info()["generic_launches"] == 5


def test_each_output_alone_and_all_together(monkeypatch):
    name = "spatial_loop"
    ms = _ms(name)
    Q, dQ, at = tr.batch_states(name, 6, M)
    mvi = _batch(monkeypatch, name, 6)
    everything = _device_call(mvi, Q, dQ, ms)
    for f in tr.FIELDS:
        alone = _device_call(mvi, Q, dQ, ms, fields=(f,))
        assert [g for g in tr.FIELDS if getattr(alone, g) is not None] == [f]
        assert np.array_equal(getattr(alone, f), getattr(everything, f)), f
    norates = _device_call(mvi, Q, None, ms)
    assert norates.velocity is None and norates.velocity_dq is None
    _same(norates, everything, fields=("length", "length_dq", "length_dqdq"))
    r = mvi.tape_measures(Q, measures=ms)
    assert r.velocity is None and r.length_dq is None and r.velocity_dq is None and r.length_dqdq is None and np.array_equal(r.length, everything.length)
    r = mvi.tape_measures(Q, dQ, ms, gradients=True)
    assert r.length_dqdq is None
    _same(r, everything, fields=("length", "velocity", "length_dq", "velocity_dq"))
    system = mvi.system
    by_name = [TapeMeasure(system, [system.frames[f] for f in ms[0]]), ["World", system.frames[11], 2]]      # measures 0 and 3 of the table
    flat = mvi.tape_measures(Q[:, 0], dQ[:, 0], by_name, hessians=True)                                       # [B][nq]: no M axis
    assert flat.length.shape == (6, 2) and flat.velocity.shape == (6, 2) and flat.length_dq is None and flat.length_dqdq.shape == (6, 2, mvi.nq, mvi.nq)
    assert list(ms[3]) == [0, 11, 2]
    for f in ("length", "velocity", "length_dqdq"):
        assert np.array_equal(getattr(flat, f), getattr(everything, f)[:, 0][:, [0, 3]]), f


# ---- 5. straight from a rollout ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("pend_on_cart", "puppet40"))
def test_device_variant_reads_a_rollouts_states(monkeypatch, name):
    N, dt = 5, 0.01
    system, d = tr.system_of(name)
    B = 3
    rng = np.random.default_rng(common.tb_seed("tape measures from a rollout", name))
    Q0, Q1, U, K = common.starts(name, d, B, N, rng)
    mvi = _batch(monkeypatch, name, B)
    mvi.initialize_from_configs(0.0, Q0, dt, Q1)
    nX, nq = mvi.nX, mvi.nq
    X_dev = mvi.device_empty(B * (N + 1) * nX)
    mvi.rollout_device(N, dt, mvi.device_array(U) if mvi.nu else None, mvi.device_array(K) if mvi.nk else None, X_dev)
    mvi.synchronize()
    assert (mvi.status()[1] == 0).all()
    X = mvi.download(X_dev, (B, N + 1, nX))
    ms = _ms(name)[:2] if name == "pend_on_cart" else _ms(name)         # (the pendulum's long walk is the table's business)
    rates = rng.uniform(-1.0, 1.0, (B, N + 1, nq))
    strided = _device_call(mvi, X, rates, ms, Q_dev=X_dev, stride=nX)
    packed = mvi.tape_measures(np.ascontiguousarray(X[:, :, :nq]), rates, ms, gradients=True, hessians=True)
    _same(packed, strided)
    want = tr.reference(system, X[1, N, :nq], rates[1, N], ms)
    assert tr.worst_ratio(name, _take(strided, (1, N)), want) <= 1.0
    if name == "puppet40":              # the strings' Distance constraints hold their lengths: control to hook is the length config
        lengths = X[:, :, [system.configs.index(system.get_config(s + "_string-length")) for s in
                           ("upper_torso", "lower_torso", "left_arm", "right_arm", "left_leg", "right_leg")]]
        assert np.abs(strided.length - np.abs(lengths)).max() <= 1e-8


# ---- 6. the state of the batch, parameters, a specialised library --------------------------------------------------------------------
def test_the_batch_state_is_unchanged_and_neither_parameters_nor_a_library_have_a_say(monkeypatch):
    name = "puppet40"
    B, N, dt = 3, 4, 0.01
    system, d = tr.system_of(name)
    ms = _ms(name)
    Q, dQ, at = tr.batch_states(name, B, 2)
    plain = _batch(monkeypatch, name, B).tape_measures(Q, dQ, ms, gradients=True, hessians=True)
    rng = np.random.default_rng(common.tb_seed("tape measures state", name))
    S0, S1, U, K = common.starts(name, d, B, N, rng)

    def fresh():
        mvi = _batch(monkeypatch, name, B, specialize="auto")
        mvi.initialize_from_configs(0.0, S0, dt, S1)
        return mvi

    X_ref = fresh().rollout(N, dt, U, K)
    mvi = fresh()
    assert mvi.kernel_info()["spec_modes"]                               # build() prepares this system's library
    state = lambda: [getattr(mvi, n).copy() for n in ("q1", "q2", "p1", "p2", "lambda1")] + list(mvi.status()) + [mvi.times()]
    before = state()
    _same(plain, mvi.tape_measures(Q, dQ, ms, gradients=True, hessians=True))
    gravity = np.tile(np.array([[0.3, -0.2, -4.0]]), (B, 1))
    mvi.set_parameters(gravity=gravity, group=1)
    _same(plain, mvi.tape_measures(Q, dQ, ms, gradients=True, hessians=True))
    mvi.clear_parameters()
    info = mvi.kernel_info()
    assert (info["generic_launch_mask"] >> TAPE_BIT) & 1 and not (info["spec_launch_mask"] >> TAPE_BIT) & 1
    assert info["par_generic_launches"] == 0 and info["par_spec_launches"] == 0
    for a, b_ in zip(before, state()):
        assert np.array_equal(a, b_)
    assert np.array_equal(mvi.rollout(N, dt, U, K), X_ref)
    assert (mvi.status()[1] == 0).all()


# ---- 7. the refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_make_no_launch(monkeypatch):
    L = _lib.lib()
    mvi = _batch(monkeypatch, "mixed_loop", 2)
    nq, nfr = mvi.nq, len(mvi.system.frames)
    Q = np.zeros((2, 3, nq))
    out = np.zeros(2 * 3 * 2 * nq * nq)
    start, sel = np.array([0, 2, 5], dtype=np.int32), np.array([0, 8, 4, 8, nfr - 1], dtype=np.int32)
    short, twice = np.array([0, 4, 5], dtype=np.int32), np.array([0, 8, 4, 4, 8], dtype=np.int32)
    q, o, s, f = Q.ctypes.data, out.ctypes.data, start.ctypes.data, sel.ctypes.data

    def host(n_states, Qp, dQp, n_measures, start_, frames, L_, V, LQ, VQ, LQQ):
        return L.tg_batch_tape_measures(mvi._h, n_states, Qp, dQp, n_measures, start_, frames, L_, V, LQ, VQ, LQQ)

    def device(n_states, Qp, dQp, n_measures, start_, frames, L_, V, LQ, VQ, LQQ, stride=nq, dq_stride=nq):
        return L.tg_batch_tape_measures_device(mvi._h, n_states, Qp, stride, dQp, dq_stride, n_measures, start_, frames, L_, V, LQ, VQ, LQQ)
    for call in (host, device):                    # (decided before a pointer is followed: the device variant gets host addresses)
        for args, message in (
                ((0, q, q, 2, s, f, o, o, o, o, o), b"n_states must be at least 1"),
                ((3, None, q, 2, s, f, o, o, o, o, o), b"null Q"),
                ((3, q, q, 0, s, f, o, o, o, o, o), b"no measures selected"),
                ((3, q, q, 2, None, f, o, o, o, o, o), b"no measures selected"),
                ((3, q, q, 2, s, None, o, o, o, o, o), b"no measures selected"),
                ((3, q, q, 2, short.ctypes.data, f, o, o, o, o, o), b"a measure needs at least two frames"),
                ((3, q, q, 2, s, twice.ctypes.data, o, o, o, o, o), b"two equal consecutive frames in a measure"),
                ((3, q, None, 2, s, f, o, o, o, None, o), b"V or VQ without dQ"),
                ((3, q, None, 2, s, f, o, None, o, o, o), b"V or VQ without dQ"),
                ((3, q, q, 2, s, f, None, None, None, None, None), b"no output asked for")):
            assert call(*args) == ERR_INVALID and L.tg_last_error() == message
        for bad in (nfr, -1):
            sel[4] = bad
            assert call(3, q, q, 2, s, f, o, o, o, o, o) == ERR_INVALID and L.tg_last_error() == b"frame index outside the system"
        sel[4] = nfr - 1
    assert device(3, q, q, 2, s, f, o, o, o, o, o, stride=nq - 1) == ERR_INVALID and L.tg_last_error() == b"row stride of Q shorter than a configuration"
    assert device(3, q, q, 2, s, f, o, o, o, o, o, dq_stride=nq - 1) == ERR_INVALID and L.tg_last_error() == b"row stride of dQ shorter than a configuration"
    other = TapeMeasure(tr.system_of("pend_on_cart")[0], [0, 3])
    for bad in ([[0, nfr]], [], None, [[3]], [[3, 3, 4]], [[0, "no such frame"]], ["World"], [other], [[]]):
        with pytest.raises(ValueError):
            mvi.tape_measures(Q, measures=bad)
    with pytest.raises(ValueError):
        mvi.tape_measures(Q[:1], measures=[[0, 3]])
    with pytest.raises(ValueError):
        mvi.tape_measures_device(3, q, measures=[[0, 3]])                 # no output
    with pytest.raises(ValueError):
        mvi.tape_measures_device(3, q, measures=[[0, 3]], velocity_dev=o)   # a rate without dQ
    assert mvi.kernel_info()["generic_launches"] == 0
