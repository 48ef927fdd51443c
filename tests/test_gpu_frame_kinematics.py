"""Batched frame kinematics on the device (BatchMidpointVI.frame_kinematics, k_frames): the case table of
frame_kinematics_reference.py at every system's own team size and at every team size of common.TEAM_CELLS, into NaN-poisoned
outputs, against the host accessors with the bounds of tests/test_frames.py; the recorded frames of the reference project; equal
bits for a state repeated in a launch, alone in a launch, through the host and the device entry points, across a rebuilt frame
table and whatever else is asked for; the device variant reading a rollout's X; the optional outputs; the untouched integrator
state under a parameter table and a specialised library; the refusals."""
import numpy as np
import pytest

import common
import frame_kinematics_reference as fr
from trep_amd import BatchMidpointVI, _lib

pytestmark = pytest.mark.gpu

FRAMES_BIT = 12
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
M = 3
TEAM_RUNS = [(n, t) for n in fr.SYSTEMS if n in common.TEAM_CELLS for t in sorted(common.TEAM_CELLS[n])]


def _batch(monkeypatch, name, B, team=None, specialize=False):
    if team is None:
        monkeypatch.delenv("TREPAMD_TEAM", raising=False)
    else:
        monkeypatch.setenv("TREPAMD_TEAM", str(team))
    mvi = BatchMidpointVI(fr.system_of(name)[0], B, specialize=specialize)
    if team is not None:
        assert mvi.kernel_info()["team"] == team
    return mvi


def _geometry(mvi):
    """(team size, does a workgroup of the kernel fit the LDS) of this batch (tg_system_frame_kinematics_lds)."""
    out = np.zeros(4, dtype=np.int32)
    rc = _lib.lib().tg_system_frame_kinematics_lds(mvi._sys_h, out.ctypes.data_as(_lib._c_ip))
    assert rc in (0, ERR_UNSUPPORTED) and out[0] == mvi.kernel_info()["team"]
    assert (rc == 0) == (int(out[2]) <= 160 * 1024)
    return int(out[0]), rc == 0


def _ragged_batch(team):
    """B with B * M teams = one full block of teams and a ragged one (at one team per block: several blocks)."""
    return (64 // team) // M + 2


def _device_call(mvi, Q, dQ=None, frames=None, jacobians=True, want_g=True, Q_dev=None, stride=None):
    """frame_kinematics_device into NaN-filled device arrays, downloaded: what the kernel leaves unwritten shows."""
    B, Mm, nq = Q.shape[0], Q.shape[1], mvi.nq
    F = len(mvi.system.frames) if frames is None else len(frames)
    shapes = {"g": (B, Mm, F, 3, 4) if want_g else None, "vb": None if dQ is None else (B, Mm, F, 6),
              "p_dq": (B, Mm, F, nq, 3) if jacobians else None, "vb_ddq": (B, Mm, F, nq, 6) if jacobians else None}
    dev = {k: None if s is None else mvi.device_array(np.full(s, np.nan)) for k, s in shapes.items()}
    mvi.frame_kinematics_device(Mm, mvi.device_array(Q) if Q_dev is None else Q_dev, stride, None if dQ is None else mvi.device_array(dQ), None,
                                frames, dev["g"], dev["vb"], dev["p_dq"], dev["vb_ddq"])
    mvi.synchronize()
    return fr.Arrays(*[None if shapes[k] is None else mvi.download(dev[k], shapes[k]) for k in fr.FIELDS])


def _same(a, b, fields=fr.FIELDS):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f
        if x is not None:
            assert np.array_equal(x, y), f


def _take(r, at):
    return fr.Arrays(*[None if getattr(r, f) is None else getattr(r, f)[at] for f in fr.FIELDS])


# ---- 1. the table on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fr.SYSTEMS)
def test_the_table_at_the_systems_own_team(monkeypatch, name):
    team, fits = _geometry(_batch(monkeypatch, name, 1))
    assert fits
    B = _ragged_batch(team)
    Q, dQ, at = fr.batch_states(name, B, M)
    mvi = _batch(monkeypatch, name, B)
    got = _device_call(mvi, Q, dQ)
    fr.compare(got, fr.expected(name, at), tag="%s team %d " % (name, team))
    off = fr.off_path(mvi.system)
    for a in (got.p_dq, got.vb_ddq):
        assert not a[:, :, off].any()
    info = mvi.kernel_info()
    assert info["generic_launch_mask"] == 1 << FRAMES_BIT and info["generic_launches"] == 1
    assert info["spec_launch_mask"] == 0 and info["spec_launches"] == 0 and info["par_generic_launches"] == 0 and info["par_spec_launches"] == 0


# ---- 2. every team size -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,team", TEAM_RUNS, ids=["%s_team%d" % c for c in TEAM_RUNS])
def test_every_team_size(monkeypatch, name, team):
    B = _ragged_batch(team)
    Q, dQ, at = fr.batch_states(name, B, M)
    mvi = _batch(monkeypatch, name, B, team)
    if not _geometry(mvi)[1]:
        with pytest.raises(_lib.LibraryError, match="system too large for the LDS-resident frame-kinematics kernel"):
            mvi.frame_kinematics(Q, dQ, jacobians=True)
        assert mvi.kernel_info()["generic_launches"] == 0
        return
    fr.compare(_device_call(mvi, Q, dQ), fr.expected(name, at), tag="%s team %d " % (name, team))


def test_both_sides_of_the_lds_limit_are_run(monkeypatch):
    seen = set()
    for name, team in TEAM_RUNS:
        seen.add(_geometry(_batch(monkeypatch, name, 1, team))[1])
    assert seen == {True, False}


# ---- 3. the reference project's recorded frames ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fr.GOLDEN_SYSTEMS)
def test_recorded_frames_on_the_device(monkeypatch, name):
    g = common.golden("frames")
    monkeypatch.delenv("TREPAMD_TEAM", raising=False)
    mvi = BatchMidpointVI(common.build(name)[0], 1, specialize=False)
    got = mvi.frame_kinematics(g[name + "_q"][None], g[name + "_dq"][None])
    want_g, want_vb = g[name + "_g"][:, :3], np.array([fr.vec6(m) for m in g[name + "_vb"]])
    assert got.g.shape == (1,) + want_g.shape and got.vb.shape == (1,) + want_vb.shape and got.p_dq is None and got.vb_ddq is None
    err_g, err_vb = float(np.abs(got.g[0] - want_g).max()), float(np.abs(got.vb[0] - want_vb).max())
    print(name, "g %.3e vb %.3e" % (err_g, err_vb))
    assert err_g <= 1e-12 * max(1.0, np.abs(want_g).max()) and err_vb <= 1e-12 * max(1.0, np.abs(want_vb).max())


# ---- 4. equal bits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("scissor4", "puppet40"))
def test_a_state_does_not_depend_on_its_launch(monkeypatch, name):
    """A state repeated within a launch, and the same state alone in a B = 1 launch: the same bits."""
    q, dq = fr.states(name)
    at = np.array([[1, 0, 1], [2, 1, 1], [1, 3, 0], [0, 1, 2], [1, 1, 1]])
    whole = _device_call(_batch(monkeypatch, name, len(at)), q[at], dq[at])
    first = _take(whole, (0, 0))
    for b, m in zip(*np.nonzero(at == 1)):
        _same(_take(whole, (b, m)), first)
    assert (at == 1).sum() == 9
    alone = _device_call(_batch(monkeypatch, name, 1), q[None, 1:2], dq[None, 1:2])
    _same(_take(alone, (0, 0)), first)


def test_host_and_device_variants_give_the_same_bits(monkeypatch):
    name = "mixed_loop"
    Q, dQ, at = fr.batch_states(name, 7, M)
    host = _batch(monkeypatch, name, 7).frame_kinematics(Q, dQ, jacobians=True)
    fr.compare(host, fr.expected(name, at), tag="host entry point ")
    mvi = _batch(monkeypatch, name, 7)
    stream = _lib.lib().tg_dopt_lane_stream(0, 1)
    assert stream
    mvi.set_stream(stream)
    try:
        _same(host, _device_call(mvi, Q, dQ))
    finally:
        mvi.close()


def test_the_cached_frame_table_is_rebuilt_for_another_selection(monkeypatch):
    name = "puppet40"
    Q, dQ, at = fr.batch_states(name, 3, 2)
    n = len(fr.system_of(name)[0].frames)
    first, other = [n - 1, 5, 40, 5, 17, 0, 73, 22, 61, 9], [3, 12]        # two passes with a repeat; a shorter table in between
    mvi = _batch(monkeypatch, name, 3)
    a = _device_call(mvi, Q, dQ, first)
    again = _device_call(mvi, Q, dQ, first)                              # the cached table
    b = _device_call(mvi, Q, dQ, other)
    c = _device_call(mvi, Q, dQ, first)                                  # rebuilt
    d = _device_call(mvi, Q, dQ, list(range(n)))                         # grown
    _same(a, again)
    _same(a, c)
    fr.compare(a, fr.expected(name, at, first), tag="first selection ")
    fr.compare(b, fr.expected(name, at, other), tag="selection in between ")
    for f in fr.FIELDS:
        assert np.array_equal(getattr(a, f), getattr(d, f)[:, :, first]), f
        assert np.array_equal(getattr(a, f)[:, :, 1], getattr(a, f)[:, :, 3]), f      # the repeated frame
    assert mvi.kernel_info()["generic_launches"] == 5


def test_g_alone_and_with_the_other_outputs(monkeypatch):
    name = "spatial_loop"
    Q, dQ, at = fr.batch_states(name, 6, M)
    mvi = _batch(monkeypatch, name, 6)
    everything = _device_call(mvi, Q, dQ)
    alone = _device_call(mvi, Q, None, jacobians=False)
    assert alone.vb is None and alone.p_dq is None and alone.vb_ddq is None
    assert np.array_equal(alone.g, everything.g)
    rates = _device_call(mvi, Q, dQ, jacobians=False, want_g=False)
    assert rates.g is None and np.array_equal(rates.vb, everything.vb)


# ---- 5. straight from a rollout ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("pend_on_cart", "puppet40"))
def test_device_variant_reads_a_rollouts_states(monkeypatch, name):
    N, dt = 5, 0.01
    system, d = fr.system_of(name)
    B = 3
    rng = np.random.default_rng(common.tb_seed("frames from a rollout", name))
    Q0, Q1, U, K = common.starts(name, d, B, N, rng)
    mvi = _batch(monkeypatch, name, B)
    mvi.initialize_from_configs(0.0, Q0, dt, Q1)
    nX, nq = mvi.nX, mvi.nq
    X_dev = mvi.device_empty(B * (N + 1) * nX)
    mvi.rollout_device(N, dt, mvi.device_array(U) if mvi.nu else None, mvi.device_array(K) if mvi.nk else None, X_dev)
    mvi.synchronize()
    assert (mvi.status()[1] == 0).all()
    X = mvi.download(X_dev, (B, N + 1, nX))
    frames = [len(system.frames) - 1, 0, 2]
    strided = _device_call(mvi, X, None, frames, Q_dev=X_dev, stride=nX)
    packed = mvi.frame_kinematics(np.ascontiguousarray(X[:, :, :nq]), frames=frames, jacobians=True)
    _same(packed, strided)
    system.q = X[1, N, :nq]
    want = np.asarray(system.frames[frames[0]].g())[:3]
    assert np.abs(strided.g[1, N, 0] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


# ---- 6. the optional outputs -------------------------------------------------------------------------------------------------------
def test_without_rates_and_without_jacobians(monkeypatch):
    name = "scissor4"
    Q, dQ, at = fr.batch_states(name, 4, M)
    want = fr.expected(name, at)
    mvi = _batch(monkeypatch, name, 4)
    r = mvi.frame_kinematics(Q)
    assert r.vb is None and r.p_dq is None and r.vb_ddq is None
    fr.compare(r, want, fields=("g",))
    r = mvi.frame_kinematics(Q, jacobians=True)
    assert r.vb is None
    fr.compare(r, want, fields=("g", "p_dq", "vb_ddq"))
    r = mvi.frame_kinematics(Q, dQ, jacobians=False)
    assert r.p_dq is None and r.vb_ddq is None
    fr.compare(r, want, fields=("g", "vb"))
    flat = mvi.frame_kinematics(Q[:, 0], dQ[:, 0], frames=["World", mvi.system.frames[3], 2], jacobians=True)      # [B][nq]: no M axis
    assert flat.g.shape == (4, 3, 3, 4) and flat.vb.shape == (4, 3, 6) and flat.p_dq.shape == (4, 3, mvi.nq, 3) and flat.vb_ddq.shape == (4, 3, mvi.nq, 6)
    fr.compare(flat, fr.Arrays(*[getattr(want, f)[:, 0][:, [0, 3, 2]] for f in fr.FIELDS]), tag="frames by name, object and index ")
    assert mvi.kernel_info()["generic_launches"] == 4


# ---- 7. the state of the batch, parameters, a specialised library --------------------------------------------------------------------
def test_the_batch_state_is_unchanged_and_neither_parameters_nor_a_library_have_a_say(monkeypatch):
    name = "puppet40"
    B, N, dt = 3, 4, 0.01
    system, d = fr.system_of(name)
    Q, dQ, at = fr.batch_states(name, B, 2)
    frames = [85, 30, 0, 61]
    plain = _batch(monkeypatch, name, B).frame_kinematics(Q, dQ, frames=frames, jacobians=True)
    rng = np.random.default_rng(common.tb_seed("frames state", name))
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
    _same(plain, mvi.frame_kinematics(Q, dQ, frames=frames, jacobians=True))
    gravity = np.tile(np.array([[0.3, -0.2, -4.0]]), (B, 1))
    mvi.set_parameters(gravity=gravity, group=1)
    _same(plain, mvi.frame_kinematics(Q, dQ, frames=frames, jacobians=True))
    mvi.clear_parameters()
    info = mvi.kernel_info()
    assert (info["generic_launch_mask"] >> FRAMES_BIT) & 1 and not (info["spec_launch_mask"] >> FRAMES_BIT) & 1
    assert info["par_generic_launches"] == 0 and info["par_spec_launches"] == 0
    for a, b_ in zip(before, state()):
        assert np.array_equal(a, b_)
    assert np.array_equal(mvi.rollout(N, dt, U, K), X_ref)
    assert (mvi.status()[1] == 0).all()


# ---- 8. the refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_make_no_launch(monkeypatch):
    L = _lib.lib()
    mvi = _batch(monkeypatch, "mixed_loop", 2)
    nq, nfr = mvi.nq, len(mvi.system.frames)
    Q = np.zeros((2, 3, nq))
    out = np.zeros(2 * 3 * 2 * nq * 6)
    sel = np.array([1, nfr - 1], dtype=np.int32)
    q, o, f = Q.ctypes.data, out.ctypes.data, sel.ctypes.data

    def host(n_states, Qp, dQp, n_frames, frames, G, VB, JP, JB):
        return L.tg_batch_frame_kinematics(mvi._h, n_states, Qp, dQp, n_frames, frames, G, VB, JP, JB)

    def device(n_states, Qp, dQp, n_frames, frames, G, VB, JP, JB, stride=nq, dq_stride=nq):
        return L.tg_batch_frame_kinematics_device(mvi._h, n_states, Qp, stride, dQp, dq_stride, n_frames, frames, G, VB, JP, JB)
    for call in (host, device):                    # (decided before a pointer is followed: the device variant gets host addresses)
        for args, message in (
                ((0, q, q, 2, f, o, o, o, o), b"n_states must be at least 1"),
                ((3, None, q, 2, f, o, o, o, o), b"null Q"),
                ((3, q, q, 0, f, o, o, o, o), b"no frames selected"),
                ((3, q, q, 2, None, o, o, o, o), b"no frames selected"),
                ((3, q, None, 2, f, o, o, o, o), b"VB without dQ"),
                ((3, q, q, 2, f, None, None, None, None), b"no output asked for")):
            assert call(*args) == ERR_INVALID and L.tg_last_error() == message
        for bad in (nfr, -1):
            sel[1] = bad
            assert call(3, q, q, 2, f, o, o, o, o) == ERR_INVALID and L.tg_last_error() == b"frame index outside the system"
        sel[1] = nfr - 1
    assert device(3, q, q, 2, f, o, o, o, o, stride=nq - 1) == ERR_INVALID and L.tg_last_error() == b"row stride of Q shorter than a configuration"
    assert device(3, q, q, 2, f, o, o, o, o, dq_stride=nq - 1) == ERR_INVALID and L.tg_last_error() == b"row stride of dQ shorter than a configuration"
    with pytest.raises(ValueError):
        mvi.frame_kinematics(Q, frames=[nfr])
    with pytest.raises(ValueError):
        mvi.frame_kinematics(Q, frames=[])
    with pytest.raises(ValueError):
        mvi.frame_kinematics(Q[:1])
    with pytest.raises(ValueError):
        mvi.frame_kinematics_device(3, q, g_dev=None)
    assert mvi.kernel_info()["generic_launches"] == 0
