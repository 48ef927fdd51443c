"""BatchMidpointVI.normal_modes on the device against the numpy specification (normal_modes_reference.py): the case table at the team
size the library gives every system (1, 16 and 64) and at team 4, a ragged block, the bounds and invariants of nr.compare,
bit-equality (a pose repeated, alone, host against device entry point), the parameter twin on the puppet, constant_q_list, the
refusals and the statuses."""
import numpy as np
import pytest

import common
import normal_modes_reference as nr
from test_equilibrium_cpu import parameter_rows
from test_parameters_cpu import rebuilt
from trep_amd import BatchMidpointVI, _lib, descriptor

pytestmark = pytest.mark.gpu

MODES_BIT = 15
OWN_TEAM = {"pendulum1": 1, "pendulum5": 16, "scissor4": 64, "spring_arm": 16, "mixed_loop": 16, "spatial_loop": 16, "ladder_mixed": 64,
            "extensor_tendon": 64, "puppet40": 64}
FORCED = [(4, "pendulum5"), (4, "mixed_loop"), (64, "pendulum1")]


def _batch(monkeypatch, name, B, team=None):
    if team is None:
        monkeypatch.delenv("TREPAMD_TEAM", raising=False)
    else:
        monkeypatch.setenv("TREPAMD_TEAM", str(team))
    mvi = BatchMidpointVI(common.build(name)[0], B, specialize=False)
    if team is not None:
        assert mvi.kernel_info()["team"] == team
    return mvi


def _same(a, b, rows=slice(None)):
    for k in nr.Modes._fields:
        assert np.array_equal(getattr(a, k)[rows], getattr(b, k)), k


def test_the_table_reaches_every_team_size():
    assert set(OWN_TEAM) == set(nr.SYSTEMS) and set(OWN_TEAM.values()) | set(t for t, _ in FORCED) == {1, 4, 16, 64}


@pytest.mark.parametrize("name", nr.SYSTEMS)
def test_table_on_the_device(monkeypatch, name):
    Q = nr.case_inputs(name)
    mvi = _batch(monkeypatch, name, len(Q))
    assert mvi.kernel_info()["team"] == OWN_TEAM[name]
    got = mvi.normal_modes(Q)
    assert mvi.kernel_info()["generic_launch_mask"] == 1 << MODES_BIT
    nr.compare(name, got)
    for k in nr.Modes._fields:                           # a pose repeated in the launch
        assert np.array_equal(getattr(got, k)[nr.REPEAT], getattr(got, k)[0]), k
    pick = list(range(len(Q) - nr.RAGGED, len(Q)))       # a ragged block: the last workgroup partly idle, the same bits
    ragged = _batch(monkeypatch, name, nr.RAGGED).normal_modes(Q[pick])
    _same(got, ragged, pick)
    alone = _batch(monkeypatch, name, 1).normal_modes(Q[3:4])
    _same(got, alone, slice(3, 4))
    assert np.array_equal(got.unstable, (got.omega2 < 0).sum(axis=1))
    f = got.frequencies
    assert np.isnan(f[got.omega2 < 0]).all() and np.allclose(f[got.omega2 >= 0], np.sqrt(got.omega2[got.omega2 >= 0]) / (2 * np.pi))


@pytest.mark.parametrize("team,name", FORCED)
def test_other_team_sizes(monkeypatch, team, name):
    pick = [0, 1, 2, 3, 4, 5, 6]
    got = _batch(monkeypatch, name, len(pick), team).normal_modes(nr.case_inputs(name)[pick])
    nr.compare(name, got, pick)


def test_host_and_device_entry_points_agree_bit_for_bit(monkeypatch):
    name = "mixed_loop"
    L = _lib.lib()
    Q = nr.case_inputs(name)
    B = len(Q)
    host = _batch(monkeypatch, name, B).normal_modes(Q)
    mvi = _batch(monkeypatch, name, B)
    nq, nc, nF = mvi.nq, mvi.nc, host.omega2.shape[1]
    q_dev = mvi.device_array(Q)
    ints = L.tg_device_alloc(0, 4 * 4 * B)
    assert ints
    try:
        o2, md, mu, res = mvi.device_empty(B * nF), mvi.device_empty(B * nF * nq), mvi.device_empty(B * nc), mvi.device_empty(B)
        _lib.check(L.tg_batch_normal_modes_device(mvi._h, q_dev, None, None, nr.RCOND, nr.MAX_SWEEPS, o2, md, ints, ints + 4 * B, mu, res,
                                                  ints + 8 * B, ints + 12 * B))
        mvi.synchronize()
        back = np.zeros(4 * B, dtype=np.int32)
        _lib.check(L.tg_memcpy_d2h(0, back.ctypes.data, ints, 16 * B))
        got = nr.Modes(mvi.download(o2, (B, nF)), mvi.download(md, (B, nF, nq)), back[:B], back[B:2 * B], mvi.download(mu, (B, nc)),
                       mvi.download(res, (B,)), back[2 * B:3 * B], back[3 * B:])
        _same(host, got)
    finally:
        L.tg_device_free(0, ints)


def test_mu_supplied(monkeypatch):
    name = "mixed_loop"
    Q = nr.case_inputs(name)
    mvi = _batch(monkeypatch, name, len(Q))
    got = mvi.normal_modes(Q)
    _same(got, mvi.normal_modes(Q, mu=got.mu))
    zero = mvi.normal_modes(Q, mu=np.zeros_like(got.mu))
    want = nr.normal_modes(name, Q, mu=np.zeros_like(got.mu))
    assert nr.eig_error(zero, want) <= nr.eig_bound(name) and not zero.mu.any()
    assert np.abs(zero.residual - want.residual).max() <= 1e-10


def test_parameter_twin_on_the_puppet(monkeypatch):
    """Each pose under its own row's masses against the reference on a system rebuilt with them."""
    name = "puppet40"
    Q = np.concatenate([nr.case_inputs(name)[:2]] * 4)
    rows = parameter_rows(name)
    mvi = _batch(monkeypatch, name, len(Q))
    mvi.set_parameters(inertia=rows["inertia"], gravity=rows["gravity"], group=2)
    got = mvi.normal_modes(Q)
    assert mvi.kernel_info()["par_generic_launch_mask"] == 1 << MODES_BIT
    for r in range(4):
        ev = nr.Pose(descriptor.flatten(rebuilt(common.BUILDERS[name], rows, r)))
        want = nr.normal_modes(name, Q[2 * r:2 * r + 2], ev=ev)
        sub = nr.Modes(*[getattr(got, k)[2 * r:2 * r + 2] for k in nr.Modes._fields])
        err = nr.eig_error(sub, want)
        print("row", r, "eigenvalue error %.3e bound %.3e" % (err, nr.eig_bound(name)))
        assert err <= nr.eig_bound(name) and np.array_equal(sub.count, want.count) and (sub.status == nr.OK).all()
        inv = nr.invariants(name, Q[2 * r:2 * r + 2], None, sub, ev=ev)
        assert inv["held"] and all(inv[k] <= v for k, v in nr.invariant_bounds(name).items()), inv
    assert np.abs(got.omega2[2:4] - got.omega2[0:2]).max() > 1e-3           # g -> 2 g moves the frequencies
    mvi.clear_parameters()
    _same(mvi.normal_modes(Q), _batch(monkeypatch, name, len(Q)).normal_modes(Q))


def test_constant_q_list(monkeypatch):
    name = "pendulum5"
    names = [c.name for c in common.build(name)[0].configs]
    ev = nr.pose_of(name)
    free = nr.default_free(ev)
    free[1] = False
    Q = nr.case_inputs(name)[:6]
    got = _batch(monkeypatch, name, 6).normal_modes(Q, constant_q_list=[names[1]])
    want = nr.normal_modes(name, Q, free)
    assert list(got.count) == [4] * 6 and got.modes.shape == (6, 4, 5) and not got.modes[:, :, 1].any()
    assert nr.eig_error(got, want) <= nr.TOL
    inv = nr.invariants(name, Q, free, got)
    assert inv["held"] and max(inv["orthonormal"], inv["eigen"]) <= nr.MARGIN * nr.INVARIANT_MIN


def test_refusals(monkeypatch):
    L = _lib.lib()
    mvi = _batch(monkeypatch, "spring_arm", 2)
    nq = mvi.nq
    Q = np.zeros((2, nq))
    kin = np.array([1 if c.kinematic else 0 for c in common.build("spring_arm")[0].configs], dtype=np.int32)
    assert kin.any()
    free = np.ones(nq, dtype=np.int32)
    o2, md = np.zeros((2, nq)), np.zeros((2, nq, nq))
    args = lambda mask, rcond, sweeps: (mvi._h, Q.ctypes.data, None, mask, rcond, sweeps, o2.ctypes.data, md.ctypes.data, None, None, None, None, None, None)
    assert L.tg_batch_normal_modes(*args(free.ctypes.data, 1e-9, 30)) == -1 and b"kinematic" in L.tg_last_error()
    assert L.tg_batch_normal_modes(*args(None, -1.0, 30)) == -1
    assert L.tg_batch_normal_modes(*args(None, 1e-9, 0)) == -1
    assert L.tg_batch_normal_modes(*args(None, 1e-9, 30)) == 0
    with pytest.raises(_lib.LibraryError, match="NonlinearConfigSpring"):
        _batch(monkeypatch, "nonlinear_spring_arm", 2).normal_modes(np.zeros((2, len(common.build("nonlinear_spring_arm")[0].configs))))


def test_statuses(monkeypatch):
    name = "pendulum5"
    Q = nr.case_inputs(name)[:3].copy()
    mvi = _batch(monkeypatch, name, 3)
    one = mvi.normal_modes(Q, max_sweeps=1)
    assert list(one.status) == [nr.NOT_CONVERGED] * 3 and list(one.sweeps) == [1] * 3 and one.omega2.any()
    Q[1, 2] = np.nan
    got = mvi.normal_modes(Q)
    assert list(got.status) == [nr.OK, nr.SINGULAR, nr.OK]
    for k in ("omega2", "modes", "count", "rank", "mu", "residual", "sweeps"):
        assert not np.asarray(getattr(got, k)[1]).any(), k
    system = common.build(name)[0]
    from trep_amd import parameters
    base = parameters.base_values(system)
    mvi.set_parameters(inertia=np.array([base["inertia"], 0.0 * base["inertia"], base["inertia"]]), group=1)
    massless = mvi.normal_modes(nr.case_inputs(name)[:3])
    assert list(massless.status) == [nr.OK, nr.SINGULAR, nr.OK] and not massless.omega2[1].any() and not massless.modes[1].any()
