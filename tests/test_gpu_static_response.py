"""BatchMidpointVI.static_response on the device against the numpy specification (static_response_reference.py): the case table at the
team size the library gives every system (1, 4, 16 and 64) and at forced team sizes, a ragged block, the bounds and invariants of sr.compare,
bit-equality (a pose repeated, alone, host against device entry point, drive subsets, without the compliance), mu supplied, the
parameter twin on the puppet, the statuses, the refusals and the launch masks."""
import numpy as np
import pytest

import common
import normal_modes_reference as nr
import projection_reference as pr
import static_response_reference as sr
from test_equilibrium_cpu import parameter_rows
from test_parameters_cpu import rebuilt
from trep_amd import BatchMidpointVI, _lib, descriptor

pytestmark = pytest.mark.gpu

RESPONSE_BIT = 16
OWN_TEAM = {"spring_link": 4, "mixed_loop": 16, "spatial_loop": 16, "scissor4_slider": 64, "scissor4_free": 64, "pendulum5_joint": 16,
            "pendulum1": 1, "ladder_mixed": 64, "puppet40": 64}
FORCED = [(4, "pendulum5_joint"), (4, "mixed_loop"), (64, "pendulum1")]


def _batch(monkeypatch, name, B, team=None):
    if team is None:
        monkeypatch.delenv("TREPAMD_TEAM", raising=False)
    else:
        monkeypatch.setenv("TREPAMD_TEAM", str(team))
    mvi = BatchMidpointVI(common.build(name)[0], B, specialize=False)
    if team is not None:
        assert mvi.kernel_info()["team"] == team
    return mvi


def _mask(case):
    """The case's mask as the arguments of static_response."""
    kind = sr.CASES[case][1]
    return dict(keep_kinematic=kind == "keep_kinematic", constant_q_list=sr.constant_names(case))


def _same(a, b, rows=slice(None)):
    for k in sr.Response._fields:
        if getattr(a, k) is None:
            assert getattr(b, k) is None, k
        else:
            assert np.array_equal(getattr(a, k)[rows], getattr(b, k)), k


def test_the_table_reaches_every_team_size():
    assert set(OWN_TEAM) == set(sr.CASES) and set(OWN_TEAM.values()) | set(t for t, _ in FORCED) == {1, 4, 16, 64}


@pytest.mark.parametrize("case", tuple(sr.CASES))
def test_table_on_the_device(monkeypatch, case):
    name = sr.system_of(case)
    Q, free = sr.case_inputs(case)
    mvi = _batch(monkeypatch, name, len(Q))
    assert mvi.kernel_info()["team"] == OWN_TEAM[case]
    assert np.array_equal(mvi.free_mask(**_mask(case)) != 0, free)
    got = mvi.static_response(Q, **_mask(case))
    assert mvi.kernel_info()["generic_launch_mask"] == 1 << RESPONSE_BIT
    sr.compare(case, got)                                # (the repeated row's bits among its checks)
    pick = list(range(len(Q) - sr.RAGGED, len(Q)))       # a ragged block: the last workgroup partly idle, the same bits
    ragged = _batch(monkeypatch, name, sr.RAGGED).static_response(Q[pick], **_mask(case))
    _same(got, ragged, pick)
    alone = _batch(monkeypatch, name, 1).static_response(Q[3:4], **_mask(case))
    _same(got, alone, slice(3, 4))


@pytest.mark.parametrize("team,case", FORCED)
def test_other_team_sizes(monkeypatch, team, case):
    pick = [0, 1, 2, 3, 4, 5, 6]
    got = _batch(monkeypatch, sr.system_of(case), len(pick), team).static_response(sr.case_inputs(case)[0][pick], **_mask(case))
    sr.compare(case, got, pick)


@pytest.mark.parametrize("case", ("mixed_loop", "puppet40"))
def test_drive_subsets_and_no_compliance(monkeypatch, case):
    name = sr.system_of(case)
    Q, free = sr.case_inputs(case)
    mvi = _batch(monkeypatch, name, len(Q))
    full = mvi.static_response(Q, **_mask(case))
    every = sr.default_drive(free)
    places = list(range(len(every)))[::-1][::2]
    names = pr.config_names(name)
    part = mvi.static_response(Q, drive=[names[every[p]] for p in places], **_mask(case))
    for k in sr.Response._fields:
        if k == "defect":                                 # (the worst over the driven columns: of fewer, no larger)
            assert (part.defect <= full.defect).all()
            continue
        want = getattr(full, k)[:, places] if k in ("dq", "dmu") else getattr(full, k)
        assert np.array_equal(getattr(part, k), want), k
    lean = mvi.static_response(Q, compliance=False, **_mask(case))
    assert lean.compliance is None and lean.reaction is None
    for k in ("dq", "dmu", "rank", "mu", "residual", "defect", "status"):
        assert np.array_equal(getattr(lean, k), getattr(full, k)), k


def test_host_and_device_entry_points_agree_bit_for_bit(monkeypatch):
    case = "mixed_loop"
    name = sr.system_of(case)
    L = _lib.lib()
    Q, free = sr.case_inputs(case)
    B = len(Q)
    host = _batch(monkeypatch, name, B).static_response(Q, **_mask(case))
    mvi = _batch(monkeypatch, name, B)
    nq, nc, nD = mvi.nq, mvi.nc, host.dq.shape[1]
    q_dev = mvi.device_array(Q)
    ints = L.tg_device_alloc(0, 2 * 4 * B)
    assert ints
    try:
        dq, dmu, cm, re = mvi.device_empty(B * nD * nq), mvi.device_empty(B * nD * nc), mvi.device_empty(B * nq * nq), mvi.device_empty(B * nq * nc)
        mu, res, dfc = mvi.device_empty(B * nc), mvi.device_empty(B), mvi.device_empty(B)
        n = mvi.static_response_device(q_dev, dq_dev=dq, dmu_dev=dmu, compliance_dev=cm, reaction_dev=re, rank_dev=ints, mu_out_dev=mu,
                                       residual_dev=res, defect_dev=dfc, status_dev=ints + 4 * B, **_mask(case))
        assert n == nD
        mvi.synchronize()
        back = np.zeros(2 * B, dtype=np.int32)
        _lib.check(L.tg_memcpy_d2h(0, back.ctypes.data, ints, 8 * B))
        got = sr.Response(mvi.download(dq, (B, nD, nq)), mvi.download(dmu, (B, nD, nc)), mvi.download(cm, (B, nq, nq)), mvi.download(re, (B, nq, nc)),
                          back[:B], mvi.download(mu, (B, nc)), mvi.download(res, (B,)), mvi.download(dfc, (B,)), back[B:])
        _same(host, got)
    finally:
        L.tg_device_free(0, ints)


def test_mu_supplied(monkeypatch):
    case = "mixed_loop"
    name = sr.system_of(case)
    Q, free = sr.case_inputs(case)
    mvi = _batch(monkeypatch, name, len(Q))
    got = mvi.static_response(Q, **_mask(case))
    _same(got, mvi.static_response(Q, mu=got.mu, **_mask(case)))
    other = 0.5 * got.mu                                  # not the pose's multipliers: another W, a residual
    half = mvi.static_response(Q, mu=other, **_mask(case))
    want = sr.static_response(name, Q, free, mu=other)
    err, bounds = sr.errors(half, want), sr.case_bounds(case)
    print(err, bounds)
    assert np.array_equal(half.mu, other) and np.array_equal(half.status, want.status)
    assert all(err[k] <= bounds[k] for k in err), (err, bounds)
    assert half.residual.max() > 1e-3


def test_parameter_twin_on_the_puppet(monkeypatch):
    """Each pose under its own row's masses against the reference on a system rebuilt with them; under g -> 2 g the pose's
    derivative stays, the multipliers' doubles and the compliance halves."""
    case = name = "puppet40"
    Q0, free = sr.case_inputs(case)
    Q = np.concatenate([Q0[:2]] * 4)
    rows = parameter_rows(name)
    mvi = _batch(monkeypatch, name, len(Q))
    plain = mvi.static_response(Q, **_mask(case))
    mvi.set_parameters(inertia=rows["inertia"], gravity=rows["gravity"], group=2)
    got = mvi.static_response(Q, **_mask(case))
    assert mvi.kernel_info()["par_generic_launch_mask"] == 1 << RESPONSE_BIT
    bounds, ib = sr.case_bounds(case), sr.invariant_bounds(case)
    for r in range(4):
        pick = np.arange(2 * r, 2 * r + 2)
        ev = nr.Pose(descriptor.flatten(rebuilt(common.BUILDERS[name], rows, r)))
        want = sr.static_response(name, Q[pick], free, ev=ev)
        sub = sr.subset(got, pick)
        err = sr.errors(sub, want)
        print("row", r, err, bounds)
        assert np.array_equal(sub.status, want.status) and np.array_equal(sub.rank, want.rank)
        assert all(err[k] <= bounds[k] for k in err), (r, err, bounds)
        if (want.status == sr.OK).all():
            inv = sr.invariants(name, Q[pick], free, sub, ev=ev)
            assert inv["held"] and all(inv[k] <= ib[k] for k in ib), inv
    base, g = np.asarray(rows["gravity"][0], dtype=float), np.asarray(rows["gravity"][1], dtype=float)
    assert np.array_equal(g, 2.0 * base) and np.array_equal(rows["inertia"][0], rows["inertia"][1]), "rows 0 and 1: g -> 2 g alone"
    a, b = sr.subset(got, [0, 1]), sr.subset(got, [2, 3])
    assert (a.status == sr.OK).all() and (b.status == sr.OK).all()
    scaled = sr.Response(a.dq, 2.0 * a.dmu, 0.5 * a.compliance, a.reaction, a.rank, 2.0 * a.mu, 2.0 * a.residual, a.defect, a.status)
    err = sr.errors(b, scaled)
    print("g -> 2 g", err)
    assert all(err[k] <= bounds[k] for k in ("dq", "dmu", "compliance")), (err, bounds)
    mvi.clear_parameters()
    _same(mvi.static_response(Q, **_mask(case)), plain)


def test_statuses(monkeypatch):
    """A pose that is not finite and a maximum (the inverted pendulum): TG_SINGULAR with every output zero; their neighbour untouched."""
    case, name = "pendulum5_joint", "pendulum5"
    Q0, free = sr.case_inputs(case)
    Q = Q0[:3].copy()
    Q[1, 0] = np.nan
    Q[2] = 0.0
    Q[2, 0] = np.pi
    mvi = _batch(monkeypatch, name, 3)
    got = mvi.static_response(Q, **_mask(case))
    assert list(got.status) == [sr.OK, sr.SINGULAR, sr.SINGULAR]
    for k in sr.Response._fields[:-1]:
        assert not np.asarray(getattr(got, k)[1:]).any(), k
    _same(mvi.static_response(Q0[:3], **_mask(case)), sr.subset(got, [0]), slice(0, 1))


def test_refusals(monkeypatch):
    L = _lib.lib()
    name = "mixed_loop"
    mvi = _batch(monkeypatch, name, 2)
    nq, nc = mvi.nq, mvi.nc
    free = np.ascontiguousarray(sr.free_mask("mixed_loop"), dtype=np.int32)
    held = np.flatnonzero(free == 0).astype(np.int32)
    assert len(held) >= 2
    Q = np.ascontiguousarray(sr.case_inputs("mixed_loop")[0][:2])
    dq, dmu, cm, re = np.zeros((2, nq, nq)), np.zeros((2, nq, nc)), np.zeros((2, nq, nq)), np.zeros((2, nq, nc))

    def call(q=Q.ctypes.data, mask=free.ctypes.data, drive=held, loads=1, rcond=1e-9):
        drive = np.ascontiguousarray(drive, dtype=np.int32)
        return L.tg_batch_static_response(mvi._h, q, None, mask, len(drive), drive.ctypes.data, loads, rcond, dq.ctypes.data, dmu.ctypes.data,
                                          cm.ctypes.data, re.ctypes.data, None, None, None, None, None)
    assert call() == 0
    assert call(q=None) == -1
    assert call(rcond=-1.0) == -1 and call(rcond=float("nan")) == -1
    assert call(drive=[int(np.flatnonzero(free)[0])]) == -1 and b"free" in L.tg_last_error()
    assert call(drive=[nq]) == -1 and call(drive=[-1]) == -1
    assert call(drive=[held[0], held[1], held[0]]) == -1 and b"twice" in L.tg_last_error()
    assert call(mask=None, drive=[held[0]]) == -1            # no mask: every config free
    assert call(drive=[], loads=0) == -1 and b"nothing to compute" in L.tg_last_error()
    assert call(drive=[], loads=1) == 0 and call(loads=0) == 0
    with pytest.raises(ValueError, match="free"):
        mvi.static_response(Q, keep_kinematic=True, drive=[pr.config_names(name)[int(np.flatnonzero(free)[0])]])
    with pytest.raises(_lib.LibraryError, match="NonlinearConfigSpring"):
        _batch(monkeypatch, "nonlinear_spring_arm", 2).static_response(np.zeros((2, len(common.build("nonlinear_spring_arm")[0].configs))))
