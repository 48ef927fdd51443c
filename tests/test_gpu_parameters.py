"""Per-trajectory masses / inertias, gravity and damping on the MI355X (BatchMidpointVI.set_parameters): every row of a parameter
batch against the oracle and against default batches of systems rebuilt with that row, the identity with the default kernels,
which kernels ran, and the refusals."""
import numpy as np
import pytest

from common import BUILDERS, relerr, trajectories
from oracle.oracle import OracleMVI
from test_parameters_cpu import random_rows, rebuilt
from trep_amd import BatchMidpointVI, descriptor, specialize
from trep_amd import _lib
from trep_amd._lib import LibraryError
from trep_amd.discopt.dsystem import BatchDSystem

pytestmark = pytest.mark.gpu

DT = 0.01
PARITY = {"pend_on_cart": 256, "pendulum5": 128, "damper_link": 128, "scissor4": 128, "puppet40": 64, "puppet_basic": 64}


def inputs(name, B, N):
    trajs = trajectories(name)
    trajs = [trajs[b % len(trajs)] for b in range(B)]
    n = min(N, min(len(t[2]) for t in trajs))
    return np.array([t[1] for t in trajs]), np.array([t[2][:n] for t in trajs]), np.array([t[3][:n] for t in trajs]), n


def started(system, B, Q0, specialize_mode=False, rows=None, group=1):
    """A batch initialised at Q0; with `rows` the table is set first, so that the initial momenta (calc_p2) use it too."""
    mvi = BatchMidpointVI(system, B, specialize=specialize_mode)
    if rows is not None:
        mvi.set_parameters(group=group, **rows)
    mvi.initialize_from_configs(0.0, Q0, DT, Q0)
    return mvi


@pytest.mark.parametrize("name", sorted(PARITY))
def test_rollout_rows_match_rebuilt_systems(name):
    make = BUILDERS[name]
    system = make()
    B = PARITY[name]
    rows = random_rows(system, B, seed=21)
    Q0, U, K, N = inputs(name, B, 200)
    mvi = started(system, B, Q0, "auto", rows)
    X = mvi.rollout(N, DT, U, K)
    iters, status = mvi.status()
    assert (status == 0).all(), name
    lam = mvi.lambda1
    nq, nd = mvi.nq, mvi.nd
    for b in range(B):
        o = OracleMVI(descriptor.flatten(rebuilt(make, rows, b)))
        o.initialize_from_configs(0.0, Q0[b], DT, Q0[b])
        Xo, _ = o.rollout(N, DT, U[b], K[b])
        assert relerr(X[b, :, :nq], Xo[:, :nq]) < 1e-10, (name, b)
        assert relerr(X[b, :, nq:nq + nd], Xo[:, nq:nq + nd]) < 1e-10, (name, b)
        if mvi.nc:
            assert relerr(lam[b], o.lambda1) < 3e-10, (name, b)
    # the generic parameter kernel, four rows against a default generic batch of the rebuilt system: same Newton iterations,
    # <= 1e-12 relative (the specialised kernels above differ from the generic ones by their FMA contraction choices)
    gen = started(system, B, Q0, False, rows)
    Xg = gen.rollout(N, DT, U, K)
    ig = gen.status()[0]
    for b in (0, 1, B // 2, B - 1):
        ref = started(rebuilt(make, rows, b), 1, Q0[b:b + 1])
        Xr = ref.rollout(N, DT, U[b:b + 1], K[b:b + 1])
        assert relerr(Xg[b], Xr[0]) < 1e-12, (name, b)
        assert int(ig[b]) == int(ref.status()[0][0]), (name, b)


@pytest.mark.parametrize("name", ["pend_on_cart", "scissor4", "puppet40"])
def test_base_rows_are_the_default_kernels(name):
    system = BUILDERS[name]()
    B = 16
    Q0, U, K, N = inputs(name, B, 50)
    for spec in (False, True):
        a = started(system, B, Q0, spec)
        Xa = a.rollout(N, DT, U, K)
        base = a.parameters()
        b = started(system, B, Q0, spec, {k: v for k, v in base.items() if v is not None})
        Xb = b.rollout(N, DT, U, K)
        (ia, sa), (ib, sb) = a.status(), b.status()
        assert np.array_equal(ia, ib) and np.array_equal(sa, sb), (name, spec)
        if spec:
            assert relerr(Xa, Xb) < 1e-12, name
            assert "rollout" in b.kernel_info()["par_spec_launched"]
        else:
            assert np.array_equal(Xa, Xb), name
            assert "rollout" in b.kernel_info()["par_generic_launched"]
        before = b.kernel_info()
        b.clear_parameters()
        b.initialize_from_configs(0.0, Q0, DT, Q0)
        assert np.array_equal(b.rollout(N, DT, U, K), Xa) or spec
        after = b.kernel_info()
        default = lambda i: i["spec_launches"] + i["generic_launches"]    # calc_p2 and the rollout
        assert default(after) == default(before) + 2 and after["par_spec_launches"] + after["par_generic_launches"] == \
            before["par_spec_launches"] + before["par_generic_launches"]


@pytest.mark.parametrize("name", ["pend_on_cart", "scissor4", "puppet40"])
def test_kernel_kinds_with_the_prebuilt_library(name):
    system = BUILDERS[name]()
    if not specialize.is_built(system):
        specialize.build(system)
    B = 8
    Q0, U, K, N = inputs(name, B, 3)
    mvi = started(system, B, Q0, True, random_rows(system, B, seed=2))
    mvi.rollout(N, DT, U, K)
    mvi.calc_deriv1()
    mvi.deriv2_contract(np.random.default_rng(1).normal(size=(B, mvi.nX)))
    mvi.dynamics(Q0, np.zeros_like(Q0), np.zeros((B, mvi.nu)) if mvi.nu else None, np.zeros((B, mvi.nk)) if mvi.nk else None)
    mvi.energy(Q0, np.zeros_like(Q0))
    info = mvi.kernel_info()
    assert set(info["par_spec_launched"]) == {"rollout", "deriv1", "deriv2z"}, info
    assert set(info["par_generic_launched"]) == {"calc_p2", "dynamics", "energy"}, info
    assert info["spec_launches"] == 0 and info["generic_launches"] == 0, info


@pytest.mark.parametrize("name", ["pend_on_cart", "scissor4", "puppet_basic"])
def test_derivatives_and_dynamics_match_rebuilt_systems(name):
    make = BUILDERS[name]
    system = make()
    B = 6
    rows = random_rows(system, B, seed=8)
    Q0, U, K, _ = inputs(name, B, 2)
    rng = np.random.default_rng(4)
    mvi = started(system, B, Q0, "auto", rows)
    mvi.rollout(1, DT, U[:, :1], K[:, :1])
    mvi.calc_deriv1()
    d1 = dict((n, mvi.deriv1(n)) for n in mvi.D1_NAMES)
    Z = rng.normal(size=(B, mvi.nX))
    ZL = rng.normal(size=(B, mvi.nc)) if mvi.nc else None
    HZ = mvi.deriv2_contract(Z)
    HZL = mvi.deriv2_contract(Z, ZL) if mvi.nc else None
    dQ = rng.uniform(-0.3, 0.3, Q0.shape)
    u = rng.normal(size=(B, mvi.nu)) if mvi.nu else None
    ddk = rng.normal(size=(B, mvi.nk)) if mvi.nk else None
    ddq, lam, st = mvi.dynamics(Q0, dQ, u, ddk)
    dd1, _ = mvi.dynamics_deriv1(Q0, dQ, u, ddk)
    en = mvi.energy(Q0, dQ)
    lag = mvi.lagrangian(Q0, dQ)
    with pytest.raises(LibraryError):
        mvi.dynamics_deriv1(Q0, dQ, u, ddk, seeds=(np.zeros(B, dtype=np.int32),))
    # subset launch (steps 1, 2 of every horizon-3 group): the remapped trajectories read their own rows
    R = HZ.shape[1]
    z_dev, hz_dev = mvi.device_array(Z), mvi.device_empty(B * R * R)
    _lib.check(mvi._L.tg_batch_deriv2_contract_device_range(mvi._h, z_dev, hz_dev, 3, 1, 3))
    mvi.synchronize()
    sub = mvi.download(hz_dev, (B, R, R))
    for t in range(B):
        if t % 3 >= 1:
            assert relerr(sub[t], HZ[t]) < 1e-12, (name, t)
    for b in range(B):
        r = started(rebuilt(make, rows, b), 1, Q0[b:b + 1])
        r.rollout(1, DT, U[b:b + 1, :1], K[b:b + 1, :1])
        r.calc_deriv1()
        for n in mvi.D1_NAMES:
            assert relerr(d1[n][b], r.deriv1(n)[0]) < 1e-10, (name, b, n)
        assert relerr(HZ[b], r.deriv2_contract(Z[b:b + 1])[0]) < 1e-10, (name, b)
        if HZL is not None:
            assert relerr(HZL[b], r.deriv2_contract(Z[b:b + 1], ZL[b:b + 1])[0]) < 1e-10, (name, b)
        sl = lambda a: None if a is None else a[b:b + 1]
        rd, rl, _ = r.dynamics(Q0[b:b + 1], dQ[b:b + 1], sl(u), sl(ddk))
        assert relerr(ddq[b], rd[0]) < 1e-12 and relerr(lam[b], rl[0]) < 1e-12, (name, b)
        rdd, _ = r.dynamics_deriv1(Q0[b:b + 1], dQ[b:b + 1], sl(u), sl(ddk))
        for n in dd1:
            assert relerr(dd1[n][b], rdd[n][0]) < 1e-12, (name, b, n)
        assert relerr(en[b], r.energy(Q0[b:b + 1], dQ[b:b + 1])[0]) < 1e-12, (name, b)
        rlag = r.lagrangian(Q0[b:b + 1], dQ[b:b + 1])
        for n in lag:
            assert relerr(lag[n][b], rlag[n][0]) < 1e-12, (name, b, n)


def test_linearize_subset_range_group_broadcast_and_closed_loop():
    make = BUILDERS["pend_on_cart"]
    system = make()
    horizon, seeds = 4, 3
    B = horizon * seeds
    rows = random_rows(system, seeds, seed=3)
    Q0, U, K, _ = inputs("pend_on_cart", B, 2)
    ds = BatchDSystem(system, np.arange(3) * DT, B, specialize=False)
    ds.set_parameters(group=horizon, **rows)                 # trajectory t uses row t // horizon
    X0 = np.zeros((B, ds._nX))
    X0[:, :len(system.configs)] = Q0
    ds.set(X0, np.zeros((B, ds._nU)), 0)
    A, Bm = ds.linearize()
    for s in range(seeds):
        one = BatchDSystem(rebuilt(make, rows, s), np.arange(3) * DT, 1, specialize=False)
        for t in range(s * horizon, (s + 1) * horizon):
            one.set(X0[t:t + 1], np.zeros((1, ds._nU)), 0)
            Ar, Br = one.linearize()
            assert relerr(A[t], Ar[0]) < 1e-10 and relerr(Bm[t], Br[0]) < 1e-10, t
    # one broadcast row == the rebuilt system in every trajectory
    one_row = {k: v[:1] for k, v in rows.items()}
    mvi = started(system, 8, Q0[:8], rows=one_row)
    X = mvi.rollout(20, DT, np.zeros((8, 20, mvi.nu)), np.zeros((8, 20, mvi.nk)))
    ref = started(rebuilt(make, rows, 0), 8, Q0[:8])
    assert relerr(X, ref.rollout(20, DT, np.zeros((8, 20, mvi.nu)), np.zeros((8, 20, mvi.nk)))) < 1e-12
    # closed loop: U = bU - K (x - bX) with the row's dynamics
    N, nX, nU = 10, mvi.nX, mvi.nU
    rng = np.random.default_rng(6)
    Kp = rng.normal(scale=0.1, size=(1, N, nU, nX))
    bX = np.zeros((8, N + 1, nX))
    bX[:, :, :len(system.configs)] = Q0[:8, None]
    bU = rng.normal(scale=0.1, size=(8, N, nU))
    mvi.initialize_from_configs(0.0, Q0[:8], DT, Q0[:8])
    ref.initialize_from_configs(0.0, Q0[:8], DT, Q0[:8])
    Xc, Uc = mvi.rollout_closed_loop(N, DT, Kp, bX, bU, group_size=8)
    Xr, Ur = ref.rollout_closed_loop(N, DT, Kp, bX, bU, group_size=8)
    assert relerr(Xc, Xr) < 1e-12 and relerr(Uc, Ur) < 1e-12


def test_parameters_changed_between_launches_and_refresh_drops_the_table():
    make = BUILDERS["pend_on_cart"]
    system = make()
    B = 4
    rows = random_rows(system, 2 * B, seed=9)
    first = {k: v[:B] for k, v in rows.items()}
    second = {k: v[B:] for k, v in rows.items()}
    Q0, U, K, N = inputs("pend_on_cart", B, 30)
    mvi = started(system, B, Q0, rows=first)
    mvi.rollout(N, DT, U, K)
    mvi.set_parameters(**second)
    mvi.initialize_from_configs(0.0, Q0, DT, Q0)
    X2 = mvi.rollout(N, DT, U, K)
    for b in range(B):
        ref = started(rebuilt(make, second, b), 1, Q0[b:b + 1])
        assert relerr(X2[b], ref.rollout(N, DT, U[b:b + 1], K[b:b + 1])[0]) < 1e-12, b
    assert mvi.kernel_info()["parameter_rows"] == B
    system.masses[0].set_mass(2.5)                           # a structure change: the next call rebuilds the schedule
    mvi.initialize_from_configs(0.0, Q0, DT, Q0)
    assert mvi.kernel_info()["parameter_rows"] == 0 and not mvi.has_parameters


def test_refusals_make_no_launch():
    pend = BUILDERS["pend_on_cart"]()
    nb, nd = len(pend.masses), len(pend.dyn_configs)
    mvi = started(pend, 8, np.tile([c.q for c in pend.configs], (8, 1)))
    before = mvi.kernel_info()
    bad = [dict(inertia=np.ones((3, nb, 4))), dict(inertia=np.ones((8, nb, 3))), dict(gravity=np.ones((8, 2))),
           dict(damping=np.full((8, nd), np.nan)), dict(gravity=[0.0, np.inf, -9.8]), dict(damping=np.ones((8, nd)), group=2)]
    for kw in bad:
        with pytest.raises(ValueError):
            mvi.set_parameters(**kw)
    for name, kw in (("scissor4", "damping"), ("damper_link", "damping")):
        s = BUILDERS[name]()
        m = started(s, 4, np.tile([c.q for c in s.configs], (4, 1)))
        with pytest.raises(ValueError, match="Damping"):
            m.set_parameters(**{kw: np.ones((4, len(s.dyn_configs)))})
        assert m.kernel_info()["parameter_rows"] == 0
    after = mvi.kernel_info()
    assert after["parameter_rows"] == 0
    for k in ("spec_launches", "generic_launches", "par_spec_launches", "par_generic_launches"):
        assert after[k] == before[k], k
