"""Per-trajectory parameters without a GPU: the packing module (trep_amd/parameters.py) and the host emulation of the PAR
kernel path (tests/emu_par, the device source compiled with g++) against the oracle on systems rebuilt with each row."""
import numpy as np
import pytest

from common import BUILDERS, build, relerr, trajectories
from emu_harness import EmuBatch
from emu_par_harness import EmuParBatch
from oracle.oracle import OracleMVI
from trep_amd import descriptor, parameters, systems
from trep_amd.dynamics import Damping, Gravity

DT = 0.01


# ---- packing -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_base_values_equal_the_descriptor_tables(name):
    system, d = build(name)
    base = parameters.base_values(system)
    fi = np.ctypeslib.as_array(d.struct.frame_inertia, shape=(int(d.n_frames), 4)) if int(d.n_masses) else np.zeros((0, 4))
    masses = np.ctypeslib.as_array(d.struct.masses, shape=(int(d.n_masses),)) if int(d.n_masses) else np.zeros(0, dtype=int)
    assert np.array_equal(base["inertia"], fi[masses])
    ng, nd = int(d.n_gravity), int(d.n_dyn)
    if ng:
        g = np.ctypeslib.as_array(d.struct.gravity, shape=(ng, 3)).sum(axis=0)
        assert np.array_equal(base["gravity"], g)
    else:
        assert base["gravity"] is None
    if int(d.n_damping):
        dm = np.ctypeslib.as_array(d.struct.damping, shape=(int(d.n_damping), nd)).sum(axis=0)
        assert np.array_equal(base["damping"], dm)
    else:
        assert base["damping"] is None


def test_pack_order_broadcast_and_group():
    system = systems.pend_on_cart()
    base = parameters.base_values(system)
    nb, nd = base["inertia"].shape[0], len(system.dyn_configs)
    inertia = np.arange(4 * nb * 4, dtype=float).reshape(4, nb, 4) + 1.0
    rows, group, blocks = parameters.pack(system, 8, inertia=inertia, gravity=[0.0, 0.0, -9.0], group=2)
    assert (rows, group) == (4, 2)
    assert np.array_equal(blocks["inertia"], inertia)
    assert blocks["gravity"].shape == (4, 3) and np.all(blocks["gravity"] == [0.0, 0.0, -9.0])
    assert blocks["damping"] is None
    rows, group, blocks = parameters.pack(system, 8, damping=np.ones(nd))
    assert (rows, group) == (1, 1) and blocks["damping"].shape == (1, nd)
    rows, group, blocks = parameters.pack(system, 8)
    assert (rows, group) == (1, 1) and all(v is None for v in blocks.values())
    assert [parameters.row_of(t, 3) for t in range(7)] == [0, 0, 0, 1, 1, 1, 2]


def test_pack_refusals():
    system = systems.pend_on_cart()
    nb, nd = len(system.masses), len(system.dyn_configs)
    with pytest.raises(ValueError, match="batch size"):
        parameters.pack(system, 8, inertia=np.ones((3, nb, 4)))
    with pytest.raises(ValueError, match="shape"):
        parameters.pack(system, 8, inertia=np.ones((8, nb + 1, 4)))
    with pytest.raises(ValueError, match="shape"):
        parameters.pack(system, 8, gravity=np.ones((8, 2)))
    with pytest.raises(ValueError, match="finite"):
        parameters.pack(system, 8, damping=np.full((8, nd), np.nan))
    with pytest.raises(ValueError, match="different row counts"):
        parameters.pack(system, 8, inertia=np.ones((8, nb, 4)), damping=np.ones((4, nd)), group=1)
    with pytest.raises(ValueError, match="group"):
        parameters.pack(system, 8, gravity=[0, 0, -9.8], group=0)
    lifter = systems.scissor_lift(4)          # no Damping force
    with pytest.raises(ValueError, match="no Damping"):
        parameters.pack(lifter, 4, damping=np.ones(len(lifter.dyn_configs)))
    link = systems.damper_link()              # LinearDamper / ConfigSpring only
    assert not any(isinstance(f, Damping) for f in link.forces)
    with pytest.raises(ValueError, match="no Damping"):
        parameters.pack(link, 4, damping=np.ones(len(link.dyn_configs)))
    if not any(isinstance(p, Gravity) for p in link.potentials):
        with pytest.raises(ValueError, match="no Gravity"):
            parameters.pack(link, 4, gravity=[0, 0, -1.0])


# ---- host emulation of the parameter kernels -----------------------------------------------------------------------------

def random_rows(system, rows, seed):
    """Masses / inertias x U(0.5, 2), damping x U(0, 3), gravity scaled x U(0.8, 1.2) and tilted up to 10 degrees."""
    rng = np.random.default_rng(seed)
    base = parameters.base_values(system)
    out = {"inertia": base["inertia"][None] * rng.uniform(0.5, 2.0, (rows,) + base["inertia"].shape)}
    if base["gravity"] is not None:
        g = np.empty((rows, 3))
        for r in range(rows):
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            a = np.radians(rng.uniform(0.0, 10.0))
            v = base["gravity"]
            rot = v * np.cos(a) + np.cross(axis, v) * np.sin(a) + axis * axis.dot(v) * (1 - np.cos(a))
            g[r] = rot * rng.uniform(0.8, 1.2)
        out["gravity"] = g
    if base["damping"] is not None:
        out["damping"] = base["damping"][None] * rng.uniform(0.0, 3.0, (rows, len(base["damping"])))
    return out


def rebuilt(make, rows, r):
    """The system rebuilt with row r's values (the reference's own setters)."""
    system = make()
    for f, v in zip(system.masses, rows["inertia"][r]):
        f.set_mass(*[float(x) for x in v])
    if "gravity" in rows:
        gs = [p for p in system.potentials if isinstance(p, Gravity)]
        gs[0].gravity = rows["gravity"][r]
        for p in gs[1:]:
            p.gravity = (0.0, 0.0, 0.0)
    if "damping" in rows:
        ds = [f for f in system.forces if isinstance(f, Damping)]
        for i, c in enumerate(system.dyn_configs):
            ds[0].set_damping_coefficient(c, rows["damping"][r][i])
            for f in ds[1:]:
                f.set_damping_coefficient(c, 0.0)
    return system


EMU_SYSTEMS = ["damper_link", "pend_on_cart", "pendulum5", "puppet_basic", "scissor4"]


def inputs(name, B, N):
    """Initial configs and open-loop inputs of B trajectories: the recorded fixtures' (tests/golden), cycled."""
    trajs = [trajectories(name)[b % len(trajectories(name))] for b in range(B)]
    Q0 = np.array([t[1] for t in trajs])
    U = np.array([t[2][:N] for t in trajs])
    K = np.array([t[3][:N] for t in trajs])
    return Q0, U, K


@pytest.mark.parametrize("name", EMU_SYSTEMS)
def test_emulated_parameter_rollout_matches_rebuilt_systems(name):
    make = BUILDERS[name]
    system = make()
    d = descriptor.flatten(system)
    B, N = 3, 20
    rows = random_rows(system, B, seed=11)
    Q0, U, K = inputs(name, B, N)
    e = EmuParBatch(d, B)
    e.set_parameters(B, 1, **rows)
    e.initialize_from_configs(0.0, Q0, DT, Q0)
    X = e.rollout(N, DT, U, K)
    assert (e.status == 0).all()
    nq, nd = int(d.n_configs), int(d.n_dyn)
    for b in range(B):
        o = OracleMVI(descriptor.flatten(rebuilt(make, rows, b)))
        o.initialize_from_configs(0.0, Q0[b], DT, Q0[b])
        Xo, _ = o.rollout(N, DT, U[b], K[b])
        assert relerr(X[b, :, :nq], Xo[:, :nq]) < 1e-10, (name, b)
        assert relerr(X[b, :, nq:nq + nd], Xo[:, nq:nq + nd]) < 1e-10, (name, b)


@pytest.mark.parametrize("name", ["pend_on_cart", "scissor4"])
def test_emulated_parameter_deriv1_and_dynamics_match_rebuilt_systems(name):
    make = BUILDERS[name]
    system = make()
    d = descriptor.flatten(system)
    B = 2
    rows = random_rows(system, B, seed=5)
    Q0, U, K = inputs(name, B, 1)
    nu, nk = int(d.n_inputs), int(d.n_kin)
    e = EmuParBatch(d, B)
    e.set_parameters(B, 1, **rows)
    e.initialize_from_configs(0.0, Q0, DT, Q0)
    e.rollout(1, DT, U, K, want_X=False)
    out = e.deriv1()
    dQ = np.random.default_rng(2).uniform(-0.3, 0.3, Q0.shape)
    ddq, lam = e.dynamics(Q0, dQ, np.zeros((B, nu)) if nu else None, np.zeros((B, nk)) if nk else None)[:2]
    for b in range(B):
        r = EmuBatch(descriptor.flatten(rebuilt(make, rows, b)), 1)
        r.initialize_from_configs(0.0, Q0[b:b + 1], DT, Q0[b:b + 1])
        r.rollout(1, DT, U[b:b + 1], K[b:b + 1], want_X=False)
        ref = r.deriv1()
        for n in ref:
            assert relerr(out[n][b], ref[n][0]) < 1e-10, (name, b, n)
        rd, rl = r.dynamics(Q0[b:b + 1], dQ[b:b + 1], np.zeros((1, nu)) if nu else None, np.zeros((1, nk)) if nk else None)[:2]
        assert relerr(ddq[b], rd[0]) < 1e-10 and relerr(lam[b], rl[0]) < 1e-10, (name, b)


@pytest.mark.parametrize("name", ["pend_on_cart", "puppet_basic"])
def test_emulated_base_row_is_bitwise_the_default(name):
    system, d = build(name)
    B, N = 2, 10
    Q0, U, K = inputs(name, B, N)
    runs = []
    for par in (False, True):
        e = EmuParBatch(d, B)
        if par:
            e.set_parameters(1, B)
        e.initialize_from_configs(0.0, Q0, DT, Q0)
        runs.append((e.rollout(N, DT, U, K), e.iters.copy(), e.status.copy()))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
