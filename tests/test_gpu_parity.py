"""Parity of the HIP path (through the C ABI, on a real MI355X) with the reference golden vectors,
the oracle, and size-independent properties at the BASELINE batch sizes."""
import numpy as np
import pytest

from common import BUILDERS, build, golden, trajectories, relerr

pytestmark = pytest.mark.gpu

DT = 0.01
TOL = 1e-10  # BASELINE.json north_star: fp64 state within 1e-10 of the reference


def _batch(system, B):
    import trep_amd
    return trep_amd.BatchMidpointVI(system, B)


# systems whose rollout / deriv1 / deriv2z kernels are ALSO run system-specialised (trep_amd/specialize.py) in the derivative
# and pivot-rule tests below; every other system runs the generic kernels only (specialize=False is then the only case)
SPEC_SYSTEMS = ("puppet40", "scissor4", "pend_on_cart")


def _spec_cases(names):
    return [(n, False) for n in names] + [(n, True) for n in names if n in SPEC_SYSTEMS]


def _assert_kernels(info, spec, modes):
    """The launches of `modes` went through the kind of kernel the test asked for -- and only through it."""
    for m in modes:
        if spec:
            assert m in info["spec_modes"] and m in info["spec_launched"] and m not in info["generic_launched"], (m, info)
            # the specialised derivative kernels of a full-wave team run two wavefronts per trajectory (helper waves)
            assert info["helper_waves"] == (2 if info["team"] == 64 else 1), info
        else:
            assert m in info["generic_launched"] and m not in info["spec_launched"], (m, info)


def test_library_reports_device():
    from trep_amd import _lib
    assert _lib.lib().tg_device_count() >= 1
    assert b"gfx950" in _lib.lib().tg_version()


def test_known_answer_single_pendulum():
    """examples/papers/tase2012/pend-single-step.py:32-41 through the drop-in MidpointVI."""
    import trep_amd as T
    g = golden("known_answer_pendulum")
    s = T.System()
    s.import_frames([T.rx('theta', name='pend_angle'), [T.tz(-1.0, name='pend_mass', mass=1.0)]])
    T.potentials.Gravity(s, (0, 0, -9.8))
    T.forces.ConfigForce(s, 'theta', 'theta-torque')
    mvi = T.MidpointVI(s)
    mvi.initialize_from_state(0.0, np.array([0.2]), np.array([0.5]))
    assert mvi.step(0.1, np.array([0.8])) == 2
    assert abs(mvi.q2[0] - 0.2471361941555716) < 1e-13
    assert abs(mvi.q2[0] - g["q2"][0]) < 1e-14
    assert abs(mvi.p2[0] - g["p2"][0]) < 1e-14
    assert abs(mvi.t1 - 0.0) < 1e-15 and abs(mvi.t2 - 0.1) < 1e-15
    assert abs(mvi.p1[0] - 0.5) < 1e-15 and abs(mvi.q1[0] - 0.2) < 1e-15


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_rollout_matches_reference(name):
    g = golden(name)
    system, d = build(name)
    trajs = trajectories(name)
    B = len(trajs)
    n = len(g[trajs[0][0] + "IT"])
    mvi = _batch(system, B)
    Q0 = np.array([t[1] for t in trajs])
    mvi.initialize_from_configs(0.0, Q0, DT, Q0)
    P0 = mvi.p2
    for b, (prefix, _, _, _) in enumerate(trajs):
        assert relerr(P0[b], g[prefix + "P"][0]) < 1e-12
    U = np.array([t[2] for t in trajs])
    K = np.array([t[3] for t in trajs])
    X = mvi.rollout(n, DT, U, K)
    iters, status = mvi.status()
    assert (status == 0).all()
    nq, nd = d.n_configs, d.n_dyn
    lam = mvi.lambda1
    for b, (prefix, _, _, _) in enumerate(trajs):
        assert relerr(X[b, :, :nq], g[prefix + "Q"]) < TOL, name
        # observed on the round-5 library over all 18 systems (tools/observed_tolerances.py): q <= 3.7e-13, p <= 1.3e-12, lambda1 <= 2.8e-11
        # (the scissor lift: the multipliers are conditioned by 1 / dt^2); the wide random sweep (profiles/r05_stress_parity.txt, 1152
        # trajectories per system and kernel variant against the oracle) sees p <= 2.8e-11, lambda1 <= 4.7e-11
        assert relerr(X[b, :, nq:nq + nd], g[prefix + "P"]) < TOL, name
        assert relerr(lam[b], g[prefix + "LAM"][n]) < 3e-10
        assert abs(int(iters[b]) - int(g[prefix + "IT"].sum())) <= max(2, n // 100)
    t1, t2 = mvi.times()
    assert abs(t2 - (n + 1) * DT) < 1e-12 and abs(t1 - n * DT) < 1e-12
    mvi.close()


@pytest.mark.parametrize("name", ["pend_on_cart", "puppet40", "scissor4"])
def test_stepwise_api_matches_reference(name):
    """MidpointVI.step() called once per step (teacher-forced from the reference's states)."""
    import trep_amd
    g = golden(name)
    system, d = build(name)
    prefix, q0, U, K = trajectories(name)[0]
    Q, P, LAM, IT = g[prefix + "Q"], g[prefix + "P"], g[prefix + "LAM"], g[prefix + "IT"]
    mvi = trep_amd.MidpointVI(system)
    for k in [0, 1, 2, 9, 49, len(Q) - 2]:
        mvi.initialize_from_state((k + 1) * DT, Q[k], P[k], LAM[k])
        it = mvi.step((k + 2) * DT, U[k], K[k])
        assert abs(it - IT[k]) <= (0 if k < 100 else 1)
        assert relerr(mvi.q2, Q[k + 1]) < 1e-11
        assert relerr(mvi.p2, P[k + 1]) < 1e-10
        assert relerr(mvi.lambda1, LAM[k + 1]) < 1e-10       # (observed: <= 6.4e-12, scissor lift)
        assert relerr(mvi.q1, Q[k]) == 0.0 and relerr(mvi.p1, P[k]) == 0.0


def test_free_running_steps_pendulum_1000():
    """BASELINE configs[0]: examples/pendulum.py, 1 link, 1000 steps."""
    import trep_amd
    g = golden("pendulum1")
    system, d = build("pendulum1")
    mvi = trep_amd.MidpointVI(system)
    q0 = g["q0"]
    mvi.initialize_from_configs(0.0, q0, DT, q0)
    its = []
    for k in range(200):
        its.append(mvi.step(mvi.t2 + DT))
        assert abs(mvi.q2[0] - g["Q"][k + 1][0]) < TOL
    assert its == list(g["IT"][:200])
    b = trep_amd.BatchMidpointVI(system, 1)
    b.initialize_from_configs(0.0, q0[None, :], DT, q0[None, :])
    X = b.rollout(1000, DT)
    assert relerr(X[0, :, 0], g["Q"][:, 0]) < TOL


def test_residual_matches_oracle():
    from oracle.oracle import OracleMVI
    system, d = build("puppet40")
    g = golden("puppet40")
    rng = np.random.default_rng(5)
    B = 8
    mvi = _batch(system, B)
    q1 = np.repeat(g["b0_Q"][10][None, :], B, 0)
    q2 = q1.copy()
    q2[:, :d.n_dyn] += rng.uniform(-1e-3, 1e-3, (B, d.n_dyn))
    q2[:, d.n_dyn:] = g["b0_K"][10]
    p1 = np.repeat(g["b0_P"][10][None, :], B, 0)
    lam = np.repeat(g["b0_LAM"][10][None, :], B, 0)
    mvi.set_times(0.1, 0.11)
    mvi.q1, mvi.q2, mvi.p1, mvi.lambda1 = q1, q2, p1, lam
    f = mvi.calc_f()
    o = OracleMVI(d)
    for b in range(B):
        o.q1, o.q2, o.p1, o.lambda1 = q1[b], q2[b], p1[b], lam[b]
        o.set_times(0.1, 0.11)
        assert relerr(f[b], o.calc_f()) < 1e-12


@pytest.mark.parametrize("name,B,N", [("puppet40", 48, 40), ("scissor4", 33, 60), ("pend_on_cart", 67, 100),
                                      ("spring_arm", 37, 80), ("nonlinear_spring_arm", 37, 80), ("spring_link", 29, 60), ("wrench_arm", 41, 80), ("wrench_torque", 23, 60), ("wrench_spatial", 19, 60), ("wrench_body", 17, 60),
                                      ("extensor_tendon", 21, 100), ("dual_pendulums", 35, 120)])
def test_random_batch_matches_oracle(name, B, N):
    """Seeded random initial conditions / inputs, HIP vs oracle, ragged batch sizes."""
    from oracle.oracle import OracleMVI
    from trep_amd import systems
    system, d = build(name)
    rng = np.random.default_rng(99)
    nq, nd, nk, nu = d.n_configs, d.n_dyn, d.n_kin, d.n_inputs
    if name == "puppet40":
        Q0 = systems.puppet_initial_conditions(system, B, seed=7)
        K = systems.puppet_string_schedule(system, Q0[:, nd:], N, DT)
        U = np.zeros((B, N, 0))
    elif name == "scissor4":
        th = rng.uniform(0.03 * np.pi, 0.12 * np.pi, B)
        Q0 = np.array([systems.scissor_q(system, t) for t in th])
        K = np.zeros((B, N, 0)); U = np.zeros((B, N, 0))
    elif name == "pend_on_cart":
        Q0 = np.stack([rng.uniform(-1, 1, B), rng.uniform(-np.pi, np.pi, B)], 1)
        U = rng.standard_normal((B, N, 1)) * 2.0
        K = np.zeros((B, N, 0))
    else:   # the synthetic systems of the spring / wrench types: random poses around the builder's, random inputs
        Q0 = system.q[None] + 0.3 * rng.standard_normal((B, nq))
        if name == "spring_link":
            Q0[:, system.get_config('e').index] = -1.0        # on the distance constraint
        U = rng.standard_normal((B, N, nu))
        K = Q0[:, None, nd:] + 0.2 * np.sin(3.0 * DT * np.arange(1, N + 1))[None, :, None] * np.ones((1, 1, nk))
    mvi = _batch(system, B)
    mvi.initialize_from_configs(0.0, Q0, DT, Q0)
    X = mvi.rollout(N, DT, U, K)
    iters, status = mvi.status()
    assert (status == 0).all()
    o = OracleMVI(d)
    for b in range(B):
        o.initialize_from_configs(0.0, Q0[b], DT, Q0[b])
        Xo, tot = o.rollout(N, DT, U[b], K[b])
        assert relerr(X[b], Xo) < TOL, (name, b)
        assert abs(tot - iters[b]) <= 1
    mvi.close()


@pytest.mark.parametrize("links,B,N", [(20, 5, 30), (36, 3, 20)])
def test_long_chain_matches_oracle(links, B, N):
    """Size edge: an n-link pendulum is one chain of n joints with n(n+1)/2 (body, config) items.  20 links use
    the 20-row register Gauss-Jordan, 36 links (nf > 32) the LDS Gauss-Jordan inside the rollout, and the
    per-trajectory LDS slice grows to ~80 KB (one wavefront per CU).  Includes first derivatives."""
    from oracle.oracle import OracleMVI
    from trep_amd import systems, descriptor
    system = systems.pendulum(links)
    d = descriptor.flatten(system)
    rng = np.random.default_rng(links)
    Q0 = rng.uniform(-0.6, 0.6, (B, links))
    mvi = _batch(system, B)
    mvi.initialize_from_configs(0.0, Q0, DT, Q0)
    X = mvi.rollout(N, DT, np.zeros((B, N, 0)), np.zeros((B, N, 0)))
    iters, status = mvi.status()
    assert (status == 0).all()
    mvi.calc_deriv1()
    o = OracleMVI(d)
    for b in range(B):
        o.initialize_from_configs(0.0, Q0[b], DT, Q0[b])
        Xo, tot = o.rollout(N, DT, np.zeros((N, 0)), np.zeros((N, 0)))
        assert relerr(X[b], Xo) < TOL, (links, b, relerr(X[b], Xo))
        # with this many links the rounding floor of the residual sits near the 1e-10 stopping tolerance, so the
        # last Newton iteration of a step is decided by rounding: counts may differ by up to one per step
        assert abs(tot - iters[b]) <= (1 if links <= 20 else N)
        o.calc_deriv1()
        for n in ("q2_dq1", "q2_dp1", "p2_dq1", "p2_dp1"):
            # derivatives are taken at the converged state, which itself agrees to ~1e-12, and the chain's sensitivity grows with its
            # length: observed 1.4e-9 at 20 links, 8.4e-8 at 36 (tools/observed_tolerances.py) -- the bounds are one decade above that
            assert relerr(mvi.deriv1(n)[b], o.deriv1(n)) < (1e-8 if links <= 20 else 1e-6), (links, b, n)
    mvi.close()


@pytest.mark.parametrize("segments,B,N", [(6, 7, 40), (8, 5, 30)])
def test_large_constrained_system_matches_oracle(segments, B, N):
    """Shape edge: scissor lifts with 13 / 17 bodies have constraints (so a Newton iteration sweeps the midpoint and the q2 poses
    in one dual pass) but more per-lane table rows than two trips of a wavefront hold, so they take the dual pass WITHOUT the
    one-phase-ahead table fetches (eval_both instead of eval_both_tab); 8 segments (nf = 33) also use the LDS Gauss-Jordan."""
    from oracle.oracle import OracleMVI
    from trep_amd import systems, descriptor
    system = systems.scissor_lift(segments)
    d = descriptor.flatten(system)
    rng = np.random.default_rng(segments)
    th = rng.uniform(0.04 * np.pi, 0.1 * np.pi, B)
    Q0 = np.array([systems.scissor_q(system, t) for t in th])
    mvi = _batch(system, B)
    mvi.initialize_from_configs(0.0, Q0, DT, Q0)
    X = mvi.rollout(N, DT, np.zeros((B, N, 0)), np.zeros((B, N, 0)))
    iters, status = mvi.status()
    assert (status == 0).all()
    o = OracleMVI(d)
    for b in range(B):
        o.initialize_from_configs(0.0, Q0[b], DT, Q0[b])
        Xo, tot = o.rollout(N, DT, np.zeros((N, 0)), np.zeros((N, 0)))
        assert relerr(X[b], Xo) < TOL, (segments, b, relerr(X[b], Xo))
    mvi.close()


def test_many_chains_matches_oracle():
    """Shape edge: 20 two-link chains hanging off the world -- more chains in a sweep round than the LDS chain
    schedule holds (16), so the sweep reads its schedule from the global tables; 40 bodies, nd = 40 > 32 (LDS
    Gauss-Jordan in the rollout)."""
    from oracle.oracle import OracleMVI
    from trep_amd import descriptor
    from test_kernel_emulation import _star
    system = _star(20, 2)
    d = descriptor.flatten(system)
    B, N = 5, 15
    rng = np.random.default_rng(8)
    Q0 = rng.uniform(-0.5, 0.5, (B, d.n_configs))
    mvi = _batch(system, B)
    mvi.initialize_from_configs(0.0, Q0, DT, Q0)
    X = mvi.rollout(N, DT, np.zeros((B, N, 0)), np.zeros((B, N, 0)))
    iters, status = mvi.status()
    assert (status == 0).all()
    o = OracleMVI(d)
    for b in range(B):
        o.initialize_from_configs(0.0, Q0[b], DT, Q0[b])
        Xo, tot = o.rollout(N, DT, np.zeros((N, 0)), np.zeros((N, 0)))
        assert relerr(X[b], Xo) < TOL, (b, relerr(X[b], Xo))
    mvi.close()


def test_full_size_properties_puppet():
    """BASELINE puppet size (B=8192, N=200): every trajectory converges, the DEL residual of the final
    state vanishes, and results do not depend on batch composition (bit-identical sub-batch)."""
    from trep_amd import systems
    from oracle.oracle import OracleMVI
    from trep_amd import descriptor
    system, d = build("puppet40")
    B, N = 8192, 200
    nd = d.n_dyn
    # the bench.py workload: 8192 DISTINCT initial conditions, except that the last 64 slots repeat the first 64
    Q0 = systems.puppet_initial_conditions(system, B, seed=20250 + 3)
    Q0[B - 64:] = Q0[:64]
    K = systems.puppet_string_schedule(system, Q0[:, nd:], N, DT)
    mvi = _batch(system, B)
    mvi.initialize_from_configs(0.0, Q0, DT, Q0)
    K_dev = mvi.device_array(K)
    X_dev = mvi.device_empty(B * (N + 1) * mvi.nX)
    mvi.rollout_device(N, DT, None, K_dev, X_dev)
    mvi.synchronize()
    iters, status = mvi.status()
    assert (status == 0).all()
    assert 2.0 <= iters.mean() / N <= 3.2   # reference: 2.57 Newton iterations per step
    f = mvi.calc_f()
    assert np.linalg.norm(f[:, :nd], axis=1).max() < 1e-10
    assert np.abs(f[:, nd:]).max() < 1e-10
    q2 = mvi.q2
    assert np.array_equal(q2[:64], q2[B - 64:])     # duplicates are bit-identical
    assert len(np.unique(np.round(q2[:B - 64], 9), axis=0)) == B - 64   # ... and the distinct ones stay distinct
    sub = _batch(system, 64)
    sub.initialize_from_configs(0.0, Q0[:64], DT, Q0[:64])
    sub.rollout(N, DT, None, K[:64])
    assert np.array_equal(sub.q2, q2[:64])          # independent of batch size / placement
    # three trajectories from the middle and the end of the batch against the oracle, whole state history
    X = mvi.download(X_dev, (B, N + 1, mvi.nX))
    o = OracleMVI(descriptor.flatten(system))
    for b in (1, 4099, B - 65):
        o.initialize_from_configs(0.0, Q0[b], DT, Q0[b])
        Xo, _ = o.rollout(N, DT, None, K[b])
        assert relerr(X[b], Xo) < TOL, b
    mvi.close(); sub.close()


def test_failure_statuses_and_edge_cases():
    import trep_amd
    system, d = build("pend_on_cart")
    mvi = _batch(system, 5)
    q0 = np.array([[0.1 * b, 1.0 + 0.1 * b] for b in range(5)])
    mvi.initialize_from_configs(0.0, q0, DT, q0)
    it, st = mvi.step(2 * DT, np.ones((5, 1)), None, max_iterations=0)
    assert (st == 1).all()                         # one Newton step is not enough: not converged
    mvi.initialize_from_configs(0.0, q0, DT, q0)
    it, st = mvi.step(2 * DT, np.ones((5, 1)), None)
    assert (st == 0).all() and (it >= 1).all()
    one = trep_amd.MidpointVI(system)
    one.initialize_from_configs(0.0, q0[0], DT, q0[0])
    with pytest.raises(trep_amd.ConvergenceError):
        one.step(2 * DT, [1.0], max_iterations=0)
    mvi.close()


@pytest.mark.parametrize("name,spec", _spec_cases(sorted(BUILDERS)))
def test_first_derivatives_match_reference(name, spec):
    """A_k / B_k ingredients: the twelve deriv1 arrays after a teacher-forced step -- generic kernels, and for the
    BASELINE systems also the system-specialised ones (the mode bits of tg_batch_info prove which ran)."""
    import trep_amd
    from common import D1
    g = golden(name)
    system, d = build(name)
    prefix, q0, U, K = trajectories(name)[0]
    Q, P, LAM = g[prefix + "Q"], g[prefix + "P"], g[prefix + "LAM"]
    steps = sorted(int(k.split("_")[-3]) for k in g if k.startswith(prefix + "d1_") and k.endswith("q2_dq1"))
    B = 3  # same case in every slot: also checks batch independence
    mvi = trep_amd.BatchMidpointVI(system, B, specialize=spec)
    for s_ in steps:
        k = s_ - 1
        mvi.initialize_from_state((k + 1) * DT, Q[k], P[k], LAM[k])
        it, st = mvi.step((k + 2) * DT, U[k] if U.shape[1] else None, K[k] if K.shape[1] else None)
        assert (st == 0).all()
        mvi.calc_deriv1()
        for n in D1:
            got = mvi.deriv1(n)
            assert relerr(got[0], g["%sd1_%d_%s" % (prefix, s_, n)]) < 1e-9, (name, s_, n)
            assert np.array_equal(got[0], got[2])
    _assert_kernels(mvi.kernel_info(), spec, ["rollout", "deriv1"])
    mvi.close()


def test_deriv1_accessors_dropin():
    """MidpointVI.q2_dq1(...) etc. keep the reference's indexing semantics (midpointvi.py:337-371)."""
    import trep_amd
    g = golden("pend_on_cart")
    system, d = build("pend_on_cart")
    mvi = trep_amd.MidpointVI(system)
    Q, P, LAM, U = g["b0_Q"], g["b0_P"], g["b0_LAM"], g["b0_U"]
    mvi.initialize_from_state(DT, Q[0], P[0], LAM[0])
    with pytest.raises(Exception):
        mvi.q2_dq1()
    mvi.step(2 * DT, U[0])
    ref = g["b0_d1_1_q2_dq1"]
    assert relerr(mvi.q2_dq1(), ref.T) < 1e-10
    x, th = system.get_config("x"), system.get_config("theta")
    assert abs(mvi.q2_dq1(th, x) - ref[0, 1]) < 1e-10
    assert relerr(mvi.p2_du1(), g["b0_d1_1_p2_du1"].T) < 1e-10
    assert mvi.q2_dk2().shape == (2, 0)


@pytest.mark.parametrize("name", ["pend_on_cart", "scissor4", "puppet40", "pendulum5", "spring_arm", "nonlinear_spring_arm", "plane_link", "wrench_arm", "puppet_forces", "wrench_torque", "wrench_spatial", "wrench_body", "damper_link", "spatial_loop", "mixed_loop"])
def test_dsystem_linearization_matches_reference(name):
    """DSystem.set(X[k],U[k],k,xk_hint=X[k+1]) -> f, fdx (A_k), fdu (B_k) vs the reference's DSystem."""
    import trep_amd
    from trep_amd import discopt
    g = golden(name)
    system, d = build(name)
    X, U = g["ds_X"], g["ds_U"]
    t = DT * np.arange(len(X))
    one = discopt.DSystem(trep_amd.MidpointVI(system), t)
    ks = [int(k) for k in g["ds_k"]]
    for k in ks:
        one.set(X[k], U[k], k, xk_hint=X[k + 1])
        assert relerr(one.f(), g["ds_%d_f" % k]) < 1e-10
        assert relerr(one.fdx(), g["ds_%d_A" % k]) < 1e-9
        assert relerr(one.fdu(), g["ds_%d_B" % k]) < 1e-9
    # batched: all captured k of the trajectory in one batch is not possible (different t), so
    # replicate one k across a small batch instead
    k = ks[1]
    bd = discopt.BatchDSystem(system, t, 4)
    it, st = bd.set(np.tile(X[k], (4, 1)), np.tile(U[k], (4, 1)), k, Xk_hint=np.tile(X[k + 1], (4, 1)))
    assert (st == 0).all()
    A, B = bd.linearize()
    assert relerr(bd.f()[3], g["ds_%d_f" % k]) < 1e-10
    assert relerr(A[3], g["ds_%d_A" % k]) < 1e-9 and relerr(B[0], g["ds_%d_B" % k]) < 1e-9
    lin = one.linearize_trajectory(X[:4], U[:3])
    assert lin.A.shape == (3, one.nX, one.nX) and lin.B.shape == (3, one.nX, one.nU)


@pytest.mark.parametrize("name,spec", _spec_cases(["pend_on_cart", "scissor4", "puppet40", "pendulum5", "spring_arm", "nonlinear_spring_arm", "plane_link", "wrench_arm", "puppet_forces", "wrench_torque", "wrench_spatial", "wrench_body", "damper_link", "spatial_loop", "mixed_loop"]))
def test_dsystem_second_order_matches_reference(name, spec):
    """fdxdx(z), fdxdu(z), fdudu(z) vs the reference DSystem (dsystem.py:320-386) for two z."""
    import trep_amd
    from trep_amd import discopt
    g = golden(name)
    system, d = build(name)
    X, U, Z = g["ds_X"], g["ds_U"], g["ds_Z"]
    t = DT * np.arange(len(X))
    one = discopt.DSystem(trep_amd.MidpointVI(system, specialize=spec), t)
    for k in [int(k) for k in g["ds_k"]]:
        one.set(X[k], U[k], k, xk_hint=X[k + 1])
        for zi in range(2):
            assert relerr(one.fdxdx(Z[zi]), g["ds_%d_fdxdx_%d" % (k, zi)]) < 1e-8, (name, k)
            assert relerr(one.fdxdu(Z[zi]), g["ds_%d_fdxdu_%d" % (k, zi)]) < 1e-8, (name, k)
            assert relerr(one.fdudu(Z[zi]), g["ds_%d_fdudu_%d" % (k, zi)]) < 1e-8, (name, k)
    _assert_kernels(one.varint._batch().kernel_info(), spec, ["rollout", "deriv2z"])
    k = int(g["ds_k"][1])
    bd = discopt.BatchDSystem(system, t, 3, specialize=spec)
    bd.set(np.tile(X[k], (3, 1)), np.tile(U[k], (3, 1)), k, Xk_hint=np.tile(X[k + 1], (3, 1)))
    xx, xu, uu = bd.second_order(np.stack([Z[0], Z[1], Z[0]]))
    assert relerr(xx[1], g["ds_%d_fdxdx_1" % k]) < 1e-8 and relerr(uu[2], g["ds_%d_fdudu_0" % k]) < 1e-8
    assert np.array_equal(xx[0], xx[2])
    _assert_kernels(bd.varint.kernel_info(), spec, ["rollout", "deriv2z"])


@pytest.mark.parametrize("name,spec", _spec_cases(["pend_on_cart", "scissor4", "puppet40", "puppet_basic", "spring_arm", "nonlinear_spring_arm", "plane_link", "wrench_arm", "puppet_forces", "wrench_torque", "wrench_spatial", "wrench_body", "damper_link", "spatial_loop", "mixed_loop"]))
def test_full_second_derivative_tensors_match_reference(name, spec):
    """MidpointVI.q2_dq1dq1() ... p2_dk2dk2(), lambda1_dq1dq1() ... accessors vs the reference's [A][B][out] tensors."""
    import trep_amd
    g = golden(name)
    system, d = build(name)
    prefix, q0, U, K = trajectories(name)[0]
    Q, P, LAM = g[prefix + "Q"], g[prefix + "P"], g[prefix + "LAM"]
    keys = [k for k in g if k.startswith(prefix + "d2_")]
    step = sorted(set(int(k.split("_")[-3]) for k in keys))[0]
    k0 = step - 1
    mvi = trep_amd.MidpointVI(system, specialize=spec)
    mvi.initialize_from_state((k0 + 1) * DT, Q[k0], P[k0], LAM[k0])
    mvi.step((k0 + 2) * DT, U[k0], K[k0])
    checked = n_lambda = 0
    for key in keys:
        parts = key.split("_")
        if int(parts[-3]) != step:
            continue
        nm = parts[-2].replace("l1", "lambda1") + "_" + parts[-1]
        got = getattr(mvi, nm)()
        assert got.shape == g[key].shape
        assert relerr(got, g[key]) < 1e-8, (name, nm)
        checked += 1
        n_lambda += nm.startswith("lambda1")
    assert checked >= 4 and (n_lambda > 0 or system.nc == 0)
    _assert_kernels(mvi._batch().kernel_info(), spec, ["rollout"])
    _assert_kernels(mvi._b2.kernel_info(), spec, ["deriv2z"])       # the unit contractions run on the accessor's own batch


def test_second_derivatives_undefined_with_linear_springs():
    """LinearSpring defines no V_dqdqdq in the reference (linearspring.c:86-88): _calc_deriv2 raises there; here the
    contraction entry points report TG_ERR_UNSUPPORTED and the drop-in accessor raises."""
    import trep_amd
    g = golden("spring_link")
    system, d = build("spring_link")
    mvi = trep_amd.MidpointVI(system)
    mvi.initialize_from_state(DT, g["b0_Q"][0], g["b0_P"][0], g["b0_LAM"][0])
    mvi.step(2 * DT, (), g["b0_K"][0])
    assert relerr(mvi.q2, g["b0_Q"][1]) < 1e-10
    assert relerr(mvi.q2_dq1(), g["b0_d1_1_q2_dq1"].T) < 1e-9
    with pytest.raises(Exception, match="LinearSpring"):
        mvi.q2_dq1dq1()


def test_hybrid_wrench_inputs_and_second_derivatives():
    """HybridWrench: input ordering, the configuration-dependent input columns and the input blocks of the second
    derivatives (D1D3fm2 / D2D3fm2) through the drop-in accessors."""
    import trep_amd
    g = golden("wrench_arm")
    system, d = build("wrench_arm")
    assert [u.name for u in system.inputs] == [str(n) for n in g["input_names"]]
    mvi = trep_amd.MidpointVI(system)
    mvi.initialize_from_state(DT, g["b0_Q"][0], g["b0_P"][0], g["b0_LAM"][0])
    mvi.step(2 * DT, g["b0_U"][0], g["b0_K"][0])
    assert relerr(mvi.q2, g["b0_Q"][1]) < 1e-10
    assert relerr(mvi.q2_du1(), g["b0_d1_1_q2_du1"].T) < 1e-9
    for nm in ("q2_dq1du1", "p2_dq1du1", "q2_du1du1", "p2_du1dk2", "q2_dp1du1", "q2_dq1dq1"):
        assert relerr(getattr(mvi, nm)(), g["b0_d2_1_" + nm]) < 1e-8, nm


def test_extrapolating_predictor_same_trajectory_fewer_iterations():
    """The opt-in warm start q2 + (q2 - q1) reaches the same root: trajectories agree with the reference-semantics
    rollout to solver tolerance, Newton iterations per step drop."""
    from trep_amd import systems
    system, d = build("puppet40")
    B, N = 64, 100
    nd = d.n_dyn
    Q0 = systems.puppet_initial_conditions(system, B, seed=3)
    K = systems.puppet_string_schedule(system, Q0[:, nd:], N, DT)
    out = {}
    for mode in ("reference", "extrapolate"):
        mvi = _batch(system, B)
        mvi.predictor = mode
        assert mvi.predictor == mode
        mvi.initialize_from_configs(0.0, Q0, DT, Q0)
        X = mvi.rollout(N, DT, None, K)
        iters, status = mvi.status()
        assert (status == 0).all()
        out[mode] = (X, iters.mean() / N)
        mvi.close()
    assert relerr(out["extrapolate"][0], out["reference"][0]) < 1e-9
    assert out["extrapolate"][1] < out["reference"][1] - 0.3
    with pytest.raises(ValueError):
        _batch(system, 1).predictor = "nonsense"


def test_dual_pendulums_first_order_only_like_the_reference():
    import trep_amd
    g = golden("dual_pendulums")
    system, d = build("dual_pendulums")
    mvi = trep_amd.MidpointVI(system)
    mvi.initialize_from_state(DT, g["b0_Q"][0], g["b0_P"][0], g["b0_LAM"][0])
    mvi.step(2 * DT)
    assert relerr(mvi.q2, g["b0_Q"][1]) < 1e-10 and relerr(mvi.p2_dq1(), g["b0_d1_1_p2_dq1"].T) < 1e-9
    with pytest.raises(Exception, match="LinearSpring"):     # the spring, not the damper: the reference raises here too
        mvi.q2_dq1dq1()


def _secondary_workload(name, B, N):
    """BASELINE configs 2 and 5 with the synthetic inputs of SURVEY.md section 8(d)."""
    from trep_amd import systems
    if name == "cart":
        system = systems.pend_on_cart()
        rng = np.random.default_rng(20250 + 2)
        Q0 = np.stack([rng.uniform(-1, 1, B), rng.uniform(-np.pi, np.pi, B)], 1)
        return system, Q0, rng.standard_normal((B, N, 1)) * 2.0
    system = systems.scissor_lift(4)
    rng = np.random.default_rng(20250 + 5)
    th = rng.uniform(0.03 * np.pi, 0.12 * np.pi, B)
    return system, np.array([systems.scissor_q(system, t) for t in th]), None


@pytest.mark.parametrize("name", ["cart", "scissor"])
def test_full_size_properties_cart_and_scissor(name):
    """BASELINE configs 2 (pend-on-cart, TEAM = 4: sixteen trajectories per wavefront, level sweep, shuffle pivots) and 5
    (scissor lift, eight holonomic constraints) at their full size B = 4096 x N = 200: every trajectory converges, the
    DEL residual of the final state vanishes, duplicated initial conditions are bit-identical wherever they sit in the
    batch, a sub-batch reproduces its trajectories bit for bit, and a sample agrees with the oracle to 1e-10."""
    from trep_amd import descriptor
    from oracle.oracle import OracleMVI
    B, N = 4096, 200
    system, Q0, U = _secondary_workload(name, B - 64, N)
    Q0 = np.concatenate([Q0, Q0[5:69]], 0)                      # 64 duplicates at the end of the batch
    U = None if U is None else np.concatenate([U, U[5:69]], 0)
    mvi = _batch(system, B)
    nd = mvi.nd
    mvi.initialize_from_configs(0.0, Q0, DT, Q0)
    X = mvi.rollout(N, DT, U, None)
    iters, status = mvi.status()
    assert (status == 0).all()
    f = mvi.calc_f()
    assert np.abs(f).max() < 1e-10
    assert np.array_equal(X[5:69], X[B - 64:])
    sub = _batch(system, 37)
    sub.initialize_from_configs(0.0, Q0[100:137], DT, Q0[100:137])
    Xs = sub.rollout(N, DT, None if U is None else U[100:137], None)
    assert np.array_equal(Xs, X[100:137])
    o = OracleMVI(descriptor.flatten(system))
    for b in (0, 1000, 4000):
        o.initialize_from_configs(0.0, Q0[b], DT, Q0[b])
        Xo, _ = o.rollout(N, DT, None if U is None else U[b], None)
        assert relerr(X[b], Xo) < TOL, (b, relerr(X[b], Xo))   # (observed: cart 5e-14, scissor lift 2.7e-12 over 200 steps)
    mvi.close(); sub.close()


def test_parameter_change_keeps_integrator_state():
    """The reference's integrator survives parameter writes (Gravity.gravity, Damping coefficients ...): they are
    plain attributes of the potential / force objects and MidpointVI only re-allocates on structure changes
    (trep/midpointvi.py:25).  Here: 40 steps, change gravity and damping, 40 more -- against the oracle doing the same."""
    import trep_amd
    from trep_amd import systems, descriptor
    from oracle.oracle import OracleMVI
    system = systems.pend_on_cart()
    mvi = trep_amd.MidpointVI(system)
    q0 = np.array([0.1, 0.7])
    mvi.initialize_from_configs(0.0, q0, DT, q0)
    o = OracleMVI(descriptor.flatten(system))
    o.initialize_from_configs(0.0, q0, DT, q0)
    u = lambda k: [0.5 * np.sin(0.1 * k)]
    for k in range(40):
        mvi.step(mvi.t2 + DT, u(k)); o.step(o.times()[1] + DT, u(k))
    grav = [p for p in system.potentials if hasattr(p, "gravity")][0]
    grav.gravity = (0.0, -3.7, 0.0)
    assert abs(mvi.t2 - 41 * DT) < 1e-12 and relerr(mvi.q2, o.q2) < TOL      # state survived the parameter write
    o2 = OracleMVI(descriptor.flatten(system))
    o2.initialize_from_state(o.times()[1], o.q2, o.p2, o.lambda1)
    o2.q1 = o.q1; o2.p1 = o.p1
    for k in range(40, 80):
        mvi.step(mvi.t2 + DT, u(k)); o2.step(o2.times()[1] + DT, u(k))
    assert relerr(mvi.q2, o2.q2) < TOL and relerr(mvi.p2, o2.p2) < TOL
    # and it did change the dynamics: with the old gravity the same 40 steps end elsewhere
    for k in range(40, 80):
        o.step(o.times()[1] + DT, u(k))
    assert np.abs(o.q2 - o2.q2).max() > 1e-3
    # a cached batch engine follows the change as well
    eng = trep_amd.BatchMidpointVI(system, 2)
    eng.initialize_from_configs(0.0, np.stack([q0, q0]), DT, np.stack([q0, q0]))
    eng.step(2 * DT, np.ones((2, 1)), None)
    grav.gravity = (0.0, -9.8, 0.0)
    eng.step(3 * DT, np.ones((2, 1)), None)
    o3 = OracleMVI(descriptor.flatten(system))
    o3.initialize_from_state(2 * DT, eng.q1[0], eng.p1[0])
    o3.step(3 * DT, [1.0])
    assert relerr(eng.q2[0], o3.q2) < TOL
    eng.close()


def test_rccl_communicator_single_rank():
    """The torch-free collective path of bench.py (C ABI tg_comm_*, RCCL through dlopen) with a world of one rank:
    unique id, communicator, all-gather of device rows, host-scalar reductions, barrier."""
    from trep_amd import rccl, _lib
    uid = rccl.Communicator.new_unique_id()
    assert len(uid) == rccl.ID_BYTES
    comm = rccl.Communicator(0, 1, 0, uid)
    try:
        comm.barrier()
        assert comm.max(3.5) == 3.5 and comm.sum(2.0) == 2.0
        rows = np.arange(12.0).reshape(4, 3)
        assert np.array_equal(comm.all_gather_rows(rows, total_rows=4), rows)
    finally:
        comm.close()


@pytest.mark.parametrize("name", ["puppet40", "scissor4", "pend_on_cart", "spring_arm"])
def test_specialised_kernel_matches_generic_and_reference(name):
    """The system-specialised rollout kernel (trep_amd/specialize.py: the schedule compiled into the kernel) is the same
    template source as the generic kernel: identical Newton iteration counts and states equal up to the compiler's
    FMA contraction (<= 1e-12 relative over 100 steps); both within 1e-10 of the reference goldens."""
    import trep_amd
    system, d = build(name)
    N = 100
    prefix, q0, U, K = trajectories(name)[0]
    g = golden(name)
    out = []
    for mode in (False, True):
        m = trep_amd.BatchMidpointVI(system, 3, specialize=mode)
        assert (m._specialized is not None) == mode
        Q0 = np.stack([q0, q0, q0])
        m.initialize_from_configs(0.0, Q0, DT, Q0)
        X = m.rollout(N, DT, None if U.shape[1] == 0 else np.stack([U[:N]] * 3), None if K.shape[1] == 0 else np.stack([K[:N]] * 3))
        it, st = m.status()
        assert (st == 0).all()
        out.append((X, it))
        m.close()
    assert np.array_equal(out[0][1], out[1][1])
    assert relerr(out[0][0], out[1][0]) < 1e-12
    nq = d.n_configs
    for X, _ in out:
        assert relerr(X[0][:, :nq], g[prefix + "Q"][:N + 1]) < TOL
        assert np.array_equal(X[0], X[2])


def _oracle_lu(A, b):
    import ctypes
    from oracle import oracle as O
    L = O.lib()
    n = len(b)
    A = np.ascontiguousarray(A, dtype=float); b = np.ascontiguousarray(b, dtype=float)
    x = np.zeros(n); idx = np.zeros(n, dtype=np.int32)
    L.to_debug_lu.restype = ctypes.c_int
    rc = L.to_debug_lu(ctypes.c_int(n), A.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p),
                       x.ctypes.data_as(ctypes.c_void_p), idx.ctypes.data_as(ctypes.c_void_p))
    return rc, x, idx


def _device_solve(A, b, exact):
    import ctypes
    from trep_amd import _lib
    L = _lib.lib()
    n = len(b)
    aug = np.ascontiguousarray(np.hstack([A, b[:, None]]), dtype=float)
    x = np.zeros(n); piv = np.zeros(n, dtype=np.int32); st = np.zeros(1, dtype=np.int32)
    _lib.check(L.tg_debug_solve(0, n, int(exact) if exact in (0, 1, 2) else (1 if exact else 0), aug.ctypes.data, x.ctypes.data, piv.ctypes.data, st.ctypes.data))
    return int(st[0]), x, piv


def _pivot_cases(rng):
    out = []
    for n in (3, 7, 12, 22, 28, 32):
        out.append(("random", rng.standard_normal((n, n))))
        # near ties: pairs of rows that differ by ~1e-9 relative in the pivot column after scaling
        A = rng.standard_normal((n, n))
        A[1] = A[0] * (1.0 + 1e-9 * rng.standard_normal(n)); A[1, 0] = A[0, 0] * (1.0 - 3e-10)
        if n > 4:
            A[4] = A[3] * (1.0 + 1e-9 * rng.standard_normal(n)); A[4, 1] = A[3, 1] * (1.0 + 2e-10)
        A += 1e-3 * rng.standard_normal((n, n)) * (np.arange(n)[:, None] > 4)
        out.append(("near ties", A))
        # exact ties: integer-valued rows with equal scale factors and equal magnitudes in the first column
        A = rng.integers(-3, 4, (n, n)).astype(float) + 4.0 * np.eye(n)
        A[:, 0] = 4.0 * np.where(np.arange(n) % 2 == 0, 1.0, -1.0); A[np.arange(n), np.arange(n)] = 4.0
        out.append(("exact ties", np.where(np.abs(A) > 4.0, 4.0, A)))
        # the structural case of the Newton systems: rows whose largest entries share a column scale to 1 +- 1 ulp
        A = rng.standard_normal((n, n))
        A[:, 0] = 10.0 * (1.0 + rng.random(n))
        out.append(("row maxima in one column", A))
    return out


def test_newton_solver_exact_pivot_rule_matches_reference_lu():
    """gj_rows_exact (tg_batch_set_pivot_rule(b, 1)) against the reference's LU_decomp (math-code.c:337-432, restated in the
    oracle): the same pivot ROW for every column -- random matrices, near ties (scaled candidates within 1e-9 relative),
    exact ties (the reference's strict `>` scan keeps the first row of its current, swapped, order), rows whose largest
    entries share a column (scaled candidates 1 +- 1 ulp) -- and the same verdict around the 1e-20 singularity threshold."""
    rng = np.random.default_rng(7)
    solved = 0
    for kind, A in _pivot_cases(rng):
        n = len(A)
        b = rng.standard_normal(n)
        rc, xo, idx = _oracle_lu(A, b)
        st, xd, piv = _device_solve(A, b, exact=True)
        if rc != 0:
            assert st == 2
            continue
        assert st == 0
        assert np.array_equal(piv, idx), (kind, n, piv, idx)
        assert relerr(xd, xo) < 1e-9 * max(1.0, np.linalg.cond(A) * 1e-6), (kind, n)
        solved += 1
    assert solved >= 20
    for eps, singular in ((1e-21, True), (1e-19, False), (0.99999e-20, True), (1.00001e-20, False)):
        A = np.eye(5); A[4, 4] = eps; A[4, 0] = 1.0
        b = np.ones(5)
        rc, xo, idx = _oracle_lu(A, b)
        st, xd, piv = _device_solve(A, b, exact=True)
        assert (rc != 0) == singular and (st == 2) == singular, (eps, rc, st)


def test_newton_solver_default_pivot_rule():
    """The default (single-precision ranking) solver: every pivot row is an arg-max of the scaled candidates to within the
    ranking resolution 2^-17 (the reference's own choice among candidates that close is decided by the last ulp: even a random
    3 x 3 matrix has two rows whose largest entry sits in column 0, both scaling to 1 +- 1 ulp), the solve is backward stable,
    and it gives the reference's solution to rounding; singular verdict away from the threshold."""
    rng = np.random.default_rng(8)
    for kind, A in _pivot_cases(rng):
        n = len(A)
        b = rng.standard_normal(n)
        rc, xo, idx = _oracle_lu(A, b)
        st, xd, piv = _device_solve(A, b, exact=False)
        if rc != 0:
            continue
        assert st == 0 and sorted(piv) == list(range(n))
        # every pivot is an arg-max of the scaled candidates up to the ranking resolution (2^-17): replay the elimination
        M = A.copy(); scale = 1.0 / np.abs(A).max(axis=1); unused = np.ones(n, dtype=bool)
        for k in range(n):
            cand = np.where(unused, np.abs(M[:, k]) * scale, -1.0)
            assert cand[piv[k]] >= cand.max() * (1.0 - 2.0 ** -16), (kind, n, k, piv[k], int(cand.argmax()))
            r = piv[k]; unused[r] = False
            others = np.arange(n) != r
            M[others] -= np.outer(M[others, k] / M[r, k], M[r])
        # a backward-stable solve: small residual whatever the conditioning (the near-tie matrices have cond ~ 1e10) ...
        res = np.abs(A.dot(xd) - b).max() / (np.abs(A).sum(axis=1).max() * np.abs(xd).max() + np.abs(b).max())
        assert res < 1e-13, (kind, n, res)
        if kind != "near ties":   # ... and the reference's solution where the matrix is well conditioned
            assert relerr(xd, xo) < 1e-9 * max(1.0, np.linalg.cond(A) * 1e-6), (kind, n, relerr(xd, xo))
    for eps, singular in ((1e-21, True), (1e-19, False)):
        A = np.eye(5); A[4, 4] = eps; A[4, 0] = 1.0
        st, xd, piv = _device_solve(A, np.ones(5), exact=False)
        assert (st == 2) == singular


def test_newton_solver_panel_variant_follows_the_default_rule():
    """gj_panel (full-wave teams, 17..31 unknowns: panels of four columns, trailing update on the matrix cores) is the default rule
    in another arithmetic order: on every test matrix -- sizes that are and are not multiples of four, near ties, exact ties, shared
    column maxima, KKT-shaped systems with a zero block -- each pivot is an arg-max of the scaled candidates up to the ranking
    resolution, the solve is backward stable, the solution is the oracle's LU solution and gj_rows' to rounding, and away from
    near-ties the pivot rows are gj_rows' rows; the singular verdict is the same."""
    rng = np.random.default_rng(81)
    cases = []
    for n in (17, 18, 20, 23, 24, 26, 28, 29, 31):
        for kind, A in _pivot_cases(rng):
            if len(A) == 28:
                B = A if n == 28 else rng.standard_normal((n, n)) if kind == "random" else None
                if B is not None:
                    cases.append((kind, B))
        # KKT shape: [[M, -C'], [C, 0]] with sparse constraint rows, the Newton matrix of a constrained step
        nc = 6 if n > 20 else 3
        nd = n - nc
        M = rng.standard_normal((nd, nd)) * 0.3 + np.diag(2.0 + rng.random(nd))
        C = rng.standard_normal((nc, nd)) * (rng.random((nc, nd)) < 0.35)
        C[np.arange(nc), rng.permutation(nd)[:nc]] = 1.0
        cases.append(("kkt", np.block([[M, -C.T], [C, np.zeros((nc, nc))]])))
    for kind, A in cases:
        n = len(A)
        b = rng.standard_normal(n)
        rc, xo, idx = _oracle_lu(A, b)
        st, xd, piv = _device_solve(A, b, exact=2)
        st0, x0, piv0 = _device_solve(A, b, exact=0)
        assert (st == 0) == (rc == 0) and st == st0, (kind, n, st, st0, rc)
        if rc != 0:
            continue
        assert sorted(piv) == list(range(n)), (kind, n, piv)
        M = A.copy(); scale = 1.0 / np.abs(A).max(axis=1); unused = np.ones(n, dtype=bool)
        for k in range(n):
            cand = np.where(unused, np.abs(M[:, k]) * scale, -1.0)
            assert cand[piv[k]] >= cand.max() * (1.0 - 2.0 ** -16), (kind, n, k, piv[k], int(cand.argmax()))
            r = piv[k]; unused[r] = False
            others = np.arange(n) != r
            M[others] -= np.outer(M[others, k] / M[r, k], M[r])
        res = np.abs(A.dot(xd) - b).max() / (np.abs(A).sum(axis=1).max() * np.abs(xd).max() + np.abs(b).max())
        assert res < 1e-13, (kind, n, res)
        if kind != "near ties":
            tol = 1e-9 * max(1.0, np.linalg.cond(A) * 1e-6)
            assert relerr(xd, xo) < tol and relerr(xd, x0) < tol, (kind, n, relerr(xd, xo), relerr(xd, x0))
        if kind in ("random", "kkt"):
            assert np.array_equal(piv, piv0), (kind, n, piv, piv0)
    for eps, singular in ((1e-21, True), (1e-19, False)):
        A = np.eye(20); A[19, 19] = eps; A[19, 0] = 1.0
        st, xd, piv = _device_solve(A, np.ones(20), exact=2)
        assert (st == 2) == singular


@pytest.mark.parametrize("spec", [False, True])
def test_exact_pivot_rollout_agrees_with_default(spec):
    """A puppet rollout under both pivot rules: same Newton iteration counts, states equal to 1e-11, and the exact rule within
    the usual 1e-10 of the reference golden.  spec=True runs k_spec<0, 0> and k_spec<0, 1> (the specialised kernels of the two
    rules), spec=False the generic ones."""
    import trep_amd
    system, d = build("puppet40")
    prefix, q0, U, K = trajectories("puppet40")[0]
    g = golden("puppet40")
    N = 100
    out = []
    for exact in (False, True):
        m = trep_amd.BatchMidpointVI(system, 2, specialize=spec)
        m.exact_pivot = exact
        Q0 = np.stack([q0, q0])
        m.initialize_from_configs(0.0, Q0, DT, Q0)
        X = m.rollout(N, DT, None, np.stack([K[:N]] * 2))
        it, st = m.status()
        assert (st == 0).all()
        out.append((X, it))
        info = m.kernel_info()
        _assert_kernels(info, spec, ["rollout"])
        assert info["exact_pivot"] == exact
        m.close()
    assert np.array_equal(out[0][1], out[1][1])
    assert relerr(out[0][0], out[1][0]) < 1e-11
    assert relerr(out[1][0][0][:, :d.n_configs], g[prefix + "Q"][:N + 1]) < TOL


def test_small_batch_step_mirror_is_invalidated_by_every_other_write():
    """tg_batch_step of a small batch returns (q2, p2, lambda1, iterations, status) in one copy and later reads are answered from
    that host mirror; anything else that changes the batch (a field write, a rollout, restore, a derivative launch) must drop it."""
    import trep_amd
    system, d = build("pend_on_cart")
    q0 = np.array([[0.1, 0.5], [0.2, -0.4], [0.0, 1.0]])
    a = trep_amd.BatchMidpointVI(system, 3)
    b = trep_amd.BatchMidpointVI(system, 3)
    for m in (a, b):
        m.initialize_from_configs(0.0, q0, DT, q0)
    U = np.array([[0.3], [-0.2], [0.0]])
    for k in range(5):
        ia, sa = a.step(a.times()[1] + DT, U)
        assert (sa == 0).all()
    Xb = b.rollout(5, DT, np.repeat(U[:, None, :], 5, axis=1), None)      # the same five steps as one device rollout
    # (t2 + DT) - t2 is not DT to the last bit, so the two paths agree to rounding, not bit for bit
    assert relerr(a.q2, Xb[:, 5, :2]) < 1e-12 and relerr(a.p2, b.p2) < 1e-12
    it2, st2 = a.status()
    assert np.array_equal(it2, ia)
    a.snapshot()
    q_new = a.q2 + 0.25
    a.q2 = q_new                                   # field write: the mirror must not answer the next read
    assert np.array_equal(a.q2, q_new)
    a.restore()
    assert relerr(a.q2, Xb[:, 5, :2]) < 1e-12
    a.step(a.times()[1] + DT, U)
    q_step = a.q2.copy()
    a.rollout(3, DT, np.repeat(U[:, None, :], 3, axis=1), None)
    assert not np.array_equal(a.q2, q_step)        # the rollout's state, not the mirrored step's
    a.close(); b.close()


def _newton_plan(mvi):
    from trep_amd import _lib
    L = _lib.lib()
    out = np.zeros(8, dtype=np.int32)
    _lib.check(L.tg_system_newton_plan(mvi._sys_h, out.ctypes.data, None, None))
    nf = int(out[5])
    pat = np.zeros((nf, nf), dtype=np.uint8)
    tab = np.zeros(128, dtype=np.int32)
    _lib.check(L.tg_system_newton_plan(mvi._sys_h, out.ctypes.data, pat.ctypes.data, tab.ctypes.data))
    return dict(ok=int(out[0]), groups=int(out[1]), ng=int(out[2]), nb=int(out[3]), t=int(out[4]), nf=nf, nd=int(out[6])), pat.astype(bool), tab


def _kernel_newton_solve(mvi, aug, skip_structured=False):
    from trep_amd import _lib
    aug = np.ascontiguousarray(aug, dtype=float)
    n, nf = aug.shape[0], aug.shape[1]
    x = np.zeros((n, nf)); path = np.zeros(n, dtype=np.int32)
    _lib.check(_lib.lib().tg_batch_debug_newton_solve(mvi._h, n, 1 if skip_structured else 0, aug.ctypes.data, x.ctypes.data, path.ctypes.data))
    return x, path


def _newton_like(rng, pat, nd, dt=0.01):
    """A matrix with the structure of the DEL Newton matrix (midpointvi.c:577-670): -M/dt + O(1) on the config block (M symmetric
    positive definite with the pattern's sparsity), Dh2 / -Dh1^T borders with Dh1 close to Dh2, zero constraint block."""
    nf = len(pat)
    L = rng.standard_normal((nd, nd)) * pat[:nd, :nd]
    M = 0.2 * (L + L.T) * pat[:nd, :nd]
    M[np.arange(nd), np.arange(nd)] = np.abs(M).sum(axis=1) + 0.5 + rng.random(nd)       # diagonally dominant: positive definite
    A = np.zeros((nf, nf))
    A[:nd, :nd] = -M / dt + 0.3 * rng.standard_normal((nd, nd)) * pat[:nd, :nd]
    D = rng.standard_normal((nf - nd, nd)) * pat[nd:, :nd]
    A[nd:, :nd] = D
    A[:nd, nd:] = -(D + 1e-3 * rng.standard_normal(D.shape) * pat[nd:, :nd]).T
    return A


@pytest.mark.parametrize("name", ["puppet40", "puppet_basic", "scissor4", "ladder_point", "ladder_mixed"])
def test_structured_newton_solve_matches_the_pivoting_solvers(name):
    """The structured solve of the specialised rollout kernels (csrc/bbd.hpp: blocks of the bordered-block-diagonal plan eliminated
    side by side without a pivot search, then the border system, then back-substitution) against the reference's LU_decomp /
    LU_solve_vec (math-code.c:337-461, the oracle's restatement) and numpy on matrices with the system's own Newton pattern; the
    same systems through the kernel's pivoting solver; a zero pivot inside a block (nonsingular matrix: the guard hands over to
    the pivoting solver, same solution); a singular matrix (reported singular, as before)."""
    import trep_amd
    system, _ = build(name)
    mvi = trep_amd.BatchMidpointVI(system, 1, specialize=True)
    plan, pat, tab = _newton_plan(mvi)
    assert plan["ok"] == 1 and plan["groups"] >= 2, plan
    nf, nd = plan["nf"], plan["nd"]
    rng = np.random.default_rng(2024)
    mats = [_newton_like(rng, pat, nd) for _ in range(48)]
    rhs = [rng.standard_normal(nf) * np.where(np.arange(nf) < nd, 1.0, 1e-3) for _ in mats]
    aug = np.array([np.hstack([A, b[:, None]]) for A, b in zip(mats, rhs)])
    x, path = _kernel_newton_solve(mvi, aug)
    assert (path == 1).all(), path
    x2, path2 = _kernel_newton_solve(mvi, aug, skip_structured=True)
    assert (path2 == 2).all(), path2
    for A, b, xs, xp in zip(mats, rhs, x, x2):
        rc, xo, _ = _oracle_lu(A, b)
        assert rc == 0
        xn = np.linalg.solve(A, b)
        scale = np.abs(xn).max()
        assert np.abs(xs - xo).max() < 1e-10 * scale and np.abs(xs - xn).max() < 1e-10 * scale, (np.abs(xs - xo).max(), scale)
        assert np.abs(xp - xo).max() < 1e-10 * scale
        res = np.abs(A.dot(xs) - b).max() / (np.abs(A).sum(axis=1).max() * np.abs(xs).max() + np.abs(b).max())
        assert res < 1e-13, res
    # a zero pivot inside a block: rows / columns of two coupled own configs carry a [[0, m], [m, 0]] block (nonsingular)
    own = [((tab[i] & 0xFF) - 1) for i in range(16) if i < plan["ng"] and (tab[i] & 0xFF)]
    a, c = [(i, j) for i in own for j in own if i < j and pat[i, j]][0]
    A = mats[0].copy(); b = rhs[0]
    A[a, a] = 0.0; A[c, c] = 0.0; A[a, c] = A[c, a] = -300.0
    xg, pg = _kernel_newton_solve(mvi, np.hstack([A, b[:, None]])[None])
    assert pg[0] == 2, pg
    xn = np.linalg.solve(A, b)
    assert np.abs(xg[0] - xn).max() < 1e-10 * np.abs(xn).max()
    # a tiny but non-zero pivot (2^-30 of the row's scale) must not be accepted either
    A = mats[1].copy(); b = rhs[1]
    A[a, a] = -300.0 * 2.0 ** -30; A[a, c] = A[c, a] = -300.0
    xg, pg = _kernel_newton_solve(mvi, np.hstack([A, b[:, None]])[None])
    xn = np.linalg.solve(A, b)
    assert pg[0] == 2 and np.abs(xg[0] - xn).max() < 1e-9 * np.abs(xn).max(), (pg, np.abs(xg[0] - xn).max())
    # singular: the last constraint's force direction is zero (a zero column)
    A = mats[2].copy(); b = rhs[2]
    A[:, nf - 1] = 0.0
    _, ps = _kernel_newton_solve(mvi, np.hstack([A, b[:, None]])[None])
    rc, _, _ = _oracle_lu(A, b)
    assert ps[0] == -1 and rc != 0, (ps, rc)


def test_packed_newton_image_and_item_form_variants(monkeypatch):
    """Two compile-time variants of the specialised puppet kernel against the default one.  -DTG_BBD_PACKED (opt-in build of the specialised puppet kernel, compiled here by hipcc): the Newton matrix written straight into the
    structured solve's own row order (csrc/bbd.hpp, BbdPacked) instead of the dense image.  The solver hook on the system's own pattern
    (dense input scattered through the plan's map), the fallback after a failed guard (the packed image unpacked for the pivoting
    solver) and a 100-step rollout against the default kernel: same Newton iteration counts, states equal to 1e-12."""
    import trep_amd
    from trep_amd import specialize, systems
    system, _ = build("puppet40")
    B, N = 32, 100
    Q0 = systems.puppet_initial_conditions(system, B, seed=9)
    K = systems.puppet_string_schedule(system, Q0[:, system.nQd:], N, DT)
    runs = []
    for packed in (False, True, None):
        if packed:
            monkeypatch.setenv("TREPAMD_SPEC_FLAGS", specialize.DEFAULT_FLAGS + " -DTG_BBD_PACKED")
        elif packed is None:        # ... and the (body, config) item form of rounds 1-4 with the composite matrix: the same kernel source without eval_world
            monkeypatch.setenv("TREPAMD_SPEC_FLAGS", specialize.DEFAULT_FLAGS + " -DTG_NO_WEV")
        mvi = trep_amd.BatchMidpointVI(system, B, specialize=True)
        mvi.initialize_from_configs(0.0, Q0, DT, Q0)
        X = mvi.rollout(N, DT, None, K)
        it, st = mvi.status()
        assert (st == 0).all()
        _assert_kernels(mvi.kernel_info(), True, ("rollout",))
        runs.append((X, it))
        if packed:
            one = trep_amd.BatchMidpointVI(system, 1, specialize=True)
            plan, pat, tab = _newton_plan(one)
            nf, nd = plan["nf"], plan["nd"]
            rng = np.random.default_rng(31)
            mats = [_newton_like(rng, pat, nd) for _ in range(16)]
            rhs = [rng.standard_normal(nf) * np.where(np.arange(nf) < nd, 1.0, 1e-3) for _ in mats]
            aug = np.array([np.hstack([A, b[:, None]]) for A, b in zip(mats, rhs)])
            x, path = _kernel_newton_solve(one, aug)
            assert (path == 1).all(), path
            for A, b, xs in zip(mats, rhs, x):
                xn = np.linalg.solve(A, b)
                assert np.abs(xs - xn).max() < 1e-10 * np.abs(xn).max()
            own = [((tab[i] & 0xFF) - 1) for i in range(16) if i < plan["ng"] and (tab[i] & 0xFF)]
            a, c = [(i, j) for i in own for j in own if i < j and pat[i, j]][0]
            A = mats[0].copy(); b = rhs[0]
            A[a, a] = 0.0; A[c, c] = 0.0; A[a, c] = A[c, a] = -300.0          # a zero pivot inside a block: the guard hands over
            xg, pg = _kernel_newton_solve(one, np.hstack([A, b[:, None]])[None])
            xn = np.linalg.solve(A, b)
            assert pg[0] == 2 and np.abs(xg[0] - xn).max() < 1e-10 * np.abs(xn).max(), pg
            one.close()
        mvi.close()
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][1], runs[2][1])
    assert relerr(runs[0][0], runs[1][0]) < 1e-12
    assert relerr(runs[0][0], runs[2][0]) < 1e-11       # world-frame against item form: a different (algebraically equal) evaluation


def test_structured_solve_reports_its_fallbacks():
    """tg_batch_solver_fallbacks: from the benchmark's dt = 0.01 down to 1e-4 no Newton system of a puppet rollout fails a pivot guard; at
    dt = 1e-5 the constraints' Schur pivots (which scale like dt^2 |Dh|^2 / m against |Dh|) fall below the 2^-20 guard and EVERY system
    goes to the pivoting solver (tools/probe_fallbacks.py: 0 / 0 / 0 / all / all at 1e-2 ... 1e-6) -- reported, and still the oracle's
    trajectory."""
    import trep_amd
    from trep_amd import systems, descriptor
    from oracle.oracle import OracleMVI
    system, d = build("puppet40")
    B, N = 16, 20
    Q0 = systems.puppet_initial_conditions(system, B, seed=3)
    for dt, expect_fallbacks in ((DT, False), (1e-4, False), (1e-5, True)):
        K = systems.puppet_string_schedule(system, Q0[:, system.nQd:], N, dt)
        mvi = trep_amd.BatchMidpointVI(system, B, specialize=True)
        mvi.initialize_from_configs(0.0, Q0, dt, Q0)
        X = mvi.rollout(N, dt, None, K)
        it, st = mvi.status()
        fb = mvi.solver_fallbacks()
        assert (st == 0).all()
        if expect_fallbacks:
            assert (fb == it).all(), (fb, it)          # every Newton system of every trajectory
        else:
            assert (fb == 0).all(), fb
        o = OracleMVI(d)
        o.initialize_from_configs(0.0, Q0[0], dt, Q0[0])
        Xo, _ = o.rollout(N, dt, None, K[0])
        nq = d.n_configs
        assert relerr(X[0][:, :nq], Xo[:, :nq]) < TOL
        assert relerr(X[0][:, nq:], Xo[:, nq:]) < (TOL if dt == DT else 1e-7)       # (momenta and rates are conditioned by 1 / dt)
        mvi.close()


def test_structured_newton_solve_is_what_the_rollout_runs():
    """The puppet rollout with the structured solve (default) and with the pivoting solver (exact pivot rule: the structured solve
    is compiled out of that kernel) take the same number of Newton iterations and agree to 1e-10 over 200 steps."""
    import trep_amd
    from trep_amd import systems
    system, _ = build("puppet40")
    B, N = 64, 200
    Q0 = systems.puppet_initial_conditions(system, B, seed=5)
    K = systems.puppet_string_schedule(system, Q0[:, system.nQd:], N, DT)
    out = []
    for exact in (False, True):
        mvi = trep_amd.BatchMidpointVI(system, B, specialize=True)
        mvi.exact_pivot = exact
        mvi.initialize_from_configs(0.0, Q0, DT, Q0)
        X = mvi.rollout(N, DT, None, K)
        it, st = mvi.status()
        assert (st == 0).all()
        out.append((X, it))
    assert relerr(out[0][0], out[1][0]) < TOL
    assert np.abs(out[0][1] - out[1][1]).max() <= 1, (out[0][1], out[1][1])
