"""The host layer of the batch ABI on the device (csrc/trepamd.hip outside its kernels): which calls it refuses and how, that a
refused call leaves the batch alone, that the two staging paths of tg_batch_step and the forwarded entry points agree bit for bit,
and that batches can be created, used through every lazily allocated buffer and destroyed over and over.  Every expected string is the
library's own text; nothing here provokes a fault: ordinary calls and ordinary refusals only."""

import numpy as np
import pytest

from common import BUILDERS, build, starts
from trep_amd import _lib

pytestmark = pytest.mark.gpu
DT = 0.01
INVALID, UNSUPPORTED, STATE = -1, -3, -4          # TG_ERR_* of include/trep_amd.h
NOT_SOLVED = "Integrator has not solved the next time step yet."
NO_SECOND = "V_dqdqdq() is undefined for LinearSpring (as in the reference): no second derivatives"
BY_TRAJECTORY = "a by-trajectory step-size list takes one-step launches only"
TOO_LONG = "rollout longer than the step-size list"
_starts = {}


def _case(name, B, N=3):
    """(d, Q0, Q1, U [B][N][nu], K [B][N][nk]) of B recorded starts of a system, computed once."""
    if (name, B, N) not in _starts:
        _, d = build(name)
        _starts[(name, B, N)] = (d,) + starts(name, d, B, N, np.random.default_rng(B + N))
    return _starts[(name, B, N)]


def _batch(name, B, solved=True, **kw):
    """A batch of B trajectories at t1 = 0, t2 = DT (solved=False: both 0, no step solved yet)."""
    import trep_amd
    d, Q0, Q1, U, K = _case(name, B)
    mvi = trep_amd.BatchMidpointVI(BUILDERS[name](), B, **kw)
    if solved:
        mvi.initialize_from_configs(0.0, Q0, DT, Q1)
    else:
        mvi.initialize_from_state(0.0, Q0, np.zeros((B, mvi.nd)))
    return mvi


def _refused(mvi, call, code, message):
    """The call returns `code` with `message` and leaves times, launch counters and the parameter table as they were."""
    L = _lib.lib()
    before = (mvi.times(), mvi.kernel_info())
    assert call() == code, L.tg_last_error().decode()
    assert L.tg_last_error().decode() == message
    assert (mvi.times(), mvi.kernel_info()) == before


@pytest.mark.parametrize("name", ["pendulum1", "pend_on_cart"])
def test_rollouts_refuse_in_order(name):
    """Every rollout entry point: bad arguments, then a by-trajectory list on more than one step, then a list shorter than the
    rollout, then (tg_batch_rollout only) missing U / K.  Afterwards the list is still the one set: a rollout as long as it ends at
    the summed times."""
    L = _lib.lib()
    B, N = 4, 3
    mvi = _batch(name, B)
    d, _, _, U, K = _case(name, B)
    nX, nU = mvi.nX, mvi.nU
    Kp, bX, bU = (mvi.device_array(np.zeros(s)) for s in ((B, N, nU, nX), (B, N + 1, nX), (B, N, max(nU, 1))))
    Xd, Ud, Uo = mvi.device_empty(B * (N + 1) * nX), mvi.device_empty(B * N * max(nU, 1)), mvi.device_array(U)
    h = mvi._h

    def calls(n, u=None, dt=DT, kp=Kp, group=1, ntraj=2):
        return [lambda: L.tg_batch_rollout(h, n, dt, u, None, Xd, 200),
                lambda: L.tg_batch_rollout_closed_loop(h, n, dt, kp, group, bX, bU, Xd, Ud, 200),
                lambda: L.tg_batch_rollout_closed_loop_subset(h, ntraj, n, dt, kp, group, None, bX, bU, Xd, Ud, 200)]

    dts = DT * np.array([0.7, 1.2])
    mvi.set_step_sizes(dts, by_trajectory=True)
    for bad in (calls(0), calls(N, dt=0.0)):                   # bad arguments come first, whatever the list
        for call in bad:
            _refused(mvi, call, INVALID, "bad arguments")
    for call in calls(N, kp=None)[1:] + calls(N, group=0)[1:] + calls(N, ntraj=0)[2:] + calls(N, ntraj=B + 1)[2:]:
        _refused(mvi, call, INVALID, "bad arguments")
    for call in calls(N):                                     # ... then the by-trajectory list, before the missing U
        _refused(mvi, call, INVALID, BY_TRAJECTORY)
    mvi.set_step_sizes(dts)
    for call in calls(N):                                     # ... then the length of a by-step list, before the missing U
        _refused(mvi, call, INVALID, TOO_LONG)
    if mvi.nu:
        _refused(mvi, calls(2)[0], INVALID, "U / K device buffers required")
    t2 = mvi.times()[1]
    assert calls(2, u=Uo)[0]() == 0
    mvi.synchronize()
    assert mvi.times() == (t2 + dts[0], t2 + dts[0] + dts[1])
    assert (mvi.status()[1] == 0).all()
    mvi.close()


@pytest.mark.parametrize("name", ["pendulum1", "pend_on_cart"])
def test_calls_that_need_a_solved_step_or_their_arguments(name):
    """TG_ERR_STATE at t2 == t1, and the null-argument refusals of the calls that stage their inputs, with a live batch."""
    L = _lib.lib()
    B = 4
    mvi = _batch(name, B, solved=False)
    h, nq, nu = mvi._h, mvi.nq, mvi.nu
    R = nq + mvi.nd + nu + mvi.nk
    z, hz, f = np.zeros((B, mvi.nX)), np.zeros((B, R, R)), np.zeros((B, mvi.nd + mvi.nc))
    zd, hzd = mvi.device_array(z), mvi.device_empty(hz.size)
    for call, message in [(lambda: L.tg_batch_deriv1(h), NOT_SOLVED),
                          (lambda: L.tg_batch_deriv2_contract(h, z.ctypes.data, hz.ctypes.data), NOT_SOLVED),
                          (lambda: L.tg_batch_deriv2_contract_lambda(h, z.ctypes.data, None, hz.ctypes.data), NOT_SOLVED),
                          (lambda: L.tg_batch_deriv2_contract_device(h, zd, hzd), NOT_SOLVED),
                          (lambda: L.tg_batch_deriv2_contract_device_range(h, zd, hzd, 2, 0, 1), NOT_SOLVED),
                          (lambda: L.tg_batch_linearize(h, hzd, hzd), NOT_SOLVED),
                          (lambda: L.tg_batch_calc_p2(h), "calc_p2 needs t2 != t1"),
                          (lambda: L.tg_batch_calc_f(h, f.ctypes.data), "calc_f needs t2 != t1"),
                          (lambda: L.tg_batch_step(h, 0.0, None, None, None, None, 200, None, None),
                           "u1 / k2 required" if nu else "step needs t2_new != t2")]:
        _refused(mvi, call, INVALID if message == "u1 / k2 required" else STATE, message)
    u = np.zeros((B, max(nu, 1)))
    _refused(mvi, lambda: L.tg_batch_step(h, 0.0, u.ctypes.data, None, None, None, 200, None, None), STATE, "step needs t2_new != t2")
    # the range is checked before the state, null arguments before both
    for hor, k0, k1 in [(0, 0, 1), (3, 0, 1), (2, -1, 1), (2, 0, 3), (2, 1, 1)]:
        _refused(mvi, lambda: L.tg_batch_deriv2_contract_device_range(h, zd, hzd, hor, k0, k1), INVALID, "bad step range")
    q = np.zeros((B, nq))
    outs = np.zeros(B * 4 * max(nq, 2) ** 2)
    qp, o = q.ctypes.data, outs.ctypes.data
    seeds = np.zeros(B, dtype=np.int32)
    nulls = [lambda: L.tg_batch_deriv2_contract(h, None, hz.ctypes.data), lambda: L.tg_batch_deriv2_contract(h, z.ctypes.data, None),
             lambda: L.tg_batch_deriv2_contract_lambda(h, None, None, hz.ctypes.data),
             lambda: L.tg_batch_deriv2_contract_lambda(h, z.ctypes.data, None, None),
             lambda: L.tg_batch_deriv2_contract_device(h, None, hzd), lambda: L.tg_batch_deriv2_contract_device(h, zd, None),
             lambda: L.tg_batch_deriv2_contract_device_range(h, None, hzd, 0, 0, 0),
             lambda: L.tg_batch_dynamics(h, None, qp, qp, None, o, None, None), lambda: L.tg_batch_dynamics(h, qp, None, qp, None, o, None, None),
             lambda: L.tg_batch_dynamics(h, qp, qp, qp, None, None, None, None),
             lambda: L.tg_batch_dynamics_deriv1(h, None, qp, qp, *[None] * 10),
             lambda: L.tg_batch_dynamics_deriv1_forward(h, qp, qp, qp, None, None, *[None] * 9),
             lambda: L.tg_batch_energy(h, None, qp, o), lambda: L.tg_batch_energy(h, qp, None, o), lambda: L.tg_batch_energy(h, qp, qp, None),
             lambda: L.tg_batch_lagrangian(h, None, qp, o, o), lambda: L.tg_batch_lagrangian(h, qp, qp, None, o),
             lambda: L.tg_batch_lagrangian(h, qp, qp, o, None), lambda: L.tg_batch_lagrangian_forward(h, qp, qp, None, None, o, o)]
    if nu:                                                     # inputs the system has must be given
        nulls += [lambda: L.tg_batch_dynamics(h, qp, qp, None, None, o, None, None),
                  lambda: L.tg_batch_dynamics_deriv1(h, qp, qp, None, *[None] * 10),
                  lambda: L.tg_batch_dynamics_deriv1_forward(h, qp, qp, None, None, seeds.ctypes.data, *[None] * 9)]
    for call in nulls:
        _refused(mvi, call, INVALID, "null argument")
    seeds[1] = 2 * nq + mvi.nk + nu                            # one past the last direction variable
    out_of_range = "direction variable out of range (q | dq | ddq_k | u)"
    _refused(mvi, lambda: L.tg_batch_lagrangian_forward(h, qp, qp, seeds.ctypes.data, None, o, o), INVALID, out_of_range)
    _refused(mvi, lambda: L.tg_batch_dynamics_deriv1_forward(h, qp, qp, qp, None, seeds.ctypes.data, *[None] * 9), INVALID, out_of_range)
    # the horizon batch: seeds x horizon must be the batch
    X, U = mvi.device_array(np.zeros((2, 3, mvi.nX))), mvi.device_array(np.zeros((2, 2, max(mvi.nU, 1))))
    for s, hor, dt, x in [(0, 2, DT, X), (2, 0, DT, X), (2, 2, 0.0, X), (2, 2, DT, None)]:
        _refused(mvi, lambda: L.tg_batch_set_from_trajectories(h, s, hor, 0.0, dt, x, U, 200), INVALID, "bad arguments")
    _refused(mvi, lambda: L.tg_batch_set_from_trajectories(h, 3, 2, 0.0, DT, X, U, 200), INVALID, "batch size must be seeds * horizon")
    mvi.close()


def test_second_derivatives_of_a_linear_spring_are_unsupported():
    L = _lib.lib()
    B = 4
    mvi = _batch("spring_link", B)
    h = mvi._h
    R = mvi.nq + mvi.nd + mvi.nu + mvi.nk
    z, hz = np.zeros((B, mvi.nX)), np.zeros((B, R, R))
    zd, hzd = mvi.device_array(z), mvi.device_empty(hz.size)
    for call in [lambda: L.tg_batch_deriv2_contract(h, z.ctypes.data, hz.ctypes.data),
                 lambda: L.tg_batch_deriv2_contract_lambda(h, z.ctypes.data, None, hz.ctypes.data),
                 lambda: L.tg_batch_deriv2_contract_device(h, zd, hzd),
                 lambda: L.tg_batch_deriv2_contract_device_range(h, zd, hzd, 2, 0, 1)]:
        _refused(mvi, call, UNSUPPORTED, NO_SECOND)
    _refused(mvi, lambda: L.tg_batch_deriv2_contract_device_range(h, zd, hzd, 3, 0, 1), INVALID, "bad step range")   # the range comes first
    mvi.close()


@pytest.mark.parametrize("name", ["pend_on_cart", "puppet_basic"])
def test_both_staging_paths_of_step_agree(name):
    """tg_batch_step stages (u1, k2, hints) through one pinned block up to 64 trajectories and through the copy engine above: the same
    64 trajectories as a batch of 64 and as the first 64 of a batch of 65 give the same bits."""
    d, Q0, Q1, U, K = _case(name, 65)
    rng = np.random.default_rng(7)
    big, small = _batch(name, 65), _batch(name, 64)
    small.initialize_from_configs(0.0, Q0[:64], DT, Q1[:64])   # (the 64 starts of _case(name, 64) are others)
    for k in range(3):
        t2 = big.times()[1] + DT
        qh = big.q2[:, :big.nd] + 1e-4 * rng.standard_normal((65, big.nd))
        lh = big.lambda1 + 1e-4 * rng.standard_normal((65, big.nc))
        res = [m.step(t2, U[:n, k] if m.nu else None, K[:n, k] if m.nk else None, q2_hint=qh[:n], lambda1_hint=lh[:n] if m.nc else None)
               for m, n in ((big, 65), (small, 64))]
        assert (res[0][1] == 0).all()
        for a, b in zip(res[0], res[1]):                       # iterations, status
            assert np.array_equal(a[:64], b)
        for f in ("q2", "p2", "lambda1", "q1", "p1"):
            assert np.array_equal(getattr(big, f)[:64], getattr(small, f)), (k, f)
        assert big.times() == small.times()
    big.close()
    small.close()


def test_forwarded_second_derivative_calls_agree():
    """tg_batch_deriv2_contract is the _lambda form without multiplier weights, tg_batch_deriv2_contract_device the _device_range form
    over every step: the same bits, on a horizon x seeds = 4 x 2 batch."""
    L = _lib.lib()
    name, B = "pend_on_cart", 8
    d, Q0, Q1, U, K = _case(name, B)
    mvi = _batch(name, B)
    assert (mvi.step(2 * DT, U[:, 0])[1] == 0).all()
    h = mvi._h
    R = mvi.nq + mvi.nd + mvi.nu + mvi.nk
    Z = np.random.default_rng(3).standard_normal((B, mvi.nX))
    zd = mvi.device_array(Z)
    out = []
    for call in (lambda p: L.tg_batch_deriv2_contract(h, Z.ctypes.data, p), lambda p: L.tg_batch_deriv2_contract_lambda(h, Z.ctypes.data, None, p)):
        HZ = np.full((B, R, R), np.nan)
        assert call(HZ.ctypes.data) == 0
        out.append(HZ)
    for call in (lambda p: L.tg_batch_deriv2_contract_device(h, zd, p), lambda p: L.tg_batch_deriv2_contract_device_range(h, zd, p, 4, 0, 4)):
        hzd = mvi.device_array(np.full((B, R, R), np.nan))
        assert call(hzd) == 0
        mvi.synchronize()
        out.append(mvi.download(hzd, (B, R, R)))
    assert np.isfinite(out[0]).all() and np.abs(out[0]).max() > 0
    assert np.array_equal(out[0], mvi.deriv2_contract(Z, ZL=None))
    for HZ in out[1:]:
        assert np.array_equal(out[0], HZ)
    mvi.close()


def _use_everything(k):
    """One batch through every lazily allocated buffer of the host layer; returns what it computed."""
    L = _lib.lib()
    name, B = "pend_on_cart", 4
    d, Q0, Q1, U, K = _case(name, B)
    mvi = _batch(name, B)                                      # (loads the specialised library: argument ring and its events)
    assert mvi.kernel_info()["spec_library"]
    mvi.timing()                                               # event timing on
    out = [mvi.step(2 * DT, U[:, 0])[0]]                       # the pinned staging block
    mvi.calc_deriv1()
    out += [mvi.deriv1("q2_dq1"), mvi.deriv2_contract(np.ones((B, mvi.nX)), np.ones((B, mvi.nc)))]
    q, dq = Q1, (Q1 - Q0) / DT
    out += list(mvi.dynamics(q, dq, U[:, 0])[:2]) + [mvi.energy(q, dq)]
    out += list(mvi.dynamics_deriv1(q, dq, U[:, 0], seeds=(np.arange(B) % mvi.nq,))[0].values())
    out += list(mvi.lagrangian(q, dq, seeds=(np.zeros(B, dtype=np.int32), np.ones(B, dtype=np.int32))).values())
    mvi.set_step_sizes(DT * np.array([0.8, 1.1, 0.9]))
    mvi.set_parameters(inertia=mvi.parameters()["inertia"] * (1.0 + 0.1 * np.arange(B))[:, None, None])
    out.append(mvi.rollout(3, DT, U))
    assert (mvi.status()[1] == 0).all()
    n = 3                                                      # the two solve hooks and their temporaries
    aug = np.hstack([np.eye(n) * 2.0, np.ones((n, 1))])
    x, piv, st = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(1, dtype=np.int32)
    _lib.check(L.tg_debug_solve(0, n, 0, aug.ctypes.data, x.ctypes.data, piv.ctypes.data, st.ctypes.data))
    nf = mvi.nd + mvi.nc
    aug = np.hstack([np.eye(nf) * 4.0, np.ones((nf, 1))])[None].repeat(2, axis=0).copy()
    xs, path = np.zeros((2, nf)), np.zeros(2, dtype=np.int32)
    _lib.check(L.tg_batch_debug_newton_solve(mvi._h, 2, 1, aug.ctypes.data, xs.ctypes.data, path.ctypes.data))
    assert mvi.timing()[0] > 0
    out += [x, xs]
    assert np.allclose(x, 0.5) and st[0] == 0
    assert (path == -1).all() and np.array_equal(xs, aug[:, :, nf])      # a library of a team below a wavefront has no solver to run
    mvi.close()
    return out


def test_batches_come_and_go():
    first = _use_everything(0)
    assert all(np.isfinite(a).all() for a in first)
    for k in range(1, 20):
        for a, b in zip(first, _use_everything(k)):
            assert np.array_equal(a, b), k


def test_a_callers_stream_outlives_the_batch():
    L = _lib.lib()
    name, B = "pend_on_cart", 4
    d, Q0, Q1, U, K = _case(name, B)
    stream = L.tg_dopt_lane_stream(0, 1)                       # a stream the batch does not own
    assert stream
    got = []
    for _ in range(2):                                         # the second batch runs on the stream the first was destroyed on
        mvi = _batch(name, B)
        mvi.set_stream(stream)
        assert mvi.stream == stream
        assert (mvi.step(2 * DT, U[:, 0])[1] == 0).all()
        got.append(mvi.q2)
        mvi.close()
    assert np.array_equal(got[0], got[1])


def test_load_specialized_refuses_a_wrong_file_and_leaves_the_batch_as_it_was(tmp_path):
    L = _lib.lib()
    name, B = "pend_on_cart", 4
    d, Q0, Q1, U, K = _case(name, B)
    mvi = _batch(name, B, specialize=False)
    junk = tmp_path / "not_a_library.so"
    junk.write_bytes(b"not an ELF file")
    before = (mvi.times(), mvi.kernel_info())
    assert L.tg_batch_load_specialized(mvi._h, str(junk).encode()) == INVALID
    assert L.tg_last_error().decode().startswith("cannot load " + str(junk))
    assert L.tg_batch_load_specialized(mvi._h, _lib.LIB_PATH.encode()) == INVALID       # a library, but not a specialised kernel
    assert L.tg_last_error().decode() == "not a specialised trep_amd kernel library"
    assert (mvi.times(), mvi.kernel_info()) == before
    assert (mvi.step(2 * DT, U[:, 0])[1] == 0).all()           # still on the generic kernel
    q2 = mvi.q2
    assert mvi.kernel_info()["generic_launched"] == ["calc_p2", "rollout"] and mvi.kernel_info()["spec_launches"] == 0
    assert mvi.specialize(build=False)                         # the right one (prebuilt for this system)
    mvi.initialize_from_configs(0.0, Q0, DT, Q1)
    assert (mvi.step(2 * DT, U[:, 0])[1] == 0).all()
    assert mvi.kernel_info()["spec_launches"] > 0
    assert np.abs(mvi.q2 - q2).max() < 1e-10                   # the same step by the specialised kernel, to the project's state tolerance
    mvi.close()
