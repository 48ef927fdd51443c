"""Shared helpers for the parity tests: golden fixtures + the systems they were made from."""
import collections
import os

import numpy as np

from trep_amd import systems, descriptor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

BUILDERS = {
    "pendulum1": lambda: systems.pendulum(1),
    "pendulum5": lambda: systems.pendulum(5),
    "pend_on_cart": lambda: systems.pend_on_cart(),
    "scissor4": lambda: systems.scissor_lift(4),
    "puppet40": lambda: systems.puppet(),
    "puppet_basic": lambda: systems.puppet_basic(),
    "spring_arm": lambda: systems.spring_arm(),
    "nonlinear_spring_arm": lambda: systems.nonlinear_spring_arm(),
    "spring_link": lambda: systems.spring_link(),
    "plane_link": lambda: systems.plane_link(),
    "wrench_arm": lambda: systems.wrench_arm(),
    "wrench_torque": lambda: systems.wrench_torque(),
    "dual_pendulums": lambda: systems.dual_pendulums(),
    "wrench_spatial": lambda: systems.wrench_spatial(),
    "wrench_body": lambda: systems.wrench_body(),
    "damper_link": lambda: systems.damper_link(),
    "puppet_forces": lambda: systems.puppet_forces(),
    "extensor_tendon": lambda: systems.extensor_tendon(),
}
D1 = ["q2_dq1", "q2_dp1", "q2_du1", "q2_dk2", "p2_dq1", "p2_dp1", "p2_du1", "p2_dk2",
      "l1_dq1", "l1_dp1", "l1_du1", "l1_dk2"]
PAIRS = ["dq1dq1", "dq1dp1", "dq1du1", "dq1dk2", "dp1dp1", "dp1du1", "dp1dk2", "du1du1", "du1dk2", "dk2dk2"]
NO_SECOND_ORDER = {"spring_link", "extensor_tendon", "dual_pendulums"}   # LinearSpring has no third derivative in the reference: deriv2 raises there too
_cache = {}


def golden(name):
    if name not in _cache:
        _cache[name] = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    return _cache[name]


def build(name):
    system = BUILDERS[name]()
    return system, descriptor.flatten(system)


def trajectories(name):
    """List of (prefix, q0, U[N][nu], K[N][nk]) recorded for a system."""
    g = golden(name)
    if name.startswith("pendulum"):
        return [("", g["q0"], g["U"], g["K"])]
    out = []
    b = 0
    while "b%d_q0" % b in g:
        n = len(g["b%d_IT" % b])
        U = g.get("b%d_U" % b, np.zeros((n, 0)))
        K = g.get("b%d_K" % b, np.zeros((n, 0)))
        out.append(("b%d_" % b, g["b%d_q0" % b], U, K))
        b += 1
    return out


def relerr(a, b):
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))

# (seeds, horizon, k_begin, k_end) of the remapped deriv2z launches (tg_batch_deriv2_contract_device_range) that the team-size
# tests run: batch = seeds * horizon, launch slots = seeds * (k_end - k_begin), a multiple of no team count per block (64/team > 1)
RANGE_CASES = [(3, 7, 2, 5), (5, 6, 1, 6), (2, 13, 0, 9)]

# Generic-kernel cells of the team-size tests (TREPAMD_TEAM forces the team): system -> {team: LDS slice kinds whose block,
# (64 / team) x slice x 8 B, is over the 160 KiB a workgroup may have -- the launches the library must refuse}.  The slice kind of
# calc_p2, calc_f, dynamics, energy and lagrangian is the rollout's.
LDS_SLICES = ("rollout", "deriv1", "deriv2z", "dynamics_deriv1")
_ALL = set(LDS_SLICES)
TEAM_CELLS = {
    "pendulum1": {1: set(), 4: set(), 16: set(), 64: set()},
    "pend_on_cart": {1: set(), 4: set(), 16: set(), 64: set()},
    "dual_pendulums": {1: set(), 4: set(), 16: set(), 64: set()},
    "damper_link": {1: {"deriv2z", "dynamics_deriv1"}, 4: set(), 16: set(), 64: set()},
    "spring_link": {1: _ALL, 4: set(), 16: set(), 64: set()},
    "plane_link": {1: {"deriv1", "deriv2z", "dynamics_deriv1"}, 4: set(), 16: set(), 64: set()},
    "pendulum5": {1: _ALL, 4: set(), 16: set(), 64: set()},
    "wrench_arm": {1: _ALL, 4: set(), 16: set(), 64: set()},
    "spring_arm": {1: {"deriv1", "deriv2z", "dynamics_deriv1"}, 4: set(), 16: set(), 64: set()},
    "scissor4": {1: _ALL, 4: {"deriv1", "deriv2z", "dynamics_deriv1"}, 16: set(), 64: set()},
    "puppet_basic": {16: {"deriv2z"}, 64: set()},
}


# ---- shared by the discopt device tests (test_gpu_discopt_device.py, test_gpu_lq_classes.py, test_gpu_discopt_sizes.py) ----


def device_pool():
    from trep_amd.discopt.batch_doptimizer import _DevicePool
    return _DevicePool(0)


def random_lq_problem(rng, S, N, nX, nU, nxh):
    A = 0.2 * rng.standard_normal((S, N, nX, nX)) / np.sqrt(nX) + 0.9 * np.eye(nX)
    B = rng.standard_normal((S, N, nX, nU)) / np.sqrt(nX)
    Q = rng.standard_normal((nX, nX)); Q = Q.dot(Q.T) / nX + np.eye(nX)
    Qf = 2.0 * Q
    R = rng.standard_normal((nU, nU)); R = R.dot(R.T) / nU + np.eye(nU)
    q = rng.standard_normal((S, N + 1, nX))
    r = rng.standard_normal((S, N, nU))
    Rz = nxh + nU
    hz = 0.05 * rng.standard_normal((S, N, Rz, Rz))
    hz = hz + np.swapaxes(hz, 2, 3)
    return A, B, Q, Qf, R, q, r, hz


def host_lq(A, B, Q, Qf, R, q, r, hz, nxh):
    """numpy reference: dlqr.solve_tv_lq with the Newton-model weights assembled like DSystem._split_hz."""
    from trep_amd.discopt import dlqr
    N, nX, nU = A.shape[0], A.shape[1], B.shape[2]

    def Qk(k):
        if k == N:
            return Qf
        M = Q.copy()
        if hz is not None:
            M[:nxh, :nxh] += hz[k][:nxh, :nxh]
        return M

    def Sk(k):
        M = np.zeros((nX, nU))
        if hz is not None:
            M[:nxh, :] = hz[k][:nxh, nxh:]
        return M

    def Rk(k):
        return R + (hz[k][nxh:, nxh:] if hz is not None else 0.0)

    if q is None:
        assert hz is None
        K, P = dlqr.solve_tv_lqr(A, B, Qk, Rk)
        return np.array(K), None, P, None
    K, C, P, b = dlqr.solve_tv_lq(A, B, q, r, Qk, Sk, Rk)
    return np.array(K), np.array(C), P, b


def dsystem_structure(rng, A, B, nd, nk, nu, dt=0.01):
    """Impose the block structure of DSystem.fdx / fdu (dsystem.py:284-317) on random A, B: states [Qd | Qk | p | v], inputs [u | rho]."""
    nq, nX = nd + nk, 2 * (nd + nk)
    Qd, Qk, p, v = slice(0, nd), slice(nd, nq), slice(nq, nq + nd), slice(nq + nd, nX)
    A[..., Qk, :] = 0.0; A[..., v, :] = 0.0; A[..., :, v] = 0.0
    B[..., Qk, :] = 0.0; B[..., v, :] = 0.0
    for m in range(nk):
        steps = dt * (1.0 + 0.3 * rng.random(A.shape[:-2]))       # any time base: the entries are read, not assumed
        A[..., nq + nd + m, nd + m] = -1.0 / steps
        B[..., nd + m, nu + m] = 1.0
        B[..., nq + nd + m, nu + m] = 1.0 / steps
    return A, B


# ---- the size classes of the LQ sweep (tg_tv_lq): test_lq_plan_cpu.py checks the table against the dispatch, test_gpu_lq_classes.py
# runs it, tools/lq_parity.py records it.  A case: sizes, horizon N, seeds S, structure ds = (nd, nk, nu) of DSystem.fdx / fdu or
# None (dense A, B), the environment switches it runs under, and the plan tg_tv_lq_plan must report: (kernel, class, NR) with
# kernel 0 = k_tv_lq (class = tile size TS), 1 = k_tv_lq_mfma, 2 = k_tv_lq_ds (class = NT tiles per dimension).
# `why`: for a structured problem that the dispatch hands to another kernel, the condition that does it.
# `select`: the seeds the launch is restricted to (the others' outputs must stay untouched); one such case per kernel.
LqCase = collections.namedtuple("LqCase", "nX nU N S ds plan env why select")


def _lqc(nX, nU, N, S, plan, ds=None, env=None, why=None, select=None):
    if ds is not None:
        assert nX == 2 * (ds[0] + ds[1]) and nU == ds[1] + ds[2]
    return LqCase(nX, nU, N, S, ds, plan, env or {}, why, select)


_LEGACY, _DENSE = {"TREPAMD_LQ_LEGACY": "1"}, {"TREPAMD_LQ_DENSE": "1"}
LQ_NX_BOUNDS = (16, 32, 48, 80)      # nX <= bound: NT = 1, 2, 3, 5; above 80: NT = 6 up to 96
LQ_NU_BOUNDS = (4, 8, 20, 32)        # nU <= bound: NR = 4, 8, 20, 32; above 32: the VALU kernel up to 64
LQ_CASES = [
    # dense, matrix cores: every reachable (NT, NR) with both sides of every nX and nU boundary
    _lqc(1, 1, 9, 2, (1, 1, 4)),
    _lqc(16, 4, 7, 2, (1, 1, 4)), _lqc(16, 5, 6, 2, (1, 1, 8)), _lqc(16, 8, 1, 2, (1, 1, 8)), _lqc(16, 9, 6, 2, (1, 1, 20)),
    _lqc(16, 20, 6, 2, (1, 1, 20)), _lqc(16, 21, 2, 2, (1, 1, 32)), _lqc(16, 32, 6, 2, (1, 1, 32)),
    _lqc(17, 4, 6, 2, (1, 2, 4)), _lqc(17, 5, 13, 3, (1, 2, 8), select=(2, 0)), _lqc(32, 8, 6, 2, (1, 2, 8)), _lqc(32, 9, 6, 2, (1, 2, 20)),
    _lqc(17, 20, 6, 2, (1, 2, 20)), _lqc(32, 21, 6, 2, (1, 2, 32)), _lqc(32, 32, 7, 2, (1, 2, 32)),
    _lqc(33, 4, 6, 2, (1, 3, 4)), _lqc(48, 5, 6, 2, (1, 3, 8)), _lqc(48, 8, 6, 2, (1, 3, 8)), _lqc(33, 9, 11, 2, (1, 3, 20)),
    _lqc(48, 20, 6, 2, (1, 3, 20)), _lqc(48, 21, 6, 2, (1, 3, 32)), _lqc(48, 32, 6, 2, (1, 3, 32)),
    _lqc(49, 4, 6, 2, (1, 5, 4)), _lqc(49, 5, 6, 2, (1, 5, 8)), _lqc(80, 8, 6, 2, (1, 5, 8)), _lqc(80, 9, 6, 2, (1, 5, 20)),
    _lqc(49, 20, 6, 2, (1, 5, 20)), _lqc(80, 20, 7, 2, (1, 5, 20)),
    _lqc(81, 4, 6, 2, (1, 6, 4)), _lqc(96, 4, 6, 2, (1, 6, 4)),
    # the VALU kernel without a switch: more than 32 inputs (its only path), and what the matrix-core kernel's LDS does not hold;
    # the largest sizes its own LDS holds at 33 and at 64 inputs
    _lqc(15, 34, 6, 2, (0, 2, 0)), _lqc(16, 33, 6, 2, (0, 4, 0)), _lqc(32, 33, 6, 2, (0, 4, 0)), _lqc(48, 33, 6, 2, (0, 5, 0)),
    _lqc(32, 64, 6, 2, (0, 5, 0)), _lqc(66, 33, 6, 2, (0, 6, 0)), _lqc(42, 64, 7, 3, (0, 6, 0), select=(2, 0)),
    _lqc(49, 21, 6, 2, (0, 4, 0)), _lqc(80, 21, 6, 2, (0, 5, 0)), _lqc(81, 5, 6, 2, (0, 6, 0)),
    # ... and with TREPAMD_LQ_LEGACY=1: its four classes at sizes the matrix-core kernels normally take
    _lqc(16, 4, 6, 2, (0, 2, 0), env=_LEGACY), _lqc(33, 9, 6, 2, (0, 4, 0), env=_LEGACY), _lqc(80, 18, 6, 2, (0, 5, 0), env=_LEGACY),
    _lqc(96, 4, 6, 2, (0, 6, 0), env=_LEGACY),
    # DSystem structure: every reachable (NT, NR) of k_tv_lq_ds
    _lqc(8, 3, 9, 2, (2, 1, 4), ds=(1, 3, 0)), _lqc(16, 4, 6, 2, (2, 1, 4), ds=(8, 0, 4)), _lqc(16, 5, 6, 2, (2, 1, 8), ds=(5, 3, 2)),
    _lqc(16, 9, 1, 2, (2, 1, 20), ds=(4, 4, 5)), _lqc(16, 21, 6, 2, (2, 1, 32), ds=(4, 4, 17)),
    _lqc(18, 4, 6, 2, (2, 2, 4), ds=(5, 4, 0)), _lqc(32, 8, 2, 2, (2, 2, 8), ds=(8, 8, 0)), _lqc(26, 9, 6, 2, (2, 2, 20), ds=(9, 4, 5)),
    _lqc(32, 32, 6, 2, (2, 2, 32), ds=(8, 8, 24)),
    _lqc(34, 4, 6, 2, (2, 3, 4), ds=(13, 4, 0)), _lqc(48, 8, 6, 2, (2, 3, 8), ds=(16, 8, 0)), _lqc(48, 20, 13, 2, (2, 3, 20), ds=(14, 10, 10)),
    _lqc(48, 21, 6, 2, (2, 3, 32), ds=(15, 9, 12)),
    _lqc(50, 4, 6, 2, (2, 5, 4), ds=(21, 4, 0)), _lqc(80, 8, 6, 2, (2, 5, 8), ds=(32, 8, 0)),
    _lqc(80, 18, 17, 3, (2, 5, 20), ds=(22, 18, 0), select=(2, 0)), _lqc(80, 12, 6, 2, (2, 5, 20), ds=(32, 8, 4)),
    _lqc(64, 31, 6, 2, (2, 5, 32), ds=(1, 31, 0)), _lqc(50, 24, 6, 2, (2, 5, 32), ds=(1, 24, 0)),
    # structured problems that the dispatch silently hands to another kernel
    _lqc(10, 3, 6, 2, (1, 1, 4), ds=(5, 0, 3), why="pad"),              # nk < round_up(nd, 4) - nd: no sparse rows to pad the dense block with
    _lqc(14, 4, 6, 2, (1, 1, 4), ds=(7, 0, 4), why="pad"),              # (8, 0, 4) above is the other side)
    _lqc(66, 32, 6, 2, (0, 6, 0), ds=(1, 32, 0), why="nk31"),           # nk > 31: ((1, 31, 0) above is the other side)
    _lqc(56, 17, 6, 2, (1, 5, 20), ds=(25, 3, 14), why="lds"),          # LDS of the structured layout over the bound
    _lqc(56, 16, 6, 2, (2, 5, 20), ds=(25, 3, 13)),                     # ... and its other side
    _lqc(80, 17, 6, 2, (1, 5, 20), ds=(25, 15, 2), why="lds+tiles"),    # more than 32 tiles in phase 1 (never without the LDS bound)
    _lqc(80, 18, 6, 2, (1, 5, 20), ds=(22, 18, 0), env=_DENSE, why="env"),
]
# (the two remaining conditions depend on more than the sizes and have tests of their own: A_dev / B_dev off a 16-byte boundary, and a
# curvature block that reaches into the v rows, hz_nx > 2 nd + nk)

# sizes the dispatch must refuse with TG_ERR_UNSUPPORTED before anything is launched: (nX, nU, environment)
LQ_REFUSED = [(97, 4, {}), (97, 1, _LEGACY), (16, 65, {}), (1, 65, _LEGACY), (96, 5, {}), (67, 33, {}), (43, 64, {}), (64, 60, {}),
              (80, 32, {}), (96, 32, {}), (48, 64, {}), (64, 48, {}), (93, 33, {}), (80, 22, _LEGACY)]


def lq_case_id(c):
    return "%dx%d_N%d%s%s" % (c.nX, c.nU, c.N, "_ds%d.%d.%d" % c.ds if c.ds else "", "_" + "+".join(sorted(k[8:].lower() for k in c.env)) if c.env else "")


def lq_case_nxh(c):
    """State part of the curvature block of a case's Newton model: a DSystem's 2 nd + nk, three quarters of a dense problem's states."""
    return 2 * c.ds[0] + c.ds[1] if c.ds else max(1, (3 * c.nX) // 4)


def lq_case_problem(c):
    """A, B, Q, Qf, R, q, r, hz of a case (different A, B, q, r, hz per seed), structure imposed."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(lq_case_id(c).encode()))
    A, B, Q, Qf, R, q, r, hz = random_lq_problem(rng, c.S, c.N, c.nX, c.nU, lq_case_nxh(c))
    if c.ds:
        # (single entries of size 1 instead of 1 / dt = 100: entries of 1e4 in P put the floor of a correct fp64 sweep at 2e-13)
        A, B = dsystem_structure(rng, A, B, *c.ds, dt=1.0)
    return A, B, Q, Qf, R, q, r, hz


LQ_MODES = ("lqr", "lq", "newton")
_lq_refs = {}


def lq_case_reference(c, mode, s):
    """(long-double reference (K, C, P0, b0), floors e_ref = relerr(fp64 dlqr.py, long double) per output, bounds max(64 e_ref, 1e-13))
    of seed s of a case in one of LQ_MODES; outputs a mode does not have are None."""
    import lq_reference as ref
    key = (lq_case_id(c), mode, s)
    if key not in _lq_refs:
        A, B, Q, Qf, R, q, r, hz = lq_case_problem(c)
        nxh = lq_case_nxh(c)
        affine, newton = mode != "lqr", mode == "newton"
        w = ref.Weights(Q, Qf, R, hz[s] if newton else None, nxh)
        K, C, P, b, _ = ref.solve_tv_lq(A[s], B[s], q[s] if affine else None, r[s] if affine else None, w)
        host = host_lq(A[s], B[s], Q, Qf, R, q[s] if affine else None, r[s] if affine else None, hz[s] if newton else None, nxh)
        want = (K, C, P, b)
        floors = tuple(None if x is None else ref.relerr(h, x) for h, x in zip(host, want))
        _lq_refs[key] = (want, floors, tuple(None if e is None else ref.bound(e) for e in floors))
    return _lq_refs[key]


# ---- launching tg_tv_lq from a test -------------------------------------------------------------------------------------------------
def lq_plan(p, monkeypatch=None, env=None):
    """(return code, (kernel, class, NR), threads, LDS bytes) of tg_tv_lq_plan for an LqProblem, optionally under environment switches."""
    import ctypes
    from trep_amd import _lib
    for k in ("TREPAMD_LQ_LEGACY", "TREPAMD_LQ_DENSE"):
        if monkeypatch is not None:
            monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    out = np.full(6, -7, dtype=np.int32)
    rc = _lib.lib().tg_tv_lq_plan(ctypes.byref(p), out.ctypes.data_as(_lib._c_ip))
    return rc, tuple(int(x) for x in out[:3]), int(out[3]), int(out[4])


def lq_struct(S, N, nX, nU, dev, affine=True, hz=None, ds=None, strides=None):
    """tg_lq_problem over the device arrays dev["A"], ... (objects with .ptr, or plain addresses); hz = (hz_R, hz_nx) adds dev["hz"];
    strides = dict(Q=(seed, step), Qf=seed, R=(seed, step)) in doubles."""
    from trep_amd import _lib
    ptr = lambda x: x if isinstance(x, int) else x.ptr
    p = _lib.LqProblem()
    p.n_problems, p.horizon, p.nX, p.nU = S, N, nX, nU
    p.A_dev, p.B_dev = ptr(dev["A"]), ptr(dev["B"])
    p.Q_dev, p.Qf_dev, p.R_dev = ptr(dev["Q"]), ptr(dev["Qf"]), ptr(dev["R"])
    if strides:
        p.Q_seed_stride, p.Q_step_stride = strides.get("Q", (0, 0))
        p.Qf_seed_stride = strides.get("Qf", 0)
        p.R_seed_stride, p.R_step_stride = strides.get("R", (0, 0))
    if affine:
        p.q_dev, p.r_dev = ptr(dev["q"]), ptr(dev["r"])
    if hz is not None:
        p.hz_dev, p.hz_R, p.hz_nx = ptr(dev["hz"]), hz[0], hz[1]
    if ds:
        p.ds_nd, p.ds_nk, p.ds_nu = ds
    return p


class LqOutputs(object):
    """NaN-filled K, C, P0, b0, b_next and a status array filled with -9, bound to a tg_lq_problem."""

    def __init__(self, pool, S, N, nX, nU):
        nan = lambda *shape: pool.upload(np.full(shape, np.nan))
        self.K, self.C, self.P0, self.b0, self.Z = nan(S, N, nU, nX), nan(S, N, nU), nan(S, nX, nX), nan(S, nX), nan(S, N, nX)
        self.status = pool.upload(np.full((S,), -9, dtype=np.int32), np.int32)

    def bind(self, p, carry=None):
        p.K_dev, p.C_dev, p.b_next_dev, p.status_dev = self.K.ptr, self.C.ptr, self.Z.ptr, self.status.ptr
        p.P0_dev, p.b0_dev = (self.P0.ptr, self.b0.ptr) if carry is None else (carry[0].ptr, carry[1].ptr)
        return p

    def get(self):
        return self.K.get(), self.C.get(), self.P0.get(), self.b0.get(), self.status.get()


def lq_check_seed(got, want, bounds, tag):
    """One seed's (K, C, P0, b0) against the long-double reference: common.relerr-style error of every output under its bound, and
    the per-entry error of K -- |a - b| / (|ref| + rowmax |ref|), which a small column cannot hide in -- under K's.  Returns the errors."""
    import lq_reference as ref
    errs = []
    for name, g, w, bd in zip("K C P0 b0".split(), got, want, bounds):
        if w is None:
            errs.append(None)
            continue
        e = ref.relerr(g, w)
        print("%s %s: relerr %.3e (bound %.3e)" % (tag, name, e, bd))
        errs.append(e)
    ek = ref.entry_relerr(got[0], want[0])
    print("%s K per entry: %.3e (bound %.3e)" % (tag, ek, bounds[0]))
    errs.append(ek)
    for name, e, bd in zip("K C P0 b0 K-per-entry".split(), errs, tuple(bounds) + (bounds[0],)):
        assert e is None or e < bd, (tag, name, e, bd)
    return errs


# ---- problems for the solver branches of the LQ sweep: all three kernels run them at the puppet's sizes and at an odd one ----------------
LQ_SPECIAL_SIZES = [(22, 18, 0), (9, 4, 5)]              # (nd, nk, nu): nX x nU = 80 x 18 and 26 x 9
LQ_KERNELS = {"structured": ({}, 2), "dense": (_DENSE, 1), "legacy": (_LEGACY, 0)}       # environment, kernel the plan must report


def lq_special_problem(ds, N, S, tag):
    """dict(A, B, Q, Qf, R, q, r, hz, nxh, ...) with the DSystem structure ds, seeded by (ds, tag)."""
    import zlib
    nd, nk, nu = ds
    nX, nU, nxh = 2 * (nd + nk), nu + nk, 2 * nd + nk
    rng = np.random.default_rng(zlib.crc32(("%s %s" % (ds, tag)).encode()))
    A, B, Q, Qf, R, q, r, hz = random_lq_problem(rng, S, N, nX, nU, nxh)
    A, B = dsystem_structure(rng, A, B, nd, nk, nu, dt=1.0)      # (single entries of size 1 like the dense ones: gamma stays well scaled)
    return dict(A=A, B=B, Q=Q, Qf=Qf, R=R, q=q, r=r, hz=hz, nxh=nxh, nX=nX, nU=nU, N=N, S=S, ds=ds, rng=rng)


def lq_reference_sweep(pr, s, keep=(), **kw):
    """Long-double Newton-model sweep of seed s of such a problem (weights with a leading seed / step axis are indexed)."""
    import lq_reference as ref
    pick = lambda M, base: M[s] if M.ndim > base and M.shape[0] == pr["S"] and pr.get("seed_axis", False) else M
    w = ref.Weights(pick(pr["Q"], 2), pick(pr["Qf"], 2), pick(pr["R"], 2), pr["hz"][s], pr["nxh"])
    return ref.solve_tv_lq(pr["A"][s], pr["B"][s], pr["q"][s], pr["r"][s], w, keep=keep, **kw)


def lq_host_sweep(pr, s):
    """The same sweep in fp64 with dlqr.py (LAPACK): its distance from the long-double sweep is the floor e_ref of the problem."""
    import lq_reference as ref
    from trep_amd.discopt import dlqr
    pick = lambda M, base: M[s] if M.ndim > base and M.shape[0] == pr["S"] and pr.get("seed_axis", False) else M
    w = ref.Weights(pick(pr["Q"], 2), pick(pr["Qf"], 2), pick(pr["R"], 2), pr["hz"][s], pr["nxh"], dtype=np.float64)
    K, C, P, b = dlqr.solve_tv_lq(pr["A"][s], pr["B"][s], pr["q"][s], pr["r"][s], lambda k: w.Qf if k == pr["N"] else w.Qk(k), w.Sk, w.Rk)
    return np.array(K), np.array(C), P, b


def lq_special_reference(pr, s, keep=()):
    """(reference (K, C, P0, b0), floors, bounds, kept) of seed s: the bounds are max(64 e_ref, 1e-13) with e_ref from this very problem."""
    import lq_reference as ref
    K, C, P, b, kept = lq_reference_sweep(pr, s, keep=keep)
    floors = tuple(ref.relerr(h, x) for h, x in zip(lq_host_sweep(pr, s), (K, C, P, b)))
    return (K, C, P, b), floors, tuple(ref.bound(e) for e in floors), kept


def lq_indefinite_problem(ds, N=6, S=2):
    """Newton model whose gamma_k = R + HZ_uu + B'PB is indefinite at EVERY step: going backwards along the long-double sweep, the
    curvature of the first half of the inputs is lowered by c_k I with c_k = 1 + the largest eigenvalue of that block of gamma_k, so
    the block's eigenvalues are <= -1 and (Cauchy interlacing) gamma_k has at least nU // 2 eigenvalues <= -1."""
    import lq_reference as ref
    pr = lq_special_problem(ds, N, S, "indefinite")
    nxh, h = pr["nxh"], pr["nU"] // 2
    for s in range(S):
        w = ref.Weights(pr["Q"], pr["Qf"], pr["R"], pr["hz"][s], nxh)      # (holds a long-double copy of hz: updated below, step by step)
        P, b = ref.ld(pr["Qf"]), ref.ld(pr["q"][s][N])
        for k in range(N - 1, -1, -1):
            g = np.asarray(ref.gamma_at(pr["A"][s][k], pr["B"][s][k], P, w, k), dtype=np.float64)
            c = 1.0 + float(np.linalg.eigvalsh(g[:h, :h]).max())
            for i in range(h):
                pr["hz"][s, k, nxh + i, nxh + i] -= c
                w.hz[k, nxh + i, nxh + i] = pr["hz"][s, k, nxh + i, nxh + i]
            _, _, P, b, _ = ref.solve_tv_lq(pr["A"][s], pr["B"][s], pr["q"][s], pr["r"][s], w, k_begin=k, k_end=k + 1, terminal=(P, b))
    return pr


def lq_zero_pivot_problem(ds, N, S, k_star):
    """Newton model whose gamma at step k_star has a leading pivot that is zero to rounding: HZ[k_star][nxh][nxh] is lowered by the fp64
    value of gamma_{k_star}[0][0], computed from P_{k_star + 1} (Qf for k_star = N - 1, else the long-double sweep's, rounded to fp64).
    An elimination in index order cannot use that pivot; one that searches the column does not notice."""
    pr = lq_special_problem(ds, N, S, "zero pivot %d" % k_star)
    nxh = pr["nxh"]
    for s in range(S):
        if k_star == N - 1:
            P = pr["Qf"]
        else:
            P = np.asarray(lq_reference_sweep(pr, s, k_begin=k_star + 1)[2], dtype=np.float64)
        Bk = pr["B"][s][k_star]
        g00 = pr["R"][0, 0] + pr["hz"][s, k_star, nxh, nxh] + Bk[:, 0].dot(P).dot(Bk[:, 0])
        pr["hz"][s, k_star, nxh, nxh] -= g00
    return pr


def lq_singular_problem(ds, N, S, seed, u, steps):
    """Input u of one seed neither acts nor costs at the given steps: column u of B_k is zero and row / column u of R_k and of HZ_uu are
    zero, so row u of gamma_k is exactly zero in any summation order.  R carries a seed and a step axis ([S][N][nU][nU]) for that."""
    pr = lq_special_problem(ds, N, S, "singular")
    nxh = pr["nxh"]
    R = np.repeat(np.repeat(pr["R"][None, None], S, axis=0), N, axis=1).copy()
    for k in steps:
        pr["B"][seed, k][:, u] = 0.0
        R[seed, k][u, :] = 0.0; R[seed, k][:, u] = 0.0
        pr["hz"][seed, k][nxh + u, :] = 0.0; pr["hz"][seed, k][:, nxh + u] = 0.0
    pr["R_sk"] = R
    return pr
