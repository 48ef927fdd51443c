"""Shared helpers for the parity tests: golden fixtures + the systems they were made from."""
import collections
import functools
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
    "spatial_loop": lambda: systems.spatial_loop(),
    "mixed_loop": lambda: systems.mixed_loop(),
    "ladder_point": lambda: systems.ladder_point(),
    "ladder_mixed": lambda: systems.ladder_mixed(),
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
    "spatial_loop": {1: _ALL, 4: set(), 16: set(), 64: set()},
    "mixed_loop": {1: _ALL, 4: set(), 16: set(), 64: set()},
}


# ---- shared by the oracle-comparison tests of the generic kernels (test_gpu_team_sizes.py, the time-base tests) ------------------------
def starts(name, d, B, N, rng, extra=0):
    """B starts (Q[k], Q[k+1]) of recorded trajectories at random k and the recorded inputs from there on (N + extra steps); forces
    get noise and unconstrained systems a random shift of the dynamic configs, so that every team of a wave has its own path."""
    g = golden(name)
    trajs = trajectories(name)
    nd, nu = d.n_dyn, d.n_inputs
    Q0, Q1, U, K = [], [], [], []
    for b in range(B):
        pre, _, u, kk = trajs[int(rng.integers(len(trajs)))]
        Q = g[pre + "Q"]
        k = int(rng.integers(0, len(Q) - N - extra - 2))
        q0, q1 = Q[k].copy(), Q[k + 1].copy()
        if d.n_constraints == 0:
            shift = 0.2 * rng.standard_normal(nd)
            q0[:nd] += shift
            q1[:nd] += shift
        uu = u[k + 1:k + 1 + N + extra]
        Q0.append(q0)
        Q1.append(q1)
        U.append(uu + 0.5 * rng.standard_normal(uu.shape) if nu else uu)
        K.append(kk[k + 1:k + 1 + N + extra])
    return np.array(Q0), np.array(Q1), np.array(U).reshape(B, N + extra, nu), np.array(K).reshape(B, N + extra, d.n_kin)


def oracle_hz(o, d, z, zl):
    """sum_o z[o] q2_dAdB[o] + z[nq + o] p2_dAdB[o] (+ zl[c] l1_dAdB[c]) from the oracle's full second-derivative tensors."""
    nq, nd, nu, nk, nc = d.n_configs, d.n_dyn, d.n_inputs, d.n_kin, d.n_constraints
    sizes = {"dq1": nq, "dp1": nd, "du1": nu, "dk2": nk}
    offs = {"dq1": 0, "dp1": nq, "du1": nq + nd, "dk2": nq + nd + nu}
    R = nq + nd + nu + nk
    H = np.zeros((R, R))
    for pair in PAIRS:
        a, b = pair[:3], pair[3:]
        if not sizes[a] or not sizes[b]:
            continue
        blk = o.deriv2("q2_" + pair) @ z[:nd] + o.deriv2("p2_" + pair) @ z[nq:nq + nd]
        if nc:
            blk = blk + o.deriv2("l1_" + pair) @ zl
        H[offs[a]:offs[a] + sizes[a], offs[b]:offs[b] + sizes[b]] = blk
        H[offs[b]:offs[b] + sizes[b], offs[a]:offs[a] + sizes[a]] = blk.T
    return H


# ---- the non-uniform time base (tg_batch_set_step_sizes): test_time_base_cpu.py keeps the table honest with the oracle alone and runs
# the emulated generic kernels over it, test_gpu_time_base.py runs it on the device, tools/time_base_parity.py records it.
# system -> (team the generic kernels get, specialised library prebuilt by build(), the path the system is in the table for)
TB_DT = 0.01
TB_N = 24
TB_SYSTEMS = collections.OrderedDict([
    ("pend_on_cart", (4, True, "nu = 1, small team")),
    ("scissor4", (64, True, "8 constraints, fused rates")),
    ("puppet40", (64, True, "18 kinematic configs, 6 constraints, team 64")),
    ("puppet_basic", (64, True, "team 64")),
    ("damper_link", (4, False, "velocity forces")),
    ("spring_arm", (16, False, "SPRINGS, one kinematic config")),
    ("wrench_arm", (16, False, "3 inputs plus one kinematic config")),
    ("puppet_forces", (64, False, "18 inputs")),
    ("plane_link", (16, False, "constraints at a small team")),
])
TB_PATTERNS = ("alternating", "random")
TB_CASES = [(n, p) for n in TB_SYSTEMS for p in TB_PATTERNS]
TB_KINDS = [(n, False) for n in TB_SYSTEMS] + [(n, True) for n in TB_SYSTEMS if TB_SYSTEMS[n][1]]
TB_CLOSED_LOOP = ("pend_on_cart", "wrench_arm", "spring_arm", "puppet_forces", "puppet40")
TB_GROUP = 2                                        # trajectories per gain set of the closed loops
# closed loops: (size of the move of rows 1..N of bX, 1-norm of the config columns of every gain row), chosen per system so that the
# feedback moves X by 1e-6 .. 1e-2 (test_time_base_cpu.py checks it): forces on a heavy puppet move it little, kinematic configs are
# set by their input directly, and on the puppet a move above 1e-4 makes the reference loop itself diverge through the string lengths
TB_LOOP = {"pend_on_cart": (3e-3, 1.0), "wrench_arm": (1e-4, 0.3), "spring_arm": (1e-4, 0.3), "puppet_forces": (3e-2, 1.0),
           "puppet40": (1e-4, 0.1), "mixed_loop": (1e-4, 0.3)}
# another start where the first one is badly conditioned (conditioning rule, test_time_base_cpu.py): of eight scissor-lift draws, the
# 1-ulp floor of X over 24 steps ranges from 3e-13 to 4e-11; this one has 3e-13
TB_START = {"scissor4": 3}
# (case, quantity) whose bound needs the second term of max(tolerance, 64 e_ref) whatever the start and whatever the horizon: the
# scissor lift's multipliers are conditioned by 1 / dt^2 at each step, and the floor does not accumulate along the rollout.  One ulp of
# the start moves lambda1 by (worst of five trajectories and both patterns, per draw of TB_START 0 .. 7)
#   24 steps: 2.7e-11 2.6e-11 1.6e-11 1.0e-11 1.3e-10 1.1e-11 2.3e-11 1.4e-11
#   12 steps: 2.1e-11 1.6e-11 9.8e-12 1.8e-11 1.6e-11 3.4e-11 1.7e-11 1.6e-11
#    6 steps: 2.6e-11 1.5e-11 8.6e-12 1.4e-11 8.5e-12 9.5e-12 1.5e-11 1.4e-11
#    1 step:  5.3e-11 5.8e-11 3.4e-11 6.7e-11 4.4e-11 3.0e-11 3.9e-11 8.1e-11
# so neither another start nor a shorter horizon brings 64 e_ref under 3e-10 (that needs 4.7e-12); draw 3 at 24 steps is the best.
TB_SECOND_TERM = {("scissor4", "lambda1")}
# The project's tolerances per quantity: states 1e-10 (BASELINE north star), the others as in test_gpu_team_sizes.py.  U of a closed
# loop is bU - K (X - bX) with every row of K below one in the 1-norm (tb_closed_loop_inputs): it inherits X's tolerance.
TB_TOL = {"X": 1e-10, "U": 1e-10, "p1": 1e-10, "p2": 1e-10, "calc_p2": 1e-12, "f": 1e-12, "lambda1": 3e-10, "d1": 1e-9, "AB": 1e-9,
          "hz": 1e-8}
_tb = {}


def tb_seed(*key):
    import zlib
    return zlib.crc32(" ".join(str(k) for k in key).encode())


def tb_batch(name):
    """One full block of teams plus a ragged one; 5 at a team of 64 (the closed-loop subset needs two gain groups and a rest)."""
    return max(2 * (64 // TB_SYSTEMS[name][0]) + 1, 5)


def tb_step_sizes(pattern, N=TB_N, name=""):
    """alternating: DT x (0.6, 1.5, 0.6, ...), the largest ratio between neighbours, so a dt taken from the step before or after is as
    wrong as it gets; random: DT x (0.6 + 0.9 r), seeded.  (Nothing below 0.6 DT: momenta and multipliers are conditioned by 1 / dt
    and 1 / dt^2, and the project's tolerances were set at DT.)"""
    if pattern == "alternating":
        return TB_DT * np.where(np.arange(N) % 2 == 0, 0.6, 1.5)
    if pattern == "uniform":                        # (no case of the table: the model-branch cases below, MB_*)
        return np.full(N, TB_DT)
    assert pattern == "random"
    return TB_DT * (0.6 + 0.9 * np.random.default_rng(tb_seed("steps", name)).random(N))       # (a shorter list is a prefix)


def tb_wrong_step_sizes(dts):
    """The three ways of getting the time base wrong that the tests must tell from the right one."""
    return collections.OrderedDict([("uniform mean", np.full(len(dts), dts.mean())), ("one step forward", np.roll(dts, -1)),
                                    ("one step back", np.roll(dts, 1))])


TB_EXTRA = 5                 # steps recorded behind a case's N: a second rollout of the same batch, a list longer than the rollout


def tb_case(name, pattern, N=TB_N, B=None):
    """dict(d, B, N, Q0, Q1, U [B][N][nu], K [B][N][nk], dts [N]) of a case: distinct starts (starts() above); U_all, K_all, dts_all are
    TB_EXTRA steps longer."""
    key = ("case", name, pattern, N, B)
    if key not in _tb:
        _, d = build(name)
        B_ = tb_batch(name) if B is None else B
        Q0, Q1, U, K = starts(name, d, B_, N, np.random.default_rng(tb_seed("starts", name, TB_START.get(name, 0))), extra=TB_EXTRA)
        dts = tb_step_sizes(pattern, N + TB_EXTRA, name)
        _tb[key] = dict(name=name, pattern=pattern, d=d, B=B_, N=N, Q0=Q0, Q1=Q1, U=np.ascontiguousarray(U[:, :N]),
                        K=np.ascontiguousarray(K[:, :N]), dts=dts[:N].copy(), U_all=U, K_all=K, dts_all=dts)
    return _tb[key]


def tb_state(o, dt):
    """X = [q2; p2; (k2 - k1) / dt] of an oracle (DSystem's state, dsystem.py:276-281)."""
    q1, q2 = o.q1, o.q2
    return np.concatenate([q2, o.p2, (q2[o.nd:] - q1[o.nd:]) / dt])


def tb_AB(d, d1, dt):
    """DSystem.fdx / fdu (dsystem.py:284-317) of one step of size dt from the twelve first-derivative blocks [variable][output]."""
    nq, nd, nk, nu = d.n_configs, d.n_dyn, d.n_kin, d.n_inputs
    nX, nU, nqd = nq + nd + nk, nu + nk, nq + nd
    A, B = np.zeros((nX, nX)), np.zeros((nX, nU))
    A[:nd, :nq], A[:nd, nq:nqd] = d1["q2_dq1"].T, d1["q2_dp1"].T
    A[nq:nqd, :nq], A[nq:nqd, nq:nqd] = d1["p2_dq1"].T, d1["p2_dp1"].T
    A[nqd:, nd:nq] = -np.eye(nk) / dt
    B[:nd, :nu], B[:nd, nu:] = d1["q2_du1"].T, d1["q2_dk2"].T
    B[nq:nqd, :nu], B[nq:nqd, nu:] = d1["p2_du1"].T, d1["p2_dk2"].T
    B[nd:nq, nu:] = np.eye(nk)
    B[nqd:, nu:] = np.eye(nk) / dt
    return A, B


def tb_oracle_derivs(o, d, dt, z=None, zl=None):
    """dict(d1, A, B[, hz]) of the oracle's last step (of size dt)."""
    o.calc_deriv1()
    d1 = dict((n, o.deriv1(n)) for n in D1)
    A, B = tb_AB(d, d1, dt)
    out = dict(d1=d1, A=A, B=B)
    if z is not None:
        o.calc_deriv2()
        out["hz"] = oracle_hz(o, d, z, zl)
    return out


def tb_oracle_rollout(d, q0, q1, dts, U=None, K=None, feedback=None, z=None, zl=None, o=None):
    """The reference of every time-base test: OracleMVI from (0, q0, DT, q1) (or a given oracle o, continued), stepped with
    o.step(o.times()[1] + dts[k], ...).  feedback = (Kp [N][nU][nX], bX [N+1][nX], bU [N][nU]): the closed loop U_k = bU_k - K_k (X_k -
    bX_k) with no correction at k = 0 and X_0 = bX_0 by definition of the projection (dsystem.py:441).  z (and zl): also the
    derivatives of the last step.  Every step must converge (OracleError otherwise).  Returns dict(X, U, iterations, o, p1, p2,
    lambda1, f, calc_p2, times[, d1, A, B, hz])."""
    from oracle.oracle import OracleMVI
    if o is None:
        o = OracleMVI(d)
        o.initialize_from_configs(0.0, q0, TB_DT, q1)
    N, nu = len(dts), o.nu
    X = np.zeros((N + 1, o.nq + o.nd + o.nk))
    Uo = np.zeros((N, o.nu + o.nk))
    t1, t2 = o.times()
    X[0] = tb_state(o, t2 - t1) if feedback is None else feedback[1][0]
    its = 0
    for k in range(N):
        if feedback is None:
            Uo[k] = np.concatenate([U[k], K[k]])
        else:
            Kp, bX, bU = feedback
            Uo[k] = bU[k] - (Kp[k].dot(X[k] - bX[k]) if k > 0 else 0.0)
        its += o.step(o.times()[1] + dts[k], Uo[k, :nu], Uo[k, nu:])
        X[k + 1] = tb_state(o, dts[k])
    out = dict(X=X, U=Uo, iterations=its, o=o, p1=o.p1, p2=o.p2, lambda1=o.lambda1, f=o.calc_f(), times=o.times())
    o.calc_p2()                                   # p2 = D2L2(q1, q2) of the last step with t2 - t1 (the solve's own p2 is put back)
    out["calc_p2"] = o.p2
    o.p2 = out["p2"]
    if z is not None:
        out.update(tb_oracle_derivs(o, d, dts[N - 1], z, zl))
    return out


def tb_contraction(name, B):
    """Z [B][nX], ZL [B][nc] of a case's deriv2z checks."""
    _, d = build(name)
    rng = np.random.default_rng(tb_seed("z", name))
    return rng.standard_normal((B, d.n_configs + d.n_dyn + d.n_kin)), rng.standard_normal((B, d.n_constraints))


def tb_reference(name, pattern, N=TB_N, B=None):
    """Open-loop oracle runs of every trajectory of a case (list of tb_oracle_rollout dicts, with derivatives), computed once."""
    key = ("ref", name, pattern, N, B)
    if key not in _tb:
        c = tb_case(name, pattern, N, B)
        Z, ZL = tb_contraction(name, c["B"])
        _tb[key] = [tb_oracle_rollout(c["d"], c["Q0"][b], c["Q1"][b], c["dts"], c["U"][b], c["K"][b], z=Z[b], zl=ZL[b])
                    for b in range(c["B"])]
    return _tb[key]



# The extrapolating predictor accepts a warm start that is already inside the solver's tolerance ball, so its trajectory is the exact
# one only to that tolerance -- and so is the oracle's: at the default 1e-10 the oracle itself is up to 2.7e-10 (pend_on_cart), 2.8e-9
# (plane_link) from the oracle at 1e-11 over the table's 24 steps.  The predictor tests therefore tighten the solver tolerance of both
# sides to 1e-11, the tightest decade at which the reference converges on every step of their systems (at 1e-12 the cart's does not),
# and keep X's tolerance.
TB_PREDICTOR_TOL = 1e-11
TB_PREDICTOR_SYSTEMS = ("pend_on_cart", "spring_arm", "puppet40")       # unconstrained, SPRINGS + a kinematic config, constrained


def tb_predictor_reference(name, pattern, N=TB_N, B=None):
    """Open-loop oracle runs of a case at the solver tolerance TB_PREDICTOR_TOL (every step must converge)."""
    key = ("predref", name, pattern, N, B)
    if key not in _tb:
        from oracle.oracle import OracleMVI
        c = tb_case(name, pattern, N, B)
        out = []
        for b in range(c["B"]):
            o = OracleMVI(c["d"], tolerance=TB_PREDICTOR_TOL)
            o.initialize_from_configs(0.0, c["Q0"][b], TB_DT, c["Q1"][b])
            out.append(tb_oracle_rollout(c["d"], None, None, c["dts"], c["U"][b], c["K"][b], o=o))
        _tb[key] = out
    return _tb[key]


def tb_wave_spread_feedback(d, team, n_items):
    """The condition under which run_trajectory spreads the feedback's gain rows over the wavefront (csrc/mvi_core.hpp, the closed-loop
    branch of the rollout loop); otherwise the per-row loop runs."""
    nX, nU = d.n_configs + d.n_dyn + d.n_kin, d.n_inputs + d.n_kin
    if team != 64 or nU == 0 or 2 * nU > 64:
        return False
    parts = min(4, 64 // nU)
    return nX <= 32 * parts and nX + 4 * nU <= 6 * n_items


def tb_closed_loop_inputs(name, pattern, N=TB_N, B=None):
    """(Kp [groups][N][nU][nX], bX [B][N+1][nX], bU [B][N][nU]) of a case's closed loop, TB_GROUP trajectories per gain set.  bX / bU
    are the oracle's open-loop trajectory on the non-uniform grid; rows 1..N of bX are moved (row 0 is exact: X_0 = bX_0).  Gains:
    random; the config columns of every row have the 1-norm g of TB_LOOP (at most 1: U inherits X's tolerance), the v columns that
    times DT and the p columns that times DT^2 -- feedback on the kinematic configs through momenta and velocities of size 1 / DT makes
    the reference loop itself diverge otherwise."""
    key = ("cl", name, pattern, N, B)
    if key not in _tb:
        c = tb_case(name, pattern, N, B)
        d, Bn = c["d"], c["B"]
        nq, nd, nk, nu = d.n_configs, d.n_dyn, d.n_kin, d.n_inputs
        nX, nU = nq + nd + nk, nu + nk
        move, g = TB_LOOP[name]
        ref = tb_reference(name, pattern, N, B)
        rng = np.random.default_rng(tb_seed("gains", name, pattern))
        bX = np.array([r["X"] for r in ref])
        bX[:, 1:] += move * rng.standard_normal(bX[:, 1:].shape)
        bU = np.array([r["U"] for r in ref])
        groups = (Bn + TB_GROUP - 1) // TB_GROUP
        Kp = rng.standard_normal((groups, N, nU, nX))
        for cols, scale in ((slice(0, nq), g), (slice(nq, nq + nd), g * TB_DT ** 2), (slice(nq + nd, nX), g * TB_DT)):
            if cols.stop > cols.start:
                Kp[..., cols] *= scale / np.abs(Kp[..., cols]).sum(axis=-1, keepdims=True)
        _tb[key] = (Kp, bX, bU)
    return _tb[key]


def tb_closed_loop_reference(name, pattern, N=TB_N, B=None):
    """The numpy loop over oracle steps of every trajectory of a case's closed loop."""
    key = ("clref", name, pattern, N, B)
    if key not in _tb:
        c = tb_case(name, pattern, N, B)
        Kp, bX, bU = tb_closed_loop_inputs(name, pattern, N, B)
        _tb[key] = [tb_oracle_rollout(c["d"], c["Q0"][b], c["Q1"][b], c["dts"], feedback=(Kp[b // TB_GROUP], bX[b], bU[b]))
                    for b in range(c["B"])]
    return _tb[key]


def _ulp(a, sign):
    return np.nextafter(a, sign * np.inf)


def tb_e_ref(name, pattern, N=TB_N, B=None, closed_loop=False):
    """Conditioning floor of a case: the start (q0, q1) of every trajectory moved by one unit in the last place (q0 up, q1 down: the
    start velocity moves most) and the oracle rerun; {quantity: largest relerr against the unperturbed run}.  Taken from the
    reference alone, never from a kernel."""
    key = ("eref", name, pattern, N, B, closed_loop)
    if key not in _tb:
        c = tb_case(name, pattern, N, B)
        out = collections.OrderedDict()

        def worst(q, e):
            out[q] = max(out.get(q, 0.0), e)
        if closed_loop:
            Kp, bX, bU = tb_closed_loop_inputs(name, pattern, N, B)
            ref = tb_closed_loop_reference(name, pattern, N, B)
        else:
            Z, ZL = tb_contraction(name, c["B"])
            ref = tb_reference(name, pattern, N, B)
        for b in range(c["B"]):
            q0, q1 = _ulp(c["Q0"][b], 1.0), _ulp(c["Q1"][b], -1.0)
            if closed_loop:
                r = tb_oracle_rollout(c["d"], q0, q1, c["dts"], feedback=(Kp[b // TB_GROUP], bX[b], bU[b]))
            else:
                r = tb_oracle_rollout(c["d"], q0, q1, c["dts"], c["U"][b], c["K"][b], z=Z[b], zl=ZL[b])
            for q in ("X", "U", "p1", "p2", "lambda1") + (() if closed_loop else ("hz",)):
                worst(q, relerr(r[q], ref[b][q]))
            if not closed_loop:
                worst("d1", max(relerr(r["d1"][n], ref[b]["d1"][n]) for n in D1))
                worst("AB", max(relerr(r["A"], ref[b]["A"]), relerr(r["B"], ref[b]["B"])))
        _tb[key] = out
    return _tb[key]



TB_HORIZON = (2, 5)          # seeds x steps of the one-step-per-trajectory batches: batch = 10, list of 5, so t % count wraps once


def tb_horizon(name, pattern):
    """The horizon batch BatchDOptimizer builds (tg_batch_set_from_trajectories): dict(d, X [S][H+1][nX], U [S][H][nU], dts [H], Z, ZL = 0,
    refs [S * H]) with refs[s * H + k] = the oracle set to X[s][k] (lambda1 = 0), stepped by dts[k] towards the hint X[s][k+1], and its
    derivatives: dict(q2, p2, lambda1, iterations, d1, A, B, hz)."""
    key = ("horizon", name, pattern)
    if key not in _tb:
        from oracle.oracle import OracleMVI
        S, H = TB_HORIZON
        c = tb_case(name, pattern, H, S)
        d, dts = c["d"], c["dts"]
        nq, nd, nu = d.n_configs, d.n_dyn, d.n_inputs
        runs = [tb_oracle_rollout(d, c["Q0"][s], c["Q1"][s], dts, c["U"][s], c["K"][s]) for s in range(S)]
        X, U = np.array([r["X"] for r in runs]), np.array([r["U"] for r in runs])
        Z = np.random.default_rng(tb_seed("zh", name)).standard_normal((S * H, X.shape[2]))
        ZL = np.zeros((S * H, d.n_constraints))
        refs = []
        for s in range(S):
            for k in range(H):
                o = OracleMVI(d)
                o.initialize_from_state(0.0, X[s, k, :nq], X[s, k, nq:nq + nd])
                it = o.step(dts[k], U[s, k, :nu], U[s, k, nu:], q2_hint=X[s, k + 1, :nd])
                r = dict(q2=o.q2, p2=o.p2, lambda1=o.lambda1, iterations=it)
                r.update(tb_oracle_derivs(o, d, dts[k], Z[s * H + k], ZL[s * H + k]))
                refs.append(r)
        _tb[key] = dict(d=d, X=X, U=U, dts=dts, Z=Z, ZL=ZL, refs=refs)
    return _tb[key]


def tb_bound(quantity, e_ref=None):
    """max(project tolerance, 64 e_ref): the rule of the LQ tests, the floor from the reference's own error."""
    return max(TB_TOL[quantity], 64.0 * (e_ref or {}).get(quantity, 0.0))


# ---- model branches only spatial_loop, mixed_loop and the two ladders reach (test_model_branches_cpu.py, test_gpu_model_branches.py,
# test_gpu_world_frame_shapes.py, tools/model_branches_parity.py).  The cases are cases of the machinery above on a uniform time base:
# MB_N steps from starts on the recorded trajectories, the oracle's run as the reference, its response to one ulp of the start as the floor.
MB_N = 12
MB_GENERIC = ("spatial_loop", "mixed_loop")        # the generic kernels, at the team the library gives them
MB_LADDERS = ("ladder_point", "ladder_mixed")      # the specialised world-frame path (team 64)
MB_TEAM = {"spatial_loop": 16, "mixed_loop": 16, "ladder_point": 64, "ladder_mixed": 64}      # test_model_branches_cpu.py holds it to the library's
MB_CLOSED_LOOP = ("mixed_loop",)
# (system, quantity) whose bound needs the second term of max(tolerance, 64 e_ref) (at most one quantity per system;
# test_model_branches_cpu.py asserts that exactly these floors are over the tolerance)
MB_SECOND_TERM = set()


def mb_batch(name):
    """One full block of teams plus a ragged one; 5 at a team of 64."""
    return max(2 * (64 // MB_TEAM[name]) + 1, 5)


def mb_case(name):
    return tb_case(name, "uniform", MB_N, mb_batch(name))


def mb_reference(name):
    return tb_reference(name, "uniform", MB_N, mb_batch(name))


def mb_e_ref(name, closed_loop=False):
    return tb_e_ref(name, "uniform", MB_N, mb_batch(name), closed_loop=closed_loop)


def mb_bound(name, quantity, e_ref):
    return tb_bound(quantity, e_ref) if (name, quantity) in MB_SECOND_TERM else TB_TOL[quantity]


def mb_contraction(name):
    return tb_contraction(name, mb_batch(name))


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


# ---- the forward-mode (dual-number) kernels of the continuous dynamics (k_forward, run_forward, csrc/dual.hpp): test_forward_cpu.py
# keeps the table honest with the oracle alone and runs the emulated kernels over it, test_gpu_forward.py runs it on the device,
# tools/forward_parity.py records it.  A kernel's output along variable v (numbered q | dq | ddq_k | u) is the directional derivative of
# arrays the oracle has in analytic form (OracleMVI.dynamics_deriv1 / lagrangian); the reference is a Richardson-extrapolated central
# difference of those arrays, accumulated in long double (fw_ladder), nested for two directions.
FW_KERNELS = ("dyn", "lag1", "lag2")        # MODE_DYN_DERIV1 on Dual<double>, MODE_LAGRANGIAN on Dual<double> and on Dual<Dual<double>>
FW_DYN_NAMES = ("f_dq", "f_ddq", "f_dddk", "f_du", "lambda_dq", "lambda_ddq", "lambda_dddk", "lambda_du")
FW_LAG_NAMES = ("L_dq", "L_ddq", "L_dqdq", "L_ddqdq", "L_ddqddq")
FW_TOL = {"dyn": 1e-10, "lag1": 1e-12, "lag2": 1e-12}       # the project's figures (test_dynamics.py)
FW_FLOOR = {"dyn": 1e-10 / 64, "lag1": 1e-12 / 64, "lag2": 1e-12 / 64}
FW_BLOCKS = ("q", "dq", "ddq_k", "u")
# system -> (trajectories, scale of the noise on the golden q); dq, ddq_k and u get unit-normal draws.
FW_SYSTEMS = collections.OrderedDict([
    ("pend_on_cart", (24, 0.05)),
    ("scissor4", (24, 0.05)),
    ("puppet40", (12, 0.05)),
    ("puppet_basic", (12, 0.05)),
    ("plane_link", (24, 0.05)),
    ("spring_arm", (24, 0.05)),
    ("spring_link", (24, 0.05)),
    ("dual_pendulums", (24, 0.05)),
    ("damper_link", (24, 0.05)),
    ("nonlinear_spring_arm", (24, 0.05)),
    ("wrench_arm", (24, 0.05)),
    ("wrench_spatial", (24, 0.05)),
    ("wrench_body", (24, 0.05)),
    ("puppet_forces", (12, 0.05)),
    ("extensor_tendon", (24, 0.05)),
    ("spatial_loop", (24, 0.05)),
    ("mixed_loop", (24, 0.05)),
])
FW_CASES = [(n, k) for n in FW_SYSTEMS for k in FW_KERNELS]
# The ladder: (base step along a q variable, halvings) per kernel, and per (system, kernel) where the default misses the floor rule of
# test_forward_cpu.py.  Along q the arrays are trigonometric (the scissor lift's and the puppets' steeply so): the step trades the
# truncation the extrapolation leaves against the rounding of the oracle's fp64 arrays, eps / h per direction.  Along dq, ddq_k and u
# every array is a polynomial of degree <= 2, so a central difference is exact at any step and the large FW_STEP_V keeps the rounding
# small.
FW_STEP_V = 0.5
FW_LADDER_DEFAULT = {"dyn": (0.08, 3), "lag1": (0.16, 3), "lag2": (0.16, 3)}
FW_LADDER = {("scissor4", "dyn"): (0.02, 3), ("scissor4", "lag2"): (0.32, 3), ("plane_link", "dyn"): (0.08, 5), ("damper_link", "dyn"): (0.02, 3),
             ("puppet_basic", "lag2"): (0.32, 3),
             ("nonlinear_spring_arm", "dyn"): (0.01, 3), ("nonlinear_spring_arm", "lag1"): (0.005, 2), ("nonlinear_spring_arm", "lag2"): (0.01, 2),
             ("dual_pendulums", "dyn"): (0.16, 5), ("dual_pendulums", "lag1"): (0.08, 4), ("spring_link", "lag1"): (0.16, 4), ("dual_pendulums", "lag2"): (0.16, 5),
             ("extensor_tendon", "dyn"): (0.16, 4), ("extensor_tendon", "lag1"): (0.16, 4), ("extensor_tendon", "lag2"): (0.08, 3),
             # spatial_loop's telescopic branch hangs on the axis of its rz joint: near its recorded states the mass matrix is close to singular
             # in that config, and the dynamics' arrays have a pole a few hundredths away along q.  The default step reaches across it (floor of
             # f_dq 3.6e-2); the floor falls with the eighth power of the step down to 0.005 and stays at 1e-11 .. 5e-11 (rounding) below
             ("spatial_loop", "dyn"): (0.005, 3)}


def fw_ladder_of(name, kernel):
    return FW_LADDER.get((name, kernel), FW_LADDER_DEFAULT[kernel])
# another draw where the first one fails the sensitivity rule of test_forward_cpu.py: (system, kernel) -> draw number
# (puppet_basic: seven of twelve references of draw 0 are under the bound.  nonlinear_spring_arm: a ladder that straddles a knot of one of
# the force splines differences a kink, and the floor of such a trajectory is 1e-6 ... 1e-3; these are draws on which no ladder does)
# mixed_loop: the (dq, q) pairs of draw 0 all join configs of different chains, whose mixed derivatives are zero -- draw 1 reaches that block)
FW_DRAW = {("puppet_basic", "lag2"): 1, ("nonlinear_spring_arm", "lag1"): 4, ("nonlinear_spring_arm", "lag2"): 3, ("mixed_loop", "lag2"): 1}
# (system, kernel, array) whose bound needs the second term of max(tolerance, 64 e_ref): measured floor e_ref (test_forward_cpu.py
# asserts that exactly these are over FW_FLOOR, and each under twice the figure here)
FW_SECOND_TERM = {
    ("pend_on_cart", "lag1"): {"L_dq": 1.7e-14, "L_ddq": 6.0e-14, "L_dqdq": 7.2e-14},
    ("pend_on_cart", "lag2"): {"L_dq": 4.8e-12, "L_ddq": 1.1e-11, "L_dqdq": 2.6e-12, "L_ddqdq": 6.2e-13, "L_ddqddq": 7.2e-13},
    ("scissor4", "dyn"): {"f_dq": 2.2e-11, "f_ddq": 2.4e-11, "lambda_dq": 4.1e-11, "lambda_ddq": 2.1e-11},
    ("scissor4", "lag1"): {"L_dq": 1.1e-13, "L_ddq": 2.0e-13, "L_dqdq": 1.9e-13, "L_ddqdq": 1.3e-13, "L_ddqddq": 5.3e-14},
    ("scissor4", "lag2"): {"L_dq": 3.5e-11, "L_ddq": 9.8e-12, "L_dqdq": 1.1e-11, "L_ddqdq": 7.7e-12, "L_ddqddq": 9.7e-13},
    ("puppet40", "dyn"): {"f_dq": 4.2e-12, "lambda_dq": 9.7e-12},
    ("puppet40", "lag1"): {"L_dq": 9.7e-14, "L_ddq": 1.6e-13, "L_dqdq": 1.0e-13, "L_ddqdq": 1.1e-13, "L_ddqddq": 2.1e-13},
    ("puppet40", "lag2"): {"L_dq": 2.2e-11, "L_ddq": 6.3e-12, "L_dqdq": 4.0e-12, "L_ddqdq": 4.5e-12, "L_ddqddq": 4.5e-12},
    ("puppet_basic", "dyn"): {"f_dq": 5.8e-12, "f_ddq": 5.0e-12, "lambda_dq": 2.6e-12, "lambda_ddq": 2.2e-12},
    ("puppet_basic", "lag1"): {"L_dq": 8.2e-13, "L_ddq": 2.0e-13, "L_dqdq": 7.8e-13, "L_ddqdq": 1.5e-13, "L_ddqddq": 4.9e-13},
    ("puppet_basic", "lag2"): {"L_dq": 7.7e-11, "L_ddq": 2.5e-11, "L_dqdq": 5.2e-11, "L_ddqdq": 5.4e-11, "L_ddqddq": 1.4e-11},
    ("plane_link", "dyn"): {"f_ddq": 2.1e-12},
    ("plane_link", "lag1"): {"L_dq": 1.6e-13, "L_ddq": 3.1e-14, "L_dqdq": 1.9e-13, "L_ddqdq": 7.4e-14, "L_ddqddq": 2.0e-14},
    ("plane_link", "lag2"): {"L_dq": 5.2e-12, "L_ddq": 9.3e-13, "L_dqdq": 1.2e-11, "L_ddqdq": 1.7e-12, "L_ddqddq": 1.2e-12},
    ("spring_arm", "lag1"): {"L_dq": 8.2e-14, "L_ddq": 6.0e-14, "L_dqdq": 2.3e-13, "L_ddqdq": 1.0e-13, "L_ddqddq": 4.8e-14},
    ("spring_arm", "lag2"): {"L_dq": 1.5e-11, "L_ddq": 2.5e-12, "L_dqdq": 2.6e-11, "L_ddqdq": 5.1e-12, "L_ddqddq": 7.9e-12},
    ("spring_link", "lag1"): {"L_dq": 1.7e-13, "L_ddq": 6.6e-14, "L_dqdq": 9.4e-14, "L_ddqdq": 5.1e-14, "L_ddqddq": 1.0e-13},
    ("spring_link", "lag2"): {"L_dq": 2.9e-11, "L_ddq": 1.2e-12, "L_dqdq": 3.7e-11, "L_ddqdq": 1.4e-12, "L_ddqddq": 4.8e-13},
    ("dual_pendulums", "dyn"): {"f_dq": 2.7e-12},
    ("dual_pendulums", "lag1"): {"L_dq": 2.7e-14, "L_dqdq": 2.3e-12},
    ("dual_pendulums", "lag2"): {"L_dq": 3.3e-10, "L_dqdq": 2.9e-10},
    ("damper_link", "lag1"): {"L_dq": 5.2e-14, "L_ddq": 7.8e-14, "L_dqdq": 3.8e-14, "L_ddqdq": 6.5e-14, "L_ddqddq": 3.9e-14},
    ("damper_link", "lag2"): {"L_dq": 6.4e-12, "L_ddq": 6.8e-12, "L_dqdq": 5.5e-12, "L_ddqdq": 1.7e-12, "L_ddqddq": 9.5e-12},
    ("nonlinear_spring_arm", "dyn"): {"f_ddq": 2.6e-12},
    ("nonlinear_spring_arm", "lag1"): {"L_dq": 4.0e-13, "L_ddq": 5.3e-13, "L_dqdq": 1.0e-12, "L_ddqdq": 1.1e-12, "L_ddqddq": 1.1e-12},
    ("nonlinear_spring_arm", "lag2"): {"L_dq": 4.0e-10, "L_ddq": 4.7e-10, "L_dqdq": 1.3e-09, "L_ddqdq": 5.2e-10, "L_ddqddq": 3.3e-10},
    ("wrench_arm", "lag1"): {"L_dq": 1.6e-13, "L_ddq": 1.3e-13, "L_dqdq": 6.0e-14, "L_ddqdq": 6.4e-14, "L_ddqddq": 3.8e-14},
    ("wrench_arm", "lag2"): {"L_dq": 8.6e-12, "L_ddq": 1.4e-11, "L_dqdq": 7.1e-12, "L_ddqdq": 5.5e-12, "L_ddqddq": 3.8e-12},
    ("wrench_spatial", "lag1"): {"L_dq": 7.6e-14, "L_ddq": 5.3e-14, "L_dqdq": 1.5e-13, "L_ddqdq": 1.1e-13, "L_ddqddq": 6.1e-14},
    ("wrench_spatial", "lag2"): {"L_dq": 4.9e-12, "L_ddq": 4.5e-12, "L_dqdq": 8.3e-12, "L_ddqdq": 3.1e-12, "L_ddqddq": 4.0e-12},
    ("wrench_body", "lag1"): {"L_dq": 5.0e-14, "L_ddq": 7.0e-14, "L_dqdq": 1.1e-13, "L_ddqdq": 4.6e-14, "L_ddqddq": 3.8e-14},
    ("wrench_body", "lag2"): {"L_dq": 9.1e-12, "L_ddq": 9.8e-12, "L_dqdq": 1.2e-11, "L_ddqdq": 8.3e-12, "L_ddqddq": 9.6e-12},
    ("puppet_forces", "lag1"): {"L_dq": 1.6e-13, "L_ddq": 1.8e-13, "L_dqdq": 8.4e-14, "L_ddqdq": 1.4e-13, "L_ddqddq": 8.1e-14},
    ("puppet_forces", "lag2"): {"L_dq": 2.7e-11, "L_ddq": 1.6e-11, "L_dqdq": 1.3e-11, "L_ddqdq": 9.1e-12, "L_ddqddq": 5.8e-12},
    ("extensor_tendon", "dyn"): {"f_dq": 6.1e-12, "f_ddq": 3.4e-12},
    ("extensor_tendon", "lag1"): {"L_dq": 5.1e-13, "L_ddq": 7.7e-13, "L_dqdq": 7.3e-13, "L_ddqdq": 1.2e-13, "L_ddqddq": 4.6e-13},
    ("extensor_tendon", "lag2"): {"L_dq": 1.3e-10, "L_ddq": 1.0e-10, "L_dqdq": 1.1e-10, "L_ddqdq": 3.1e-11, "L_ddqddq": 1.5e-10},
    ("spatial_loop", "dyn"): {"f_dq": 2.6e-11, "f_ddq": 6.6e-12, "f_dddk": 9.2e-12, "lambda_dq": 1.4e-11, "lambda_ddq": 1.7e-12},
    ("spatial_loop", "lag1"): {"L_dq": 1.5e-13, "L_ddq": 8.9e-14, "L_dqdq": 2.6e-13, "L_ddqdq": 1.3e-13, "L_ddqddq": 7.3e-14},
    ("spatial_loop", "lag2"): {"L_dq": 2.7e-12, "L_ddq": 4.0e-12, "L_dqdq": 2.6e-11, "L_ddqdq": 1.1e-12, "L_ddqddq": 4.2e-12},
    ("mixed_loop", "dyn"): {"f_dq": 1.8e-12},
    ("mixed_loop", "lag1"): {"L_dq": 1.7e-14, "L_ddq": 1.4e-13, "L_dqdq": 5.6e-13, "L_ddqddq": 1.3e-13},
    ("mixed_loop", "lag2"): {"L_dq": 2.0e-12, "L_ddq": 2.3e-12, "L_dqdq": 1.9e-11, "L_ddqdq": 2.8e-12, "L_ddqddq": 8.5e-13},
}


def fw_golden_states(name):
    """The recorded configurations the draws are made near: the states of dynamics.npz, or (the two systems it does not have) every
    fifth configuration of the system's recorded trajectory."""
    g = dict(np.load(os.path.join(GOLDEN, "dynamics.npz"))) if "dynamics" not in _cache else _cache["dynamics"]
    _cache["dynamics"] = g
    if name + "_q" in g:
        return g[name + "_q"]
    return golden(name)["b0_Q"][::5][:4]


def fw_sizes(d):
    nq, nk, nu = d.n_configs, d.n_kin, d.n_inputs
    return nq, nk, nu, 2 * nq + nk + nu


def fw_block(d, v):
    """Index into FW_BLOCKS of direction variable v (None for -1)."""
    nq, nk, nu, nvar = fw_sizes(d)
    if v < 0:
        return None
    return 0 if v < nq else (1 if v < 2 * nq else (2 if v < 2 * nq + nk else 3))


def fw_neighbour(d, kernel, v):
    """The variable next to v (the one before the last): what a seed offset that is off by one would follow."""
    nq, nk, nu, nvar = fw_sizes(d)
    top = nvar if kernel == "dyn" else 2 * nq
    return v + 1 if v + 1 < top else v - 1


@functools.lru_cache(maxsize=None)
def fw_case(name, kernel):
    """dict(d, B, Q, dQ, U, ddK, seeds) of a case: every trajectory has its own state (golden q plus noise, unit-normal dq, u, ddq_k) and
    its own direction(s); seeds = (s1,) or, for "lag2", (s1, s2).  Over the case the seeds cover the first and the last variable of
    every block the system has (dyn: q | dq | ddq_k | u, "lag1": q | dq); "lag2" has the pairs (q, q) with equal and unequal indices,
    (q, dq), (dq, q), (dq, dq) and (v, -1).  Trajectory 2 has no direction (-1) and the last trajectory is an
    exact copy of an earlier one whose derivative is not zero (duplicates = (earlier, last)).  The arrays are read-only."""
    _, d = build(name)
    B, scale = FW_SYSTEMS[name]
    nq, nk, nu, nvar = fw_sizes(d)
    rng = np.random.default_rng(tb_seed("fw", name, kernel, FW_DRAW.get((name, kernel), 0)))
    gq = fw_golden_states(name)
    Q = gq[rng.integers(len(gq), size=B)] + scale * rng.standard_normal((B, nq))
    dQ, U, ddK = rng.standard_normal((B, nq)), rng.standard_normal((B, nu)), rng.standard_normal((B, nk))
    q0, q1, v0, v1 = 0, nq - 1, nq, 2 * nq - 1
    if kernel == "dyn":
        must = [(v,) for lo, hi in ((0, nq), (nq, 2 * nq), (2 * nq, 2 * nq + nk), (2 * nq + nk, nvar)) if hi > lo for v in (lo, hi - 1)]
        top, width = nvar, 1
    elif kernel == "lag1":
        must, top, width = [(q0,), (q1,), (v0,), (v1,)], 2 * nq, 1
    else:
        # (random dynamic configs instead of the first and last variable: on the puppets those are a translation and a string length, which
        # the Lagrangian's third and fourth derivatives do not see)
        must = []
        for _ in range(2):
            a, b = (int(x) for x in rng.choice(d.n_dyn, size=2, replace=False))
            must += [(a, a), (a, b), (a, nq + b), (nq + a, b)]
        must += [(nq + a, nq + b), (b, -1)]
        top, width = 2 * nq, 2
    assert len(must) + 2 <= B
    if kernel == "dyn":
        free = [(int(rng.integers(0, top)),) for _ in range(B - 2 - len(must))]
    elif kernel == "lag1":
        # (free directions: the dynamic configurations and their velocities -- the Lagrangian does not see a massless string length)
        free = [(int(rng.integers(0, d.n_dyn) + nq * rng.integers(0, 2)),) for _ in range(B - 2 - len(must))]
    else:
        # (free pairs: a variable of q | dq and a configuration next to its own -- coupled in a linkage, where two drawn at random
        # mostly are not, and two velocities leave only L_dqdq)
        free = []
        for _ in range(B - 2 - len(must)):
            a = int(rng.integers(0, top))
            free.append((a, int(np.clip(a % nq + rng.integers(-1, 2), 0, nq - 1))))
    rows = must + free
    rows = [rows[i] for i in rng.permutation(len(rows))]
    rows.insert(2, (-1,) * width)
    # the trajectory that is repeated: the first whose derivative is there to be compared (one plain central difference of the oracle's
    # arrays has an entry above 1e-6), so that equal bits are not equal zeros
    from oracle.oracle import OracleMVI
    o, names = OracleMVI(d), FW_DYN_NAMES if kernel == "dyn" else FW_LAG_NAMES
    probe = lambda b: fw_derivative(name, kernel, np.concatenate([Q[b], dQ[b], ddK[b], U[b]]), rows[b], o, d, (fw_ladder_of(name, kernel)[0], 0))[0]
    dup = next(b for b in range(1, B - 1) if min(rows[b]) >= 0 and max(np.abs(a).max(initial=0.0) for a in probe(b).values()) > 1e-6)
    rows.append(rows[dup])
    for a in (Q, dQ, U, ddK):
        a[B - 1] = a[dup]
    S = np.array(rows, dtype=np.int32)
    out = dict(name=name, kernel=kernel, d=d, B=B, Q=Q, dQ=dQ, U=U, ddK=ddK, seeds=tuple(np.ascontiguousarray(S[:, i]) for i in range(width)),
               duplicates=(dup, B - 1), names=names)
    for a in (Q, dQ, U, ddK) + out["seeds"]:
        a.setflags(write=False)
    return out


def fw_x(c, b):
    """The state of trajectory b as one vector in the numbering of the direction variables: q | dq | ddq_k | u."""
    return np.concatenate([c["Q"][b], c["dQ"][b], c["ddK"][b], c["U"][b]])


def fw_oracle_arrays(o, kernel, x):
    """The oracle's analytic arrays at x = q | dq | ddq_k | u as one flat long-double vector (fw_split undoes it): the eight first-derivative
    arrays of the continuous dynamics ("dyn", [output][variable] each), or L_dq, L_ddq, L_dqdq, L_ddqdq, L_ddqddq."""
    nq, nk = o.nq, o.nk
    q, dq = x[:nq], x[nq:2 * nq]
    if kernel == "dyn":
        r = o.dynamics_deriv1(q, dq, x[2 * nq + nk:], x[2 * nq:2 * nq + nk])
        parts = [r[n.replace("lambda_", "lam_")] for n in FW_DYN_NAMES]
    else:
        parts = o.lagrangian(q, dq)
    return np.concatenate([np.asarray(p, dtype=np.longdouble).ravel() for p in parts])


def fw_split(d, kernel, flat):
    """dict of the arrays of a flat vector, in the layout of BatchMidpointVI.dynamics_deriv1 / lagrangian for one trajectory."""
    nq, nd, nk, nu, nc = d.n_configs, d.n_dyn, d.n_kin, d.n_inputs, d.n_constraints
    if kernel == "dyn":
        shapes = [(o_, w) for o_ in (nd, nc) for w in (nq, nq, nk, nu)]
        names = FW_DYN_NAMES
    else:
        shapes, names = [(nq,), (nq,), (nq, nq), (nq, nq), (nq, nq)], FW_LAG_NAMES
    out, at = {}, 0
    for n, s in zip(names, shapes):
        size = int(np.prod(s))
        out[n] = np.asarray(flat[at:at + size], dtype=np.float64).reshape(s)
        at += size
    return out


def fw_ladder(fun, x, v, h, levels):
    """Richardson-extrapolated central difference of fun (-> long-double array) along variable v of x: the steps h / 2^k, k = 0 ..
    levels + 1, each divided by the step actually taken, x+ - x-; returns the extrapolation of steps 0 .. levels (the reference) and
    that of steps 1 .. levels + 1 (its rival: the two base steps differ by a factor of two, their disagreement is the floor e_ref)."""
    D = []
    for k in range(levels + 2):
        xp, xm = x.copy(), x.copy()
        xp[v] += h / 2.0 ** k
        xm[v] -= h / 2.0 ** k
        D.append((fun(xp) - fun(xm)) / (np.longdouble(xp[v]) - np.longdouble(xm[v])))

    def extrapolate(T):
        j = 1
        while len(T) > 1:
            T = [T[i + 1] + (T[i + 1] - T[i]) / (np.longdouble(4.0) ** j - 1) for i in range(len(T) - 1)]
            j += 1
        return T[0]
    return extrapolate(D[:levels + 1]), extrapolate(D[1:])


def fw_derivative(name, kernel, x, seeds, o=None, d=None, ladder=None):
    """(reference, rival) dicts of arrays: the derivative of the oracle's arrays at x along seeds = (v,) or nested along (v1, v2), by the
    ladder at the system's base step and at half of it.  A -1 among the seeds: zeros.  (d, ladder: a system outside the table.)"""
    if d is None:
        _, d = build(name)
    if o is None:
        from oracle.oracle import OracleMVI
        o = OracleMVI(d)
    hq, levels = ladder or fw_ladder_of(name, kernel)
    step = lambda v: hq if v < d.n_configs else FW_STEP_V
    base = lambda y: fw_oracle_arrays(o, kernel, y)
    x = np.asarray(x, dtype=np.float64)
    if min(seeds) < 0:
        z = np.zeros_like(base(x))
        return fw_split(d, kernel, z), fw_split(d, kernel, z)
    if len(seeds) == 1:
        a, b = fw_ladder(base, x, seeds[0], step(seeds[0]), levels)
    else:
        inner = lambda y: np.stack(fw_ladder(base, y, seeds[0], step(seeds[0]), levels))
        (a, _), (_, b) = fw_ladder(inner, x, seeds[1], step(seeds[1]), levels)
    return fw_split(d, kernel, a), fw_split(d, kernel, b)


@functools.lru_cache(maxsize=None)
def fw_reference(name, kernel):
    """Per trajectory of a case (reference, rival) of fw_derivative, computed once."""
    from oracle.oracle import OracleMVI
    c = fw_case(name, kernel)
    o = OracleMVI(c["d"])
    return [fw_derivative(name, kernel, fw_x(c, b), tuple(int(s[b]) for s in c["seeds"]), o) for b in range(c["B"])]


@functools.lru_cache(maxsize=None)
def fw_e_ref(name, kernel):
    """{array: floor} of a case: the largest relerr between the ladders of the two base steps.  From the reference alone."""
    c = fw_case(name, kernel)
    return collections.OrderedDict((n, max(relerr(alt[n], ref[n]) for ref, alt in fw_reference(name, kernel))) for n in c["names"])


def fw_bound(name, kernel, array):
    """max(project tolerance, 64 e_ref)"""
    return max(FW_TOL[kernel], 64.0 * fw_e_ref(name, kernel)[array])


def fw_errors(name, kernel, got):
    """{array: worst relerr over the trajectories} of got = {array: [B][...]} against the reference."""
    ref = fw_reference(name, kernel)
    return collections.OrderedDict((n, max(relerr(got[n][b], ref[b][0][n]) for b in range(len(ref)))) for n in fw_case(name, kernel)["names"])


# ---- the LDS limit of the forward-mode kernels: one wavefront per trajectory, the slice is sizeof(Real) / 8 times the double kernel's
FW_LDS_LIMIT = 160 * 1024
FW_REAL_BYTES = {"dyn": 16, "lag1": 16, "lag2": 32}


def fw_lds_bytes(d, kernel):
    """The LDS block launch_forward_mode asks for (csrc/trepamd.hip), from the host emulation's slice sizes."""
    import emu_harness
    s = emu_harness.lds_slices(d)
    per_team = max(s["rollout"], s["dynamics_deriv1"]) if kernel == "dyn" else s["rollout"]
    return per_team * FW_REAL_BYTES[kernel]


@functools.lru_cache(maxsize=None)
def fw_chain(links):
    from trep_amd import systems
    system = systems.pendulum(links)
    return system, descriptor.flatten(system)


@functools.lru_cache(maxsize=None)
def fw_chain_limit(kernel, most=64):
    """The shortest n-link pendulum (the chain of test_long_chain_matches_oracle) whose forward-mode block is over the limit, by
    bisection (the slice grows with the chain); None if a chain of `most` links still fits."""
    over = lambda n: fw_lds_bytes(fw_chain(n)[1], kernel) > FW_LDS_LIMIT
    if not over(most):
        return None
    lo, hi = 1, most                      # lo fits, hi does not
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if over(mid) else (mid, hi)
    return hi


@functools.lru_cache(maxsize=None)
def fw_chain_case(kernel, links, B=3):
    """B states of the chain with a direction in q, in dq and in q again (lag2: a (q, q), a (q, dq) and a (dq, dq) pair), and their
    (reference, rival) by the default ladder of the kernel."""
    from oracle.oracle import OracleMVI
    _, d = fw_chain(links)
    rng = np.random.default_rng(tb_seed("fw chain", kernel, links))
    Q, dQ = rng.uniform(-0.6, 0.6, (B, links)), 0.3 * rng.standard_normal((B, links))
    a, b = (int(x) for x in rng.choice(links, size=2, replace=False))
    rows = [(a,), (links + b,), (links - 1,)] if kernel != "lag2" else [(a, b), (b, links + a), (links + a, links + b)]
    S = np.array(rows[:B], dtype=np.int32)
    o = OracleMVI(d)
    c = dict(d=d, B=B, Q=Q, dQ=dQ, U=np.zeros((B, 0)), ddK=np.zeros((B, 0)), seeds=tuple(np.ascontiguousarray(S[:, i]) for i in range(S.shape[1])),
             names=FW_DYN_NAMES if kernel == "dyn" else FW_LAG_NAMES)
    c["reference"] = [fw_derivative(None, kernel, fw_x(c, t), tuple(int(s_[t]) for s_ in c["seeds"]), o, d, FW_LADDER_DEFAULT[kernel]) for t in range(B)]
    c["e_ref"] = dict((n, max(relerr(alt[n], ref[n]) for ref, alt in c["reference"])) for n in c["names"])
    return c
