"""Specification of the batched inverse dynamics (BatchMidpointVI.inverse_dynamics, csrc/mvi_inverse.hpp): numpy on the oracle alone.

For every step (b, k) of a path Q [B][N+1][nq] with step sizes dts [N]:
  p_k  = p0[b] (k = 0; zero when absent) or the oracle's calc_p2 of the pair (Q[k-1], Q[k]) with dt[k-1];
  r0,h = the oracle's calc_f of the pair (Q[k], Q[k+1]) with p1 = p_k, u1 = 0, lambda1 = 0 and dt[k];
  A~   = the exact differences calc_f(e_i) - r0: input columns with u1 = e_i / dt[k] (a unit IMPULSE), multiplier columns with
         lambda1 = e_c.  The residual is affine in (u, lambda): checked against a random (u, lambda) within AFFINITY;
  z~   = argmin |r0 + A~ z|^2 + ridge |z|^2, by QR least squares on the stacked [A~; sqrt(ridge) I] -- the answer -- and by the
         augmented system [[I, A~], [A~', -ridge I]] in fp64, the kernel's formulation.  Their difference is the floor e_ref.
Outputs as the kernel's: U = z~_u / dt[k], lam, rho = r0 + A~ z~, h, P[k+1] = calc_p2 of the pair (Q[k], Q[k+1]), P[0] = p0.
Without p0 step 0 is not solved: P[0] = -r0 at p = 0, U = lam = rho = 0.

The case table (CASES) is what the emulated kernel (test_inverse_dynamics_cpu.py), the device (test_gpu_inverse_dynamics.py) and
tools/inverse_dynamics_parity.py run.  Bound of a case and quantity: max(1e-10, 64 e_ref) relative to max(1, |z~|inf)."""
import collections

import numpy as np

import common
from oracle.oracle import OracleMVI

OK, SINGULAR = 0, 2
DT = common.TB_DT
AFFINITY = 1e-13
TOL, MARGIN = 1e-10, 64.0
NOISE = 1e-3                     # off-path noise on the dynamic configs of unconstrained systems, so that rho != 0
B, N = 5, 13                     # 65 teams: one full block of teams plus a ragged one at TEAM = 1

Case = collections.namedtuple("Case", "name B N ridge pattern covers")
CASES = [
    Case("pend_on_cart", B, N, 0.0, "uniform", "underactuated, rho != 0"),
    Case("wrench_arm", B, N, 0.0, "uniform", "HybridWrench, nu = nd, a kinematic slider"),
    Case("wrench_spatial", B, N, 0.0, "uniform", "SpatialWrench"),
    Case("wrench_body", B, N, 0.0, "uniform", "BodyWrench"),
    Case("wrench_torque", B, N, 0.0, "uniform", "wrench torques"),
    Case("scissor4", B, N, 0.0, "uniform", "nc = 8, no inputs"),
    Case("spatial_loop", B, N, 0.0, "uniform", "a 3-D loop"),
    Case("spring_link", B, N, 0.0, "uniform", "the SPRINGS instantiation"),
    Case("mixed_loop", B, N, 1e-4, "uniform", "n > nd: ridge"),
    Case("puppet_forces", B, N, 1e-4, "uniform", "rank-deficient: ridge"),
    Case("puppet40", 3, 5, 0.0, "uniform", "team 64; the parameter twin"),
    Case("pend_on_cart", B, N, 0.0, "alternating", "non-uniform by-step list"),
    Case("scissor4", B, N, 0.0, "alternating", "non-uniform by-step list, constraints"),
]
Result = collections.namedtuple("Result", "U lam P rho h status z z_aug rho_aug A r0")
FIELDS = ("U", "lam", "P", "rho", "h", "status")
_cache = {}


def case_id(c):
    return "%s_%dx%d%s%s" % (c.name, c.B, c.N, "_ridge" if c.ridge else "", "" if c.pattern == "uniform" else "_" + c.pattern)


def step_sizes(c):
    return common.tb_step_sizes(c.pattern, c.N, c.name)


def case_paths(c):
    """dict(d, dts [N], Q [B][N+1][nq] the table's paths, Q_clean the oracle's own rollouts, p0 [B][nd] their incoming momenta, U [B][N][nu]
    the applied (noisy) inputs, lam [B][N][nc] the rollouts' multipliers): every row its own start on a recorded trajectory."""
    key = ("paths", case_id(c))
    if key not in _cache:
        _, d = common.build(c.name)
        rng = np.random.default_rng(common.tb_seed("inverse dynamics", c.name, c.pattern))
        Q0, Q1, U, K = common.starts(c.name, d, c.B, c.N, rng)
        dts = step_sizes(c)
        nd = int(d.n_dyn)
        Q, P0, LAM = [], [], []
        for b in range(c.B):
            o = OracleMVI(d)
            o.initialize_from_configs(0.0, Q0[b], DT, Q1[b])
            P0.append(o.p2)
            q, lam = [o.q2], []
            for k in range(c.N):
                o.step(o.times()[1] + dts[k], U[b, k], K[b, k])
                q.append(o.q2)
                lam.append(o.lambda1)
            Q.append(q)
            LAM.append(lam)
        clean = np.array(Q)
        noisy = clean.copy()
        if int(d.n_constraints) == 0:
            noisy[:, :, :nd] += NOISE * rng.standard_normal(noisy[:, :, :nd].shape)
        _cache[key] = dict(d=d, dts=dts, Q=noisy, Q_clean=clean, p0=np.array(P0), U=U, lam=np.array(LAM).reshape(c.B, c.N, int(d.n_constraints)))
    return _cache[key]


# what a mutated reference gets wrong (test_inverse_dynamics_cpu.py): each names one ingredient of a step
SPEC = dict(dh_at_next=False, p_from_same_pair=False, dt_twice=False)


def solve_step(A, r0, ridge):
    """(z by QR on the stacked system, z by the augmented system, rho of each)."""
    nd, n = A.shape
    if n == 0:
        return np.zeros(0), np.zeros(0), r0.copy(), r0.copy()
    stacked = np.vstack([A, np.sqrt(ridge) * np.eye(n)]) if ridge > 0 else A
    rhs = np.concatenate([-r0, np.zeros(n)]) if ridge > 0 else -r0
    Qm, R = np.linalg.qr(stacked)
    z = np.linalg.solve(R, Qm.T.dot(rhs))
    Kk = np.block([[np.eye(nd), A], [A.T, -ridge * np.eye(n)]])
    x = np.linalg.solve(Kk, np.concatenate([-r0, np.zeros(n)]))
    return z, x[nd:], r0 + A.dot(z), -x[:nd]


def inverse_dynamics(d, Q, dts, p0=None, ridge=0.0, spec=SPEC, rng=None):
    """The specification on one system: Q [B][N+1][nq], dts [N], p0 [B][nd] or None.  Returns Result with z = (dt u, lambda) [B][N][n]
    (QR), z_aug and rho_aug (the augmented system), A [B][N][nd][n] and r0 [B][N][nd]."""
    Q = np.asarray(Q, dtype=float)
    Bn, N1, nq = Q.shape
    Nn = N1 - 1
    nd, nu, nc = int(d.n_dyn), int(d.n_inputs), int(d.n_constraints)
    n = nu + nc
    o = OracleMVI(d)
    rng = rng or np.random.default_rng(7)
    out = Result(np.zeros((Bn, Nn, nu)), np.zeros((Bn, Nn, nc)), np.zeros((Bn, Nn + 1, nd)), np.zeros((Bn, Nn, nd)), np.zeros((Bn, Nn, nc)),
                 np.zeros((Bn, Nn), dtype=np.int32), np.zeros((Bn, Nn, n)), np.zeros((Bn, Nn, n)), np.zeros((Bn, Nn, nd)),
                 np.zeros((Bn, Nn, nd, n)), np.zeros((Bn, Nn, nd)))

    def p2_of(qa, qb, dt):
        o.set_times(0.0, dt)
        o.q1, o.q2 = qa, qb
        o.calc_p2()
        return o.p2

    def f_of(qa, qb, dt, p, u, lam):
        o.set_times(0.0, dt)
        o.q1, o.q2, o.p1, o.u1, o.lambda1 = qa, qb, p, u, lam
        return o.calc_f()

    for b in range(Bn):
        for k in range(Nn):
            dt = float(dts[k])
            if k == 0:
                pk = np.zeros(nd) if p0 is None else np.asarray(p0[b], dtype=float)
            elif spec["p_from_same_pair"]:
                pk = p2_of(Q[b, k], Q[b, k + 1], dt)
            else:
                pk = p2_of(Q[b, k - 1], Q[b, k], float(dts[k - 1]))
            f0 = f_of(Q[b, k], Q[b, k + 1], dt, pk, np.zeros(nu), np.zeros(nc))
            r0, h = f0[:nd].copy(), f0[nd:].copy()
            A = np.zeros((nd, n))
            for i in range(nu):
                e = np.zeros(nu)
                e[i] = (1.0 if spec["dt_twice"] else 1.0 / dt)
                A[:, i] = f_of(Q[b, k], Q[b, k + 1], dt, pk, e, np.zeros(nc))[:nd] - r0
            for c in range(nc):
                e = np.zeros(nc)
                e[c] = 1.0
                if spec["dh_at_next"]:
                    A[:, nu + c] = f_of(Q[b, k + 1], Q[b, k + 1], dt, pk, np.zeros(nu), e)[:nd] - f_of(Q[b, k + 1], Q[b, k + 1], dt, pk, np.zeros(nu), np.zeros(nc))[:nd]
                else:
                    A[:, nu + c] = f_of(Q[b, k], Q[b, k + 1], dt, pk, np.zeros(nu), e)[:nd] - r0
            if n and not any(spec.values()):
                zt = rng.standard_normal(n)
                r = f_of(Q[b, k], Q[b, k + 1], dt, pk, zt[:nu] / dt, zt[nu:])[:nd]
                lin = r0 + A.dot(zt)
                miss = np.abs(r - lin).max() / max(1.0, np.abs(lin).max())
                assert miss <= AFFINITY, ("the residual is not affine in (u, lambda)", b, k, miss)
            out.P[b, k + 1] = p2_of(Q[b, k], Q[b, k + 1], dt)
            out.h[b, k] = h
            out.A[b, k], out.r0[b, k] = A, r0
            if k == 0 and p0 is None:
                out.P[b, 0] = -r0
                continue
            if k == 0:
                out.P[b, 0] = pk
            z, z_aug, rho, rho_aug = solve_step(A, r0, ridge)
            out.z[b, k], out.z_aug[b, k], out.rho[b, k], out.rho_aug[b, k] = z, z_aug, rho, rho_aug
            out.U[b, k], out.lam[b, k] = z[:nu] / dt, z[nu:]
    return out


def case_reference(c, with_p0):
    key = ("ref", case_id(c), bool(with_p0))
    if key not in _cache:
        p = case_paths(c)
        _cache[key] = inverse_dynamics(p["d"], p["Q"], p["dts"], p["p0"] if with_p0 else None, c.ridge)
    return _cache[key]


def impulses(nu, U, lam, dts):
    """z~ = (dt u, lambda) [B][N][nu + nc] of an answer."""
    return np.concatenate([np.asarray(U) * np.asarray(dts)[None, :, None], np.asarray(lam)], axis=2) if nu else np.asarray(lam)


def floors(ref):
    """e_ref per quantity: the two fp64 solves of the reference against each other, relative to max(1, |z~|inf)."""
    scale = max(1.0, float(np.abs(ref.z).max(initial=0.0)))
    return {"z": float(np.abs(ref.z - ref.z_aug).max(initial=0.0)) / scale, "rho": float(np.abs(ref.rho - ref.rho_aug).max(initial=0.0)) / scale,
            "scale": scale}


def bound(ref):
    f = floors(ref)
    return max(TOL, MARGIN * max(f["z"], f["rho"]))


def errors(c, ref, got):
    """Worst error of an answer (anything with U, lam, P, rho, h, status) per quantity, relative to max(1, |z~|inf)."""
    p = case_paths(c)
    nu = int(p["d"].n_inputs)
    scale = floors(ref)["scale"]
    z = impulses(nu, got.U, got.lam, p["dts"])
    err = lambda a, b_: float(np.abs(np.asarray(a) - b_).max(initial=0.0)) / scale
    return {"z": err(z, ref.z), "rho": err(got.rho, ref.rho), "P": err(got.P, ref.P), "h": err(got.h, ref.h)}


def compare(c, with_p0, got, ref=None, tag=""):
    """An answer against the reference of a case: status all TG_OK, every quantity within the case's bound.  Prints the figures first."""
    ref = ref or case_reference(c, with_p0)
    e, bd = errors(c, ref, got), bound(ref)
    print("%s%s p0 %s: z %.3e rho %.3e P %.3e h %.3e  bound %.3e  floors z %.3e rho %.3e  |z|inf %.3e  |rho|inf %.3e" % (
        tag, case_id(c), "given" if with_p0 else "absent", e["z"], e["rho"], e["P"], e["h"], bd, floors(ref)["z"], floors(ref)["rho"],
        floors(ref)["scale"], float(np.abs(ref.rho).max(initial=0.0))))
    assert np.array_equal(np.asarray(got.status), ref.status), got.status
    for q in ("z", "rho", "P", "h"):
        assert e[q] <= bd, (case_id(c), q, e[q], bd)
    return e


# ---- the parameter twin: trajectory b under row b of a table of masses, inertias and gravity -------------------------------------
def parameter_rows(name, R):
    """R rows: row 0 the system's own values, row r > 0 the masses and inertias scaled body by body and gravity scaled by 1 + r / 2."""
    from trep_amd import parameters
    base = parameters.base_values(common.build(name)[0])
    nb = len(base["inertia"])
    scale = lambda r: 1.0 + 0.5 * r * np.arange(1, nb + 1)[:, None] / nb
    return {"inertia": np.array([base["inertia"] * scale(r) for r in range(R)]),
            "gravity": np.array([base["gravity"] * (1.0 + 0.5 * r) for r in range(R)])}


def parameter_table(name, rows):
    """The rows as the kernels read them: [mass, Ixx, Iyy, Izz of every body | gravity [3] | damping [nd]]."""
    from trep_amd import parameters
    system = common.build(name)[0]
    damping = parameters.base_values(system)["damping"]
    damping = np.zeros(len(system.dyn_configs)) if damping is None else damping
    return np.array([np.concatenate([rows["inertia"][r].ravel(), rows["gravity"][r], damping]) for r in range(len(rows["inertia"]))])


def parameter_reference(c, with_p0, rows):
    """Every trajectory by the specification on a descriptor rebuilt with its row's values (one trajectory per row)."""
    from test_parameters_cpu import rebuilt
    from trep_amd import descriptor
    key = ("par", case_id(c), bool(with_p0))
    if key not in _cache:
        p = case_paths(c)
        outs = [inverse_dynamics(descriptor.flatten(rebuilt(common.BUILDERS[c.name], rows, b)), p["Q"][b:b + 1], p["dts"],
                                 p["p0"][b:b + 1] if with_p0 else None, c.ridge) for b in range(c.B)]
        _cache[key] = Result(*[np.concatenate([getattr(o, f) for o in outs]) for f in Result._fields])
    return _cache[key]
