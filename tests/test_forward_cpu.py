"""The case table of the forward-mode (dual-number) kernels (common.FW_*), kept honest with the oracle alone, and the emulated kernels
over it.  No device.  test_gpu_forward.py runs the same table on the device against the same reference and the same bounds.

The reference of a forward-mode output along variable v is the directional derivative of arrays the oracle has in analytic form
(OracleMVI.dynamics_deriv1 / lagrangian): Richardson-extrapolated central differences in long double, common.fw_ladder, nested for two
directions.  Errors are common.relerr: relative to the array's largest entry, or to 1."""
import os

import numpy as np
import pytest

import common as C
from common import GOLDEN, relerr

# ---- the ladder is the right operation -------------------------------------------------------------------------------------------------
D2_NAMES = ["pendulum5", "pend_on_cart", "scissor4", "spring_arm", "plane_link", "wrench_arm", "wrench_torque", "wrench_body", "puppet40"]
CONVENTION_NAMES = ["damper_link", "nonlinear_spring_arm"]
# golden array <- (first-derivative array, block of the direction variable)
D2_PARTS = {"dqdq": ("dq", 0), "ddqdq": ("ddq", 0), "dddkdq": ("dddk", 0), "dudq": ("du", 0), "ddqddq": ("ddq", 1), "duddq": ("du", 1),
            "dudu": ("du", 3)}
# worst relerr of the ladder against dynamics2.npz at the first golden state (every variable of q | dq | u; puppet40: the first and last
# of q and of dq and two drawn ones), measured; the test asserts one decade above
D2_MEASURED = {
    "pendulum5": 1.4e-10, "pend_on_cart": 9.4e-15, "scissor4": 2.5e-12, "spring_arm": 7.4e-14, "plane_link": 2.4e-12,
    "wrench_arm": 4.2e-14, "wrench_torque": 3.2e-14, "wrench_body": 1.7e-13, "puppet40": 2.6e-13, "damper_link": 1.0e-13,
    "nonlinear_spring_arm": 5.7e-13
}
HIGHER_NAMES = ["pendulum5", "scissor4", "plane_link", "puppet40"]
HIGHER_MEASURED = {
    "pendulum5": (2.3e-13, 1.8e-12), "scissor4": (2.1e-15, 7.4e-14), "plane_link": (4.5e-15, 2.7e-15), "puppet40": (8.7e-15, 1.4e-13)
}


def golden_state(name):
    g, g2 = np.load(os.path.join(GOLDEN, "dynamics.npz")), np.load(os.path.join(GOLDEN, "dynamics2.npz"))
    s = int(g2[name + "_states"][0])
    return s, np.concatenate([g[name + "_q"][s], g[name + "_dq"][s], g[name + "_ddqk"][s], g[name + "_u"][s]]), g2


def ladder_second_derivatives(name, x, variables):
    """{golden key: (ladder's [var1][len(variables in the block)][output], the positions of those variables in the block)}"""
    from oracle.oracle import OracleMVI
    _, d = C.build(name)
    nq, nk, nu, nvar = C.fw_sizes(d)
    o = OracleMVI(d)
    ref = dict((v, C.fw_derivative(name, "dyn", x, (v,), o)[0]) for v in variables)
    starts = (0, nq, 2 * nq, 2 * nq + nk)
    out = {}
    for key, (arr, block) in D2_PARTS.items():
        vs = [v for v in variables if C.fw_block(d, v) == block]
        for pre in ("f", "lambda"):
            cols = [ref[v]["%s_%s" % (pre, arr)].T for v in vs]               # [var1][output] each
            out["%s_%s" % (pre, key)] = (np.stack(cols, axis=1) if cols else None, [v - starts[block] for v in vs])
    return out


def d2_variables(name, d):
    nq, nk, nu, nvar = C.fw_sizes(d)
    if name != "puppet40":
        return list(range(2 * nq)) + list(range(2 * nq + nk, nvar))
    rng = np.random.default_rng(C.tb_seed("fw d2 variables"))
    return [0, nq - 1, nq, 2 * nq - 1] + [int(v) for v in rng.choice(d.n_dyn, size=2, replace=False)]


@pytest.mark.parametrize("name", D2_NAMES)
def test_the_ladder_reproduces_the_second_derivatives_of_the_reference(name):
    """dynamics2.npz (System.f_dqdq() ... lambda_dudu() of the real reference) at a golden state.  Measured (worst array): pendulum5
    1.4e-10, pend_on_cart 9.4e-15, scissor4 2.5e-12, spring_arm 7.4e-14, plane_link 2.4e-12, wrench_arm 4.2e-14, wrench_torque
    3.2e-14, wrench_body 1.7e-13, puppet40 2.6e-13 (first and last variable of q and of dq and two drawn ones; the others every
    variable of q | dq | u); asserted one decade above (D2_MEASURED)."""
    _, d = C.build(name)
    s, x, g2 = golden_state(name)
    got = ladder_second_derivatives(name, x, d2_variables(name, d))
    worst = 0.0
    for key, (a, cols) in got.items():
        if a is None or a.size == 0:
            continue
        want = g2["%s_%s" % (name, key.replace("lambda_", "lam_"))][s][:, cols, :]
        assert a.shape == want.shape, (name, key, a.shape, want.shape)
        worst = max(worst, relerr(a, want))
    print("%s: ladder against dynamics2.npz %.3e" % (name, worst))
    assert worst <= 10.0 * D2_MEASURED[name], (name, worst)


@pytest.mark.parametrize("name", CONVENTION_NAMES)
def test_the_ladder_reproduces_the_reference_after_its_element_conventions(name):
    """The two systems where the reference's own second derivatives are not the derivatives of its first ones (LinearDamper,
    NonlinearConfigSpring): the ladder's arrays differ from dynamics2.npz by O(1) in f_ddqdq / f_dqdq, and match after
    System._apply_reference_conventions with the oracle's mass matrix.  Measured: 0.85 / 0.96 before, damper_link 1.0e-13, nonlinear_spring_arm 5.7e-13 after; asserted one decade above."""
    from oracle.oracle import OracleMVI
    system, d = C.build(name)
    nq, nk, nu, nvar = C.fw_sizes(d)
    s, x, g2 = golden_state(name)
    parts = ladder_second_derivatives(name, x, list(range(2 * nq)) + list(range(2 * nq + nk, nvar)))
    nd, nc = d.n_dyn, d.n_constraints
    empty = {"dqdq": (nq, nq), "ddqdq": (nq, nq), "ddqddq": (nq, nq), "dddkdq": (nk, nq), "dudq": (nu, nq), "duddq": (nu, nq), "dudu": (nu, nu)}
    out = {}
    for key, (a, _) in parts.items():
        pre, k = key.split("_")
        out[key] = np.array(a) if a is not None else np.zeros(empty[k] + (nd if pre == "f" else nc,))
    raw = max(relerr(out[k], g2["%s_%s" % (name, k.replace("lambda_", "lam_"))][s]) for k in out if out[k].size)
    assert raw > 1e-3, (name, raw)
    system.q, system.dq, system.ddqk, system.u = x[:nq], x[nq:2 * nq], x[2 * nq:2 * nq + nk], x[2 * nq + nk:]
    system._apply_reference_conventions(out, mass_matrix=OracleMVI(d).lagrangian(x[:nq], x[nq:2 * nq])[4])
    worst = max(relerr(out[k], g2["%s_%s" % (name, k.replace("lambda_", "lam_"))][s]) for k in out if out[k].size)
    print("%s: ladder against dynamics2.npz %.3e raw, %.3e with the reference's conventions" % (name, raw, worst))
    assert worst <= 10.0 * D2_MEASURED[name], (name, worst)


@pytest.mark.parametrize("name", HIGHER_NAMES)
def test_the_nested_ladder_reproduces_the_higher_lagrangian_derivatives_of_the_reference(name):
    """lagrangian_higher.npz (System.L_dqdqdq ... L_ddqddqdqdq of the real reference), twelve index tuples, relative to the accessor's
    largest value over the tuples (or 1).  Measured, third / fourth order: pendulum5 2.3e-13 / 1.8e-12, scissor4 2.1e-15 / 7.4e-14,
    plane_link 4.5e-15 / 2.7e-15, puppet40 8.7e-15 / 1.4e-13; asserted one decade above (HIGHER_MEASURED)."""
    from oracle.oracle import OracleMVI
    g = np.load(os.path.join(GOLDEN, "dynamics.npz"))
    gh = np.load(os.path.join(GOLDEN, "lagrangian_higher.npz"))
    _, d = C.build(name)
    o = OracleMVI(d)
    x = np.concatenate([g[name + "_q"][0], g[name + "_dq"][0]])
    idx, ref = gh[name + "_idx"][:12], gh[name + "_vals"][:12]
    scale = np.maximum(1.0, np.abs(gh[name + "_vals"]).max(axis=0))
    worst = np.zeros(5)
    for (a, b, c, e), r in zip(idx, ref):
        t3 = C.fw_derivative(name, "lag1", x, (int(c),), o)[0]
        t4 = C.fw_derivative(name, "lag2", x, (int(c), int(e)), o)[0]
        got = np.array([t3["L_dqdq"][a, b], t3["L_ddqdq"][a, b], t4["L_ddqdq"][a, b], t3["L_ddqddq"][a, b], t4["L_ddqddq"][a, b]])
        worst = np.maximum(worst, np.abs(got - r) / scale)
    third, fourth = worst[[0, 1, 3]].max(), worst[[2, 4]].max()
    print("%s: nested ladder against lagrangian_higher.npz, third order %.3e, fourth order %.3e" % (name, third, fourth))
    assert third <= 10.0 * HIGHER_MEASURED[name][0] and fourth <= 10.0 * HIGHER_MEASURED[name][1], (name, third, fourth)


# ---- the floor ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.FW_SYSTEMS))
def test_the_floor_of_the_reference_is_under_the_rule_or_named(name):
    """e_ref -- the ladder of half the base step against the ladder -- is at most 1e-10 / 64 (dynamics) and 1e-12 / 64 (Lagrangian), so
    that the bound max(tolerance, 64 e_ref) is the project's tolerance; every (system, kernel, array) over that is named in
    common.FW_SECOND_TERM with its measured floor, is really over it, and stays within twice the figure."""
    for kernel in C.FW_KERNELS:
        named = C.FW_SECOND_TERM.get((name, kernel), {})
        for n, e in C.fw_e_ref(name, kernel).items():
            print("%s %s %s: e_ref %.3e%s" % (name, kernel, n, e, " (named: %.1e)" % named[n] if n in named else ""))
            if n in named:
                assert C.FW_FLOOR[kernel] < e <= 2.0 * named[n], (name, kernel, n, e, named[n])
            else:
                assert e <= C.FW_FLOOR[kernel], (name, kernel, n, e)
        assert set(named) <= set(C.fw_case(name, kernel)["names"])


# ---- sensitivity -------------------------------------------------------------------------------------------------------------------------
# trajectories whose reference is zero although they have a direction -- no entry above the array's bound; the ladder leaves rounding
# where the derivative is identically zero: the derivative does not exist in the system (a translation the dynamics do not depend on, an
# input the arrays are linear in, a string length the Lagrangian does not see, two velocities in the mass matrix, ...).  They cannot tell a
# direction from its neighbour; every other trajectory must.  A derivative that is a constant of the system (a
# translational velocity through the mass matrix) is the same at every state: such a trajectory tells the variable, not the state.
# (case -> (zero references, state-blind trajectories), held so that a new draw cannot quietly turn a case into zeros.)
INSENSITIVE = {
    ("pend_on_cart", "dyn"): (4, 0), ("pend_on_cart", "lag1"): (4, 0), ("pend_on_cart", "lag2"): (10, 0), ("scissor4", "dyn"): (4, 0),
    ("scissor4", "lag1"): (2, 0), ("scissor4", "lag2"): (11, 0), ("puppet40", "lag1"): (3, 0), ("puppet40", "lag2"): (5, 0),
    ("puppet_basic", "lag1"): (2, 0), ("plane_link", "lag1"): (0, 5), ("plane_link", "lag2"): (7, 0), ("spring_arm", "dyn"): (7, 0),
    ("spring_arm", "lag1"): (0, 1), ("spring_arm", "lag2"): (2, 0), ("spring_link", "dyn"): (1, 0), ("spring_link", "lag2"): (9, 0),
    ("dual_pendulums", "lag1"): (0, 16), ("dual_pendulums", "lag2"): (11, 0), ("damper_link", "lag1"): (0, 6), ("damper_link",
    "lag2"): (11, 0), ("nonlinear_spring_arm", "dyn"): (6, 0), ("nonlinear_spring_arm", "lag2"): (4, 0), ("wrench_arm", "dyn"): (4, 0),
    ("wrench_arm", "lag1"): (1, 0), ("wrench_arm", "lag2"): (4, 0), ("wrench_spatial", "dyn"): (2, 0), ("wrench_spatial", "lag1"): (1, 0),
    ("wrench_spatial", "lag2"): (3, 0), ("wrench_body", "dyn"): (4, 0), ("wrench_body", "lag1"): (1, 0), ("wrench_body", "lag2"): (3, 0),
    ("puppet_forces", "dyn"): (1, 0), ("puppet_forces", "lag1"): (1, 0), ("puppet_forces", "lag2"): (2, 0), ("extensor_tendon",
    "lag2"): (4, 0), ("spatial_loop", "lag1"): (0, 2), ("spatial_loop", "lag2"): (11, 0), ("mixed_loop", "dyn"): (4, 0),
    ("mixed_loop", "lag1"): (1, 2), ("mixed_loop", "lag2"): (10, 0)
}
MARGIN = 1000.0


def zero_reference(ref, bound):
    return all(np.abs(ref[n]).max(initial=0.0) <= bound[n] for n in bound)


def sensitivity(name, kernel, o):
    """(smallest margin, zero references, state-blind trajectories, [trajectories under the margin]) of a case"""
    c, refs = C.fw_case(name, kernel), C.fw_reference(name, kernel)
    d, B, names = c["d"], c["B"], c["names"]
    bound = dict((n, C.fw_bound(name, kernel, n)) for n in names)
    zeros, blind, smallest, failed = 0, 0, np.inf, []
    for b in range(B):
        seeds = tuple(int(s[b]) for s in c["seeds"])
        if min(seeds) < 0:
            assert all(not np.any(refs[b][0][n]) for n in names)
            continue
        if zero_reference(refs[b][0], bound):
            zeros += 1
            continue
        other = (C.fw_neighbour(d, kernel, seeds[0]),) + seeds[1:]
        margin = lambda alt: max(relerr(alt[n], refs[b][0][n]) / bound[n] for n in names if alt[n].size)
        by_variable = margin(C.fw_derivative(name, kernel, C.fw_x(c, b), other, o)[0])
        by_state = margin(C.fw_derivative(name, kernel, C.fw_x(c, (b + 1) % B), seeds, o)[0])
        if by_state < 1.0:
            blind += 1
        for what, m in (("variable", by_variable),) + ((("state", by_state),) if by_state >= 1.0 else ()):
            smallest = min(smallest, m)
            if m < MARGIN:
                failed.append((b, seeds, what, m))
    return smallest, zeros, blind, failed


@pytest.mark.parametrize("name", list(C.FW_SYSTEMS))
def test_every_direction_is_told_from_its_neighbours(name):
    """The reference along v differs from the reference along the variable next to v, and from the reference along v at the state of
    the next trajectory, by at least 1000 times the bound of the device test (largest ratio over the arrays): a seed offset that is
    off by one, or a trajectory index that is, cannot pass.  Held on every trajectory with a direction, except those INSENSITIVE
    counts: a reference that is zero tells nothing, and one that does not depend on the state (under the bound at the next
    trajectory's state as well) still tells the variable."""
    from oracle.oracle import OracleMVI
    _, d = C.build(name)
    o = OracleMVI(d)
    for kernel in C.FW_KERNELS:
        smallest, zeros, blind, failed = sensitivity(name, kernel, o)
        print("%s %s: smallest margin %.3e, %d zero references, %d state-blind" % (name, kernel, smallest, zeros, blind))
        assert not failed, (name, kernel, failed)
        assert (zeros, blind) == INSENSITIVE.get((name, kernel), (0, 0)), (name, kernel, zeros, blind)
        assert zeros <= C.fw_case(name, kernel)["B"] // 2, (name, kernel, zeros)


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------
# (system, kernel) -> the "array/block" combinations whose reference is zero over the case: no entry above the array's bound (block:
# where the direction variable lies; two blocks for the nested directions).  Empty arrays are not listed.
ALL_ZERO = {
    ("pend_on_cart", "dyn"): ['f_ddq/u', 'f_du/dq', 'f_du/u'],
    ("pend_on_cart", "lag1"): ['L_ddqddq/dq'],
    ("pend_on_cart", "lag2"): ['L_ddq/dq,dq', 'L_ddqddq/dq,dq', 'L_ddqddq/dq,q', 'L_ddqddq/q,dq', 'L_ddqdq/dq,dq'],
    ("scissor4", "lag1"): ['L_ddqddq/dq'],
    ("scissor4", "lag2"): ['L_ddq/dq,dq', 'L_ddq/q,dq', 'L_ddqddq/dq,dq', 'L_ddqddq/dq,q', 'L_ddqddq/q,dq', 'L_ddqdq/dq,dq', 'L_ddqdq/q,dq', 'L_dq/dq,dq', 'L_dq/q,dq', 'L_dqdq/dq,dq', 'L_dqdq/q,dq'],
    ("puppet40", "dyn"): ['f_dddk/ddq_k', 'f_dddk/dq', 'f_ddq/ddq_k', 'lambda_dddk/ddq_k', 'lambda_dddk/dq', 'lambda_ddq/ddq_k'],
    ("puppet40", "lag1"): ['L_ddqddq/dq'],
    ("puppet40", "lag2"): ['L_ddq/dq,dq', 'L_ddqddq/dq,dq', 'L_ddqddq/dq,q', 'L_ddqddq/q,dq', 'L_ddqdq/dq,dq'],
    ("puppet_basic", "lag1"): ['L_ddqddq/dq'],
    ("puppet_basic", "lag2"): ['L_ddq/dq,dq', 'L_ddqddq/dq,dq', 'L_ddqddq/dq,q', 'L_ddqddq/q,dq', 'L_ddqdq/dq,dq'],
    ("plane_link", "lag1"): ['L_ddqddq/dq'],
    ("plane_link", "lag2"): ['L_ddq/dq,dq', 'L_ddq/q,dq', 'L_ddqddq/dq,dq', 'L_ddqddq/dq,q', 'L_ddqddq/q,dq', 'L_ddqdq/dq,dq', 'L_ddqdq/q,dq', 'L_dq/dq,dq', 'L_dq/q,dq', 'L_dqdq/dq,dq', 'L_dqdq/q,dq'],
    ("spring_arm", "dyn"): ['f_dddk/ddq_k', 'f_dddk/dq', 'f_dddk/u', 'f_ddq/ddq_k', 'f_ddq/u', 'f_du/ddq_k', 'f_du/dq', 'f_du/u'],
    ("spring_arm", "lag1"): ['L_ddqddq/dq'],
    ("spring_arm", "lag2"): ['L_ddq/dq,dq', 'L_ddqddq/dq,dq', 'L_ddqddq/dq,q', 'L_ddqddq/q,dq', 'L_ddqdq/dq,dq'],
    ("spring_link", "dyn"): ['f_dddk/ddq_k', 'f_dddk/dq', 'f_ddq/ddq_k', 'lambda_dddk/ddq_k', 'lambda_dddk/dq', 'lambda_dddk/q', 'lambda_ddq/ddq_k', 'lambda_ddq/q', 'lambda_dq/ddq_k'],
    ("spring_link", "lag1"): ['L_ddqddq/dq'],
    ("spring_link", "lag2"): ['L_ddq/dq,dq', 'L_ddqddq/dq,dq', 'L_ddqddq/dq,q', 'L_ddqddq/q,dq', 'L_ddqdq/dq,dq', 'L_dq/dq,dq', 'L_dqdq/dq,dq', 'L_dqdq/q,dq'],
    ("dual_pendulums", "dyn"): ['f_ddq/dq'],
    ("dual_pendulums", "lag1"): ['L_ddq/q', 'L_ddqddq/dq', 'L_ddqddq/q', 'L_ddqdq/dq', 'L_ddqdq/q', 'L_dq/dq', 'L_dqdq/dq'],
    ("dual_pendulums", "lag2"): ['L_ddq/dq,dq', 'L_ddq/dq,q', 'L_ddq/q,dq', 'L_ddq/q,q', 'L_ddqddq/dq,dq', 'L_ddqddq/dq,q', 'L_ddqddq/q,dq', 'L_ddqddq/q,q', 'L_ddqdq/dq,dq', 'L_ddqdq/dq,q', 'L_ddqdq/q,dq', 'L_ddqdq/q,q', 'L_dq/dq,dq', 'L_dq/dq,q', 'L_dq/q,dq', 'L_dqdq/dq,dq', 'L_dqdq/dq,q', 'L_dqdq/q,dq'],
    ("damper_link", "lag1"): ['L_ddqddq/dq'],
    ("damper_link", "lag2"): ['L_ddq/dq,dq', 'L_ddq/q,dq', 'L_ddqddq/dq,dq', 'L_ddqddq/dq,q', 'L_ddqddq/q,dq', 'L_ddqdq/dq,dq', 'L_ddqdq/q,dq', 'L_dq/dq,dq', 'L_dq/q,dq', 'L_dqdq/dq,dq', 'L_dqdq/q,dq'],
    ("nonlinear_spring_arm", "dyn"): ['f_dddk/ddq_k', 'f_dddk/dq', 'f_dddk/u', 'f_ddq/ddq_k', 'f_ddq/u', 'f_du/ddq_k', 'f_du/dq', 'f_du/u'],
    ("nonlinear_spring_arm", "lag1"): ['L_ddqddq/dq'],
    ("nonlinear_spring_arm", "lag2"): ['L_ddq/dq,dq', 'L_ddqddq/dq,dq', 'L_ddqddq/dq,q', 'L_ddqddq/q,dq', 'L_ddqdq/dq,dq'],
    ("wrench_arm", "dyn"): ['f_dddk/ddq_k', 'f_dddk/dq', 'f_dddk/u', 'f_ddq/ddq_k', 'f_ddq/u', 'f_du/ddq_k', 'f_du/dq', 'f_du/u'],
    ("wrench_arm", "lag1"): ['L_ddqddq/dq'],
    ("wrench_arm", "lag2"): ['L_ddq/dq,dq', 'L_ddqddq/dq,dq', 'L_ddqddq/dq,q', 'L_ddqddq/q,dq', 'L_ddqdq/dq,dq'],
    ("wrench_spatial", "dyn"): ['f_dddk/ddq_k', 'f_dddk/dq', 'f_dddk/u', 'f_ddq/ddq_k', 'f_ddq/u', 'f_du/ddq_k', 'f_du/dq', 'f_du/u'],
    ("wrench_spatial", "lag1"): ['L_ddqddq/dq'],
    ("wrench_spatial", "lag2"): ['L_ddq/dq,dq', 'L_ddqddq/dq,dq', 'L_ddqddq/dq,q', 'L_ddqddq/q,dq', 'L_ddqdq/dq,dq'],
    ("wrench_body", "dyn"): ['f_dddk/ddq_k', 'f_dddk/dq', 'f_dddk/u', 'f_ddq/ddq_k', 'f_ddq/u', 'f_du/ddq_k', 'f_du/dq', 'f_du/u'],
    ("wrench_body", "lag1"): ['L_ddqddq/dq'],
    ("wrench_body", "lag2"): ['L_ddq/dq,dq', 'L_ddqddq/dq,dq', 'L_ddqddq/dq,q', 'L_ddqddq/q,dq', 'L_ddqdq/dq,dq'],
    ("puppet_forces", "dyn"): ['f_ddq/u', 'f_du/dq', 'f_du/u'],
    ("puppet_forces", "lag1"): ['L_ddqddq/dq'],
    ("puppet_forces", "lag2"): ['L_ddq/dq,dq', 'L_ddqddq/dq,dq', 'L_ddqddq/dq,q', 'L_ddqddq/q,dq', 'L_ddqdq/dq,dq'],
    ("extensor_tendon", "lag1"): ['L_ddqddq/dq'],
    ("extensor_tendon", "lag2"): ['L_ddq/dq,dq', 'L_ddqddq/dq,dq', 'L_ddqddq/dq,q', 'L_ddqddq/q,dq', 'L_ddqdq/dq,dq', 'L_dq/dq,dq', 'L_dqdq/dq,dq'],
    ("spatial_loop", "dyn"): ['f_dddk/ddq_k', 'f_dddk/dq', 'f_ddq/ddq_k', 'lambda_dddk/ddq_k', 'lambda_dddk/dq', 'lambda_ddq/ddq_k'],
    ("spatial_loop", "lag1"): ['L_ddqddq/dq'],
    ("spatial_loop", "lag2"): ['L_ddq/dq,dq', 'L_ddq/q,dq', 'L_ddqddq/dq,dq', 'L_ddqddq/dq,q', 'L_ddqddq/q,dq', 'L_ddqdq/dq,dq', 'L_ddqdq/q,dq', 'L_dq/dq,dq', 'L_dq/q,dq', 'L_dqdq/dq,dq', 'L_dqdq/q,dq'],
    ("mixed_loop", "dyn"): ['f_dddk/ddq_k', 'f_dddk/dq', 'f_dddk/u', 'f_ddq/ddq_k', 'f_ddq/u', 'f_du/ddq_k', 'f_du/dq', 'f_du/u', 'lambda_dddk/ddq_k', 'lambda_dddk/dq',
                            'lambda_dddk/u', 'lambda_ddq/ddq_k', 'lambda_ddq/u', 'lambda_du/ddq_k', 'lambda_du/dq', 'lambda_du/u'],
    ("mixed_loop", "lag1"): ['L_ddqddq/dq'],
    ("mixed_loop", "lag2"): ['L_ddq/dq,dq', 'L_ddqddq/dq,dq', 'L_ddqddq/dq,q', 'L_ddqddq/q,dq', 'L_ddqdq/dq,dq', 'L_dq/dq,dq', 'L_dqdq/dq,dq'],
}


def block_label(d, seeds):
    return ",".join(C.FW_BLOCKS[C.fw_block(d, v)] for v in seeds)


@pytest.mark.parametrize("name", list(C.FW_SYSTEMS))
def test_every_output_is_reached_from_every_block_it_depends_on(name):
    """Every (output array, block of the direction) of a case either has a reference entry above 1e-6 on some trajectory, or is
    zero on all of them (nothing above the bound) and listed in ALL_ZERO."""
    _, d = C.build(name)
    for kernel in C.FW_KERNELS:
        c, refs = C.fw_case(name, kernel), C.fw_reference(name, kernel)
        largest = {}
        for b in range(c["B"]):
            seeds = tuple(int(s[b]) for s in c["seeds"])
            if min(seeds) < 0:
                continue
            for n in c["names"]:
                if refs[b][0][n].size:
                    key = "%s/%s" % (n, block_label(d, seeds))
                    largest[key] = max(largest.get(key, 0.0), float(np.abs(refs[b][0][n]).max()))
        zero = sorted(k for k, v in largest.items() if v <= C.fw_bound(name, kernel, k.split("/")[0]))
        print("%s %s: identically zero %r" % (name, kernel, zero))
        assert zero == sorted(ALL_ZERO.get((name, kernel), [])), (name, kernel, zero)
        small = dict((k, v) for k, v in largest.items() if k not in zero and v <= 1e-6)
        assert not small, (name, kernel, small)
        if kernel == "dyn":
            blocks = set(k.split("/")[1] for k in largest)
            nq, nk, nu, nvar = C.fw_sizes(d)
            assert blocks == set(bl for bl, size in zip(C.FW_BLOCKS, (nq, nq, nk, nu)) if size), (name, blocks)


# ---- the emulated kernels ----------------------------------------------------------------------------------------------------------------
def emulated(c, kernel):
    from emu_harness import EmuBatch
    e = EmuBatch(c["d"], c["B"])
    if kernel == "dyn":
        out, status = e.dynamics_deriv1(c["Q"], c["dQ"], c["U"], c["ddK"], seeds=c["seeds"])
        assert (status == 0).all(), status
        return dict((k.replace("lam_", "lambda_"), v) for k, v in out.items())
    o1, o2 = e.lagrangian(c["Q"], c["dQ"], seeds=c["seeds"])
    return {"L_dq": o1[:, 0], "L_ddq": o1[:, 1], "L_dqdq": o2[:, 0], "L_ddqdq": o2[:, 1], "L_ddqddq": o2[:, 2]}


@pytest.mark.parametrize("name,kernel", C.FW_CASES)
def test_emulated_forward_kernels_match_the_ladder(name, kernel):
    """run_forward compiled for the host (one lane) over the table, within the bounds of the device test; exact zeros without a
    direction, equal bits for equal trajectories."""
    c = C.fw_case(name, kernel)
    got = emulated(c, kernel)
    errs = C.fw_errors(name, kernel, got)
    for n in c["names"]:
        print("%s %s %s: emulated %.3e, bound %.3e" % (name, kernel, n, errs[n], C.fw_bound(name, kernel, n)))
    for n in c["names"]:
        assert errs[n] <= C.fw_bound(name, kernel, n), (name, kernel, n, errs[n], C.fw_bound(name, kernel, n))
    for b in range(c["B"]):
        if min(int(s[b]) for s in c["seeds"]) < 0:
            assert all(np.all(got[n][b] == 0.0) for n in c["names"]), (name, kernel, b)
    i, j = c["duplicates"]
    ref = C.fw_reference(name, kernel)[i][0]
    assert max(np.abs(ref[n]).max(initial=0.0) for n in c["names"]) > 1e-6, (name, kernel, i)     # equal bits, not equal zeros
    assert all(np.array_equal(got[n][i], got[n][j]) for n in c["names"])


@pytest.mark.parametrize("kernel", C.FW_KERNELS)
def test_emulated_forward_kernels_match_the_ladder_on_the_longest_chain(kernel):
    """The chain one link under the LDS limit of each kernel (the device test's launch), through the emulation."""
    limit = C.fw_chain_limit(kernel)
    c = C.fw_chain_case(kernel, limit - 1)
    got = emulated(c, kernel)
    for n in c["names"]:
        e = max(relerr(got[n][t], c["reference"][t][0][n]) for t in range(c["B"]))
        assert e <= max(C.FW_TOL[kernel], 64.0 * c["e_ref"][n]), (kernel, n, e)


def test_the_table_has_the_seeds_it_promises():
    for name, kernel in C.FW_CASES:
        c = C.fw_case(name, kernel)
        d, B = c["d"], c["B"]
        nq, nk, nu, nvar = C.fw_sizes(d)
        assert B == (12 if name in ("puppet40", "puppet_basic", "puppet_forces") else 24)
        S = np.stack(c["seeds"], axis=1)
        assert S.shape == (B, 2 if kernel == "lag2" else 1) and S.min() == -1 and S.max() < (nvar if kernel == "dyn" else 2 * nq)
        i, j = c["duplicates"]
        assert all(np.array_equal(c[k][i], c[k][j]) for k in ("Q", "dQ", "U", "ddK")) and np.array_equal(S[i], S[j]) and S[i].min() >= 0
        others = [b for b in range(B) if b != j]
        assert len(set(c["Q"][others].tobytes()[k * 8 * nq:(k + 1) * 8 * nq] for k in range(len(others)))) == len(others)
        have = set(int(v) for v in S[:, 0])
        if kernel == "dyn":
            edges = [v for lo, hi in ((0, nq), (nq, 2 * nq), (2 * nq, 2 * nq + nk), (2 * nq + nk, nvar)) if hi > lo for v in (lo, hi - 1)]
            assert set(edges) <= have, (name, edges, have)
        elif kernel == "lag1":
            assert {0, nq - 1, nq, 2 * nq - 1} <= have
        else:
            kinds = set()
            for a, b in S:
                if a < 0 or b < 0:
                    kinds.add("none")
                else:
                    kinds.add(("q" if a < nq else "dq") + ("q" if b < nq else "dq") + ("=" if a == b else ""))
            assert {"qq=", "qq", "qdq", "dqq", "dqdq", "none"} <= kinds, (name, kinds)
