"""The forward-mode (dual-number) kernels of the continuous dynamics on the device: k_forward<MODE, SPRINGS, Real> (csrc/trepamd.hip),
run_forward (csrc/mvi_core.hpp), the scalars of csrc/dual.hpp -- BatchMidpointVI.dynamics_deriv1(..., seeds=) and lagrangian(..., seeds=),
which stand behind System.f_dqdq() ... lambda_dudu() and L_dqdqdq ... L_ddqddqdqdq.

Reference: Richardson-extrapolated central differences of the oracle's analytic arrays, in long double (common.fw_ladder); the case
table, the floors e_ref and the bounds max(tolerance, 64 e_ref) are common.FW_*, kept honest by test_forward_cpu.py without a device.
Every trajectory of a case has its own state and its own direction(s); the raw kernel output is compared (no reference conventions).
tools/forward_parity.py records the figures through the functions of this file."""
import numpy as np
import pytest

import common as C
from common import relerr

pytestmark = pytest.mark.gpu

MODE_BIT = {"dyn": 6, "lag1": 8, "lag2": 8}         # BatchMidpointVI.ALL_MODES: dynamics_deriv1, lagrangian
TILED = 300                                          # more trajectories than the 256 CUs


def launch(eng, c, kernel, rows):
    """The kernel of a case over the trajectories `rows` (as many as eng holds): ({array: [len(rows)][...]}, status or None)."""
    rows = np.asarray(rows)
    seeds = tuple(s[rows] for s in c["seeds"])
    if kernel == "dyn":
        return eng.dynamics_deriv1(c["Q"][rows], c["dQ"][rows], c["U"][rows], c["ddK"][rows], seeds=seeds)
    return eng.lagrangian(c["Q"][rows], c["dQ"][rows], seeds=seeds), None


def generic_launches(eng, kernel):
    info = eng.kernel_info()
    assert info["spec_launches"] == 0 and info["par_spec_launches"] == 0 and info["par_generic_launches"] == 0, info
    assert info["generic_launch_mask"] == 1 << MODE_BIT[kernel], info
    return info["generic_launches"]


def run_case(name, kernel):
    """One case on the device; returns {array: worst error against the reference}."""
    import trep_amd
    c = C.fw_case(name, kernel)
    system, _ = C.build(name)
    B, names = c["B"], c["names"]
    eng = trep_amd.BatchMidpointVI(system, B)
    try:
        got, status = launch(eng, c, kernel, np.arange(B))
        assert generic_launches(eng, kernel) == 1
    finally:
        eng.close()
    assert status is None or (status == 0).all(), status
    errs = C.fw_errors(name, kernel, got)
    for n in names:
        print("%s %s %s: worst %.3e, e_ref %.3e, bound %.3e" % (name, kernel, n, errs[n], C.fw_e_ref(name, kernel)[n], C.fw_bound(name, kernel, n)))
    for n in names:
        assert errs[n] <= C.fw_bound(name, kernel, n), (name, kernel, n, errs[n], C.fw_bound(name, kernel, n))
    # no direction: exact zeros
    none = [b for b in range(B) if min(int(s[b]) for s in c["seeds"]) < 0]
    assert none
    for b in none:
        assert all(np.all(got[n][b] == 0.0) for n in names), (name, kernel, b)
    # equal trajectories: equal bits
    i, j = c["duplicates"]
    assert any(np.abs(got[n][i]).max() > 0.0 for n in names if got[n][i].size)
    assert all(np.array_equal(got[n][i], got[n][j]) for n in names), (name, kernel)
    # one trajectory per launch
    eng = trepamd_batch(system, 1)
    try:
        for b in range(B):
            one, st = launch(eng, c, kernel, [b])
            assert st is None or st[0] == 0
            assert all(np.array_equal(one[n][0], got[n][b]) for n in names), (name, kernel, b)
        assert generic_launches(eng, kernel) == B
    finally:
        eng.close()
    # more trajectories than compute units: the case tiled
    rows = np.arange(TILED) % B
    eng = trepamd_batch(system, TILED)
    try:
        big, st = launch(eng, c, kernel, rows)
        assert generic_launches(eng, kernel) == 1
    finally:
        eng.close()
    assert st is None or (st == 0).all()
    assert all(np.array_equal(big[n], got[n][rows]) for n in names), (name, kernel)
    return errs


def trepamd_batch(system, B):
    import trep_amd
    return trep_amd.BatchMidpointVI(system, B)


@pytest.mark.parametrize("name", list(C.FW_SYSTEMS))
def test_dynamics_second_derivatives_match_the_ladder(name):
    """k_forward<MODE_DYN_DERIV1, ., Dual<double>>: every trajectory its own state and its own direction over q | dq | ddq_k | u."""
    run_case(name, "dyn")


@pytest.mark.parametrize("name", list(C.FW_SYSTEMS))
def test_lagrangian_third_derivatives_match_the_ladder(name):
    """k_forward<MODE_LAGRANGIAN, ., Dual<double>>: single directions in q and in dq."""
    run_case(name, "lag1")


@pytest.mark.parametrize("name", list(C.FW_SYSTEMS))
def test_lagrangian_fourth_derivatives_match_the_nested_ladder(name):
    """k_forward<MODE_LAGRANGIAN, ., Dual<Dual<double>>>: pairs (q, q) with equal and unequal indices, (q, dq), (dq, q), (dq, dq), (v, -1)."""
    run_case(name, "lag2")


KINEMATIC = [n for n in C.FW_SYSTEMS if C.build(n)[1].n_kin > 0]


@pytest.mark.parametrize("name", KINEMATIC)
def test_directions_along_ddqk_mirror_the_directions_along_q_and_dq(name):
    """Mixed partials from two different launches at one state: d(f_dq)/d(ddq_k) from directions along ddq_k (seeds 2 nq ... 2 nq + nk - 1)
    is d(f_dddk)/dq from directions along q, transposed -- the columns System.f_dddkdq() is made of -- and the same for dq and for
    lambda.  f and lambda are linear in ddq_k: along ddq_k the derivative of *_dddk is zero."""
    c = C.fw_case(name, "dyn")
    system, d = C.build(name)
    nq, nk, nu, nvar = C.fw_sizes(d)
    state = lambda M: [np.repeat(c[k][:1], M, axis=0) for k in ("Q", "dQ", "U", "ddK")]
    a = trepamd_batch(system, 2 * nq)
    b = trepamd_batch(system, nk)
    try:
        along_q, sa = a.dynamics_deriv1(*state(2 * nq), seeds=(np.arange(2 * nq, dtype=np.int32),))
        along_k, sb = b.dynamics_deriv1(*state(nk), seeds=(2 * nq + np.arange(nk, dtype=np.int32),))
    finally:
        a.close()
        b.close()
    assert (sa == 0).all() and (sb == 0).all()
    seen = 0.0
    for pre in ("f", "lambda"):
        dddk = along_q[pre + "_dddk"]                      # [v][output][k]
        for var, lo in (("dq", 0), ("ddq", nq)):
            mirror = along_k["%s_%s" % (pre, var)]         # [k][output][j]
            want = np.transpose(dddk[lo:lo + nq], (2, 1, 0))
            bound = max(C.fw_bound(name, "dyn", pre + "_dddk"), C.fw_bound(name, "dyn", "%s_%s" % (pre, var)))
            e = relerr(mirror, want)
            print("%s %s_%s along ddq_k against %s_dddk along %s: %.3e (bound %.3e)" % (name, pre, var, pre, var[1:], e, bound))
            assert e <= bound, (name, pre, var, e, bound)
            seen = max(seen, float(np.abs(want).max()) if want.size else 0.0)
        assert np.abs(along_k[pre + "_dddk"]).max(initial=0.0) <= C.fw_bound(name, "dyn", pre + "_dddk")
    assert seen > 1e-6, (name, seen)


def test_the_seeded_device_pointer_entry_is_not_public():
    """tg_batch_dynamics_deriv1_device has no seeded form in the ABI: the forward-mode launch is reached through the host entry
    tg_batch_dynamics_deriv1_forward alone (csrc/trepamd.hip: dyn_deriv1_device with a direction array is file-local), so there is no
    second route whose results could differ.  If one is added, it belongs in run_case next to the host entry."""
    from trep_amd import _lib
    assert not [n for n in _lib.exported_symbols() if "forward" in n and "device" in n]


def test_a_parameter_table_refuses_the_forward_entry_points():
    """With set_parameters active both forward entry points raise ("clear the parameter table first") and launch nothing; after
    clear_parameters() the same calls match the reference."""
    from trep_amd import _lib
    name = "pend_on_cart"
    system, _ = C.build(name)
    cases = dict((k, C.fw_case(name, k)) for k in C.FW_KERNELS)
    B = cases["dyn"]["B"]
    eng = trepamd_batch(system, B)
    try:
        eng.set_parameters(gravity=np.array([0.0, 0.0, -3.0]))
        assert eng.has_parameters
        before = eng.kernel_info()
        for k, c in cases.items():
            with pytest.raises(_lib.LibraryError, match="clear the parameter table first"):
                launch(eng, c, k, np.arange(B))
        after = eng.kernel_info()
        for key in ("generic_launches", "spec_launches", "par_generic_launches", "par_spec_launches", "generic_launch_mask"):
            assert after[key] == before[key], key
        eng.clear_parameters()
        for k, c in cases.items():
            got, status = launch(eng, c, k, np.arange(B))
            assert status is None or (status == 0).all()
            errs = C.fw_errors(name, k, got)
            for n in c["names"]:
                assert errs[n] <= C.fw_bound(name, k, n), (k, n, errs[n])
        assert eng.kernel_info()["generic_launches"] == before["generic_launches"] + 3
    finally:
        eng.close()


def run_chain(kernel):
    """The LDS limit of one kernel on n-link pendulums; returns (links refused, {array: worst error one link shorter})."""
    from trep_amd import _lib
    limit = C.fw_chain_limit(kernel)
    assert limit is not None
    assert C.fw_lds_bytes(C.fw_chain(limit)[1], kernel) > C.FW_LDS_LIMIT >= C.fw_lds_bytes(C.fw_chain(limit - 1)[1], kernel)
    B = 3
    system, d = C.fw_chain(limit)
    eng = trepamd_batch(system, B)
    try:
        z = np.zeros((B, limit))
        seeds = (np.zeros(B, dtype=np.int32),) * (2 if kernel == "lag2" else 1)
        with pytest.raises(_lib.LibraryError, match="too large"):
            if kernel == "dyn":
                eng.dynamics_deriv1(z, z, seeds=seeds)
            else:
                eng.lagrangian(z, z, seeds=seeds)
        info = eng.kernel_info()
        assert info["generic_launches"] == 0 and info["generic_launch_mask"] == 0, info
    finally:
        eng.close()
    c = C.fw_chain_case(kernel, limit - 1, B)
    system, _ = C.fw_chain(limit - 1)
    eng = trepamd_batch(system, B)
    try:
        got, status = launch(eng, c, kernel, np.arange(B))
        assert generic_launches(eng, kernel) == 1
    finally:
        eng.close()
    assert status is None or (status == 0).all()
    errs = {}
    for n in c["names"]:
        errs[n] = max(relerr(got[n][t], c["reference"][t][0][n]) for t in range(B))
        bound = max(C.FW_TOL[kernel], 64.0 * c["e_ref"][n])
        print("chain of %d links, %s %s: worst %.3e, e_ref %.3e, bound %.3e" % (limit - 1, kernel, n, errs[n], c["e_ref"][n], bound))
    for n in c["names"]:
        assert errs[n] <= max(C.FW_TOL[kernel], 64.0 * c["e_ref"][n]), (kernel, n, errs[n])
    return limit, errs


@pytest.mark.parametrize("kernel", C.FW_KERNELS)
def test_the_lds_limit_refuses_one_link_more_than_runs(kernel):
    """The block of a forward-mode launch is sizeof(Real) / 8 times the double kernel's slice.  On the n-link pendulum of
    test_long_chain_matches_oracle the shortest chain over 160 KiB (found on the host: 26 links for the dynamics kernel, 35 and 24 for
    the Lagrangian kernels on Dual<double> and Dual<Dual<double>>) is refused with "too large" and nothing is launched; one link shorter
    the launch runs, and three trajectories match the reference."""
    limit, _ = run_chain(kernel)
    assert limit == {"dyn": 26, "lag1": 35, "lag2": 24}[kernel]
