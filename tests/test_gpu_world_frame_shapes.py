"""The world-frame path of the specialised kernels (eval_world, newton_matrix_world / _composite in mvi_core.hpp) on shapes of model the
puppets do not have, against the oracle: ladder_point (PointToPoint3D: two-sided point constraints, no length config, an odd Newton
system nf = 19) and ladder_mixed (point, plane and distance constraints at once, bodies behind a constant rotation); neither has a
floating base, translation runs or the packed image of the structured solve (test_model_branches_cpu.py pins those plan cells).

B = 5 (one partly filled block), MB_N = 12 steps from starts on the recorded trajectories.  Bounds: common.TB_TOL under the rule of
common.mb_bound; Newton iterations equal to the oracle's.  Nothing is compiled here: the libraries are the ones build() made."""
import numpy as np
import pytest

from common import (D1, MB_LADDERS, MB_N, TB_DT, build, mb_batch, mb_bound, mb_case, mb_contraction, mb_e_ref, mb_reference, relerr)
from test_gpu_time_base import _force, _in
from test_parameters_cpu import random_rows, rebuilt
from trep_amd import BatchMidpointVI, descriptor, specialize

pytestmark = pytest.mark.gpu

DT = TB_DT
N = MB_N
SPEC_VS_GENERIC = 1e-12          # the claim of csrc/spec_kernel.hip's header: same arithmetic up to the compiler's FMA contraction


def _batch(monkeypatch, name, spec):
    for k in ("TREPAMD_TEAM", "TREPAMD_NO_SPECIALIZE", "TREPAMD_SPEC_OVERRIDE"):
        monkeypatch.delenv(k, raising=False)
    system, _ = build(name)
    assert specialize.is_built(system), "build() prebuilds the ladders' specialisations"
    mvi = BatchMidpointVI(system, mb_batch(name), specialize="auto" if spec else False)
    info = mvi.kernel_info()
    assert info["team"] == 64 and (info["spec_library"] is not None) == spec, info
    return mvi


def _rollout(mvi, c):
    mvi.initialize_from_configs(0.0, c["Q0"], DT, c["Q1"])
    X = mvi.rollout(N, DT, _in(c, "U", 0, N), _in(c, "K", 0, N))
    iters, status = mvi.status()
    assert (status == 0).all(), status
    return X, iters


def run_specialised(monkeypatch, name, exact):
    """The checks of test_specialised_rollout_matches_oracle; returns the worst error per quantity (tools/model_branches_parity.py)."""
    c, ref, e_ref = mb_case(name), mb_reference(name), mb_e_ref(name)
    mvi = _batch(monkeypatch, name, True)
    mvi.exact_pivot = exact
    X, iters = _rollout(mvi, c)
    p1, p2, lam = mvi.p1, mvi.p2, mvi.lambda1
    info = mvi.kernel_info()
    mvi.close()
    assert "rollout" in info["spec_launched"] and "rollout" not in info["generic_launched"], info
    assert info["exact_pivot"] == exact
    worst = {}
    for b, r in enumerate(ref):
        for q, got in (("X", X[b]), ("p1", p1[b]), ("p2", p2[b]), ("lambda1", lam[b])):
            e = relerr(got, r[q])
            worst[q] = max(worst.get(q, 0.0), e)
            print("%s exact=%d %s[%d] %.2e (bound %.2e)" % (name, exact, q, b, e, mb_bound(name, q, e_ref)))
            assert e < mb_bound(name, q, e_ref), (name, exact, q, b, e)
    assert np.array_equal(iters, [r["iterations"] for r in ref]), (name, exact, iters)
    return worst


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", MB_LADDERS)
def test_specialised_rollout_matches_oracle(monkeypatch, name, exact):
    """Both pivot rules (the structured solve and the dense exact-pivot one): states, p1, p2, lambda1, iteration counts."""
    run_specialised(monkeypatch, name, exact)


@pytest.mark.parametrize("name", MB_LADDERS)
def test_specialised_derivatives_match_oracle(monkeypatch, name):
    """deriv1 and deriv2z (with the lambda contraction) of the specialised library at the oracles' last step."""
    c, ref, e_ref = mb_case(name), mb_reference(name), mb_e_ref(name)
    Z, ZL = mb_contraction(name)
    mvi = _batch(monkeypatch, name, True)
    _rollout(mvi, c)
    _force(mvi, ref)
    mvi.calc_deriv1()
    d1 = dict((n, mvi.deriv1(n)) for n in D1)
    HZ = mvi.deriv2_contract(Z, ZL)
    info = mvi.kernel_info()
    mvi.close()
    for m in ("rollout", "deriv1", "deriv2z"):
        assert m in info["spec_launched"] and m not in info["generic_launched"], (m, info)
    for b, r in enumerate(ref):
        e1 = max(relerr(d1[n][b], r["d1"][n]) for n in D1)
        eh = relerr(HZ[b], r["hz"])
        print("%s d1[%d] %.2e hz %.2e" % (name, b, e1, eh))
        assert e1 < mb_bound(name, "d1", e_ref), (name, b, e1)
        assert eh < mb_bound(name, "hz", e_ref), (name, b, eh)


@pytest.mark.parametrize("name", MB_LADDERS)
def test_specialised_agrees_with_generic(monkeypatch, name):
    """Same arithmetic: identical iteration counts, states within 1e-12 relative."""
    c = mb_case(name)
    runs = {}
    for spec in (False, True):
        mvi = _batch(monkeypatch, name, spec)
        X, iters = _rollout(mvi, c)
        runs[spec] = (X, iters)
        info = mvi.kernel_info()
        assert "rollout" in info["spec_launched" if spec else "generic_launched"], info
        mvi.close()
    assert np.array_equal(runs[True][1], runs[False][1]), (runs[True][1], runs[False][1])
    for b in range(c["B"]):
        e = relerr(runs[True][0][b], runs[False][0][b])
        print("%s specialised against generic [%d] %.2e" % (name, b, e))
        assert e < SPEC_VS_GENERIC, (name, b, e)


@pytest.mark.parametrize("name", MB_LADDERS)
def test_specialised_parameter_table_matches_oracle(monkeypatch, name):
    """One run under a per-trajectory parameter table (k_spec_par): every trajectory against the oracle of the system rebuilt with its row."""
    from common import BUILDERS
    from oracle.oracle import OracleMVI
    c = mb_case(name)
    B = c["B"]
    system, _ = build(name)
    rows = random_rows(system, B, seed=61)
    mvi = _batch(monkeypatch, name, True)
    mvi.set_parameters(**rows)
    X, iters = _rollout(mvi, c)
    info = mvi.kernel_info()
    mvi.close()
    assert "rollout" in info["par_spec_launched"] and "rollout" not in info["par_generic_launched"], info       # (calc_p2 is generic)
    assert info["spec_launches"] == 0 and info["generic_launches"] == 0, info
    for b in range(B):
        o = OracleMVI(descriptor.flatten(rebuilt(BUILDERS[name], rows, b)))
        o.initialize_from_configs(0.0, c["Q0"][b], DT, c["Q1"][b])
        Xo, tot = o.rollout(N, DT, c["U"][b], c["K"][b])
        e = relerr(X[b], Xo)
        print("%s parameter row %d: %.2e" % (name, b, e))
        assert e < 1e-10, (name, b, e)
        assert tot == int(iters[b]), (name, b, tot, iters[b])
