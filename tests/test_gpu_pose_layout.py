"""The specialised rollout kernels on the world-frame path (eval_world, pose_sweep_dual, chain_round_quads, newton_matrix_world in
csrc/mvi_core.hpp) after a change of their LDS record layout: the composite records 18 doubles apart where the plan
has room (program.hpp: kCmpStride; both puppets) and 16 apart where it has not (both ladders), the stride read back from the plan, and
the copied rows of the translation runs taken from the plan cell tr_rows.  The change moves data without changing a value or the order
of an operation, so nothing here is looser than what the kernels were held to before.  (The pose arrays keep their 12-double records:
the half-record layout measured with the same change is not in the tree, docs/LOG.md; the cases were chosen for it -- every joint kind,
every column -- and stay.)

Four systems specialise with the world-frame evaluation (the test fails, it does not skip, if one should lose it): puppet40 (all six
joint kinds; translation runs with copied rows; a floating base; nine subtree groups), puppet_basic (no kinematic configs),
ladder_point (an odd Newton system, nf = 19; two-sided point constraints) and ladder_mixed (wev_rc_ident = 0: the body lanes use all
twelve pose entries with a constant rotation).  B = 5 (one partly filled block), N = 3 steps, both pivot rules (k_spec<0, 0> and
k_spec<0, 1>), with the trajectory X and without it (then q2, p2, lambda1 of the state).

Two witnesses.  The oracle, at the tolerances of tests/test_gpu_rollout_step_edge.py: TOL on the states (relerr), common.TB_TOL on
lambda1, Newton iterations per trajectory equal.  And the generic kernel, which has neither composites nor translation runs:
within 1e-12 (the claim of csrc/spec_kernel.hip: same arithmetic up to the compiler's FMA contraction;
tests/test_gpu_world_frame_shapes.py), iteration counts equal.  One puppet case under a per-trajectory parameter table (k_spec_par),
and one that runs deriv1 of the specialised library right after a rollout on the same batch: the derivative kernels overlay the same
LDS areas with their own layout.  Its bound is common.TB_TOL["d1"], the project's bound for these arrays against the oracle: both
kernels meet it, they differ from each other by FMA contraction alone, and a record read in the wrong place is wrong in the first
digit.

Starts and inputs are common.tb_case's for every system (distinct starts on the recorded trajectories, as tests/test_gpu_time_base.py
and tests/test_gpu_world_frame_shapes.py use them): the starts the project's 1e-12 between specialised and generic kernels is stated
for.  (The scaled starts of tests/test_gpu_rollout_step_edge.py are not: from puppet_basic's start at rest the specialised kernel of
the commit before this one already differs from the generic one by 1.14e-12, and this tree's specialised rollouts are that commit's
bit for bit.)  Every reference is computed once and read-only."""
import functools
import re

import numpy as np
import pytest

from common import BUILDERS, D1, TB_TOL, build, relerr, tb_case, tb_oracle_rollout
from test_parameters_cpu import random_rows, rebuilt

pytestmark = pytest.mark.gpu

DT = 0.01
TOL = 1e-10                      # tests/test_gpu_rollout_step_edge.py
SPEC_VS_GENERIC = 1e-12          # tests/test_gpu_world_frame_shapes.py
B, N = 5, 3
SYSTEMS = ("puppet40", "puppet_basic", "ladder_point", "ladder_mixed")


@functools.lru_cache(maxsize=None)
def _reference(name):
    """dict(system, d, Q0, Q1, U, K [B][N], X [B][N + 1], its [B], lam [B][nc]) of the oracle's N steps from each start."""
    system, d = build(name)
    c = tb_case(name, "uniform", N, B)
    runs = [tb_oracle_rollout(d, c["Q0"][b], c["Q1"][b], np.full(N, DT), c["U"][b], c["K"][b]) for b in range(B)]
    out = dict(Q0=c["Q0"], Q1=c["Q1"], U=c["U"], K=c["K"], X=np.array([r["X"] for r in runs]),
               its=np.array([r["iterations"] for r in runs]), lam=np.array([r["lambda1"] for r in runs]))
    out = dict((k, np.ascontiguousarray(v)) for k, v in out.items())
    for v in out.values():
        v.setflags(write=False)
    out.update(system=system, d=d)
    return out


def _batch(monkeypatch, system, spec, exact=False):
    import trep_amd
    from trep_amd import specialize
    for k in ("TREPAMD_TEAM", "TREPAMD_NO_SPECIALIZE", "TREPAMD_SPEC_OVERRIDE", "TREPAMD_SPEC_FLAGS"):
        monkeypatch.delenv(k, raising=False)
    if spec:
        assert specialize.is_built(system), "build() prebuilds the specialisations of the four systems"
    mvi = trep_amd.BatchMidpointVI(system, B, specialize=bool(spec))
    mvi.exact_pivot = exact
    return mvi


def _inputs(r):
    d = r["d"]
    return (r["U"] if d.n_inputs else None, r["K"] if d.n_kin else None)


def _run(mvi, r, with_X=True):
    """(X or None, q2, p2, lambda1, iterations) of N steps from the reference's starts."""
    mvi.initialize_from_configs(0.0, r["Q0"], DT, r["Q1"])
    U, K = _inputs(r)
    X = None
    if with_X:
        X = mvi.rollout(N, DT, U, K)
    else:
        mvi.rollout_device(N, DT, mvi.device_array(U) if U is not None else None, mvi.device_array(K) if K is not None else None, None)
        mvi.synchronize()
    iters, status = mvi.status()
    assert (status == 0).all(), status
    return X, mvi.q2, mvi.p2, mvi.lambda1, iters


@functools.lru_cache(maxsize=None)
def _generic_run(name, exact):
    """The same rollout through the generic kernel: computed once per (system, pivot rule)."""
    mp = pytest.MonkeyPatch()
    try:
        r = _reference(name)
        mvi = _batch(mp, r["system"], False, exact)
        out = _run(mvi, r)
        info = mvi.kernel_info()
        mvi.close()
    finally:
        mp.undo()
    assert "rollout" in info["generic_launched"] and "rollout" not in info["spec_launched"], info
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _world_frame(name):
    """wev_ok of the system's schedule, from the header its specialisation is compiled against"""
    from trep_amd import specialize
    return int(re.search(r"static constexpr int wev_ok = (-?\d+);", specialize.header(_reference(name)["system"])).group(1))


def _assert_world_frame(mvi, name, exact):
    kinfo = mvi.kernel_info()
    assert "rollout" in kinfo["spec_launched"] and "rollout" not in kinfo["generic_launched"], kinfo
    assert kinfo["exact_pivot"] == exact
    assert _world_frame(name) == 1, "%s lost the world-frame evaluation" % name


@pytest.mark.parametrize("with_X", [True, False], ids=["X", "noX"])
@pytest.mark.parametrize("exact", [False, True], ids=["ranked", "exact"])
@pytest.mark.parametrize("name", SYSTEMS)
def test_specialised_rollout_matches_oracle_and_generic_kernel(monkeypatch, name, exact, with_X):
    r = _reference(name)
    nq, nd = r["d"].n_configs, r["d"].n_dyn
    mvi = _batch(monkeypatch, r["system"], True, exact)
    X, q2, p2, lam1, iters = _run(mvi, r, with_X)
    _assert_world_frame(mvi, name, exact)
    mvi.close()
    Xg, q2g, p2g, lam1g, itersg = _generic_run(name, exact)
    worst = dict(X=0.0, q2=0.0, p2=0.0, lambda1=0.0)
    generic = dict(X=0.0, q2=0.0, p2=0.0)
    for b in range(B):
        if with_X:
            worst["X"] = max(worst["X"], relerr(X[b], r["X"][b]))
            generic["X"] = max(generic["X"], relerr(X[b], Xg[b]))
        worst["q2"] = max(worst["q2"], relerr(q2[b], r["X"][b, N, :nq]))
        worst["p2"] = max(worst["p2"], relerr(p2[b], r["X"][b, N, nq:nq + nd]))
        worst["lambda1"] = max(worst["lambda1"], relerr(lam1[b], r["lam"][b]))
        generic["q2"] = max(generic["q2"], relerr(q2[b], q2g[b]))
        generic["p2"] = max(generic["p2"], relerr(p2[b], p2g[b]))
    print("%s exact=%d X=%d: oracle" % (name, exact, with_X), " ".join("%s %.2e" % kv for kv in sorted(worst.items())),
          "| generic", " ".join("%s %.2e" % kv for kv in sorted(generic.items())),
          "| iterations %s / oracle %s / generic %s" % (iters.tolist(), r["its"].tolist(), itersg.tolist()))
    assert worst["X"] < TOL and worst["q2"] < TOL and worst["p2"] < TOL, (name, worst)
    assert worst["lambda1"] < TB_TOL["lambda1"], (name, worst)
    assert np.array_equal(iters, r["its"])
    assert generic["X"] < SPEC_VS_GENERIC and generic["q2"] < SPEC_VS_GENERIC and generic["p2"] < SPEC_VS_GENERIC, (name, generic)
    assert np.array_equal(iters, itersg)


def test_parameter_table_kernel_matches_rebuilt_systems(monkeypatch):
    """k_spec_par<0, 0>: every trajectory of the puppet under its own masses, inertias, gravity and damping, against the oracle of the
    system rebuilt with that row (as tests/test_gpu_world_frame_shapes.py does for the ladders)."""
    from oracle.oracle import OracleMVI
    from trep_amd import descriptor
    name = "puppet40"
    r = _reference(name)
    rows = random_rows(r["system"], B, seed=61)
    mvi = _batch(monkeypatch, r["system"], True)
    mvi.set_parameters(**rows)
    X, q2, p2, lam1, iters = _run(mvi, r)
    info = mvi.kernel_info()
    mvi.close()
    assert "rollout" in info["par_spec_launched"] and "rollout" not in info["par_generic_launched"], info
    assert info["spec_launches"] == 0 and info["generic_launches"] == 0, info
    for b in range(B):
        o = OracleMVI(descriptor.flatten(rebuilt(BUILDERS[name], rows, b)))
        o.initialize_from_configs(0.0, r["Q0"][b], DT, r["Q1"][b])
        Xo, tot = o.rollout(N, DT, r["U"][b] if r["d"].n_inputs else None, r["K"][b])
        e = relerr(X[b], Xo)
        print("%s parameter row %d: %.2e, iterations %d / %d" % (name, b, e, int(iters[b]), tot))
        assert e < TOL, (b, e)
        assert tot == int(iters[b]), (b, tot, iters[b])


def test_deriv1_after_a_rollout_matches_generic_kernel(monkeypatch):
    """The derivative kernels of the specialised library lay their own tables over the LDS areas the rollout has just used for the
    composites and the twist records; every launch forms what it reads."""
    name = "puppet40"
    r = _reference(name)
    got = {}
    for spec in (True, False):
        mvi = _batch(monkeypatch, r["system"], spec)
        _run(mvi, r)
        mvi.calc_deriv1()
        got[spec] = dict((n, mvi.deriv1(n)) for n in D1)
        info = mvi.kernel_info()
        mvi.close()
        launched = info["spec_launched" if spec else "generic_launched"]
        assert "rollout" in launched and "deriv1" in launched, info
    for n in D1:
        for b in range(B):
            e = relerr(got[True][n][b], got[False][n][b])
            print("%s deriv1 %s[%d]: specialised against generic %.2e" % (name, n, b, e))
            assert e < TB_TOL["d1"], (n, b, e)
