"""The dispatch of tg_tv_lq and tg_tangent_rollout, asked on the host (tg_tv_lq_plan / tg_tangent_rollout_plan; no GPU): the table
common.LQ_CASES that test_gpu_lq_classes.py runs names every kernel class a problem can reach and both sides of every boundary,
every silent structured -> dense hand-over happens for the reason the table gives, and what the entry points must refuse is refused
before a device is touched."""
import ctypes

import numpy as np
import pytest

from common import (LQ_CASES, LQ_NU_BOUNDS, LQ_NX_BOUNDS, LQ_REFUSED, lq_case_id, lq_plan, lq_struct)

ERR_INVALID, ERR_UNSUPPORTED = -1, -3
FAKE = dict(A=4096, B=4096, Q=4096, Qf=4096, R=4096, q=4096, r=4096, hz=4096)      # addresses: the plan looks at their alignment only
LDS_BOUND = 160 * 1024 - 256


def _plan(nX, nU, ds=None, monkeypatch=None, env=None, dev=FAKE, hz=None, N=4):
    return lq_plan(_problem(1, N, nX, nU, dev, affine=False, hz=hz, ds=ds), monkeypatch, env)


def _problem(*args, **kw):
    p = lq_struct(*args, **kw)
    p.K_dev = 4096
    return p


def _round_up(n, m):
    return (n + m - 1) // m * m


def _ds_layout(ldx, nU, nd, nq):
    """The LDS layout of k_tv_lq_ds restated (LqDsLayout, csrc/dopt.hip): bytes and 16-column tiles of the compact A block."""
    nUp, ldw, KC, ldc = _round_up(nU, 4), nU + 1 + ldx, 2 * _round_up(nd, 4), 16 * ((nq + nd + 15) // 16)
    lda = ldc if ldc % 32 == 16 else ldc + 16
    doubles = ldx * ldx + 2 * _round_up(KC * lda, 128) + _round_up(ldx * nU, 128) + 64 + nUp * ldx + nUp * ldw + 2 * ldx + 3 * nUp + 66
    return 8 * doubles, ldc // 16


def _mfma_lds(ldx, nU):
    """LqLayout (k_tv_lq_mfma) restated, in bytes, for nX padded to ldx."""
    nUp, ldw = _round_up(nU, 4), nU + 1 + ldx
    return 8 * (2 * ldx * ldx + ldx * nU + 2 * nUp * ldx + nU * ldw + 2 * ldx + 2 * nUp + (0 if nU > 32 else 64))


def _valu_lds(nX, nU, ts):
    ldx = _round_up(nX, ts)
    return 8 * (2 * ldx * ldx + ldx * nU + 2 * nU * ldx + nU * (nU + 1 + ldx) + 2 * ldx + 3 * nU)


@pytest.mark.parametrize("case", LQ_CASES, ids=lq_case_id)
def test_case_runs_the_kernel_the_table_says(case, monkeypatch):
    rc, plan, threads, lds = _plan(case.nX, case.nU, case.ds, monkeypatch, case.env, N=case.N)
    assert rc == 0 and plan == case.plan, (plan, case.plan)
    assert threads == (256 if plan[0] == 0 else 512)
    want = {0: lambda: _valu_lds(case.nX, case.nU, plan[1]), 1: lambda: _mfma_lds(16 * plan[1], case.nU),
            2: lambda: _ds_layout(16 * plan[1], case.nU, case.ds[0], case.ds[0] + case.ds[1])[0]}[plan[0]]()
    assert lds == want and lds <= (LDS_BOUND if plan[0] else 160 * 1024 - 64)
    if case.ds and not case.why:
        assert plan[0] == 2 or case.env
    if case.why:
        assert case.ds and plan[0] != 2


def test_table_names_every_reachable_class(monkeypatch):
    """Enumerate the sizes through the plan: which (kernel, class, NR) exist at all, and does the table have a case for each."""
    table = set((c.plan, bool(c.env.get("TREPAMD_LQ_LEGACY"))) for c in LQ_CASES)
    dense, valu, structured, legacy = set(), set(), set(), set()
    for nX in range(1, 97):
        for nU in range(1, 65):
            rc, plan, _, _ = _plan(nX, nU, monkeypatch=monkeypatch)
            if rc == 0:
                (dense if plan[0] == 1 else valu).add(plan)
                assert plan[0] != 2 and (nU <= 32 or plan[0] == 0)
            else:
                assert rc == ERR_UNSUPPORTED
    for nd in range(1, 49):
        for nk in range(0, 49):
            for nu in range(0, 49):
                nX, nU = 2 * (nd + nk), nu + nk
                if 1 <= nU <= 64 and nX <= 96:
                    rc, plan, _, _ = _plan(nX, nU, (nd, nk, nu), monkeypatch)
                    if rc == 0 and plan[0] == 2:
                        structured.add(plan)
    for nX in range(1, 97):
        for nU in range(1, 65):
            rc, plan, _, _ = _plan(nX, nU, monkeypatch=monkeypatch, env={"TREPAMD_LQ_LEGACY": "1"})
            if rc == 0:
                assert plan[0] == 0
                legacy.add(plan)
    print("reachable classes: dense matrix-core %d of 20, structured %d of 20, VALU %d (default) / %d (TREPAMD_LQ_LEGACY=1)"
          % (len(dense), len(structured), len(valu), len(legacy)))
    # LDS, not the template list, ends the matrix-core classes: NT = 5 stops at NR = 20 (dense; the structured layout holds NR = 32)
    # and NT = 6 (two 96 x 96 matrices: 147 KB) at NR = 4 (dense) or nowhere (structured)
    assert dense == set((1, nt, nr) for nt in (1, 2, 3) for nr in (4, 8, 20, 32)) | {(1, 5, 4), (1, 5, 8), (1, 5, 20), (1, 6, 4)}
    assert structured == set((2, nt, nr) for nt in (1, 2, 3, 5) for nr in (4, 8, 20, 32))
    assert valu == legacy == {(0, 2, 0), (0, 4, 0), (0, 5, 0), (0, 6, 0)}
    for plan in sorted(dense | structured | valu):
        assert (plan, False) in table, "no case of LQ_CASES runs class %r" % (plan,)
    for plan in sorted(legacy):
        assert (plan, True) in table, "no case of LQ_CASES runs VALU class %r under TREPAMD_LQ_LEGACY=1" % (plan,)
    # the VALU kernel is the only path above 32 inputs: in the table on its own, up to the largest sizes its LDS holds
    assert any(c.nU == 33 and not c.env and c.plan[0] == 0 for c in LQ_CASES) and any(c.nU == 64 and c.plan[0] == 0 for c in LQ_CASES)


def test_both_sides_of_every_boundary_are_in_the_table(monkeypatch):
    dense = [c for c in LQ_CASES if c.ds is None and not c.env]
    sizes_x, sizes_u = set(c.nX for c in dense if c.plan[0] == 1), set(c.nU for c in dense if c.plan[0] == 1)
    for b, (lo, hi) in zip(LQ_NX_BOUNDS, ((1, 2), (2, 3), (3, 5), (5, 6))):
        assert b in sizes_x and b + 1 in sizes_x, b
        assert _plan(b, 4, monkeypatch=monkeypatch)[1] == (1, lo, 4) and _plan(b + 1, 4, monkeypatch=monkeypatch)[1] == (1, hi, 4)
    assert 96 in sizes_x and (97, 4, {}) in LQ_REFUSED
    for b, (lo, hi) in zip(LQ_NU_BOUNDS[:3], ((4, 8), (8, 20), (20, 32))):
        assert b in sizes_u and b + 1 in sizes_u, b
        assert _plan(16, b, monkeypatch=monkeypatch)[1] == (1, 1, lo) and _plan(16, b + 1, monkeypatch=monkeypatch)[1] == (1, 1, hi)
    assert 32 in sizes_u and any(c.nU == 33 and c.plan[0] == 0 for c in dense)
    assert _plan(16, 32, monkeypatch=monkeypatch)[1] == (1, 1, 32) and _plan(16, 33, monkeypatch=monkeypatch)[1][0] == 0
    assert any(c.nU == 64 for c in dense) and (16, 65, {}) in LQ_REFUSED
    # the VALU kernel's own limits (its LDS): both sides at 33 and at 64 inputs
    for nX, nU in ((66, 33), (42, 64)):
        assert any((c.nX, c.nU) == (nX, nU) for c in dense) and (nX + 1, nU, {}) in LQ_REFUSED
    # horizons: one step, two steps, lengths that are a multiple of nothing
    horizons = set(c.N for c in LQ_CASES)
    assert {1, 2, 7, 13} <= horizons and all(c.S >= 2 for c in LQ_CASES)
    for kernel in (0, 1, 2):
        assert any(c.select and c.plan[0] == kernel and len(c.select) < c.S for c in LQ_CASES), kernel


def test_silent_handovers_happen_for_the_reason_given(monkeypatch):
    seen = set()
    for c in LQ_CASES:
        if not c.why:
            continue
        nd, nk, nu = c.ds
        rc, plan, _, _ = _plan(c.nX, c.nU, c.ds, monkeypatch, c.env)
        assert rc == 0 and plan[0] != 2
        pad, nk31 = nk < _round_up(nd, 4) - nd, nk > 31
        if plan[0] == 0:      # more than 31 kinematic configs: 66 states and 32 inputs at least, which no matrix-core layout holds either
            assert c.why == "nk31" and nk31 and not pad and _mfma_lds(80, c.nU) > LDS_BOUND
            seen.add(c.why)
            continue
        nt = _plan(c.nX, min(c.nU, 32), monkeypatch=monkeypatch)[1][1]
        lds, ctiles = _ds_layout(16 * nt, c.nU, nd, nd + nk)
        tiles = nt * ctiles + nt * ((c.nU + 15) // 16) > 32
        reasons = dict(pad=pad, nk31=nk31, lds=lds > LDS_BOUND, tiles=tiles)
        if c.why == "env":
            assert not any(reasons.values()) and _plan(c.nX, c.nU, c.ds, monkeypatch)[1][0] == 2
        else:
            assert set(k for k, v in reasons.items() if v) == set(c.why.split("+")), (c, reasons)
        seen.add(c.why)
    assert seen == {"pad", "nk31", "lds", "lds+tiles", "env"}
    # the other side of each: one less / one more and the structured kernel runs
    assert _plan(16, 4, (8, 0, 4), monkeypatch)[1][0] == 2 and _plan(16, 4, (7, 1, 3), monkeypatch)[1][0] == 2
    assert _plan(64, 31, (1, 31, 0), monkeypatch)[1] == (2, 5, 32)
    assert _plan(56, 16, (25, 3, 13), monkeypatch)[1] == (2, 5, 20)
    # the tile limit of phase 1 never decides alone: wherever it holds the LDS bound holds too (so it has no case of its own)
    for nd in range(1, 49):
        for nk in range(0, 32):
            for nu in range(0, 33 - nk):
                nX, nU = 2 * (nd + nk), nu + nk
                if nU >= 1 and nX <= 96:
                    nt = next(t for t, b in zip((1, 2, 3, 5, 6), (16, 32, 48, 80, 96)) if nX <= b)
                    lds, ctiles = _ds_layout(16 * nt, nU, nd, nd + nk)
                    assert lds > LDS_BOUND or nt * ctiles + nt * ((nU + 15) // 16) <= 32


def test_misaligned_structured_problem_takes_the_dense_kernel(monkeypatch):
    """k_tv_lq_ds fills LDS with 16-byte global_load_lds from A_k and B_k: a base that sits on an 8-byte boundary only is handed to the
    dense kernel (8-byte loads), whichever of the two arrays it is."""
    ds, nX, nU = (22, 18, 0), 80, 18
    assert _plan(nX, nU, ds, monkeypatch)[1] == (2, 5, 20)
    for name in ("A", "B"):
        dev = dict(FAKE, **{name: 4096 + 8})
        assert _plan(nX, nU, ds, monkeypatch, dev=dev)[1] == (1, 5, 20), name
    assert _plan(nX, nU, ds, monkeypatch, dev=dict(FAKE, A=4096 + 16, B=4096 + 48))[1] == (2, 5, 20)
    assert _plan(nX, nU, ds, monkeypatch, dev=dict(FAKE, Q=4096 + 8, R=4096 + 8, Qf=4096 + 8))[1] == (2, 5, 20)      # weights: 8-byte loads


def test_curvature_in_the_v_rows_takes_the_dense_kernel(monkeypatch):
    """k_tv_lq_ds never computes the v columns of Kpart and K: a curvature block whose state part reaches past [Qd | Qk | p] (S_k then has
    v rows) is handed to the dense kernel."""
    nd, nk, nu = ds = (22, 18, 0)
    nX, nU, nxh = 80, 18, 2 * nd + nk
    assert _plan(nX, nU, ds, monkeypatch, hz=(nxh + nU, nxh))[1] == (2, 5, 20)
    assert _plan(nX, nU, ds, monkeypatch, hz=(nU, 0))[1] == (2, 5, 20)
    assert _plan(nX, nU, ds, monkeypatch, hz=(nxh + 1 + nU, nxh + 1))[1] == (1, 5, 20)
    assert _plan(nX, nU, ds, monkeypatch, hz=(nX + nU, nX))[1] == (1, 5, 20)


def test_sizes_beyond_the_kernels_are_refused_on_the_host(monkeypatch):
    from trep_amd import _lib
    L = _lib.lib()
    for nX, nU, env in LQ_REFUSED:
        p = _problem(2, 5, nX, nU, FAKE, affine=False)
        rc = lq_plan(p, monkeypatch, env)[0]
        assert rc == ERR_UNSUPPORTED, (nX, nU, env, rc)
        assert L.tg_tv_lq(0, ctypes.byref(p)) == ERR_UNSUPPORTED            # nothing launched: the same refusal without a device
    # the LDS bound is what refuses 96 x 5: both layouts are over it, one input less is under
    assert _mfma_lds(96, 4) <= LDS_BOUND < _mfma_lds(96, 5) and _valu_lds(96, 5, 6) > 160 * 1024 - 64
    assert _valu_lds(66, 33, 6) <= 160 * 1024 - 64 < _valu_lds(67, 33, 6)
    # 48 x 64, 64 x 48, 93 x 33: inside the VALU classes' nX * nU <= 3072, but not inside its LDS
    for nX, nU in ((48, 64), (64, 48), (93, 33)):
        assert nX * nU <= 3072 and _valu_lds(nX, nU, 6) > 160 * 1024 - 64


def test_terminal_conditions_that_are_refused(monkeypatch):
    """tg_tv_lq validates before it touches a device: a terminal P without its b on an affine problem (the kernels would continue the
    vector recursion from different leftovers), and a terminal (P, b) for a sweep that starts at the horizon's end (it would silently
    replace Qf and q_N)."""
    from trep_amd import _lib
    L = _lib.lib()
    N = 9

    def rc_of(affine, k_range, Pt, bt):
        p = _problem(2, N, 26, 9, FAKE, affine=affine, ds=(9, 4, 5))
        p.k_begin, p.k_end = k_range
        p.Pt_dev, p.bt_dev = Pt, bt
        rc = lq_plan(p, monkeypatch)[0]
        if rc != 0:          # the entry point refuses it the same way, before a device is touched (an accepted problem is never launched here: the
            assert L.tg_tv_lq(0, ctypes.byref(p)) == rc          # pointers are made up)
        return rc

    assert rc_of(True, (3, 6), 4096, None) == ERR_INVALID
    assert rc_of(True, (3, 6), 4096, 4096) == 0
    assert rc_of(False, (3, 6), 4096, None) == 0                 # LQR: there is no b
    assert rc_of(True, (3, 6), None, None) == ERR_INVALID        # (as before: the steps behind need their (P, b))
    for k_range in ((0, 0), (0, N), (4, N)):
        assert rc_of(True, k_range, 4096, 4096) == ERR_INVALID, k_range
        assert rc_of(False, k_range, 4096, None) == ERR_INVALID, k_range
        assert rc_of(True, k_range, None, None) == 0


def _tangent_plan(nX, nU, A=4096, B=4096, K=4096):
    from trep_amd import _lib
    out = np.full(6, -7, dtype=np.int32)
    rc = _lib.lib().tg_tangent_rollout_plan(nX, nU, A, B, K, out.ctypes.data_as(_lib._c_ip))
    return rc, tuple(int(x) for x in out)


def test_tangent_rollout_plan(monkeypatch):
    monkeypatch.delenv("TREPAMD_TANGENT_LDS", raising=False)
    monkeypatch.delenv("TREPAMD_TANGENT_NO_PAIRS", raising=False)
    threads = lambda nX, nU: (max(4 * nX, 8 * nU) + 63) // 64 * 64
    # three register classes x paired / unpaired, both sides of their boundaries (nX 32 | 33, 80 | 81; nU 16 | 17, 24 | 25)
    for nX, nU, cls in ((32, 16, (8, 4, 4)), (34, 16, (20, 6, 10)), (32, 18, (20, 6, 10)), (80, 24, (20, 6, 10)), (82, 24, (24, 8, 12)),
                        (80, 26, (24, 8, 12)), (96, 32, (24, 8, 12)), (2, 2, (8, 4, 4)), (80, 18, (20, 6, 10))):
        assert _tangent_plan(nX, nU) == (0, (1,) + cls + (1, threads(nX, nU))), (nX, nU)
        for which in range(3):          # any of A, B, K on an 8-byte boundary only: one column per thread, 8-byte loads
            ptrs = [4096, 4096, 4096]
            ptrs[which] += 8
            assert _tangent_plan(nX, nU, *ptrs) == (0, (1,) + cls + (0, threads(nX, nU))), (nX, nU, which)
    for nX, nU, cls in ((32, 16, (8, 4, 4)), (33, 16, (20, 6, 10)), (31, 17, (20, 6, 10)), (80, 24, (20, 6, 10)), (81, 24, (24, 8, 12)),
                        (79, 25, (24, 8, 12)), (95, 31, (24, 8, 12)), (1, 1, (8, 4, 4)), (33, 32, (24, 8, 12))):
        if nX % 2 or nU % 2:           # odd sizes are never paired
            assert _tangent_plan(nX, nU) == (0, (1,) + cls + (0, threads(nX, nU))), (nX, nU)
    # the first sizes that leave the register kernel: 33 inputs (LDS-staged kernel), 97 states (refused: over its limits too)
    assert _tangent_plan(16, 33) == (0, (0, 0, 0, 0, 0, 256))
    assert _tangent_plan(96, 32)[1][0] == 1 and _tangent_plan(97, 4)[0] == ERR_UNSUPPORTED
    assert _tangent_plan(96, 33)[0] == ERR_UNSUPPORTED            # nX * nU over 12 x 256
    monkeypatch.setenv("TREPAMD_TANGENT_LDS", "1")
    assert _tangent_plan(80, 18) == (0, (0, 0, 0, 0, 0, 256))
    monkeypatch.delenv("TREPAMD_TANGENT_LDS")
    monkeypatch.setenv("TREPAMD_TANGENT_NO_PAIRS", "1")
    assert _tangent_plan(80, 18) == (0, (1, 20, 6, 10, 0, 320))
