"""The translational prefix of a floating base in the plan of the world-frame rollout kernels (program.hpp, fb_*), read back
from the generated specialisation header (no GPU needed), and the exactness of what the kernel does with it, in numpy on the formulas of
tools/proto/world_eval.py:

* the plan constants of the BASELINE systems -- prefix, the shorter pair list (the old one minus the off-diagonal pairs whose first
  config is in the prefix), the shorter lists (the whole prefix replaced by one shared record), the shape of the constraint records;
* small trees that must NOT qualify, or only with a shorter prefix;
* the four inner products of a prefix pair in the kernel's operation order against their closed forms, and the list sum with the shared
  record against the entry-by-entry sum: equal value for value (np.array_equal), for 200 random puppet states and rates."""
import re

import numpy as np
import pytest

from common import build


def _parse(system):
    from trep_amd import specialize
    text = specialize.header(system)
    ints = {m.group(1): int(m.group(2)) for m in re.finditer(r"static constexpr int (\w+) = (-?\d+);", text)}
    pool = np.array([int(x) for x in re.search(r"spec_ipool\[\d+\] = \{([^}]*)\}", text, re.S).group(1).replace("\n", "").split(",")], dtype=np.int64)
    offs = {m.group(1): int(m.group(2)) for m in re.finditer(r"static constexpr const int \*(\w+) = spec_ipool \+ (\d+);", text)}
    return ints, pool, offs


def _header(name):
    system, _ = build(name)
    return (system,) + _parse(system)


def _lists(pool, offs, table, nd):
    lane = pool[offs[table]:offs[table] + 256].reshape(64, 4)
    out = []
    for l in range(64):
        b = [(int(lane[l, e >> 2]) >> (8 * (e & 3))) & 0xFF for e in range(12)]
        n = next((i for i, v in enumerate(b) if v == nd), 12)
        assert all(v == nd for v in b[n:])
        out.append(b[:n])
    return out


@pytest.mark.parametrize("name", ["puppet40", "puppet_basic"])
def test_puppet_plan_has_the_three_translations(name):
    system, ints, pool, offs = _header(name)
    nd = ints["nd"]
    assert ints["fb_n"] == 3 and ints["fb_on"] == 1
    assert [ints["fb_cfg_%d" % i] for i in range(3)] == [0, 1, 2] and [ints["fb_axis_%d" % i] for i in range(3)] == [0, 1, 2]
    # pairs: 97 = the old set minus the off-diagonal pairs with a prefix config first; diagonal pairs first and in config order
    old = [(int(w) & 0xFFFF, int(w) >> 16) for w in pool[offs["cmp_pair"]:offs["cmp_pair"] + ints["n_cmpairs"]]]
    new = [(int(w) & 0xFFFF, int(w) >> 16) for w in pool[offs["fb_pair"]:offs["fb_pair"] + ints["fb_npairs"]]]
    assert ints["n_cmpairs"] == 157 and ints["fb_npairs"] == 97 and len(old) - len(new) == 60
    assert new == [p for p in old if p[0] == p[1] or p[0] > 2]
    assert new[:nd] == [(c, c) for c in range(nd)]
    assert (ints["fb_npairs"] + 63) // 64 == 2 and (ints["n_cmpairs"] + 63) // 64 == 3      # phase D loses a trip
    # the dropped entries: lane b's count of prefix configs above it
    m = [(int(pool[offs["fb_abx"] + 2 * b]) & 0xFFFFFFFF) >> 30 for b in range(nd)]
    assert sorted((a, b) for b in range(nd) for a in range(m[b])) == sorted(p for p in old if p[0] != p[1] and p[0] <= 2)
    # lists: the whole prefix at the start of a list becomes the record nd + 1; the lists of the prefix configs stay as they are
    was, now = _lists(pool, offs, "wev_lane", nd), _lists(pool, offs, "fb_lane", nd)
    for l in range(64):
        assert now[l] == ([nd + 1] + was[l][3:] if was[l][:3] == [0, 1, 2] else was[l]), l
    assert now[:3] == [[], [0], [0, 1]]
    assert ints["fb_depth"] == max(len(x) for x in now) == ints["wev_depth"] - 2
    # room for the record: the per-config vectors start behind nd + 2 twist records
    assert ints["o_ccz"] == ints["o_csw"] + 12 * (nd + 2) and nd + 3 * ints["n_bodies"] < 63
    assert ints["dhr_sides"] == 1 and ints["dhr_types"] == 1


def test_packed_places_of_the_closed_form_entries():
    system, ints, pool, offs = _header("puppet40")
    nf, nd = ints["nf"], ints["nd"]
    m = pool[offs["bbd_map"]:offs["bbd_map"] + nf * (nf + 1)].reshape(nf, nf + 1)
    for b in range(nd):
        w0, w1 = int(pool[offs["fb_abx"] + 2 * b]) & 0xFFFFFFFF, int(pool[offs["fb_abx"] + 2 * b + 1]) & 0xFFFFFFFF
        at = [w0 & 0x3FF, (w0 >> 10) & 0x3FF, (w0 >> 20) & 0x3FF, w1 & 0x3FF, (w1 >> 10) & 0x3FF, (w1 >> 20) & 0x3FF]
        for a in range(w0 >> 30):
            assert at[2 * a] == m[a, b] and at[2 * a + 1] == m[b, a] and m[a, b] >= 0 and m[b, a] >= 0
    pairx = pool[offs["fb_pairx"]:offs["fb_pairx"] + ints["fb_npairs"]].astype(np.uint32)
    for x in pairx:
        a, b, ab, ba = int(x) & 63, (int(x) >> 6) & 63, (int(x) >> 12) & 0x3FF, (int(x) >> 22) & 0x3FF
        assert ab == m[a, b] and ba == m[b, a]


@pytest.mark.parametrize("name,want", [
    # scissor lift (the slider) and pendulum on a cart (the cart): one translation along x each, rotary joints below it, and no world-frame
    # evaluation to use it in; the lift's constraints are two-sided point constraints, the cart has none
    ("scissor4", dict(fb_n=1, fb_on=0, fb_cfg_0=0, fb_axis_0=0, fb_cfg_1=-1, dhr_sides=3, dhr_types=2)),
    ("pend_on_cart", dict(fb_n=1, fb_on=0, fb_cfg_0=0, fb_axis_0=0, fb_cfg_1=-1, dhr_sides=0, dhr_types=0)),
])
def test_other_baseline_plans_are_pinned(name, want):
    _, ints, _, _ = _header(name)
    assert {k: ints[k] for k in want} == want
    assert ints["fb_npairs"] == 0 and ints["fb_depth"] == 0


def _tree(frames):
    import trep_amd as T
    system = T.System()
    system.import_frames(frames(T))
    T.potentials.Gravity(system, (0, 0, -9.8))
    return _parse(system)[0]


def test_synthetic_trees_fall_back():
    body = lambda T: [T.rx('a', name='A'), [T.tz(-0.5, name='M', mass=1.0)]]
    full = _tree(lambda T: [T.tx('x'), [T.ty('y'), [T.tz('z'), body(T)]]])
    assert (full["fb_n"], full["fb_cfg_0"], full["fb_cfg_1"], full["fb_cfg_2"], full["fb_on"]) == (3, 0, 1, 2, 0)      # (too small for the world-frame kernels)
    order = _tree(lambda T: [T.tz('z'), [T.tx('x'), body(T)]])
    assert (order["fb_n"], order["fb_axis_0"], order["fb_axis_1"]) == (2, 2, 0)
    # a rotated pre-transform on the second translation: the prefix ends before it
    rotated = _tree(lambda T: [T.tx('x'), [T.rz(0.3), [T.ty('y'), [T.tz('z'), body(T)]]]])
    assert rotated["fb_n"] == 1 and rotated["fb_cfg_1"] == -1
    # a translated one, likewise (the pose would no longer be the sum of the rates' axes alone -- kept out: identity only)
    shifted = _tree(lambda T: [T.tx('x'), [T.tz(0.25), [T.ty('y'), body(T)]]])
    assert shifted["fb_n"] == 1
    # two translations on one axis
    twice = _tree(lambda T: [T.tx('x'), [T.tx('x2'), [T.tz('z'), body(T)]]])
    assert twice["fb_n"] == 1 and twice["fb_cfg_1"] == -1
    # a kinematic root translation
    kinematic = _tree(lambda T: [T.tx('x', kinematic=True), [T.ty('y'), body(T)]])
    assert kinematic["fb_n"] == 0
    # a rotary joint first
    rotary = _tree(lambda T: [T.rz('r'), [T.tx('x'), [T.ty('y'), body(T)]]])
    assert rotary["fb_n"] == 0


# ---- exactness -----------------------------------------------------------------------------------------------------------------------

def _bracket(a, b):      # mvi_core.hpp bracket(): [a, b] for twists (v, w), term by term in its order
    r = np.empty(6)
    r[0] = a[4] * b[2] - a[5] * b[1] + a[1] * b[5] - a[2] * b[4]
    r[1] = a[5] * b[0] - a[3] * b[2] + a[2] * b[3] - a[0] * b[5]
    r[2] = a[3] * b[1] - a[4] * b[0] + a[0] * b[4] - a[1] * b[3]
    r[3] = a[4] * b[5] - a[5] * b[4]
    r[4] = a[5] * b[3] - a[3] * b[5]
    r[5] = a[3] * b[4] - a[4] * b[3]
    return r


def _world_state(system, q, dq):
    """s, u = s dq, paths, per-config composites (M, C, D, H) as tools/proto/world_eval.py forms them"""
    for c, x, v in zip(system.configs, q, dq):
        c.q, c.dq = x, v
    nq = len(system.configs)
    idx = {c: i for i, c in enumerate(system.configs)}
    s, path_of = np.zeros((nq, 6)), {}
    for f in system.frames:
        if f.config is None:
            continue
        g = f.g()
        kind = f.transform_type.name if hasattr(f.transform_type, "name") else str(f.transform_type)
        ax = {"x": 0, "y": 1, "z": 2}[kind[-1].lower()]
        a, p = g[:3, ax], g[:3, 3]
        s[idx[f.config]] = np.concatenate([a, np.zeros(3)]) if kind.lower().startswith("t") else np.concatenate([-np.cross(a, p), a])
        path_of[idx[f.config]] = [idx[x.config] for x in f._path() if x.config is not None]
    u = s * np.asarray(dq)[:, None]
    M, C, D, H = np.zeros(nq), np.zeros((nq, 3)), np.zeros((nq, 3, 3)), np.zeros((nq, 6))
    body_paths = []
    for f in system.masses:
        g = f.g()
        R, p = g[:3, :3], g[:3, 3]
        path = [idx[x.config] for x in f._path() if x.config is not None]
        body_paths.append(path)
        V = sum(u[j] for j in path)
        I = R.dot(np.diag([f.Ixx, f.Iyy, f.Izz])).dot(R.T)
        lin = f.mass * (V[:3] + np.cross(V[3:], p))
        ang = I.dot(V[3:]) + np.cross(p, lin)
        for j in path:
            M[j] += f.mass; C[j] += f.mass * p; D[j] += I + f.mass * (p.dot(p) * np.eye(3) - np.outer(p, p)); H[j] += np.concatenate([lin, ang])
    return s, u, path_of, body_paths, (M, C, D, H)


def _apply(M, C, D, x):      # I x = (M v - C x w, C x v + D w): newton_matrix_world's phase C
    return np.concatenate([M * x[:3] - np.cross(C, x[3:]), np.cross(C, x[:3]) + D.dot(x[3:])])


def _states(system, n, seed):
    from trep_amd import systems
    rng = np.random.default_rng(seed)
    Q = systems.puppet_initial_conditions(system, n, seed=seed)
    for q in Q:
        yield q, rng.uniform(-2, 2, len(q))


def test_prefix_pairs_equal_their_closed_forms():
    """mab, lqq, cab, cba of a pair (a, b) with a in the prefix, accumulated as phase D does (fma(x, y, acc) per component from 0.0, lqq from
    its angular part), against (I s_b)[x], 0, Z_b[x], 0.  numpy has no fma: every product here has an exact 0 or 1 as a factor, so
    x * y + acc rounds once, like the fma."""
    system, _ = build("puppet40")
    nd = sum(1 for c in system.configs if not c.kinematic)
    checked = 0
    for q, dq in _states(system, 200, 11):
        s, u, path_of, _, (M, C, D, H) = _world_state(system, q, dq)
        for a in range(3):
            Vm = np.zeros(6)
            for j in path_of[a][:-1]:
                Vm = Vm + u[j]
            w_a = _bracket(Vm, s[a])
            e = np.zeros(6); e[a] = 1.0
            assert np.array_equal(s[a], e) and np.array_equal(w_a, np.zeros(6))
            for b in range(a + 1, nd):
                if a not in path_of[b]:
                    continue
                Vb = np.zeros(6)
                for j in path_of[b][:-1]:
                    Vb = Vb + u[j]
                w_b = _bracket(Vb, s[b])
                Is, Iw = _apply(M[b], C[b], D[b], s[b]), _apply(M[b], C[b], D[b], w_b)
                h, sb = H[b], s[b]
                Z = Iw + np.concatenate([np.cross(sb[3:], h[:3]), np.cross(sb[:3], h[:3]) + np.cross(sb[3:], h[3:])])
                GG = np.cross(M[b] * sb[:3] + np.cross(sb[3:], C[b]), np.array([0.0, 0.0, -9.8]))
                mab, cab, cba = 0.0, 0.0, 0.0
                lqq = s[a][3] * GG[0] + s[a][4] * GG[1] + s[a][5] * GG[2]
                for r in range(6):
                    mab = s[a][r] * Is[r] + mab; lqq = w_a[r] * Z[r] + lqq; cab = s[a][r] * Z[r] + cab; cba = w_a[r] * Is[r] + cba
                assert np.array_equal([mab, lqq, cab, cba], [Is[a], 0.0, Z[a], 0.0]), (a, b)
                checked += 1
    assert checked == 200 * 60


def test_shared_record_equals_the_prefix_entries():
    """((0 + u_0) + u_1) + u_2 + the rest, against (0 + record) + the rest, record = (dq_x, dq_y, dq_z, 0, 0, 0): every list of the plan"""
    system, ints, pool, offs = _header("puppet40")
    nd = ints["nd"]
    was, now = _lists(pool, offs, "wev_lane", nd), _lists(pool, offs, "fb_lane", nd)
    for q, dq in _states(system, 200, 12):
        s, u, _, _, _ = _world_state(system, q, dq)
        rec = np.zeros((nd + 2, 6))
        rec[:nd] = u[:nd]
        for i in range(3):
            rec[nd + 1][ints["fb_axis_%d" % i]] = dq[ints["fb_cfg_%d" % i]]
        for l in range(64):
            A, B = np.zeros(6), np.zeros(6)
            for e in was[l]:
                A = A + rec[e]
            for e in now[l]:
                B = B + rec[e]
            assert np.array_equal(A, B), l
