"""The translation runs of the rollout's dual pose sweep in the plan (program.hpp, tr_*), read back from the generated
specialisation header (no GPU needed), and the exactness of what the kernel does with them, in numpy:

* the run joints of the BASELINE systems with the contributor of every position component, and the second sweep plan (the chains
  without their run joints) next to the first, which keeps its contents (tests/test_newton_plan_cpu.py pins it);
* small trees on which the rule must stop: a folded rotation, a rotary joint above, two contributors on one component, a repeated axis;
* the local-transform and chain-step arithmetic of the run joints, replayed operation by operation, against the closed form the kernel
  stores instead: equal value for value (np.array_equal) for random configurations of both pose sets."""
import re

import numpy as np
import pytest

from common import build

TG_TX = 1      # include/trep_amd.h: TG_TX, TG_TY, TG_TZ = 1, 2, 3


def _parse(system):
    from trep_amd import specialize
    text = specialize.header(system)
    ints = {m.group(1): int(m.group(2)) for m in re.finditer(r"static constexpr int (\w+) = (-?\d+);", text)}
    ipool = np.array([int(x) for x in re.search(r"spec_ipool\[\d+\] = \{([^}]*)\}", text, re.S).group(1).replace("\n", "").split(",")], dtype=np.int64)
    dpool = np.array([float.fromhex(x.strip()) for x in re.search(r"spec_dpool\[\d+\] = \{([^}]*)\}", text, re.S).group(1).replace("\n", "").split(",")])
    ioff = {m.group(1): int(m.group(2)) for m in re.finditer(r"static constexpr const int \*(\w+) = spec_ipool \+ (\d+);", text)}
    doff = {m.group(1): int(m.group(2)) for m in re.finditer(r"static constexpr const double \*(\w+) = spec_dpool \+ (\d+);", text)}
    return ints, (lambda name, n: ipool[ioff[name]:ioff[name] + n]), (lambda name, n: dpool[doff[name]:doff[name] + n])


def _plan(system):
    """ints, and per run joint (joint, [contributor of x, y, z]): a config index, or ('const', value)"""
    c, I, D = _parse(system)
    n = c["tr_n"]
    joints = [int(j) for j in I("tr_joint", n)]
    src, cst = I("tr_src", 3 * n).reshape(n, 3), D("tr_const", 3 * n).reshape(n, 3)
    runs = [(joints[i], [int(src[i, r]) if src[i, r] >= 0 else ("const", float(cst[i, r])) for r in range(3)]) for i in range(n)]
    return c, runs, I, D


def _second_plan(c):
    return ([c["tr_np_%d" % i] for i in range(4)], [c["tr_len_%d" % i] for i in range(16)], [c["tr_inst_%d" % i] for i in range(80)])


def test_puppet_runs_and_second_plan():
    system, _ = build("puppet40")
    c, runs, I, _ = _plan(system)
    names = [x.name for x in system.configs]
    assert c["tr_n"] == 15 and c["tr_on"] == 1
    Z = ("const", 0.0)
    t = [names.index(n) for n in ("torso_tx", "torso_ty", "torso_tz")]
    assert runs[:3] == [(0, [t[0], Z, Z]), (1, [t[0], t[1], Z]), (2, [t[0], t[1], t[2]])]
    # the six string carriers: tx(kinematic) then ty(kinematic) below the fixed string plane tz(2) -- chain slots 1..6 of round 0
    assert [j for j, _ in runs[3:]] == list(range(6, 18))
    for s in range(6):
        (jx, px), (jy, py) = runs[3 + 2 * s], runs[4 + 2 * s]
        cx, cy = px[0], py[1]
        assert system.configs[cx].kinematic and system.configs[cy].kinematic and cx != cy
        assert px == [cx, Z, ("const", 2.0)] and py == [cx, cy, ("const", 2.0)]
    # second plan: round 0 = one pass of length 3 with the torso's two instances (first joint 3, parent joint 2); round 1 unchanged
    np_, ln, inst = _second_plan(c)
    assert np_ == [1, 2, 0, 0] and ln[:8] == [3, 0, 0, 0, 4, 4, 0, 0] and not any(ln[8:]) and c["tr_maxlen"] == 4
    assert inst[:5] == [512, 768, 0, 0, 0] and not any(inst[5:20])
    assert inst[20:28] == [c["sw_inst_%d" % i] for i in range(20, 28)] == [512, 768, 513, 769, 514, 770, 515, 771] and not any(inst[28:])
    assert sum(ln) == 11 and sum(c["sw_len_%d" % i] for i in range(16)) == 16           # step-passes per evaluation
    sched = I("tr_sched", 32 * c["n_rounds"]).reshape(c["n_rounds"], 16, 2)
    assert sched[0, 0].tolist() == [12 * 3 | (3 << 16), 12 * 2]
    assert all(sched[0, s].tolist() == [0, -1] for s in range(1, 16))                   # the string chains are gone
    first = I("ch_first", c["n_chains"]); length = I("ch_len", c["n_chains"]); parent = I("ch_parent", c["n_chains"]); off = I("round_off", 3)
    for s in range(16):
        k = off[1] + s
        assert sched[1, s].tolist() == ([12 * first[k] | (length[k] << 16), 12 * parent[k]] if k < off[2] else [0, -1])
    # the first plan and the lists keep their contents
    assert [c["sw_np_%d" % i] for i in range(4)] == [2, 2, 0, 0] and [c["sw_len_%d" % i] for i in range(8)] == [6, 2, 0, 0, 4, 4, 0, 0]
    assert c["sw_maxlen"] == 6 and c["n_sj"] == 54
    # LDS: the second schedule is staged behind the base region; eight workgroups per CU still fit (160 KiB / 8)
    assert c["o_sched2"] + 16 * c["n_rounds"] == c["lds_per_team"] and 8 * c["lds_per_team"] <= 20480


def test_puppet_basic_runs_and_second_plan():
    system, _ = build("puppet_basic")
    c, runs, I, _ = _plan(system)
    Z = ("const", 0.0)
    assert c["tr_n"] == 3 and c["tr_on"] == 1
    assert runs == [(0, [0, Z, Z]), (1, [0, 1, Z]), (2, [0, 1, 2])]
    np_, ln, inst = _second_plan(c)
    assert np_ == [1, 2, 0, 0] and ln[:8] == [3, 0, 0, 0, 4, 4, 0, 0] and sum(ln) == 11
    assert inst[:5] == [512, 768, 0, 0, 0] and inst[20:28] == [512, 768, 513, 769, 514, 770, 515, 771]
    assert I("tr_sched", 2).tolist() == [12 * 3 | (3 << 16), 12 * 2]


@pytest.mark.parametrize("name,want", [
    # the lift's slider and the cart: one translation along x off the world each -- a run of one joint, and no second plan (their
    # rollout kernels have no world-frame evaluation and keep the first); the pendulum has no prismatic joint at all
    ("scissor4", dict(tr_n=1, tr_on=0, tr_maxlen=0, o_sched2=0)),
    ("pend_on_cart", dict(tr_n=1, tr_on=0, tr_maxlen=0, o_sched2=0)),
    ("pendulum1", dict(tr_n=0, tr_on=0, tr_maxlen=0, o_sched2=0)),
])
def test_other_baseline_plans_are_pinned(name, want):
    system, _ = build(name)
    c, runs, _, _ = _plan(system)
    assert {k: c[k] for k in want} == want
    assert runs == ([(0, [0, ("const", 0.0), ("const", 0.0)])] if want["tr_n"] else [])
    assert not any(_second_plan(c)[0]) and not any(_second_plan(c)[1]) and not any(_second_plan(c)[2])


def _tree(frames):
    import trep_amd as T
    system = T.System()
    system.import_frames(frames(T))
    T.potentials.Gravity(system, (0, 0, -9.8))
    return system


def _runs(frames):
    system = _tree(frames)
    c, runs, _, _ = _plan(system)
    names = [x.name for x in system.configs]
    return [(j, [names[p] if not isinstance(p, tuple) else p[1] for p in src]) for j, src in runs], c


def test_synthetic_trees():
    body = lambda T: [T.rx('a', name='A'), [T.tz(-0.5, name='M', mass=1.0)]]
    full, c = _runs(lambda T: [T.tx('x'), [T.ty('y'), [T.tz('z'), body(T)]]])
    assert full == [(0, ['x', 0.0, 0.0]), (1, ['x', 'y', 0.0]), (2, ['x', 'y', 'z'])] and c["tr_on"] == 0       # (too small for the world-frame kernels)
    # any order of the axes, and constants on the components no config moves (the string carriers' shape)
    order, _ = _runs(lambda T: [T.tz('z'), [T.tx('x'), body(T)]])
    assert order == [(0, [0.0, 0.0, 'z']), (1, ['x', 0.0, 'z'])]
    plane, _ = _runs(lambda T: [T.tz(2.0), [T.tx('x'), [T.ty(0.0), [T.ty('y'), body(T)]]]])
    assert plane == [(0, ['x', 0.0, 2.0]), (1, ['x', 'y', 2.0])]
    # fall back: a fixed rotation folded in front of a prismatic joint ends the run there
    rotated, _ = _runs(lambda T: [T.tx('x'), [T.rz(0.3), [T.ty('y'), [T.tz('z'), body(T)]]]])
    assert rotated == [(0, ['x', 0.0, 0.0])]
    turned, _ = _runs(lambda T: [T.rz(0.3), [T.tx('x'), body(T)]])
    assert turned == []
    # a rotary joint above a prismatic one
    rotary, _ = _runs(lambda T: [T.rz('r'), [T.tx('x'), [T.ty('y'), body(T)]]])
    assert rotary == []
    # two contributors on x: a constant then a config, and a config then a constant
    twice, _ = _runs(lambda T: [T.tx(0.5), [T.tx('x'), body(T)]])
    assert twice == []
    after, _ = _runs(lambda T: [T.tx('x'), [T.tx(0.5), [T.ty('y'), body(T)]]])
    assert after == [(0, ['x', 0.0, 0.0])]
    # a fourth prismatic joint has to repeat an axis: the run stops at three, the joint and everything below it stay in the chains
    fourth, _ = _runs(lambda T: [T.tx('x'), [T.ty('y'), [T.tz('z'), [T.tx('x2'), body(T)]]]])
    assert fourth == [(0, ['x', 0.0, 0.0]), (1, ['x', 'y', 0.0]), (2, ['x', 'y', 'z'])]
    again, _ = _runs(lambda T: [T.tx('x'), [T.tx('x2'), [T.tz('z'), body(T)]]])
    assert again == [(0, ['x', 0.0, 0.0])]
    # kinematic and dynamic configs are both accepted (kinematic configs are numbered behind the dynamic ones; the joints are not)
    kin, _ = _runs(lambda T: [T.tx('x', kinematic=True), [T.ty('y'), body(T)]])
    assert kin == [(0, ['x', 0.0, 0.0]), (1, ['x', 'y', 0.0])]
    # a body anchored at a run joint changes nothing; a run may branch
    anchored, _ = _runs(lambda T: [T.tx('x', mass=1.0), [T.ty('y', name='Y', mass=2.0), [T.tz('z'), body(T)]]])
    assert anchored == full
    branch, _ = _runs(lambda T: [T.tx('x'), [T.ty('y1'), [T.rx('a1', name='A1', mass=1.0)], T.tz('z2'), [T.rx('a2', name='A2', mass=1.0)]]])
    assert sorted((src for _, src in branch), key=repr) == sorted([['x', 0.0, 0.0], ['x', 'y1', 0.0], ['x', 0.0, 'z2']], key=repr)


# ---- exactness -----------------------------------------------------------------------------------------------------------------------

def _values(rng, n):
    """configurations with zeros, both signs and magnitudes from 1e-8 to 1e8"""
    v = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-8, 8, n)
    v[rng.random(n) < 0.15] = 0.0
    return v


def _local(pre, axis, x):
    """pre * translation(axis, x) as the local-transform pass forms it: rotation = pre's, translation row l = fma(pre[l, axis], x, pre[l, 3])"""
    L = pre.copy()
    for l in range(3):
        L[l, 3] = pre[l, axis] * x + pre[l, 3]
    return L


def _chain_step(G, L):
    """chain_round_quads: G(r, c) <- fma(G(r, 2), L(2, c), fma(G(r, 1), L(1, c), fma(G(r, 0), L(0, c), last))), last = G(r, 3) for c = 3, else 0"""
    out = np.empty((3, 4))
    for r in range(3):
        for c in range(4):
            acc = G[r, 3] if c == 3 else 0.0
            for k in range(3):
                acc = G[r, k] * L[k, c] + acc
            out[r, c] = acc
    return out


def _swept_and_closed(system, q_of_set):
    """per run joint: its world pose through the chain (locals, then one chain step per joint from the world down) and the closed form"""
    c, runs, I, D = _plan(system)
    nj = c["n_joints"]
    parent, kind, cfg = I("j_parent", nj), I("j_kind", nj), I("j_cfg", nj)
    pre = D("j_pre", 12 * nj).reshape(nj, 3, 4)
    out = []
    for q in q_of_set:
        world = {-1: np.hstack([np.eye(3), np.zeros((3, 1))])}
        for j, src in runs:
            world[j] = _chain_step(world[int(parent[j])], _local(pre[j], int(kind[j]) - TG_TX, q[cfg[j]]))
            closed = np.hstack([np.eye(3), np.array([[q[p] if not isinstance(p, tuple) else p[1]] for p in src])])
            out.append((world[j], closed))
    return out


@pytest.mark.parametrize("name", ["puppet40", "puppet_basic"])
def test_chain_equals_closed_form_on_the_run_joints(name):
    """numpy has no fma: every product in the local transform and the chain steps of a run joint has an exact 0 or 1 as a factor, so it is
    exact and x * y + acc rounds once, like the fma.  Equality is on VALUES (np.array_equal: -0.0 == 0.0 -- a sum of zeros of both signs
    is +0.0 where the copy keeps the sign)."""
    system, _ = build(name)
    rng = np.random.default_rng(5)
    nq = len(system.configs)
    checked = 0
    for _ in range(200):
        q1, q2 = _values(rng, nq), _values(rng, nq)
        for swept, closed in _swept_and_closed(system, [0.5 * (q2 + q1), q2]):          # the two pose sets: qval(0, .) and qval(2, .)
            assert np.array_equal(swept, closed)
            checked += 1
    assert checked == 200 * 2 * {"puppet40": 15, "puppet_basic": 3}[name]


@pytest.mark.parametrize("name", ["puppet40", "puppet_basic"])
def test_kernel_tables_give_the_closed_form(name):
    """what the lane of a (pose set, run joint) item stores: rotation and fma(A, x, D) from tr_prm, a row with a tr_sj bit from the config"""
    system, _ = build(name)
    c, runs, I, D = _plan(system)
    nj, n_sj = c["n_joints"], c["n_sj"]
    sj, trw = I("sj_list", n_sj), I("tr_sj", n_sj)
    prm = D("tr_prm", 12 * nj).reshape(nj, 3, 4)
    assert np.array_equal(np.delete(prm, [j for j, _ in runs], axis=0), np.delete(D("j_prm", 12 * nj).reshape(nj, 3, 4), [j for j, _ in runs], axis=0))
    by_joint = dict(runs)
    rng = np.random.default_rng(6)
    q1, q2 = _values(rng, len(system.configs)), _values(rng, len(system.configs))
    seen = set()
    for w, t in zip(sj, trw):
        cf, kind, j, second = int(w) & 0xFFF, (int(w) >> 12) & 0xF, (int(w) >> 16) & 0xFFF, int(w) >> 28
        if j not in by_joint:
            assert t == 0
            continue
        q = q2 if second else 0.5 * (q2 + q1)
        a = kind - TG_TX
        g = np.zeros((3, 4))
        for l in range(3):
            A, B, C, Dl = prm[j, l]
            g[l, a], g[l, (a + 1) % 3], g[l, (a + 2) % 3] = A, B, C
            v = A * q[cf] + Dl
            g[l, 3] = q[(int(t) >> (8 * l)) & 0xFF] if (int(t) >> (24 + l)) & 1 else v
        closed = np.hstack([np.eye(3), np.array([[q[p] if not isinstance(p, tuple) else p[1]] for p in by_joint[j]])])
        assert np.array_equal(g, closed), (j, second)
        seen.add((j, second))
    # every run joint the rollout reads is stored: the torso's in both pose sets, the carriers' at q2
    assert len(seen) == {"puppet40": 6 + 12, "puppet_basic": 6}[name]


def test_two_contributors_are_not_a_copy():
    """teeth: on tx(0.5) -> tx('x') the chain forms fma(1, x, 0.5); neither contributor alone is that value"""
    system = _tree(lambda T: [T.tx(0.5), [T.tx('x'), [T.rx('a', name='A'), [T.tz(-0.5, name='M', mass=1.0)]]]])
    c, runs, I, D = _plan(system)
    assert runs == []
    pre = D("j_pre", 12).reshape(3, 4)
    assert pre[0, 3] == 0.5
    differs = 0
    for x in _values(np.random.default_rng(7), 100):
        G = _chain_step(np.hstack([np.eye(3), np.zeros((3, 1))]), _local(pre, 0, x))
        assert G[0, 3] == x + 0.5
        differs += int(G[0, 3] != x) + int(G[0, 3] != 0.5)
    assert differs >= 150
