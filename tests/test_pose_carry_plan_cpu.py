"""The plan of the carried poses (schedule.hpp, pose_carry; program.hpp, PoseCarry), read back from the generated
specialisation headers (no GPU needed): which systems may take the poses of a step's first evaluation behind the step edge from the q2
poses of the converged evaluation before it, the joints without a q2 twin the local-transform pass keeps on its idle lanes for that, and
the items a kinematic config moves.  The cells (pc_on, pc_n, pc_kin_0 / pc_kin_1, pc_item) exist only in the header of a system that
carries: every other header is the text it was, so the kernels compiled from it are the ones they were.  Nothing else of the plan
moves: n_sj, sj_list, tr_* and the LDS slice are pinned here next to the new cells."""
import hashlib
import re

import numpy as np
import pytest

from common import build

# name -> (carried joints by the name of their config, lanes they get) or None where the system does not carry
PLAN = {
    "puppet40": (["lknee_rx", "rknee_rx"], [54, 55]),            # the knees carry the shins; no string ends below them
    "puppet_basic": (["LKneeTheta", "RKneeTheta"], [42, 43]),
    "ladder_point": None,                                        # no translation run: the second sweep plan is off
    "ladder_mixed": None,
    "scissor4": None,                                            # a run of one joint, no world-frame evaluation
    "pend_on_cart": None,
}
# cells of the plans this change reads and may not move: n_sj, n_sj_rot, tr_n, tr_on, tr_maxlen, o_sched2, tr_rows, 8-byte words of LDS
PINNED = {
    "puppet40": dict(n_sj=54, n_sj_rot=36, tr_n=15, tr_on=1, tr_maxlen=4, tr_rows=0b011, lds_per_team=2548),
    "puppet_basic": dict(n_sj=42, tr_n=3, tr_on=1, tr_maxlen=4, tr_rows=0b011, lds_per_team=2440),
    "ladder_point": dict(n_sj=32, tr_n=0, tr_on=0, lds_per_team=1536),
    "ladder_mixed": dict(n_sj=32, tr_n=0, tr_on=0, lds_per_team=1552),
    "scissor4": dict(n_sj=18, tr_n=1, tr_on=0, lds_per_team=1024),
    "pend_on_cart": dict(n_sj=2, tr_n=1, tr_on=0, lds_per_team=154),
}
# the contents of sj_list as the parent commit's headers have them: sha256 of the comma-joined words, first 16 hex digits
SJ_LIST = {
    "puppet40": "647dcaa9141589c9",
    "puppet_basic": "87c1300515f55187",
    "ladder_point": "97192aa50ad226b4",
    "ladder_mixed": "97192aa50ad226b4",
    "scissor4": "2ed2b56308ec36dc",
    "pend_on_cart": "894d4058cf4ecc10",
}
TG_TX, TG_RX = 1, 4


def _parse(system):
    from trep_amd import specialize
    text = specialize.header(system)
    ints = {m.group(1): int(m.group(2)) for m in re.finditer(r"static constexpr int (\w+) = (-?\d+);", text)}
    ipool = np.array([int(x) for x in re.search(r"spec_ipool\[\d+\] = \{([^}]*)\}", text, re.S).group(1).replace("\n", "").split(",")], dtype=np.int64)
    ioff = {m.group(1): int(m.group(2)) for m in re.finditer(r"static constexpr const int \*(\w+) = spec_ipool \+ (\d+);", text)}
    return text, ints, (lambda table, n: [int(x) for x in ipool[ioff[table]:ioff[table] + n]])


def _expected(c, I):
    """The plan from the tables alone: (joints with a midpoint item and no q2 item, lanes of the items a kinematic config moves)"""
    nj, nd = c["n_joints"], c["nd"]
    sj, parent, cfg = I("sj_list", c["n_sj"]), I("j_parent", nj), I("j_cfg", nj)
    sets = {}
    for w in sj:
        sets.setdefault((w >> 16) & 0xFFF, set()).add(w >> 28)
    lonely = sorted(j for j, s in sets.items() if s == {0})

    def moved(j):
        while j >= 0:
            if cfg[j] >= nd:
                return True
            j = parent[j]
        return False
    return lonely, [n for n, w in enumerate(sj) if moved((w >> 16) & 0xFFF)], moved


@pytest.mark.parametrize("name", sorted(PLAN))
def test_carry_cells_and_list(name):
    system, _ = build(name)
    text, c, I = _parse(system)
    for cell, want in PINNED[name].items():
        assert c[cell] == want, (name, cell, c[cell])
    assert hashlib.sha256(",".join(str(w) for w in I("sj_list", c["n_sj"])).encode()).hexdigest()[:16] == SJ_LIST[name], name
    if PLAN[name] is None:
        assert "pc_" not in text, name                       # not a cell, not an array, not an accessor
        return
    configs, lanes = PLAN[name]
    assert c["pc_on"] == 1 and c["pc_n"] == len(configs)
    lonely, kin_lanes, moved = _expected(c, I)
    items = [c["pc_item_%d" % i] for i in range(8)]
    assert items[c["pc_n"]:] == [0] * (8 - c["pc_n"])
    kinds, cfgs = I("j_kind", c["n_joints"]), I("j_cfg", c["n_joints"])
    assert [(w >> 16) & 0xFFF for w in items[:c["pc_n"]]] == lonely
    for w in items[:c["pc_n"]]:
        j = (w >> 16) & 0xFFF
        assert w >> 28 == 1 and (w & 0xFFF) == cfgs[j] and (w >> 12) & 0xF == kinds[j] and not moved(j)      # sj_list's layout, pose set 1
    assert [system.configs[w & 0xFFF].name for w in items[:c["pc_n"]]] == configs
    assert [c["n_sj"] + i for i in range(c["pc_n"])] == lanes and lanes[-1] < 64
    mask = (c["pc_kin_0"] & 0xFFFFFFFF) | ((c["pc_kin_1"] & 0xFFFFFFFF) << 32)
    assert [n for n in range(64) if (mask >> n) & 1] == kin_lanes
    # every moved item is a prismatic joint of a translation run
    run = set(I("tr_joint", c["tr_n"]))
    for n in kin_lanes:
        w = I("sj_list", c["n_sj"])[n]
        assert (w >> 16) & 0xFFF in run and TG_TX <= (w >> 12) & 0xF < TG_RX


def test_puppet_moved_items_are_the_twelve_string_joints():
    system, _ = build("puppet40")
    _, c, I = _parse(system)
    mask = (c["pc_kin_0"] & 0xFFFFFFFF) | ((c["pc_kin_1"] & 0xFFFFFFFF) << 32)
    lanes = [n for n in range(64) if (mask >> n) & 1]
    sj = I("sj_list", c["n_sj"])
    assert len(lanes) == 12 and all(sj[n] >> 28 == 1 and (sj[n] & 0xFFF) >= c["nd"] for n in lanes)      # q2 poses only: no body hangs from a string
    _, c2, _ = _parse(build("puppet_basic")[0])
    assert c2["pc_kin_0"] == 0 and c2["pc_kin_1"] == 0       # its strings hang from fixed frames: nothing moves but q2


def test_carried_joint_is_swept_by_the_second_plan_in_pose_set_1():
    """The chain step that leaves a carried joint's q2 world pose in G2 runs already: its chain has an instance in pose set 1 in the
    rollout's second plan and reaches the joint; no pass or round is added (tr_np / tr_len are the parent's: test_translation_runs_plan_cpu)."""
    for name in ("puppet40", "puppet_basic"):
        _, c, I = _parse(build(name)[0])
        sched = I("tr_sched", 32 * c["n_rounds"])
        for i in range(c["pc_n"]):
            j = (c["pc_item_%d" % i] >> 16) & 0xFFF
            hits = []
            for r in range(c["n_rounds"]):
                for slot in range(16):
                    w = sched[2 * (16 * r + slot)]
                    first, length = (w & 0xFFFF) // 12, w >> 16
                    if length and first <= j < first + length:
                        hits.append((r, slot))
            assert len(hits) == 1, (name, j, hits)
            r, slot = hits[0]
            assert (slot | (1 << 8) | (1 << 9)) in [c["tr_inst_%d" % k] for k in range(20 * r, 20 * r + 20)], (name, j)


def test_off_when_a_chain_joint_hangs_below_a_kinematic_config():
    """A rotary joint below a string carrier, with a constraint end point behind it: its q2 pose moves with the carrier's targets and
    only a chain can form it, so the q2 poses of the step before are not this step's and the system does not carry."""
    import trep_amd
    from trep_amd import systems
    system = systems.puppet()
    info = sorted(system.string_constraints.values(), key=lambda i: i["name"])[0]
    system.get_frame(info["control_hook"]).import_frames([trep_amd.rz("spin", kinematic=True), [trep_amd.tz(-0.25, name="spun_hook")]])
    trep_amd.constraints.Distance(system, info["hook"], "spun_hook", 3.0, name="spun_string")
    text, c, I = _parse(system)
    assert c["tr_on"] == 1 and c["tr_n"] == 15 and "pc_" not in text
    # (the second sweep plan itself is as it was: the new joint is no run joint, and it is listed in pose set 1)
    nj = c["n_joints"]
    spin = [j for j in range(nj) if I("j_cfg", nj)[j] == [x.name for x in system.configs].index("spin")]
    assert len(spin) == 1 and spin[0] not in I("tr_joint", c["tr_n"])
    assert any((w >> 16) & 0xFFF == spin[0] and w >> 28 == 1 for w in I("sj_list", c["n_sj"]))
