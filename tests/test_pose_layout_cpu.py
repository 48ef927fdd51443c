"""The plan cells behind the LDS record layout of the specialised rollout kernels' composites (program.hpp: kCmpStride, cmp_stride;
schedule.hpp), read back from the generated specialisation headers (no GPU needed): the composite records 18 doubles
apart inside the J area where the twist records and the per-config vectors still fit behind them and 16 apart otherwise, no LDS
added, and the cell tr_rows -- the rows of a run joint's position that some item of the plan copies from another joint's config.

The pose arrays keep their 12-double records (the half-record layout the same change measured is not in the tree: docs/LOG.md); what
the kernels need of them here is that both areas start on an even double."""
import hashlib
import re

import numpy as np
import pytest

from common import build

# program.hpp: kCmpStride where the twist records behind the composites still fit the J area with it, kCmpRecord otherwise.  The puppets
# have the room (puppet40: 18 * 9 + 12 * 24 = 450 of 528 doubles).  The ladders do not: 18 * 8 + 12 * 17 = 348 of 6 * 56 = 336 -- at the
# wide stride they would lose the world-frame evaluation (tests/test_model_branches_cpu.py pins it), so they keep 16.
CMP_STRIDE, CMP_RECORD = 18, 16
WORLD_FRAME = {"puppet40": CMP_STRIDE, "puppet_basic": CMP_STRIDE, "ladder_point": CMP_RECORD, "ladder_mixed": CMP_RECORD}


def _parse(name):
    from trep_amd import specialize
    system, _ = build(name)
    text = specialize.header(system)
    ints = {m.group(1): int(m.group(2)) for m in re.finditer(r"static constexpr int (\w+) = (-?\d+);", text)}
    ipool = np.array([int(x) for x in re.search(r"spec_ipool\[\d+\] = \{([^}]*)\}", text, re.S).group(1).replace("\n", "").split(",")], dtype=np.int64)
    ioff = {m.group(1): int(m.group(2)) for m in re.finditer(r"static constexpr const int \*(\w+) = spec_ipool \+ (\d+);", text)}
    return text, ints, (lambda table, n: ipool[ioff[table]:ioff[table] + n])


@pytest.mark.parametrize("name", sorted(WORLD_FRAME))
def test_composite_records_inside_the_J_area(name):
    _, c, _ = _parse(name)
    nd, ng, ni = c["nd"], c["n_cgroups"], c["n_items"]
    assert c["cmp_ok"] == 1 and c["wev_ok"] == 1 and 1 <= ng <= 16       # (18 g modulo 32 is distinct for sixteen groups)
    # the wide stride exactly where nd + 2 twist records and the per-config vectors fit behind it
    wide = CMP_STRIDE * ng + 12 * (nd + 2) <= 6 * ni and CMP_STRIDE * ng + 12 * (nd + 2) + 15 * nd <= 12 * ni
    stride = CMP_STRIDE if wide else CMP_RECORD
    assert stride == WORLD_FRAME[name]
    assert c["o_cmp"] == c["o_J"] and c["o_csw"] == c["o_cmp"] + stride * ng
    assert c["o_cmp"] % 2 == 0 and c["o_csw"] % 2 == 0
    records = nd + 2 if c["fb_on"] else nd + 1
    assert c["o_ccz"] == c["o_csw"] + 12 * records
    # the twist records inside the J area (the q2 poses sit in W while they are read), the per-config vectors inside J and W
    assert c["o_W"] == c["o_J"] + 6 * ni and c["o_ccz"] <= c["o_W"]
    assert c["o_ccz"] + 15 * nd <= c["o_J"] + 12 * ni
    # the 16-byte reads of the pose arrays (eval_world: a body lane's anchor pose, an end point's row)
    assert c["o_G"] % 2 == 0 and c["o_W"] % 2 == 0


def test_prefix_record_is_pinned_where_there_is_a_prefix():
    for name in ("puppet40", "puppet_basic"):
        _, c, _ = _parse(name)
        assert c["fb_on"] == 1 and c["o_ccz"] == c["o_csw"] + 12 * (c["nd"] + 2), name
    for name in ("ladder_point", "ladder_mixed"):
        _, c, _ = _parse(name)
        assert c["fb_on"] == 0 and c["o_ccz"] == c["o_csw"] + 12 * (c["nd"] + 1), name


def test_puppet_lds_slice_is_unchanged():
    _, c, _ = _parse("puppet40")
    assert 8 * c["lds_per_team"] == 20384                                # eight workgroups per CU
    assert CMP_STRIDE * c["n_cgroups"] + 27 * c["nd"] + 24 == 780 <= 12 * c["n_items"] == 1056


@pytest.mark.parametrize("name,rows", [("puppet40", 0b011), ("puppet_basic", 0b011), ("ladder_point", None), ("ladder_mixed", None), ("scissor4", 0)])
def test_tr_rows_is_the_or_of_the_copy_bits(name, rows):
    _, c, I = _parse(name)
    want = 0
    for w in I("tr_sj", c["n_sj"]):
        want |= (int(w) >> 24) & 7
    assert c["tr_rows"] == want
    if rows is not None:
        assert c["tr_rows"] == rows


def test_header_without_the_world_frame_evaluation_gains_one_cell_only():
    """scissor4 has neither the composite form nor the world-frame evaluation: apart from the appended cell its header is the one of the
    commit before the layouts (sha256 of the text without the pool of doubles, whose digits are the host's libm's)."""
    text, c, _ = _parse("scissor4")
    assert c["wev_ok"] == 0 and c["cmp_ok"] == 0 and c["o_cmp"] == 0 and c["o_csw"] == 0 and c["o_ccz"] == 0
    assert text.count("    static constexpr int tr_rows = 0;\n") == 1
    before = text.replace("    static constexpr int tr_rows = 0;\n", "")
    before = re.sub(r"__device__ const double spec_dpool\[\d+\] = \{[^}]*\};\n", "", before)
    assert hashlib.sha256(before.encode()).hexdigest() == "c39f69e3c29f81dd6069673a2ee987c7a0c2d7e31177d033b9e735db91f6fff5"
    # ... and the cell is the last integer of the list
    cells = re.findall(r"static constexpr int (\w+) = -?\d+;", text)
    assert cells[[i for i, n in enumerate(cells) if not re.search(r"_\d+$", n)][-1]] == "tr_rows"
