"""The launch-geometry arithmetic of the kernels (mvi_core.hpp), through the host build of the kernel source: the workgroup order
of the rollout grid (tg_xcd_block) and the subset remapping of the range launches (tg_remap_trajectory)."""
import numpy as np
import pytest

from common import LDS_SLICES, RANGE_CASES, TEAM_CELLS, build
from emu_harness import lds_slices, remap_trajectory, xcd_block


def test_xcd_block_is_a_bijection():
    """Every workgroup of a G-workgroup rollout grid works on its own block, and every block is worked on (G = 1 .. 4096)."""
    for G in range(1, 4097):
        seen = np.zeros(G, dtype=np.int32)
        for b in range(G):
            v = xcd_block(b, G)
            assert 0 <= v < G, (b, G, v)
            seen[v] += 1
        assert (seen == 1).all(), (G, np.flatnonzero(seen != 1)[:8])


def test_xcd_block_keeps_neighbours_on_one_xcd():
    """Blocks 8i + x go to XCD x, which takes the x-th contiguous share of the blocks (the layout the comment describes)."""
    for G in (8, 64, 100, 257, 1000, 4096):
        q, r = divmod(G, 8)
        for b in range(G):
            x = b & 7
            lo = x * q + min(x, r)
            assert lo <= xcd_block(b, G) < lo + q + (1 if x < r else 0), (b, G)


def test_remap_identity_without_a_range():
    assert remap_trajectory(37) == list(range(37))


@pytest.mark.parametrize("seeds,horizon,k0,k1", RANGE_CASES)
@pytest.mark.parametrize("team", [1, 4, 16, 64])
def test_remap_trajectory_of_a_step_range(seeds, horizon, k0, k1, team):
    """tg_batch_deriv2_contract_device_range's remapping: the first seeds * (k1 - k0) launch slots are the trajectories
    s * horizon + k, k0 <= k < k1, in that order and each once; the slots of the last workgroup past them are idle (A.batch)."""
    batch, n = seeds * horizon, k1 - k0
    count = seeds * n
    per_block = 64 // team
    slots = -(-count // per_block) * per_block          # every team of the launched workgroups
    got = remap_trajectory(batch, n, horizon, k0, count, slots=slots)
    want = [s * horizon + k for s in range(seeds) for k in range(k0, k1)]
    assert got[:count] == want
    assert len(set(got[:count])) == count and all(0 <= t < batch for t in got[:count])
    assert got[count:] == [batch] * (slots - count)


@pytest.mark.parametrize("name", sorted(TEAM_CELLS))
def test_team_cell_refusals_follow_the_lds_budget(name):
    """The refusals the GPU team-size tests expect are exactly the slices whose block exceeds 160 KiB at that team."""
    _, d = build(name)
    sl = lds_slices(d)
    assert set(sl) == set(LDS_SLICES)
    for team, refused in TEAM_CELLS[name].items():
        over = set(k for k, v in sl.items() if (64 // team) * v * 8 > 160 * 1024)
        assert over == refused, (name, team, sl)
