"""tools/step16_obs_schedule.py (the chunk schedule of step16_kernel's observation encoder, in numpy): both phases together
write each of the 192 chunks of an env exactly once, phase 2 is six map-row chunks per lane, the phase-1 pattern is chunk
k's, and the bytes are crop -> one-hot -> channel-last for every position.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import step16_obs_schedule as sched  # noqa: E402


@pytest.mark.parametrize("pos0", range(16))
def test_every_chunk_once_and_phase2_is_six_map_row_chunks_per_lane(pos0):
    lo = 6 * (16 - pos0)
    seen = np.zeros(192, np.int64)
    for row in range(16):
        p1, p2 = sched.phase1(pos0, row), sched.phase2(pos0, row)
        for k, pattern in p1:
            assert k % 16 == row and not lo <= k < lo + 96
            assert pattern == k % 3
            seen[k] += 1
        assert len(p2) == 6
        for j, (k, off) in enumerate(p2):
            assert k % 16 == row and lo <= k < lo + 96, "a map-row chunk of this lane"
            t = k - lo
            assert off == 112 * (t // 6) + 16 * (t % 6), "chunk t % 6 of map row t // 6"
            assert off + 16 <= 16 * 112
            seen[k] += 1
        assert [k for k, _ in p2] == sorted(k for k, _ in p2)
        assert len(p1) + len(p2) == 12
    assert (seen == 1).all()


@pytest.mark.parametrize("row", range(16))
def test_phase1_quads_are_the_out_of_bounds_chunk_of_their_phase(row):
    quads = sched.lane_quads(row)
    for it in range(12):
        k = 16 * it + row
        assert np.array_equal(quads[it % 3], sched.oob_pattern((16 * k) % 3))
        assert np.array_equal(quads[it % 3], sched.oob_pattern(k % 3))


def test_bytes_are_crop_onehot_channel_last_for_every_position():
    rng = np.random.default_rng(16)
    for pos0 in range(16):
        for pos1 in range(16):
            tiles = rng.integers(0, 2, (16, 16))
            for group in (0, (pos0 + pos1) % 3 + 1):
                obs, count = sched.assemble(tiles, pos0, pos1, group=group)
                assert (count == 1).all()
                want = np.eye(3, dtype=np.uint8)[np.pad(tiles + 1, 16)[pos0:pos0 + 32, pos1:pos1 + 32]]
                assert np.array_equal(obs, want), (pos0, pos1, group)


def test_uniform_maps_and_the_reference_helper():
    for fill in (0, 1):
        tiles = np.full((16, 16), fill)
        for pos in ((0, 0), (15, 15), (0, 15), (15, 0), (7, 8)):
            obs, _ = sched.assemble(tiles, *pos)
            assert np.array_equal(obs, sched.reference(tiles, *pos))
            assert obs[..., 0].sum() == 32 * 32 - 256 and obs[..., 1 + fill].sum() == 256
