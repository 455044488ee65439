"""tools/step16_obs_regs.py (encode_obs16_regs of step16_kernel, in numpy): six unconditional border stores per lane that are
each border chunk once and no map chunk, with the pattern quad of the chunk's phase; the map part of a row as twelve dwords
from the tile bits, byte-aligned into thirteen dword writes that stay inside the row; and the assembled bytes against the
padded-window reference for every position.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import step16_obs_regs as regs  # noqa: E402


def _reference(tiles, pos0, pos1):
    return np.eye(3, dtype=np.uint8)[np.pad(np.asarray(tiles) + 1, 16)[pos0:pos0 + 32, pos1:pos1 + 32]]


@pytest.mark.parametrize("pos0", range(16))
def test_six_border_chunks_per_lane_cover_the_border_once(pos0):
    lo = 6 * (16 - pos0)
    b0, r0 = regs.border_split(pos0)
    seen = np.zeros(192, np.int64)
    for row in range(16):
        ks = regs.border_chunks(pos0, row)
        assert len(ks) == 6
        d = (row - lo) & 15
        assert sorted(ks) == sorted((lo + 96 + d + 16 * j) % 192 for j in range(6)), "the lane's six border chunks k = row (mod 16)"
        quads = regs.lane_quads(pos0, row)
        for j, k in enumerate(ks):
            assert k % 16 == row
            assert not lo <= k < lo + 96, "no map chunk"
            assert k % 3 == (b0 + row + j) % 3, "the chunk's pattern phase"
            assert np.array_equal(quads[j % 3], regs.oob_pattern(k % 3)), "store j takes quad j % 3"
            if j >= 1:
                assert k // 16 == (b0 + j) % 12, "stores 1..5: one 256-byte-aligned block for all sixteen lanes"
            else:
                assert k // 16 == (b0 if row >= r0 else b0 + 6) % 12, "store 0: the lane's chunk of a boundary block"
            seen[k] += 1
    border = np.ones(192, np.int64)
    border[lo:lo + 96] = 0
    assert np.array_equal(seen, border), "each border chunk exactly once"


def test_the_twelve_dwords_of_a_row_in_both_forms_and_as_bytes():
    rng = np.random.default_rng(3)
    rows = [0, 0xFFFF, 0x5555, 0xAAAA, 0x0001, 0x8000] + [int(x) for x in rng.integers(0, 1 << 16, 200)]
    for bits in rows:
        m = regs.cell_dwords(bits)
        assert m == regs.cell_dwords_arith(bits)
        want = np.zeros(48, np.uint8)
        for x in range(16):
            want[3 * x + 1 + ((bits >> x) & 1)] = 1
        assert np.array_equal(np.array(m, "<u4").view(np.uint8), want), hex(bits)


@pytest.mark.parametrize("pos1", range(16))
def test_thirteen_aligned_dwords_stay_inside_the_row(pos1):
    s = 48 - 3 * pos1
    assert s % 4 == pos1 % 4 and s % 3 == 0
    for bits in (0, 0xFFFF, 0x5555, 0xA5C3):
        dw0, dws = regs.row_dwords(bits, pos1)
        assert len(dws) == 13 and dw0 == (s - 1) // 4 and 0 <= 4 * dw0 and 4 * (dw0 + 13) <= 96
        row = np.concatenate([regs.oob_pattern((16 * q) % 3) for q in range(6)])
        row[4 * dw0:4 * dw0 + 52] = np.array(dws, "<u4").view(np.uint8)
        want = np.array([j % 3 == 0 for j in range(96)], np.uint8)
        for x in range(16):
            want[s + 3 * x:s + 3 * x + 3] = (0, 1 - ((bits >> x) & 1), (bits >> x) & 1)
        assert np.array_equal(row, want), (pos1, hex(bits))
        if pos1 % 4 == 0:  # the spare dword is the border dword in front of the map
            assert dws[0] == regs.FRONT and 4 * dw0 == s - 4


def test_bytes_are_crop_onehot_channel_last_for_every_position():
    rng = np.random.default_rng(41)
    for pos0 in range(16):
        for pos1 in range(16):
            tiles = rng.integers(0, 2, (16, 16))
            obs, count = regs.assemble(tiles, pos0, pos1)
            assert (count == 1).all()
            assert np.array_equal(obs, _reference(tiles, pos0, pos1)), (pos0, pos1)


@pytest.mark.parametrize("name", ["empty", "solid", "columns", "columns_shifted"])
def test_uniform_and_striped_maps_at_every_position(name):
    tiles = {"empty": np.zeros((16, 16), np.int64), "solid": np.ones((16, 16), np.int64),
             "columns": np.tile(np.arange(16) % 2, (16, 1)), "columns_shifted": np.tile((np.arange(16) + 1) % 2, (16, 1))}[name]
    for pos0 in range(16):
        for pos1 in range(16):
            obs, count = regs.assemble(tiles, pos0, pos1)
            assert (count == 1).all() and np.array_equal(obs, _reference(tiles, pos0, pos1)), (pos0, pos1)


def test_dword_write_conflict_degree_is_what_the_comment_says():
    assert regs.write_bank_conflicts([5, 5, 5, 5]) == 4  # narrow: four envs at one pos1
    assert max(regs.write_bank_conflicts([a, b, c, d]) for a in (0, 7) for b in (1, 8) for c in (2, 13) for d in (3, 15)) <= 4
