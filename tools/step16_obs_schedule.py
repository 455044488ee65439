#!/usr/bin/env python3
"""The chunk schedule of encode_obs16 (csrc/step16/pcgrl_k_step16.hip), restated in numpy: which lane stores which 16-byte
chunk of a binary 16x16 env's 32x32x3 observation in which phase, and from where.

The observation of one env is 192 chunks of 16 bytes (32 rows x 6); chunk k lies at byte 16 k.  The map fills observation
rows [16 - pos0, 32 - pos0), i.e. chunks [lo, lo + 96) with lo = 6 (16 - pos0); the other 96 chunks show nothing but "outside
the map" (byte j of a row is 1 iff j % 3 == 0).

Phase 1 (from registers): lane `row` owns chunks k = 16 it + row, it = 0..11, and stores those outside [lo, lo + 96); the
pattern of chunk k starts at phase k % 3 = (it + row) % 3 of the dword sequence SEQ.
Phase 2 (through LDS): lane `row` builds the 96 bytes of map row `row` (stride 112), and the group streams the 96 map-row
chunks: lane `row` takes t = d + 16 j, j = 0..5, with d = (row + 6 pos0) & 15; chunk t is read 16 (t + t // 6) bytes into the
env's LDS rows -- in the kernel as three addresses and six constant offsets -- and stored as chunk lo + t.
Run it for a self-check:  python tools/step16_obs_schedule.py"""
import numpy as np

C, LPE, CHUNK = 3, 16, 16
ROW_CHUNKS = 32 * C // CHUNK        # 6
N_CHUNKS = 32 * ROW_CHUNKS          # 192
STRIDE = ROW_CHUNKS * CHUNK + 16    # 112: LDS bytes between the rows of two lanes
SEQ = (0x01000001, 0x00010000, 0x00000100)            # dwords 0, 1, 2 of the out-of-bounds row, period 3
READ_OFFSETS = (0, 288, 592, 896, 1184, 1488)         # the constant part of the six LDS reads of a lane
READ_BASE = (0, 1, 2, 0, 1, 2)                        # ... and which of the lane's three addresses each read uses


def lo_chunk(pos0):
    return ROW_CHUNKS * (16 - pos0)


def oob_pattern(phase):
    """the 16 bytes of an out-of-bounds chunk whose first byte has index = phase (mod 3) in its row"""
    return np.array([(phase + j) % C == 0 for j in range(CHUNK)], np.uint8)


def lane_quads(row):
    """the three quads lane `row` keeps: quad t = dwords (x_t, x_t+1, x_t+2, x_t+3) of the sequence from row % 3 on"""
    x = [SEQ[(row + i) % 3] for i in range(3)]
    return [np.array([x[(t + i) % 3] for i in range(4)], "<u4").view(np.uint8) for t in range(3)]


def phase1(pos0, row):
    """[(chunk, pattern index)] of the border chunks lane `row` stores, in issue order"""
    lo, out = lo_chunk(pos0), []
    for it in range(N_CHUNKS // LPE):
        k = LPE * it + row
        if (k - lo) % (1 << 32) >= 96:  # the kernel's one unsigned compare
            out.append((k, (it + row) % 3))
    return out


def phase2(pos0, row):
    """[(chunk, byte offset into the env's LDS rows)] of the six map-row chunks lane `row` streams, in issue order"""
    lo = lo_chunk(pos0)
    d = (row + 6 * pos0) & 15
    m0 = (d >= 6) + (d >= 12)
    q0 = d - 6 * m0
    s0 = CHUNK * (d + m0)
    base = (s0, s0 + (16 if q0 >= 2 else 0), s0 + (16 if q0 >= 4 else 0))
    return [(lo + d + LPE * j, base[READ_BASE[j]] + READ_OFFSETS[j]) for j in range(6)]


def lds_rows(tiles, pos1, group=0):
    """the env's sixteen 112-byte LDS rows: the out-of-bounds pattern, then one byte pair per cell (env `group` of the
    wave starts its scatter at cell 4 * group: the order does not show in the bytes).  tiles: (16, 16) of 0 / 1"""
    lds = np.zeros((16, STRIDE), np.uint8)
    left = pos1 - 16
    for row in range(16):
        for q in range(ROW_CHUNKS):
            lds[row, CHUNK * q:CHUNK * (q + 1)] = oob_pattern((CHUNK * q) % C)
        for x in range(16):
            xx = (x + 4 * group) & 15
            o = (xx - left) * C
            lds[row, o] = 0
            lds[row, o + 1 + int(tiles[row, xx])] = 1
    return lds.reshape(-1)


def assemble(tiles, pos0, pos1, group=0, fill=0xAA):
    """the 3072 observation bytes the schedule writes (bytes no chunk covers keep `fill`), and how often each chunk is written"""
    obs = np.full(N_CHUNKS * CHUNK, fill, np.uint8)
    count = np.zeros(N_CHUNKS, np.int64)
    lds = lds_rows(tiles, pos1, group)
    for row in range(LPE):
        quads = lane_quads(row)
        for k, _ in phase1(pos0, row):
            obs[CHUNK * k:CHUNK * (k + 1)] = quads[(k // LPE) % 3]  # trip `it` stores quad it % 3
            count[k] += 1
        for k, off in phase2(pos0, row):
            obs[CHUNK * k:CHUNK * (k + 1)] = lds[off:off + CHUNK]
            count[k] += 1
    return obs.reshape(32, 32, C), count


def reference(tiles, pos0, pos1):
    """crop -> one-hot -> channel-last: np.pad(map + 1, 16) windowed at pos, then np.eye(3)[...]"""
    padded = np.pad(np.asarray(tiles, np.int64) + 1, 16)
    return np.eye(C, dtype=np.uint8)[padded[pos0:pos0 + 32, pos1:pos1 + 32]]


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    for pos0 in range(16):
        for pos1 in range(16):
            tiles = rng.integers(0, 2, (16, 16))
            obs, count = assemble(tiles, pos0, pos1, group=(pos0 + pos1) & 3)
            assert (count == 1).all() and np.array_equal(obs, reference(tiles, pos0, pos1)), (pos0, pos1)
    per_it = [sum(any((16 * it + row - lo_chunk(p0)) % (1 << 32) >= 96 for row in range(16)) for it in range(12)) for p0 in range(16)]
    print("phase-1 trips with a non-empty mask, by pos0:", per_it)
    print("ok: 256 positions, every chunk once, bytes equal crop -> one-hot -> channel-last")
