#!/usr/bin/env python3
"""encode_obs16_regs (csrc/step16/pcgrl_k_step16.hip, PCGRL_STEP16_OBS_REGS=1), restated in numpy: which lane stores which
16-byte chunk of a binary 16x16 env's 32x32x3 observation from which registers, and how a lane makes the 96 bytes of its
map row without a byte write.  (tools/step16_obs_schedule.py describes the PCGRL_STEP16_OBS_REGS=0 build.)

Piece A.  The 96 border chunks of an env are the cyclic range [T, T + 96) mod 192, T = lo + 96 = 192 - 6 pos0.  Lane `row` owns
the chunks k = row (mod 16): chunk 16 B + row of the 256-byte block B.  With B0 = T >> 4 and r0 = T & 15 its six border chunks
are those of blocks B0 + 1 .. B0 + 5 (mod 12) and one boundary chunk: block B0 when row >= r0, block B0 + 6 otherwise.  Store 0
is the boundary chunk, store j >= 1 block B0 + j for all sixteen lanes (256 aligned bytes).  In the kernel the lane holds two
byte offsets 3072 apart (`far`: block B0 with a bias of 3072 that the instruction's offset field 256 j - 3072 takes back,
`near`: twelve blocks lower) and store j selects `near` exactly when B0 + j >= 12.  Chunk 16 B + row shows pattern phase
(B + row) % 3; the lane keeps three quads rotated by (B0 + row) % 3, made with three byte alignments of the pattern's dwords,
and store j takes quad j % 3.

Piece B.  Four cells of a map row are twelve bytes [0, !c, c] x 4 = three dwords, made from the four tile bits by one 24-bit
multiply (bit i to bit 8 i), a mask, its complement and three byte permutes.  The row's 48 map bytes start at byte
s = 48 - 3 pos1 of the 96-byte row; the dword in front of them is 0x00000100 and the one behind them 0x01000001 (s is a
multiple of 3).  Thirteen byte alignments over [0x00000100, m0..m11, 0x01000001] with shift (4 - pos1 % 4) & 3 give the
aligned dwords from dword (s - 1) >> 2 of the row on; they are written over the prefilled out-of-bounds row.  Phase 2 then
reads chunks from LDS as before (step16_obs_schedule.phase2).
Run it for a self-check:  python tools/step16_obs_regs.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from step16_obs_schedule import C, CHUNK, LPE, N_CHUNKS, ROW_CHUNKS, STRIDE, lo_chunk, oob_pattern, phase2, reference  # noqa: E402

ENV_BYTES = N_CHUNKS * CHUNK                 # 3072
SPREAD = 0x204081                            # n * SPREAD has bit i of n (i = 0..3) at bit 8 i: the shifted copies do not overlap
SEL = (0x0C00040C, 0x060C0105, 0x03070C02)   # v_perm_b32 selectors of the three dwords of four cells
FRONT, BEHIND = 0x00000100, 0x01000001       # the border dword in front of the map's 48 bytes and the one behind them
M32 = 0xFFFFFFFF


def alignbyte(hi, lo, shift):
    """v_alignbyte_b32: ({hi, lo} >> 8 * (shift & 3)) & 0xffffffff"""
    return (((hi << 32) | lo) >> (8 * (shift & 3))) & M32


def perm(s0, s1, sel):
    """v_perm_b32: byte i of the result is byte sel_i of {s0, s1} (0-3: s1, 4-7: s0) or 0x00 for selector 0x0c"""
    both = (s0 << 32) | s1
    out = 0
    for i in range(4):
        k = (sel >> (8 * i)) & 0xFF
        assert k < 8 or k == 0x0C, "only the selectors the kernel uses"
        out |= (0 if k == 0x0C else (both >> (8 * k)) & 0xFF) << (8 * i)
    return out


# ---- piece A
def border_split(pos0):
    """(B0, r0): the block and the row at which the border range starts"""
    t = 192 - 6 * pos0
    assert t == lo_chunk(pos0) + 96
    return t >> 4, t & 15


def border_chunks(pos0, row):
    """[k_0..k_5]: the border chunks lane `row` stores, in issue order -- from the kernel's offsets: select, then the field"""
    b0, r0 = border_split(pos0)
    near = 256 * b0 + CHUNK * row            # (without the group's 3072 (lane >> 4), which rides along in both)
    far = near + ENV_BYTES
    first = near + 6 * 256 if row < r0 else (near if b0 >= 12 else far)
    out = []
    for j in range(6):
        off = (first if j == 0 else near if b0 >= 12 - j else far) + 256 * j - ENV_BYTES
        assert 0 <= off < ENV_BYTES and off % CHUNK == 0, (pos0, row, j, off)
        out.append(off // CHUNK)
    return out


def lane_quads(pos0, row):
    """the three quads of lane `row` as 16 bytes each: quad t = dwords (x_t, x_t+1, x_t+2, x_t) with indices mod 3"""
    x = border_split(pos0)[0] + row
    ph = x - 3 * ((11 * x) >> 5)
    assert x < 32 and ph == x % 3
    x = (alignbyte(0x00010000, 0x01000001, ph), alignbyte(0x00010000, 0x01000001, ph + 1), alignbyte(0x01000001, 0x00000100, ph))
    return [np.array([x[(t + i) % 3] for i in range(4)], "<u4").view(np.uint8) for t in range(3)]


# ---- piece B
def cell_dwords(bits):
    """m0..m11 of a map row given as its 16 tile bits (bit x = cell x is solid)"""
    m = []
    for q in range(4):
        n = (bits >> (4 * q)) & 15
        spread = (n * SPREAD) & M32          # (v_mul_u32_u24: both factors below 2^24, the product below 2^32)
        solid = spread & 0x01010101
        empty = solid ^ 0x01010101
        m += [perm(empty, solid, s) for s in SEL]
    return m


def cell_dwords_arith(bits):
    """the same twelve dwords in the issue's arithmetic form: 0x100 + c0 0xFF00, 0x01000001 + c1 0xFF - c2 0x01000000,
    0x10000 + c2 + c3 0xFF0000"""
    m = []
    for q in range(4):
        c0, c1, c2, c3 = ((bits >> (4 * q + i)) & 1 for i in range(4))
        m += [0x100 + c0 * 0xFF00, 0x01000001 + c1 * 0xFF - c2 * 0x01000000, 0x10000 + c2 + c3 * 0xFF0000]
    return m


def row_dwords(bits, pos1):
    """(first dword index in the row, the thirteen aligned dwords) of one lane"""
    seq = [FRONT] + cell_dwords(bits) + [BEHIND]
    sh = (-pos1) & 3
    assert sh == (4 - pos1 % 4) & 3
    dw0 = (47 - 3 * pos1) >> 2
    assert dw0 == (48 - 3 * pos1 - 1) // 4 and 0 <= dw0 and dw0 + 13 <= ROW_CHUNKS * CHUNK // 4, "inside the row, off its 16-byte pad"
    return dw0, [alignbyte(seq[i + 1], seq[i], sh) for i in range(13)]


def lds_rows(tiles, pos1):
    """the env's sixteen 112-byte LDS rows: the six prefilled chunks, then the thirteen dwords; the pad keeps 0xEE"""
    lds = np.full((16, STRIDE), 0xEE, np.uint8)
    for row in range(16):
        for q in range(ROW_CHUNKS):
            lds[row, CHUNK * q:CHUNK * (q + 1)] = oob_pattern((CHUNK * q) % C)
        bits = sum(int(tiles[row, x]) << x for x in range(16))
        dw0, dws = row_dwords(bits, pos1)
        lds[row, 4 * dw0:4 * dw0 + 52] = np.array(dws, "<u4").view(np.uint8)
    assert (lds[:, ROW_CHUNKS * CHUNK:] == 0xEE).all(), "the pad between two rows is never written"
    return lds.reshape(-1)


def write_bank_conflicts(pos1_of_env):
    """the worst conflict degree of one dword write of a wave (bank = dword address % 32, inside a 32-lane half), for
    the four envs' pos1"""
    worst = 0
    for half in range(2):
        banks = {}
        for lane in range(32 * half, 32 * half + 32):
            a = lane * (STRIDE // 4) + ((47 - 3 * pos1_of_env[lane >> 4]) >> 2)
            banks.setdefault(a % 32, set()).add(a)
        worst = max(worst, max(len(v) for v in banks.values()))
    return worst


def assemble(tiles, pos0, pos1, fill=0xAA):
    """the 3072 observation bytes both pieces write (bytes no chunk covers keep `fill`), and how often each chunk is written"""
    obs = np.full(ENV_BYTES, fill, np.uint8)
    count = np.zeros(N_CHUNKS, np.int64)
    lds = lds_rows(tiles, pos1)
    for row in range(LPE):
        quads = lane_quads(pos0, row)
        for j, k in enumerate(border_chunks(pos0, row)):
            obs[CHUNK * k:CHUNK * (k + 1)] = quads[j % 3]
            count[k] += 1
        for k, off in phase2(pos0, row):
            obs[CHUNK * k:CHUNK * (k + 1)] = lds[off:off + CHUNK]
            count[k] += 1
    return obs.reshape(32, 32, C), count


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    for bits in range(1 << 16):
        assert cell_dwords(bits) == cell_dwords_arith(bits), bits
    for pos0 in range(16):
        for pos1 in range(16):
            tiles = rng.integers(0, 2, (16, 16))
            obs, count = assemble(tiles, pos0, pos1)
            assert (count == 1).all() and np.array_equal(obs, reference(tiles, pos0, pos1)), (pos0, pos1)
    print("dword-write conflict degree, four envs at one pos1:", write_bank_conflicts([0, 0, 0, 0]),
          "| at pos1 = 0, 1, 2, 3:", write_bank_conflicts([0, 1, 2, 3]))
    print("ok: 65536 rows as perm == arithmetic dwords; 256 positions, every chunk once, bytes equal crop -> one-hot -> channel-last")
