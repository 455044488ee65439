"""Microstructure maps, recorded from the REFERENCE on the CPU (through oracle/ref_env.py's shim) ->
tests/golden/microstructure/*.npz.  Data only; needs the reference tree; a few minutes on one core.  Not for the GPU machine.

    python tools/gen_golden_microstructure.py

The reference can no longer construct MicroStructureProblem (it calls Problem.__init__() without cfg), so what is recorded is
what is still callable: MicroStructureProblem.get_stats on an instance made without __init__ and with render_path = False,
which calls helper.calc_tortuosity.

Per file (one map shape, maps of tests/microstructure_levels.py) and per map:
  grids        uint8 [n][H][W]
  stats_bits   uint64 [n][2]: get_stats(map) in its dict order (`stat_keys`), each value as the 64-bit pattern of its float64
  regions      int32 [n]: the number of regions, the mean's divisor
  region_rec   int16 [n][32][5], region_tort_bits uint64 [n][32]: for the first 32 regions in visit order start row, start
               column, far row, far column, d (all -1 past the last region) and the pattern of tort (0 past it).  From
               tests/microstructure_rules.py's copy of the loop, whose totals are checked against the reference's here.
  names        what made the map

The script refuses to write unless tests/microstructure_rules.py reproduces every recorded field, its numpy-order sum equals
np.mean bit for bit for every length 0 .. 2 100, and the sets hold each of CASES.  Files are written with fixed zip
timestamps, so a rerun is byte-identical.
"""
import io
import os
import sys
import time
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import microstructure_levels as ml  # noqa: E402
import microstructure_rules as R  # noqa: E402
import ref_env  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "microstructure")
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (8, 8), (16, 16), (33, 17), (3, 64), (64, 3), (64, 64)]
REC_CAP = 32
EXACT_COUNTS = (7, 8, 9, 127, 128, 129)
CASES = (["all solid", "all empty", "one empty cell", "64 x 64 checkerboard", "64 x 64 serpentine", "two regions of equal d",
          "cross: the greatest distance in several cells", "more than 256 regions of differing tort"]
         + [f"{k} regions of differing tort" for k in EXACT_COUNTS])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def maps_of(h, w, seed):
    """(name, map) for one shape"""
    rng = np.random.default_rng(seed)
    out = [("all-solid", ml.all_solid(h, w)), ("all-empty", ml.all_empty(h, w)), ("one-cell", ml.one_cell(h, w, h // 2, w // 2)),
           ("one-cell-last", ml.one_cell(h, w, h - 1, w - 1)), ("checker", ml.checkerboard(h, w)),
           ("checker-shifted", ml.checkerboard(h, w, first_empty=False)), ("serpentine", ml.serpentine(h, w))]
    if min(h, w) >= 5:
        out.append(("cross", ml.cross(h, w, 2)))
    if min(h, w) >= 2:
        out.append(("equal-pair", ml.equal_pair(h, w)))
    nblocks = (h // ml.BLOCK_H) * (w // ml.BLOCK_W)
    for k in EXACT_COUNTS:
        if k <= nblocks:
            out.append((f"l-shapes-{k}", ml.l_shapes(rng, h, w, k)))
    n_random = 8 if h * w >= 4096 else (16 if h * w > 64 else 24)
    for i in range(n_random):
        out.append((f"random-{i}", ml.random_map(rng, h, w)))
    for p in (0.1, 0.9):
        out.append((f"random-p{p}", ml.random_map(rng, h, w, p)))
    return out


class Recorder:
    def __init__(self):
        from control_pcgrl.envs import helper
        from control_pcgrl.envs.probs.microstructure.microstructure_prob import MicroStructureProblem
        self.helper = helper
        self.prob = MicroStructureProblem.__new__(MicroStructureProblem)  # __init__ raises TypeError in this checkout
        self.prob.render_path = False
        assert self.prob.get_tile_types() == R.TILES
        self.seconds, self.levels = 0.0, 0

    def level(self, m):
        str_map = [[R.TILES[t] for t in row] for row in m]
        t0 = time.perf_counter()
        stats = self.prob.get_stats(str_map)
        if m.shape == (64, 64):
            self.seconds += time.perf_counter() - t0
            self.levels += 1
        assert list(stats) == R.STAT_KEYS
        if not (m == R.EMPTY).any():
            assert stats["path-length"] == 0 and stats["tortuosity"] == 0 and isinstance(stats["tortuosity"], int)
        return [float(stats[k]) for k in R.STAT_KEYS]


def check_sum_order():
    rng = np.random.default_rng(2100)
    for n in range(0, 2101):
        v = rng.random(n) * rng.choice([1.0, 1e-3, 1e3], n)
        if n == 0:
            assert R.numpy_sum(v) == 0.0
            continue
        assert bits(R.numpy_mean(v)) == bits(np.mean(list(v))), n
        assert bits(R.numpy_sum(v)) == bits(np.add.reduce(v)), n


def cases_of(name, m, regs):
    got = set()
    h, w = m.shape
    empty = int((m == R.EMPTY).sum())
    if empty == 0:
        got.add("all solid")
    if empty == h * w:
        got.add("all empty")
    if empty == 1:
        got.add("one empty cell")
    if (h, w) == (64, 64) and name == "checker":
        assert len(regs) == 2048 and all(r[5] == 0.0 for r in regs)
        got.add("64 x 64 checkerboard")
    if (h, w) == (64, 64) and name == "serpentine":
        assert len(regs) == 1 and regs[0][4] == 32 * 64 + 31 - 1
        got.add("64 x 64 serpentine")
    if len(regs) == 2 and regs[0][4] == regs[1][4] > 0:
        got.add("two regions of equal d")
    if name == "cross":
        dist = R.flood(R.clean(m) == R.EMPTY, regs[0][0], regs[0][1])
        if int((dist == dist.max()).sum()) > 1:
            got.add("cross: the greatest distance in several cells")
    differing = len({r[5] for r in regs}) > 2
    if differing and len(regs) in EXACT_COUNTS:
        got.add(f"{len(regs)} regions of differing tort")
    if differing and len(regs) > 256:
        got.add("more than 256 regions of differing tort")
    return got


def write_npz(path, arrays):
    """np.savez_compressed with fixed timestamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    assert ref_env.available(), "the reference tree is needed"
    check_sum_order()
    print("numpy-order sum == np.mean bit for bit, lengths 0 .. 2100", flush=True)
    rec = Recorder()
    seen, files, total = {}, {}, 0
    for seed, (h, w) in enumerate(SHAPES):
        named = maps_of(h, w, 300 + seed)
        n = len(named)
        stats_bits = np.zeros((n, 2), np.uint64)
        counts = np.zeros(n, np.int32)
        region_rec = np.full((n, REC_CAP, R.REC_FIELDS), -1, np.int16)
        tort_bits = np.zeros((n, REC_CAP), np.uint64)
        for i, (name, m) in enumerate(named):
            ref = rec.level(m)
            regs = R.regions(m)
            mine, count, rrec, rtort = R.outputs(m, REC_CAP)
            assert bits(mine).tolist() == bits(ref).tolist(), ((h, w), name, mine, ref)
            assert count == len(regs)
            if regs:  # the instrumented loop against the reference's totals
                assert max(r[4] for r in regs) == ref[0] and bits(np.mean([r[5] for r in regs])) == bits(ref[1])
            stats_bits[i] = bits(ref)
            counts[i] = count
            region_rec[i] = np.asarray(rrec, np.int16)
            tort_bits[i] = bits(rtort)
            for c in cases_of(name, m, regs):
                seen.setdefault(c, []).append(f"{h}x{w}:{name}")
        files[f"ms_{h}x{w}"] = {
            "grids": np.stack([m for _, m in named]).astype(np.uint8), "stats_bits": stats_bits, "regions": counts,
            "region_rec": region_rec, "region_tort_bits": tort_bits, "names": np.asarray([k for k, _ in named]),
            "stat_keys": np.asarray(R.STAT_KEYS),
        }
        print(f"{h}x{w}: {n} maps, up to {counts.max()} regions", flush=True)
    missing = [c for c in CASES if not seen.get(c)]
    assert not missing, f"no map shows: {missing}"
    os.makedirs(OUT, exist_ok=True)
    for name, arrays in files.items():
        path = os.path.join(OUT, name + ".npz")
        write_npz(path, arrays)
        size = os.path.getsize(path)
        assert size <= 100 * 1024, (path, size)
        total += size
    for c in CASES:
        print(f"{c}: {len(seen[c])} maps, e.g. {seen[c][0]}")
    print(f"reference get_stats on the {rec.levels} maps of 64 x 64: {rec.seconds / rec.levels:.4f} s per map")
    print(total, "bytes in all")


if __name__ == "__main__":
    main()
