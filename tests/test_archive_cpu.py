"""The quality-diversity grid archive, the parts that need no GPU: the header against the symbol table, the argument checks of
the C ABI (include/pcgrl_amd_archive.h: made before any HIP call, so they answer without a device), archive_for's bounds, the
placement rule on hand-computed cases, the batch rule against one-at-a-time insertion, and the numpy twins of ask()."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import archive_rules as R
from control_pcgrl_amd import _lib, archive
from control_pcgrl_amd import (ddave_spec, loderunner_spec, mdungeon_spec, microstructure_spec, problem_spec, smb_spec)

SYMBOLS = {"pcgrl_archive_create", "pcgrl_archive_destroy", "pcgrl_archive_add", "pcgrl_archive_cells", "pcgrl_archive_stats",
           "pcgrl_archive_elites", "pcgrl_archive_ask", "pcgrl_archive_state_bytes", "pcgrl_archive_export",
           "pcgrl_archive_import", "pcgrl_archive_poll_error", "pcgrl_archive_last_error"}
BOUNDS, DIMS, placement_values = R.BOUNDS, R.DIMS, R.placement_values


def test_header_units_and_symbols():
    _lib.build()
    unit, header = "archive/pcgrl_k_archive.hip", "archive/pcgrl_archive.h"
    assert unit in _lib.UNITS and header in _lib.HEADERS
    assert os.path.exists(os.path.join(_lib.CSRC, unit)) and os.path.exists(os.path.join(_lib.CSRC, header))
    text = re.sub(r"/\*.*?\*/", "", open(_lib.ARCHIVE_HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(pcgrl_[a-z0-9_]+)\s*\(", text))
    assert declared == SYMBOLS == set(_lib.ARCHIVE_SYMBOLS)
    others = [getattr(_lib, k) for k in dir(_lib) if k.endswith("SYMBOLS") and k != "ARCHIVE_SYMBOLS"]
    assert len(others) >= 21 and not any(declared & set(o) for o in others)
    L = _lib.lib()
    for name in declared:
        fn = getattr(L, name)
        want = _lib.ARCHIVE_SYMBOLS[name]
        assert fn.argtypes == want[1] and fn.restype == want[0], name
    for name, params in re.findall(r"\b(pcgrl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        n_params = 0 if params.strip() == "void" else len(params.split(","))
        assert n_params == len(_lib.ARCHIVE_SYMBOLS[name][1]), name
    for macro, value in (("MAX_AXES", archive.MAX_AXES), ("MAX_CELLS", None), ("MAX_MAP_BYTES", archive.MAX_MAP_BYTES),
                         ("MAX_TILES", archive.MAX_TILES), ("HEADER_BYTES", _lib.PCGRL_ARCHIVE_HEADER_BYTES)):
        m = re.search(r"#define PCGRL_ARCHIVE_%s (\S+)" % macro, text)
        assert m and (value is None or int(m.group(1)) == value), macro
    assert archive.MAX_CELLS == 1 << 20 and "#define PCGRL_ARCHIVE_MAX_CELLS (1 << 20)" in text
    # the engine's sources are not this unit's business
    src = open(os.path.join(_lib.CSRC, unit)).read() + open(os.path.join(_lib.CSRC, header)).read()
    assert "pcgrl_engine" not in src and "pcgrl_common.h" not in src


def _create(D=2, dims=(4, 4), lo=(0.0, 0.0), hi=(1.0, 1.0), L=96, T=8):
    h = C.c_void_p()
    k = max(len(dims), 1)
    rc = _lib.lib().pcgrl_archive_create(D, (C.c_int32 * k)(*dims), (C.c_double * k)(*lo), (C.c_double * k)(*hi), L, T, 0,
                                         C.byref(h))
    return rc, h


def test_bad_arguments_are_refused_without_a_device():
    L = _lib.lib()
    EINVAL = 1
    who = b"pcgrl_archive_create:"
    inf, nan = math.inf, math.nan
    cases = {
        "D = 0": dict(D=0), "D = 5": dict(D=5, dims=(2,) * 5, lo=(0.0,) * 5, hi=(1.0,) * 5), "a zero dim": dict(dims=(4, 0)),
        "a negative dim": dict(dims=(-1, 4)), "lo == hi": dict(lo=(0.0, 1.0)), "lo > hi": dict(lo=(2.0, 0.0)),
        "inf bound": dict(hi=(1.0, inf)), "-inf bound": dict(lo=(-inf, 0.0)), "nan bound": dict(lo=(nan, 0.0)),
        "L = 0": dict(L=0), "L = 4097": dict(L=4097), "T = 0": dict(T=0), "T = 257": dict(T=257),
        "2^20 + 1024 cells": dict(dims=(1025, 1024)),
        "2^21 cells in 4 axes": dict(D=4, dims=(64, 64, 32, 16), lo=(0.0,) * 4, hi=(1.0,) * 4),
    }
    for what, kw in cases.items():
        rc, h = _create(**kw)
        assert rc == EINVAL and h.value is None and who in L.pcgrl_archive_last_error(), what
    assert b"2^20" in L.pcgrl_archive_last_error()
    assert L.pcgrl_archive_create(2, None, None, None, 96, 8, 0, None) == EINVAL
    # a null handle is refused by every call before anything is read
    p = 0x1000
    assert L.pcgrl_archive_add(None, 4, p, p, p, None, p, p, p, None) == EINVAL
    assert b"pcgrl_archive_add: null" in L.pcgrl_archive_last_error()
    assert L.pcgrl_archive_cells(None, 4, p, p, None) == EINVAL
    assert L.pcgrl_archive_stats(None, p, None) == EINVAL
    assert L.pcgrl_archive_elites(None, 4, p, p, p, p, None) == EINVAL
    assert L.pcgrl_archive_ask(None, 4, 0, 0.01, p, p, None) == EINVAL
    assert L.pcgrl_archive_export(None, p, None) == EINVAL
    assert L.pcgrl_archive_import(None, p, 128, p, None) == EINVAL
    assert L.pcgrl_archive_state_bytes(None) == -1 and L.pcgrl_archive_poll_error(None, None) == -1
    L.pcgrl_archive_destroy(None)


def test_archive_for_bounds_and_the_unknown_name():
    six = archive.MEASURE_NAMES
    assert six == ("emptiness", "entropy", "symmetry", "symmetry-horizontal", "symmetry-vertical", "co-occurance")
    specs = {"loderunner": loderunner_spec(), "smb": smb_spec(), "microstructure": microstructure_spec(), "ddave": ddave_spec(),
             "mdungeon": mdungeon_spec(), "binary": problem_spec("binary", (16, 16)), "zelda": problem_spec("zelda", (16, 16))}
    for name, spec in specs.items():
        for k in six:
            assert archive.archive_shape(spec, [k]) == ([100], [(0.0, 1.0)]), (name, k)
        for k, (lo, hi) in spec.cond_bounds.items():
            dims, bounds = archive.archive_shape(spec, ["emptiness", k], bins=7)
            assert dims == [7, 7] and bounds == [(0.0, 1.0), (float(lo), float(hi))], (name, k)
    assert archive.archive_shape(specs["loderunner"], ("emptiness", "path-length")) == ([100, 100], [(0.0, 1.0), (0.0, 103.0)])
    assert archive.archive_shape(specs["smb"], "sol-length")[1] == [(0.0, 348.0)]
    assert archive.archive_shape(specs["microstructure"], ["tortuosity", "path-length"])[1] == [(0.0, 1040.0), (0.0, 2080.0)]
    assert archive.archive_shape(specs["binary"], ["regions", "path-length"])[1] == [(0.0, 128.0), (0.0, 136.0)]
    for name, bad in (("loderunner", "NONE"), ("ddave", "sol-length"), ("mdungeon", "brightness"), ("binary", "jumps")):
        with pytest.raises(Exception) as e:
            archive.archive_shape(specs[name], ["emptiness", bad])
        assert str(e.value) == (f"Behavior characteristic / measure `{bad}` not found in self.bc_bounds."
                                "You probably need to specify the lower/upper bounds of this measure in prob.cond_bounds.")
    with pytest.raises(TypeError, match="LodeRunnerEvaluator.*VecPcgrlEnv.*not dict"):
        archive.archive_for({}, ["emptiness"])


@pytest.mark.parametrize("lo,hi", BOUNDS)
@pytest.mark.parametrize("dims", DIMS)
def test_placement_on_hand_computed_cases(lo, hi, dims):
    v = placement_values(lo, hi, dims)
    got = archive.placed_cells(v[:, None], (dims,), [(lo, hi)])
    # the rule in Python floats, one rounding per operation
    want = [min(int(((min(max(float(x), lo), hi) - lo) / (hi - lo)) * dims), dims - 1) for x in v]
    assert got.tolist() == want == [R.place([x], [dims], [(lo, hi)]) for x in v]
    # lo, hi, their neighbours, outside, +-inf
    assert got[:12].tolist() == [0, dims - 1, 0, 0, dims - 1, dims - 1, 0, 0, dims - 1, dims - 1, 0, dims - 1]
    # a bin edge lands in its own bin or, where the quotient rounds below the edge, in the one under it; never elsewhere
    edges = got[12:]
    k = np.arange(dims + 1)
    assert ((edges == np.minimum(k, dims - 1)) | (edges == k - 1)).all() and edges[0] == 0 and edges[-1] == dims - 1
    assert (np.diff(edges) >= 0).all()


def test_placement_by_hand():
    one = lambda x, lo, hi, d: int(archive.placed_cells([[x]], (d,), [(lo, hi)])[0])
    assert one(0.5, 0, 1, 100) == 50 and one(0.25, 0, 1, 3) == 0 and one(0.34, 0, 1, 3) == 1 and one(0.99, 0, 1, 1) == 0
    assert one(0.29, 0, 1, 100) == 28  # 0.29 * 100 = 28.999999999999996 in float64: the rule is the float rule
    assert one(47, 0, 95, 100) == 49 and one(95, 0, 95, 100) == 99 and one(94, 0, 95, 100) == 98 and one(1, 0, 95, 100) == 1
    assert one(-2.5, -2.5, 7, 100) == 0 and one(2.25, -2.5, 7, 100) == 50 and one(6.9999, -2.5, 7, 3) == 2
    # C order over the axes; a NaN anywhere refuses the vector
    got = archive.placed_cells([[0.5, 47, 2.25], [0.0, 0, -2.5], [1.0, 95, 7], [0.5, math.nan, 0]], (100, 100, 100),
                               BOUNDS)
    assert got.tolist() == [50 * 10000 + 49 * 100 + 50, 0, 999999, -1] and got.dtype == np.int32
    assert R.place([0.5, 47, 2.25], (100, 100, 100), BOUNDS) == 504950 and R.place([math.nan], (3,), [(0, 1)]) is None
    # what an 8 x 12 map can give: k / 96 and the integers 0..95
    k = np.arange(97)
    assert (archive.placed_cells((k / 96.0)[:, None], (100,), [(0, 1)])
            == [R.place([x], [100], [(0, 1)]) for x in k / 96.0]).all()
    assert (archive.placed_cells(k[:96, None].astype(float), (100,), [(0, 95)])
            == [R.place([x], [100], [(0, 95)]) for x in range(96)]).all()


def test_batch_rule_equals_one_at_a_time_insertion():
    rng = np.random.default_rng(20)
    values = np.array([-1.5, 0.0, 2.0])
    for trial in range(200):
        dims = [(4, 4), (1,), (3, 2, 2)][trial % 3]
        bounds = [(0.0, 1.0)] * len(dims)
        arc = R.SeqArchive(dims, bounds, (2, 3))
        for batch in range(2):  # the second batch meets occupants
            n = int(rng.integers(1, 40))
            beh = rng.random((n, len(dims)))
            obj = values[rng.integers(0, 3, n)]
            if trial % 5 == 0:
                obj[rng.integers(0, n)] = math.nan
            grids = rng.integers(0, 8, (n, 2, 3), dtype=np.uint8)
            before = arc.copy()
            status, cell, counts = arc.add(grids, obj, beh)
            cells = [None if math.isnan(o) else R.place(b, dims, bounds) for b, o in zip(beh, obj)]
            win = R.batch_rule({c: bool(before.flag[c]) for c in range(arc.cells)}, before.obj, cells, obj.tolist())
            want = np.zeros(n, np.uint8)
            for i, c in enumerate(cells):
                if c is None:
                    want[i] = 3
            for c, i in win.items():
                want[i] = 1 if before.flag[c] else 2
            assert (status == want).all() and cell.tolist() == [-1 if c is None else c for c in cells]
            for c in range(arc.cells):
                if c in win:
                    i = win[c]
                    assert arc.flag[c] and arc.obj[c] == obj[i] and (arc.maps[c] == grids[i]).all() and (arc.beh[c] == beh[i]).all()
                else:
                    assert arc.flag[c] == before.flag[c] and (arc.maps[c] == before.maps[c]).all()
                    assert arc.obj[c] == before.obj[c] and (arc.beh[c] == before.beh[c]).all()
            assert counts.tolist() == [(want == 2).sum(), (want == 1).sum(), (want == 3).sum(), arc.flag.sum()]
            assert counts[3] == before.flag.sum() + counts[0]


def test_signed_zero_and_infinities_in_the_restatement():
    arc = R.SeqArchive((1,), [(0, 1)], (1,))
    assert arc.insert([1], -math.inf, [0.5]) == (0, 2) and arc.insert([2], -math.inf, [0.5]) == (0, 0)
    assert arc.insert([3], 0.0, [0.5]) == (0, 1) and arc.insert([4], -0.0, [0.5]) == (0, 0) and arc.maps[0, 0] == 3
    assert arc.insert([5], math.inf, [0.5]) == (0, 1) and arc.insert([6], math.inf, [0.5]) == (0, 0)
    arc = R.SeqArchive((1,), [(0, 1)], (1,))
    assert arc.insert([1], -0.0, [0.5]) == (0, 2) and arc.insert([2], 0.0, [0.5]) == (0, 0) and math.copysign(1, arc.obj[0]) == -1
    assert arc.insert([1], math.nan, [0.5]) == (None, 0) and arc.insert([1], 1.0, [math.nan]) == (None, 0)
    assert arc.insert([1], 1.0, cell=1) == (None, 0) and arc.insert([1], 1.0, cell=-1) == (None, 0)


def test_sampled_parents_are_uniform():
    n, k = 100000, 7
    p = archive.sampled_parents(5, 0, n, k)
    assert p.dtype == np.int64 and p.min() == 0 and p.max() == k - 1
    hist = np.bincount(p, minlength=k)
    sigma = math.sqrt(n * (1 / k) * (1 - 1 / k))
    assert (hist > 0).all() and (np.abs(hist - n / k) <= 6 * sigma).all()
    # another counter or seed is another stream; one cell leaves no choice
    assert (archive.sampled_parents(5, 1, n, k) != p).mean() > 0.5 and (archive.sampled_parents(6, 0, n, k) != p).mean() > 0.5
    assert (archive.sampled_parents(5, 0, n, k) == p).all() and (archive.sampled_parents(5, 0, 100, 1) == 0).all()
    assert (archive.sampled_parents(5, 0, 100, k) == p[:100]).all()  # child c's draw does not depend on n
    with pytest.raises(ValueError):
        archive.sampled_parents(0, 0, 4, 0)


def test_mutated_rate_and_tiles():
    rng = np.random.default_rng(3)
    parents = rng.integers(0, 8, (10000, 10, 10), dtype=np.uint8)  # 10^6 cells
    kids = archive.mutated(parents, 11, 0, 0.01, 8)
    changed = int((kids != parents).sum())
    assert abs(changed - 10000) <= 6 * 99.5, changed  # binomial(10^6, 0.01): sigma = 99.5
    assert kids.dtype == np.uint8 and kids.shape == parents.shape and kids.max() < 8
    assert (archive.mutated(parents, 11, 0, 0.0, 8) == parents).all()
    assert (archive.mutated(parents, 11, 1, 0.01, 8) != kids).any() and (archive.mutated(parents, 11, 0, 0.01, 8) == kids).all()
    ones = np.zeros((100, 100), np.uint8)
    assert (archive.mutated(ones, 1, 0, 1.0, 1) == ones).all()  # T == 1 mutates nothing
    for T in (2, 7, 8):
        p = rng.integers(0, T, (1000, 100), dtype=np.uint8)
        k = archive.mutated(p, 2, 3, 1.0, T)
        assert (k != p).all() and k.max() < T  # a mutated tile always changes
        step = (k.astype(int) - p - 1) % T  # r, uniform over [0, T - 2]
        hist = np.bincount(step.ravel(), minlength=T)
        assert hist[T - 1] == 0
        n = step.size
        sigma = math.sqrt(n * (1 / (T - 1)) * (1 - 1 / (T - 1))) if T > 2 else 0.0
        assert (np.abs(hist[:T - 1] - n / (T - 1)) <= 6 * sigma).all(), (T, hist)
