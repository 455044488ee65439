"""Microstructure levels, the parts that need no GPU: the plain-Python rules (tests/microstructure_rules.py) against the
fixtures recorded from the reference (tests/golden/microstructure, tools/gen_golden_microstructure.py), the restated numpy-order
sum against np.mean, microstructure_spec's tables, the restated loss on hand-computed cases, the header, the symbols and the
config struct, the argument checks of the C ABI (include/pcgrl_amd_microstructure.h: made before any HIP call, so they answer
without a device), the Python surface, and what stays outside the engine."""
import ctypes as C
import glob
import inspect
import os
import re

import numpy as np
import pytest

import measures_numpy as mn
import microstructure_rules as R
from conftest import GOLDEN
from control_pcgrl_amd import _lib, microstructure, problems
from control_pcgrl_amd.vec_env import build_config

DIR = os.path.join(GOLDEN, "microstructure")
FILES = sorted(glob.glob(os.path.join(DIR, "*.npz")))
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (8, 8), (16, 16), (33, 17), (3, 64), (64, 3), (64, 64)]
SYMBOLS = {"pcgrl_microstructure_evaluate", "pcgrl_microstructure_measures_for_grids",
           "pcgrl_microstructure_diversity_scratch_bytes", "pcgrl_microstructure_diversity_for_grids"}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _load(h, w):
    return np.load(os.path.join(DIR, f"ms_{h}x{w}.npz"))


def test_fixture_set_is_complete():
    assert sorted(os.path.basename(f) for f in FILES) == sorted(f"ms_{h}x{w}.npz" for h, w in SHAPES)
    assert max(os.path.getsize(f) for f in FILES) <= 100 * 1024
    for f in FILES:
        z = np.load(f)  # (allow_pickle is off: arrays only)
        n = len(z["grids"])
        assert z["grids"].dtype == np.uint8 and z["grids"].max() <= 1 and list(z["stat_keys"]) == R.STAT_KEYS
        assert z["stats_bits"].shape == (n, 2) and z["stats_bits"].dtype == np.uint64 and z["regions"].shape == (n,)
        assert z["region_rec"].shape == (n, 32, 5) and z["region_tort_bits"].shape == (n, 32) and len(z["names"]) == n
        assert {"all-solid", "all-empty", "one-cell", "checker", "serpentine"} <= set(z["names"])


def test_fixtures_show_the_cases():
    z = _load(64, 64)
    names = list(z["names"])
    stats = z["stats_bits"].view(np.float64)
    i = names.index("checker")  # 2 048 one-cell regions: the mean of 2 048 zeros
    assert z["regions"][i] == 2048 and stats[i].tolist() == [0.0, 0.0] and (z["region_rec"][i, :, 4] == 0).all()
    i = names.index("serpentine")  # one region, the longest shortest path a 64 x 64 map has
    assert z["regions"][i] == 1 and stats[i, 0] == 32 * 64 + 31 - 1 and z["region_rec"][i, 0].tolist() == [0, 0, 62, 0, 2078]
    assert stats[i, 1] == 2078 / 62
    i = names.index("all-solid")
    assert z["regions"][i] == 0 and stats[i].tolist() == [0.0, 0.0] and (z["region_rec"][i] == -1).all()
    i = names.index("all-empty")  # the far cell of (0, 0) is (63, 63), and from there the far distance is 126 again
    assert z["regions"][i] == 1 and stats[i].tolist() == [126.0, 126 / np.sqrt(63 ** 2 + 63 ** 2)]
    i = names.index("one-cell")
    assert z["regions"][i] == 1 and stats[i].tolist() == [0.0, 0.0] and z["region_rec"][i, 0].tolist() == [32, 32, 32, 32, 0]
    for k in (7, 8, 9, 127, 128, 129):  # the lengths at which numpy's sum changes its order
        i = names.index(f"l-shapes-{k}")
        assert z["regions"][i] == k
        assert len(set(z["region_tort_bits"][i][:min(k, 32)].tolist())) > 2
    assert (z["regions"] > 256).sum() >= 4
    # a cross: from the tip of its upper arm the three other tips are equally far, and np.argmax takes the first (the left tip)
    z = _load(5, 9)
    i = list(z["names"]).index("cross")
    assert z["region_rec"][i, 0].tolist() == [0, 2, 2, 0, 4] and z["regions"][i] == 1
    # two regions of the same d: the first keeps path-length (replaced only on `>`), both count in the mean
    z = _load(8, 8)
    i = list(z["names"]).index("equal-pair")
    assert z["regions"][i] == 2 and z["region_rec"][i, 0, 4] == z["region_rec"][i, 1, 4] == 3
    # one-cell regions contribute 0.0 and shift what follows: some map has one before a larger region
    shifted = 0
    for f in FILES:
        z = np.load(f)
        for rec, cnt in zip(z["region_rec"], z["regions"]):
            d = rec[:min(int(cnt), 32), 4]
            shifted += bool(len(d) > 1 and (d[:-1] == 0).any() and d[np.argmax(d == 0):].max() > 0)
    assert shifted > 10


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_rules_equal_fixtures(path):
    z = np.load(path)
    cap = z["region_rec"].shape[1]
    for i, m in enumerate(z["grids"]):
        stats, count, rec, tort = R.outputs(m, cap)
        assert _bits(stats).tolist() == z["stats_bits"][i].tolist(), (i, stats)
        assert count == z["regions"][i] and rec == z["region_rec"][i].tolist(), i
        assert _bits(tort).tolist() == z["region_tort_bits"][i].tolist(), i
        assert not R.has_error(m)


def test_numpy_order_sum_equals_np_mean_for_every_length():
    rng = np.random.default_rng(2100)
    assert R.numpy_sum([]) == 0.0
    for n in range(1, 2101):
        v = rng.random(n) * rng.choice([1.0, 1e-3, 1e3], n)
        assert _bits(R.numpy_mean(v)) == _bits(np.mean(list(v))), n
    # and in sequence it is not: the order matters at these magnitudes
    v = rng.random(2100) * rng.choice([1.0, 1e-3, 1e3], 2100)
    seq = 0.0
    for x in v:
        seq += x
    assert seq != R.numpy_sum(v)


def test_rules_on_hand_made_maps():
    # an id above 1 reads as solid and is an error
    m = np.array([[0, 2, 0], [0, 255, 0]], np.uint8)
    assert R.has_error(m) and R.get_stats(m) == R.get_stats(np.array([[0, 1, 0], [0, 1, 0]]))
    # an L: first cell (0, 0), far cell (2, 1) at distance 3; from there the greatest distance is 3; l2 = sqrt(1 + 4)
    m = np.array([[0, 1], [0, 1], [0, 0]], np.uint8)
    assert R.regions(m) == [(0, 0, 2, 1, 3, 3 / np.sqrt(5))]
    # a one-cell region before a segment: the mean is over two values
    m = np.array([[0, 1, 1, 1], [1, 1, 0, 0]], np.uint8)
    assert [r[:5] for r in R.regions(m)] == [(0, 0, 0, 0, 0), (1, 2, 1, 3, 1)] and R.get_stats(m) == [1.0, 0.5]
    assert R.outputs(m, 3)[2] == [[0, 0, 0, 0, 0], [1, 2, 1, 3, 1], [-1] * 5] and R.outputs(m, 1)[1] == 2


def test_spec_tables():
    for shape in ((64, 64), (5, 9)):  # frozen at the stock size whatever the map
        spec = microstructure.microstructure_spec(shape)
        assert spec.name == "microstructure" and spec.stat_keys == R.STAT_KEYS == ["path-length", "tortuosity"]
        assert spec.tile_types == R.TILES == ["empty", "solid"] and spec.n_tiles == 2
        assert spec.static_trgs == R.STATIC_TRGS == {"tortuosity": 1040.0}
        assert spec.cond_bounds == R.COND_BOUNDS == {"path-length": (0, 2080.0), "tortuosity": (0, 1040.0)}
        assert spec.default_weights == R.DEFAULT_WEIGHTS == spec.problem_weights == {"tortuosity": 1}
    cfg = microstructure.microstructure_config((5, 9))
    assert (cfg.h, cfg.w) == (5, 9) and list(cfg.has_trg) == [0, 1]  # path-length has no target
    assert cfg.trg_lo[1] == cfg.trg_hi[1] == 1040.0 and list(cfg.weight) == [0, 1]
    assert list(microstructure.microstructure_config(weights={"tortuosity": 2.5, "path-length": 3}).weight) == [3, 2.5]
    with pytest.raises(ValueError):
        microstructure.microstructure_config(weights={"regions": 1})


def test_loss_of_the_rules_on_hand_computed_cases():
    # on the target: no loss; path-length has no target and adds nothing whatever its weight
    assert R.loss([0, 1040.0]) == 0.0 and R.loss([2078, 1040.0], {"tortuosity": 1, "path-length": 7}) == 0.0
    assert R.loss([126, 1.5]) == -1038.5 and R.loss([0, 0]) == -1040.0
    assert R.loss([10, 1041.25], {"tortuosity": 4}) == -5.0  # above the target counts the same
    # not dyadic: the term is one rounded subtraction and one rounded multiplication
    assert R.loss([3, 3 / np.sqrt(5)], {"tortuosity": 0.1}) == -(1040.0 - 3 / np.sqrt(5)) * 0.1
    assert R.loss([3, 2.0], {}) == 0.0  # no weight given: 0


def test_header_units_symbols_and_config():
    _lib.build()
    unit, header = "microstructure/pcgrl_k_microstructure.hip", "microstructure/pcgrl_microstructure.h"
    assert unit in _lib.UNITS and header in _lib.HEADERS and "measures/pcgrl_measures_wave.h" in _lib.HEADERS
    assert os.path.exists(os.path.join(_lib.CSRC, unit)) and os.path.exists(os.path.join(_lib.CSRC, header))
    assert os.path.exists(_lib.MICROSTRUCTURE_HEADER)
    text = re.sub(r"/\*.*?\*/", "", open(_lib.MICROSTRUCTURE_HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(pcgrl_[a-z0-9_]+)\s*\(", text))
    assert declared == SYMBOLS == set(_lib.MICROSTRUCTURE_SYMBOLS)
    others = [table for _, table in _lib.ABI if table is not _lib.MICROSTRUCTURE_SYMBOLS]
    assert len(others) == len(_lib.ABI) - 1
    assert not any(declared & set(o) for o in others)
    L = _lib.lib()
    for name in declared:
        fn = getattr(L, name)  # (exported by the library)
        want = _lib.MICROSTRUCTURE_SYMBOLS[name]
        assert fn.argtypes == want[1] and fn.restype == want[0], name
    for name, params in re.findall(r"\b(pcgrl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        assert len(params.split(",")) == len(_lib.MICROSTRUCTURE_SYMBOLS[name][1]), name
    # the measures and the diversity take the Lode Runner argument lists
    for a, b in (("measures_for_grids", "measures_for_grids"), ("diversity_scratch_bytes", "diversity_scratch_bytes"),
                 ("diversity_for_grids", "diversity_for_grids")):
        assert _lib.MICROSTRUCTURE_SYMBOLS["pcgrl_microstructure_" + a] == _lib.LODERUNNER_MEASURES_SYMBOLS["pcgrl_loderunner_" + b]
    assert C.sizeof(_lib.PcgrlMicrostructureConfig) == 8 + 8 + 3 * 16 and _lib.PCGRL_MICROSTRUCTURE_STATS == 2
    # the kernel is plain HIP C++ that instantiates the shared wave body and takes the engine's sweeps by inclusion
    src = open(os.path.join(_lib.CSRC, header)).read()
    assert "asm" not in src.replace("namespace", "")
    assert "meas_wave_map<MS_MEAS_TILES, MS_MEAS_PLANES, MS_MAX_CELLS>" in src and '#include "../pcgrl_kernels2d.h"' in src
    assert "MS_MEAS_TILES = 2, MS_MEAS_PLANES = 1" in src and "MS_MAX_CELLS = MS_MAX_H * MS_MAX_W" in src
    assert b"0.7.0" in L.pcgrl_version()


def test_abi_argument_checks_need_no_device():
    L = _lib.lib()
    # pointers that are never dereferenced: every call below is refused before any HIP call
    grids, stats = 0x1000, 0x3000
    EINVAL, EUNSUPPORTED = 1, 2
    who = b"pcgrl_microstructure_evaluate:"

    def call(cfg, n=2, g=grids, cap=8, st=stats):
        return L.pcgrl_microstructure_evaluate(C.byref(cfg) if cfg is not None else None, n, g, cap, st, None, None, None, None,
                                               None, None)

    ok = microstructure.microstructure_config((64, 64))
    for kw in (dict(cfg=None), dict(cfg=ok, g=None), dict(cfg=ok, st=None), dict(cfg=ok, n=0), dict(cfg=ok, n=-3)):
        assert call(**kw) == EINVAL and who in L.pcgrl_last_error(), kw
    assert call(ok, cap=-1) == EINVAL and who + b" region_cap must not be negative" in L.pcgrl_last_error()
    for shape in ((0, 12), (65, 12), (8, 0), (8, 65), (-1, 4)):
        assert call(microstructure.microstructure_config(shape)) == EUNSUPPORTED, shape
        assert who in L.pcgrl_last_error() and b"1..64 rows and 1..64 columns" in L.pcgrl_last_error()

    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    p += 8 - p % 8
    meas, div = L.pcgrl_microstructure_measures_for_grids, L.pcgrl_microstructure_diversity_for_grids
    scratch = L.pcgrl_microstructure_diversity_scratch_bytes
    for args in ((8, 12, 1, None, p, p, None, None, None, None), (8, 12, 1, p, None, p, None, None, None, None),
                 (8, 12, 1, p, p, None, None, None, None, None), (8, 12, 1, p, p, p, None, p, None, None),
                 (8, 12, -1, p, p, p, None, None, None, None)):
        assert meas(*args) == EINVAL and b"pcgrl_microstructure_measures_for_grids:" in L.pcgrl_last_error()
    rest = (None,) * 6
    for args in ((8, 12, 8, None, 4, p, p), (8, 12, 8, p, 4, None, p), (8, 12, 8, p, 4, p, None), (8, 12, 8, p, 4, p + 4, p),
                 (8, 12, -8, p, 4, p, p)):
        assert div(*args, *rest) == EINVAL and b"pcgrl_microstructure_diversity_for_grids:" in L.pcgrl_last_error()
    for h, w in ((0, 12), (65, 12), (8, 0), (8, 65)):
        assert meas(h, w, 1, p, p, p, None, None, None, None) == EUNSUPPORTED
        assert b"pcgrl_microstructure_measures_for_grids: maps of 1..64 rows and 1..64 columns" in L.pcgrl_last_error()
        assert div(h, w, 8, p, 4, p, p, *rest) == EUNSUPPORTED
        assert b"pcgrl_microstructure_diversity_for_grids: maps of 1..64 rows and 1..64 columns" in L.pcgrl_last_error()
        assert scratch(h, w, 8) == 0
    for group in (1, 3, 0, -2):
        assert div(8, 12, 8, p, group, p, p, *rest) == EINVAL
        assert b"group must be at least 2 and divide the number of maps" in L.pcgrl_last_error()
    # no maps: a no-op
    assert meas(8, 12, 0, None, None, None, None, None, None, None) == 0
    assert div(8, 12, 0, None, 4, None, None, None, None, None, None, None) == 0
    assert scratch(8, 12, 0) == 0 and scratch(8, 12, -3) == 0
    # 8 * (ceil(h * w / 64) + 1) per map: one plane
    assert scratch(1, 1, 3) == 3 * 2 * 8 and scratch(64, 64, 4096) == 4096 * 65 * 8 and scratch(5, 13, 1) == 3 * 8

    for shape in ((0, 12), (65, 12), (8, 65)):
        with pytest.raises(NotImplementedError):
            microstructure.MicrostructureEvaluator(shape, device="cuda:0")
    with pytest.raises(ValueError):
        microstructure.MicrostructureEvaluator((8, 12), device="cpu")  # no CPU fallback
    with pytest.raises(ValueError):
        microstructure.MicrostructureEvaluator((8, 12, 2))
    with pytest.raises(ValueError):
        microstructure.MicrostructureEvaluator((8, 12), max_levels=0)


def test_python_surface_is_in_place():
    import control_pcgrl_amd
    from control_pcgrl_amd import MICROSTRUCTURE_BC_NAMES, MicrostructureEvaluator
    from control_pcgrl_amd.measures import MeasuresMixin
    E = MicrostructureEvaluator
    assert issubclass(E, MeasuresMixin) and E is microstructure.MicrostructureEvaluator
    assert control_pcgrl_amd.microstructure_spec is microstructure.microstructure_spec
    assert list(inspect.signature(E.evaluate).parameters) == ["self", "grids", "region_cap"]
    assert inspect.signature(E.evaluate).parameters["region_cap"].default == 0
    assert list(inspect.signature(E.measures).parameters) == ["self", "grids", "entropy"]
    assert inspect.signature(E.measures).parameters["entropy"].default is True
    sig = inspect.signature(E.diversity).parameters
    assert list(sig) == ["self", "grids", "group", "pairwise"] and sig["group"].default is None and sig["pairwise"].default is False
    assert list(inspect.signature(E.behaviour).parameters) == ["self", "grids", "names"]
    assert list(inspect.signature(E.check_errors).parameters) == ["self"] and list(inspect.signature(E.close).parameters) == ["self"]
    assert hasattr(E, "__enter__") and hasattr(E, "__exit__")
    sig = inspect.signature(E.__init__).parameters
    assert list(sig) == ["self", "map_shape", "device", "weights", "max_levels"] and sig["map_shape"].default == (64, 64)
    assert MICROSTRUCTURE_BC_NAMES is microstructure.MICROSTRUCTURE_BC_NAMES
    assert tuple(MICROSTRUCTURE_BC_NAMES) == ("path-length", "tortuosity", "emptiness", "entropy", "symmetry",
                                              "symmetry-horizontal", "symmetry-vertical", "co-occurance", "NONE")
    assert tuple(MICROSTRUCTURE_BC_NAMES[2:8]) == tuple(mn.BC_NAMES) == tuple(microstructure.MICROSTRUCTURE_MEASURE_NAMES)
    assert "stepping microstructure environments is not built" in microstructure.__doc__


def test_microstructure_stays_outside_the_engine():
    import control_pcgrl_amd
    assert "microstructure" not in problems.PROBLEMS
    with pytest.raises(ValueError):
        problems.problem_spec("microstructure", (64, 64))
    with pytest.raises(ValueError):
        build_config("microstructure", "narrow", (64, 64))
    assert control_pcgrl_amd.__version__ == "0.7.0" and b"0.7.0" in _lib.lib().pcgrl_version()
