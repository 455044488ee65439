"""NCA evolution, the parts that need no GPU (include/pcgrl_amd_evo.h): aggregated() against numpy itself,
the normal draw against Python's statistics.NormalDist, the distribution of the stream, the independence of the streams, the
header against the symbol table and the argument checks made before any HIP call."""
import ctypes as C
import math
import re
from statistics import NormalDist

import numpy as np
import pytest

import evo_rules as E
from control_pcgrl_amd import _lib, archive, evo

ND = NormalDist()
SEED = 20  # the distribution test's seed: kept, see test_distribution


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_aggregated_equals_numpy(D):
    for S in E.S_ALL:
        obj, beh, ns = E.aggregate_data(12, S, D, seed=1000 * D + S)
        got = evo.aggregated(obj, beh, ns, weight=10.0)
        mean, o, tp, var, valid = E.numpy_fold(obj, beh, ns, 10.0)
        assert E.same_bits(got.behaviours, mean), (S, D)
        assert E.same_bits(got.objective, o), (S, D)
        assert E.same_bits(got.variance_penalty, var), (S, D)
        assert np.array_equal(got.time_penalty, tp) and got.valid.all()
        # all-equal values: the std is exactly 0 (genomes 1, 7 are of that class)
        assert (got.variance_penalty[1] == 0.0) and not math.copysign(1.0, got.variance_penalty[1]) > 0


@pytest.mark.parametrize("S", [1, 2, 9, 128])
def test_aggregated_refuses_a_negative_n_step(S):
    obj, beh, ns = E.aggregate_data(6, S, 2, seed=S)
    obj[:], beh[:] = 1.5, 0.25
    where = {0: 0, 2: S // 2, 4: S - 1}  # genome -> the seed the generator refused
    for g, s in where.items():
        ns[g, s] = -1
    got = evo.aggregated(obj, beh, ns, weight=3.0)
    assert got.valid.tolist() == [0, 1, 0, 1, 0, 1]
    for g in range(6):
        if g in where:
            assert np.isnan(got.objective[g]) and np.isnan(got.behaviours[g]).all()
        else:
            assert got.objective[g] == (3.0 * sum([1.5] * S)) / S and (got.behaviours[g] == 0.25).all()
        assert got.time_penalty[g] == -int(ns[g].sum())
    mean, o, tp, var, valid = E.numpy_fold(obj, beh, ns, 3.0)
    assert E.same_bits(got.objective, o) and E.same_bits(got.behaviours, mean) and np.array_equal(got.valid, valid)


def test_normal_from_uniform_equals_inv_cdf():
    u = E.probe_uniforms(evo.normal_uniforms(7, 0, 100, 1000))
    assert u.min() == 2.0 ** -54 and u.max() == 1.0 - 2.0 ** -53 and len(u) > 120000
    z = evo.normal_from_uniform(u)
    want = np.array([ND.inv_cdf(float(v)) for v in u])
    rel = np.abs(z - want) / np.maximum(np.abs(want), np.finfo(np.float64).tiny)
    rel = np.where(z == want, 0.0, rel)
    print("largest relative difference to NormalDist().inv_cdf:", rel.max())
    # a result is rounded to float32 (2^-24): a deviation below 2^-40 moves fewer than one rounded draw in 65 536
    assert rel.max() <= 2.0 ** -40
    assert E.same_bits(z.astype(np.float32), want.astype(np.float32))
    # odd symmetry where 1 - u is exact, and monotone
    v = u[u >= 0.5]  # (1 - v is exact there)
    assert len(v) > 40000 and ((1.0 - (1.0 - v)) == v).all() and E.same_bits(evo.normal_from_uniform(1.0 - v), -evo.normal_from_uniform(v))
    # monotone: strictly on the sorted stream sample; on the whole probe set in float32, the form that is handed out (in
    # float64 AS241 itself steps back by one unit in the last place at the seam u = 0.075, between neighbouring doubles)
    stream = np.sort(u[:100000])
    assert (np.diff(evo.normal_from_uniform(stream)) > 0).all()
    order = np.argsort(u, kind="stable")
    assert (np.diff(z[order].astype(np.float32)) >= 0).all()
    assert np.isfinite(z).all() and z.min() < -8.2 and z.max() > 8.2


def test_log64():
    rng = np.random.default_rng(3)
    x = np.concatenate([10.0 ** rng.uniform(-17, 0, 50000), [2.0 ** -54, 0.5, math.sqrt(0.5), np.nextafter(math.sqrt(0.5), 0), 1.0]])
    got = evo.log64(x)
    want = np.array([math.log(float(v)) for v in x])
    assert got[-1] == 0.0
    assert (np.abs(got - want) <= 4e-16 * np.maximum(np.abs(want), 0.05)).all()


def test_distribution():
    """10^6 float32 draws of one seed, children 0..999 at P = 1000.  The Kolmogorov bound 2.0 / sqrt(n) fails a true normal
    sample about once in 1500 seeds; SEED is one where the twin passes."""
    z = evo.normal_draws(SEED, 0, 1000, 1000).reshape(-1).astype(np.float64)
    n = len(z)
    assert n == 10 ** 6
    assert abs(z.mean()) < 0.005 and abs(z.var() - 1.0) < 0.01
    z.sort()
    erf = np.vectorize(math.erf)
    cdf = 0.5 * (1.0 + erf(z / math.sqrt(2.0)))  # NormalDist().cdf
    assert cdf[12345] == ND.cdf(z[12345])
    i = np.arange(n)
    dist = max(((i + 1) / n - cdf).max(), (cdf - i / n).max())
    print("Kolmogorov distance x sqrt(n):", dist * math.sqrt(n))
    assert dist * math.sqrt(n) < 2.0


def test_streams_are_independent():
    a = evo.normal_uniforms(5, 0, 2, 4096)
    assert not np.intersect1d(a[0], a[1]).size  # two children
    b = evo.normal_uniforms(5, 1, 1, 4096)
    assert not np.intersect1d(a[0], b[0]).size  # two draws
    assert np.array_equal(evo.normal_uniforms(5, 0, 1, 4096, first_child=1)[0], a[1])
    # the tile-mutation stream of the same seed, child and elements (include/pcgrl_amd_archive.h), in the normal stream's form
    c, k = np.uint64(0), np.arange(4096, dtype=np.uint64)
    with np.errstate(over="ignore"):
        cb = archive._mix64(archive._base(5, 0) ^ (c * np.uint64(archive._CHILD) + np.uint64((2 * archive._SALT) & archive._M64)))
        q = archive._mix64(cb + (k + np.uint64(1)) * np.uint64(archive._GOLDEN))
    tile = ((q >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    assert not np.intersect1d(a[0], tile).size
    # children of equal parents differ, the same call twice does not
    p = np.zeros((3, 50), np.float32)
    kids = evo.gaussian_children(p, 9, 0, 0.1)
    assert not np.array_equal(kids[0], kids[1]) and E.same_bits(kids, evo.gaussian_children(p, 9, 0, 0.1))
    assert E.same_bits(evo.gaussian_children(p + 1, 9, 0, 0.0), p + 1)


def test_header_symbols_and_constants():
    _lib.build()
    assert "evo/pcgrl_evo.h" in _lib.HEADERS and "archive/pcgrl_k_archive.hip" in _lib.UNITS
    text = re.sub(r"/\*.*?\*/", "", open(_lib.EVO_HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(pcgrl_[a-z0-9_]+)\s*\(", text))
    assert declared == set(_lib.EVO_SYMBOLS) == {"pcgrl_archive_create_genomes", "pcgrl_archive_ask_genomes",
                                                  "pcgrl_archive_sample_genomes", "pcgrl_evo_aggregate"}
    L = _lib.lib()
    for name, params in re.findall(r"\b(pcgrl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        assert len(params.split(",")) == len(_lib.EVO_SYMBOLS[name][1]), name
        assert getattr(L, name).argtypes == _lib.EVO_SYMBOLS[name][1]
    for macro, value in (("MAX_PARAMS", evo.MAX_PARAMS), ("MAX_SEEDS", evo.MAX_SEEDS), ("MAX_BEHAVIOURS", evo.MAX_BEHAVIOURS)):
        m = re.search(r"#define PCGRL_EVO_%s (\S+)" % macro, text)
        assert m and int(m.group(1)) == value == getattr(_lib, "PCGRL_EVO_" + macro)
    kernel = open(_lib.os.path.join(_lib.CSRC, "evo/pcgrl_evo.h")).read()
    assert "fp contract(off)" in kernel
    assert evo._LN2_HI == 6.93147180369123816490e-01 and evo._LN2_LO == 1.90821492927058770002e-10


def _create(dims=(4, 4), P=8):
    h = C.c_void_p()
    k = len(dims)
    rc = _lib.lib().pcgrl_archive_create_genomes(k, (C.c_int32 * k)(*dims), (C.c_double * k)(*([0.0] * k)),
                                                 (C.c_double * k)(*([1.0] * k)), P, 0, C.byref(h))
    return rc, _lib.lib().pcgrl_archive_last_error().decode()


def test_argument_checks_before_any_hip_call():
    for P in (0, -1, 16385):
        rc, msg = _create(P=P)
        assert rc == 1 and "genome length" in msg
    rc, msg = _create(dims=(1024, 1024), P=16384)  # 2^20 cells x 64 KiB
    assert rc == 1 and "2^32" in msg
    rc, msg = _create(dims=(1024, 1025), P=1)
    assert rc == 1 and "2^20" in msg
    L = _lib.lib()
    assert L.pcgrl_archive_ask_genomes(None, 1, 0, 0.1, None, None, None) == 1
    assert L.pcgrl_archive_sample_genomes(None, 1, 0, 0.1, None, None, None) == 1
    assert L.pcgrl_evo_aggregate(0, 1, 1, 10.0, *([None] * 9)) == 1
    assert L.pcgrl_evo_aggregate(1, 129, 1, 10.0, *([None] * 9)) == 1 and "[1, 128]" in L.pcgrl_archive_last_error().decode()
    assert L.pcgrl_evo_aggregate(1, 1, 5, 10.0, *([None] * 9)) == 1
    assert L.pcgrl_evo_aggregate(1, 1, 1, 10.0, *([None] * 9)) == 1


def test_cpu_device_is_refused():
    with pytest.raises(ValueError, match="cuda device"):
        evo.GenomeArchive((4, 4), [(0, 1), (0, 1)], 10, device="cpu")
    with pytest.raises(ValueError, match="device tensors"):
        evo.aggregate(np.zeros((1, 1)), np.zeros((1, 1, 1)), np.zeros((1, 1), np.int32))


def test_the_package_imports_the_layer_at_first_use():
    """importing the package for the env engine alone leaves evo.py out; its exports resolve from the package all the same"""
    import subprocess
    import sys
    code = ("import sys, control_pcgrl_amd as c\n"
            "assert 'control_pcgrl_amd.evo' not in sys.modules\n"
            "from control_pcgrl_amd import GenomeArchive, NcaEvolution, aggregate, evaluator_score, genome_archive_for, evo\n"
            "import control_pcgrl_amd.evo as e\n"
            "assert e is evo is c.evo and c.GenomeArchive is e.GenomeArchive and 'NcaEvolution' in dir(c)\n"
            "try:\n    c.no_such_name\nexcept AttributeError:\n    print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=_lib.os.path.dirname(_lib.os.path.dirname(_lib.CSRC)))
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]

