"""Helpers of the evolution tests (include/pcgrl_amd_evo.h): the data classes of the aggregate tests,
the probe set of the normal draw, and the archive restated on genome rows with tests/archive_rules.py's insertion.  The pins are
numpy itself (np.mean, np.std), Python's statistics.NormalDist and archive_rules.SeqArchive; nothing here imports
control_pcgrl_amd/evo.py.
"""
import numpy as np

import archive_rules as R

S_ALL = list(range(1, 129))
S_GPU = [1, 2, 7, 8, 9, 10, 16, 17, 127, 128]


def aggregate_data(G, S, D, seed):
    """objective [G, S], behaviours [G, S, D], n_step [G, S]: genome g cycles through the data classes -- random values over
    ten decades, all-equal values (std exactly 0), +-0.0, +-inf and NaN."""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-5, 5, size=(G, S, D + 1))
    x = rng.standard_normal((G, S, D + 1)) * mag
    for g in range(G):
        kind = g % 6
        if kind == 1:
            x[g] = rng.integers(-1000, 1000, size=(1, D + 1)) * 0.125  # all seeds equal; S copies sum exactly: the std is 0
        elif kind == 2:
            x[g] = np.where(rng.random((S, D + 1)) < 0.5, 0.0, -0.0)
        elif kind == 3:
            x[g] = -0.0
        elif kind == 4:
            x[g, rng.integers(S), rng.integers(D + 1)] = np.inf * (1 if rng.random() < 0.5 else -1)
        elif kind == 5:
            x[g, rng.integers(S), rng.integers(D + 1)] = np.nan
    n_step = rng.integers(0, 10, size=(G, S)).astype(np.int32)
    return np.ascontiguousarray(x[:, :, 0]), np.ascontiguousarray(x[:, :, 1:]), n_step


def numpy_fold(objective, behaviours, n_step, weight):
    """the arbiter: np.mean and np.std of each genome's S values (a contiguous vector each), the Python loop acc -= p"""
    G, S = objective.shape
    D = behaviours.shape[2]
    mean, obj, var = np.empty((G, D)), np.empty(G), np.empty(G)
    tp, valid = np.empty(G, np.int32), np.empty(G, np.uint8)
    with np.errstate(all="ignore"):
        for g in range(G):
            stds = []
            for j in range(D):
                v = np.ascontiguousarray(behaviours[g, :, j])
                mean[g, j] = np.mean(v)
                stds.append(np.std(v))
            acc = 0
            for s in range(S):
                p = -objective[g, s]  # the level's penalty
                acc -= p
            obj[g] = (np.float64(weight) * acc) / np.float64(S)
            t = stds[0]
            for sd in stds[1:]:
                t = t + sd
            var[g] = -t / np.float64(D)
            tp[g] = -int(n_step[g].sum())
            valid[g] = (n_step[g] >= 0).all()
            if not valid[g]:
                mean[g], obj[g] = np.nan, np.nan
    return mean, obj, tp, var, valid


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind == "f":  # every NaN is one NaN
        a, b = np.where(np.isnan(a), np.nan, a), np.where(np.isnan(b), np.nan, b)
        u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(u), b.view(u))
    return a.shape == b.shape and np.array_equal(a, b)


def probe_uniforms(stream):
    """the probe set of the normal draw: `stream` (the stream's own uniforms), the ends, the region edges from one float64
    below to one above, and 2 x 10^4 uniforms with exponents down to 1e-16"""
    def around(v):
        v = np.float64(v)
        return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]

    u = [np.float64(2.0) ** -54, 1.0 - np.float64(2.0) ** -53] + around(0.075) + around(0.925)
    e5 = np.exp(np.float64(-25.0))  # r = 5
    near = [e5]
    for _ in range(40):
        near.append(np.nextafter(near[-1], np.inf))
    lo = e5
    for _ in range(40):
        lo = np.nextafter(lo, -np.inf)
        near.append(lo)
    u += near + [1.0 - v for v in near]
    rng = np.random.default_rng(241)
    small = 10.0 ** rng.uniform(-16, -0.5, size=10000)
    small = np.maximum(small, 2.0 ** -54)
    return np.concatenate([np.asarray(stream, np.float64).reshape(-1), np.array(u, np.float64), small, 1.0 - small])


class SeqGenomes(R.SeqArchive):
    """archive_rules.SeqArchive on float32 rows: the row travels as its bytes, so the insertion is archive_rules' own"""

    def __init__(self, dims, bounds, n_params):
        super().__init__(dims, bounds, (4 * int(n_params),))
        self.n_params = int(n_params)

    def add_genomes(self, genomes, objectives, behaviours=None, cells=None):
        g = np.ascontiguousarray(genomes, dtype=np.float32).reshape(-1, self.n_params)
        return self.add(g.view(np.uint8), objectives, behaviours, cells)

    def genomes(self):
        return self.maps.reshape(self.cells, -1).view(np.float32)[self.occupied()]
