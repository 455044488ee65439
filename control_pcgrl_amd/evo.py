"""NCA evolution on the device (include/pcgrl_amd_evo.h, csrc/evo/pcgrl_evo.h): the reference's default
evolution -- `--model NCA --representation cellular` -- evolves the weights of the NCA, not maps.  GenomeArchive keeps genome
elites in the grid archive of archive.py (same placement, insertion and image), hands out Gaussian children
(w += randn_like(w) * sqrt(step_size), evo/models.py:31-38) and first-generation samples; aggregate() is what simulate folds over
the S levels of a genome (evo/evolve.py:1125-1154, :1209-1244); NcaEvolution chains ask -> generate -> score -> aggregate ->
diversity -> add on one stream with no host sync.

The normal draws are stated arithmetic, not a library's: a counter-based uniform on the archive's splitmix64 stream, Wichura's
AS241 PPND16 as the inverse CDF, and a float64 logarithm of this project's own (log64), all with + - * / and sqrt only.  The
numpy twins below ARE that statement (log64, normal_from_uniform, normal_uniforms, gaussian_children, aggregated) and the
kernels equal them bit for bit.  torch's randn stream is not reproduced.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, nca
from .archive import _CHILD, _GOLDEN, _M64, _SALT, DeviceGridArchive, _base, _check, _mix64, archive_shape, sampled_parents  # noqa: F401

MAX_PARAMS, MAX_SEEDS, MAX_BEHAVIOURS = 16384, 128, 4
_LN2_HI, _LN2_LO = nca._LN2_HI, nca._LN2_LO
_SQRT_HALF = 0.70710678118654757

# AS241 PPND16 (Wichura 1988), highest power first
_A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
      1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0)
_B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
      5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0)
_C = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
      3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0)
_D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
      6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0)
_E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
      2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0)
_F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
      1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555888793770e-1, 1.0)


# ---- the numpy twins: the same functions the device computes ---------------------------------------------------------------

def _horner(coef, r):
    p = np.full_like(r, coef[0])
    for c in coef[1:]:
        p = p * r + c
    return p


def log64(x):
    """This project's float64 natural logarithm of positive normal x: x = m 2^e with m in [sqrt(1/2), sqrt(2)),
    f = (m - 1) / (m + 1), p the Horner polynomial in f^2 with the coefficients 1/25, 1/23, ..., 1/1, and
    e ln2_hi + ((2 f) p + e ln2_lo).  Every step is one float64 + - * / (or an exact scaling)."""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)  # m in [1/2, 1)
    low = m < _SQRT_HALF
    m = np.where(low, m * 2.0, m)
    e = (e - low).astype(np.float64)
    f = (m - 1.0) / (m + 1.0)
    s = f * f
    p = _horner([1.0 / n for n in range(25, 0, -2)], s)
    return e * _LN2_HI + ((2.0 * f) * p + e * _LN2_LO)


def normal_from_uniform(u):
    """z = ppnd(u) for 0 < u < 1, float64: Wichura's AS241 PPND16, numerator and denominator by Horner, one division; the tail
    regions use r = sqrt(-log64(min(u, 1 - u)))."""
    u = np.asarray(u, dtype=np.float64)
    shape = u.shape
    u = u.reshape(-1)
    q = u - 0.5
    z = np.empty_like(u)
    mid = np.abs(q) <= 0.425
    qm = q[mid]
    r = 0.180625 - qm * qm
    z[mid] = (_horner(_A, r) * qm) / _horner(_B, r)
    tail = ~mid
    qt = q[tail]
    t = np.where(qt <= 0.0, u[tail], 1.0 - u[tail])
    r = np.sqrt(-log64(t))
    near = r <= 5.0
    rn, rf = r - 1.6, r - 5.0
    x = np.where(near, _horner(_C, rn), _horner(_E, rf)) / np.where(near, _horner(_D, rn), _horner(_F, rf))
    z[tail] = np.where(qt < 0.0, -x, x)
    return z.reshape(shape)


def normal_uniforms(seed, draw, n, n_params, first_child=0):
    """The uniforms behind the normal draws of children first_child .. first_child + n - 1 at draw counter `draw`: float64
    [n, P], u = ((q >> 11) + 0.5) 2^-53, never 0 or 1."""
    c = np.arange(int(first_child), int(first_child) + int(n), dtype=np.uint64)[:, None]
    k = np.arange(int(n_params), dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        gb = _mix64(_base(seed, draw) ^ (c * np.uint64(_CHILD) + np.uint64((3 * _SALT) & _M64)))
        q = _mix64(gb + (k + np.uint64(1)) * np.uint64(_GOLDEN))
    return ((q >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def normal_draws(seed, draw, n, n_params, first_child=0):
    """The float32 N(0, 1) draws of those children: float32 [n, P]."""
    return normal_from_uniform(normal_uniforms(seed, draw, n, n_params, first_child)).astype(np.float32)


def gaussian_children(parents, seed, draw, sigma):
    """The children of `parents` float32 [n, P] (row c the genome of child c's parent, or the mean of a sample) at draw counter
    `draw`: parent[k] + ((float32)z * sigma), one float32 multiply, then one float32 add; sigma == 0 returns the parents' bits."""
    p = np.ascontiguousarray(parents, dtype=np.float32)
    n, P = p.shape
    if np.float32(sigma) == 0:
        return p.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        return p + normal_draws(seed, draw, n, P) * np.float32(sigma)


def _np_sum(x):
    """numpy's own sum of float64 vectors of at most 128 elements, restated along axis 0 of x [n, ...]: sequential below 8;
    else eight accumulators over the first n - n % 8 elements, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remainder in order.
    The sum starts from +0.0, so -0.0 is never returned."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    if n < 8:
        res = np.zeros(x.shape[1:])
        for v in x:
            res = res + v
        return res
    r = [x[j] for j in range(8)]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] = r[j] + x[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in x[i:]:
        res = res + v
    return res + 0.0  # (numpy adds the sum to its initial 0.0: a sum of -0.0 comes out as +0.0)


def aggregated(objective, behaviours, n_step, weight=10.0):
    """simulate's fold over the S levels of each genome, in numpy: objective float64 [G, S], behaviours float64 [G, S, D],
    n_step int32 [G, S].  Returns behaviours [G, D] (the mean), objective [G] ((weight * acc) / S with acc the sequential sum in
    seed order from 0), time_penalty int32 [G] (-sum n_step), variance_penalty [G] (-(std_0 + ... + std_{D-1}) / D) and valid
    uint8 [G] (0 with a negative n_step; the objective and behaviours of such a genome are NaN)."""
    obj = np.asarray(objective, dtype=np.float64)
    beh = np.asarray(behaviours, dtype=np.float64)
    ns = np.asarray(n_step, dtype=np.int32)
    G, S = obj.shape
    beh = beh.reshape(G, S, -1)
    D = beh.shape[2]
    if not (1 <= S <= MAX_SEEDS and 1 <= D <= MAX_BEHAVIOURS and ns.shape == (G, S)):
        raise ValueError("aggregated() takes objective [G, S], behaviours [G, S, D], n_step [G, S] with S in 1..128, D in 1..4")
    fS = np.float64(S)
    valid = (ns >= 0).all(axis=1)
    with np.errstate(all="ignore"):
        acc = np.zeros(G)
        for s in range(S):
            acc = acc + obj[:, s]
        x = np.moveaxis(beh, 1, 0)  # [S, G, D]
        mean = _np_sum(x) / fS
        d = x - mean
        std = np.sqrt(_np_sum(d * d) / fS)  # [G, D]
        stds = std[:, 0]
        for j in range(1, D):
            stds = stds + std[:, j]
        return SimpleNamespace(behaviours=np.where(valid[:, None], mean, np.nan),
                               objective=np.where(valid, (np.float64(weight) * acc) / fS, np.nan),
                               time_penalty=(-ns.astype(np.int64).sum(axis=1)).astype(np.int32),
                               variance_penalty=-stds / np.float64(D), valid=valid.astype(np.uint8))


# ---- the device side ----------------------------------------------------------------------------------------------------------

class GenomeArchive(DeviceGridArchive):
    """DeviceGridArchive whose elite is a genome: a float32 [n_params] row per cell (n_params in 1..16384) where the map archive
    has its map.  add(), cell_of(), stats(), elites() (with .genomes), state_dict() / load_state_dict() and check_errors() are
    the archive's own calls on the payload rows; ask() hands out Gaussian children and sample() the first generation.  As
    there, everything but stats(), elites(), check_errors() and load_state_dict() only enqueues kernels on the current
    stream."""

    def __init__(self, dims, bounds, n_params, device="cuda:0"):
        self.dims = tuple(int(d) for d in ([dims] if np.isscalar(dims) else dims))
        bounds = [tuple(float(v) for v in b) for b in bounds]
        if len(bounds) != len(self.dims):
            raise ValueError(f"{len(self.dims)} dims but {len(bounds)} bounds")
        self.bounds = tuple(bounds)
        self.n_params = int(n_params)
        self.map_shape, self.map_bytes, self.n_tiles = (4 * self.n_params,), 4 * self.n_params, 0  # (the payload row in bytes)
        self.device = torch.device(device)
        self._h = None
        if self.device.type != "cuda":
            raise ValueError("GenomeArchive needs a cuda device: there is no CPU fallback")
        self._L = _lib.lib()
        D = len(self.dims)
        h = C.c_void_p()
        index = self.device.index if self.device.index is not None else 0
        _check(self._L.pcgrl_archive_create_genomes(
            D, (C.c_int32 * max(D, 1))(*self.dims), (C.c_double * max(D, 1))(*[b[0] for b in bounds]),
            (C.c_double * max(D, 1))(*[b[1] for b in bounds]), self.n_params, index, C.byref(h)),
            "pcgrl_archive_create_genomes")
        self._h = h
        self.n_cells = int(np.prod(self.dims))

    def _rows(self, genomes):
        g = torch.as_tensor(genomes, device=self.device)
        if g.dtype != torch.float32:
            raise ValueError(f"genomes must be float32, got {g.dtype}")
        if g.dim() == 1:
            g = g.unsqueeze(0)
        if g.dim() != 2 or g.shape[1] != self.n_params:
            raise ValueError(f"genomes must have shape [n, {self.n_params}], got {list(g.shape)}")
        return g.contiguous()

    def add(self, genomes, objectives, behaviours=None, cells=None):
        """DeviceGridArchive.add with genomes float32 [n, n_params] (any 4-byte alignment) as the payload."""
        g = self._rows(genomes)
        return super().add(g.view(torch.uint8), objectives, behaviours, cells)

    def _out(self, n, out):
        if out is None:
            out = torch.empty((n, self.n_params), dtype=torch.float32, device=self.device)
        if (out.dtype != torch.float32 or tuple(out.shape) != (n, self.n_params) or not out.is_contiguous()
                or out.device != self.device):
            raise ValueError(f"out genomes must be contiguous float32 [{n}, {self.n_params}] on {self.device}")
        return out

    def ask(self, n, seed=0, sigma=0.1, out=None):
        """n children: each draws its parent as DeviceGridArchive.ask does (sampled_parents is the twin of both) and is
        parent + (float32)z * sigma with z ~ N(0, 1) (the reference's sigma is sqrt(0.01)).  Returns (genomes float32
        [n, n_params], parent_cell int32 [n]) on the device; `out=` (such a pair, or the genomes alone) is written in place.
        The device's draw counter advances by one per call; gaussian_children at that counter is the numpy twin.  On an
        empty archive nothing is written and check_errors() raises."""
        n = int(n)
        if n < 1:
            raise ValueError("ask() needs n >= 1")
        genomes = parent = None
        if out is not None:
            genomes, parent = out if isinstance(out, (tuple, list)) else (out, None)
        genomes = self._out(n, genomes)
        if parent is None:
            parent = torch.empty(n, dtype=torch.int32, device=self.device)
        if parent.dtype != torch.int32 or tuple(parent.shape) != (n,) or not parent.is_contiguous() or parent.device != self.device:
            raise ValueError(f"out parent_cell must be contiguous int32 [{n}] on {self.device}")
        with torch.cuda.device(self.device):
            _check(self._L.pcgrl_archive_ask_genomes(self._handle(), n, int(seed) & _M64, float(sigma), genomes.data_ptr(),
                                                     parent.data_ptr(), self._stream()), "pcgrl_archive_ask_genomes")
        return genomes, parent

    def sample(self, n, seed=0, sigma=0.1, mean=None, out=None):
        """n draws mean + (float32)z * sigma (mean float32 [n_params], zero when None): the first generation around an initial
        genome.  Works on an empty archive; advances the draw counter by one."""
        n = int(n)
        if n < 1:
            raise ValueError("sample() needs n >= 1")
        genomes = self._out(n, out)
        if mean is not None:
            mean = torch.as_tensor(mean, device=self.device)
            if mean.dtype != torch.float32 or tuple(mean.shape) != (self.n_params,):
                raise ValueError(f"mean must be float32 [{self.n_params}]")
            mean = mean.contiguous()
        with torch.cuda.device(self.device):
            _check(self._L.pcgrl_archive_sample_genomes(self._handle(), n, int(seed) & _M64, float(sigma),
                                                        mean.data_ptr() if mean is not None else None, genomes.data_ptr(),
                                                        self._stream()), "pcgrl_archive_sample_genomes")
        return genomes

    def elites(self):
        """DeviceGridArchive.elites with .genomes float32 [k, n_params] (.grids is the same storage as bytes)."""
        out = super().elites()
        out.genomes = out.grids.view(torch.float32)
        return out

    def dense(self):
        out = super().dense()
        out.genomes = out.grids.contiguous().view(torch.float32)
        return out

    def state_dict(self):
        state = super().state_dict()
        state["n_params"] = self.n_params
        return state


def genome_archive_for(evaluator_or_env, names, bins=100, device=None, n_params=None):
    """The genome archive for the behaviour characteristics `names` of an evaluator or a 2-D VecPcgrlEnv: the dims and bounds
    of archive_for, and genomes of nca.n_params(spec.n_tiles) weights -- or of `n_params` weights, as a generator's n_params
    gives them (the 3-D generator's genomes are nca3d.n_params(spec.n_tiles) long)."""
    e = evaluator_or_env
    spec = getattr(e, "spec", None)
    if spec is None or not hasattr(spec, "n_tiles") or not hasattr(spec, "cond_bounds"):
        raise TypeError(f"genome_archive_for takes an evaluator or a VecPcgrlEnv, not {type(e).__name__}: it needs the problem's "
                        "cond_bounds and tiles")
    dims, bounds = archive_shape(spec, names, bins)
    return GenomeArchive(dims, bounds, nca.n_params(spec.n_tiles) if n_params is None else int(n_params),
                         device=e.device if device is None else device)


_AGG_FIELDS = (("behaviours", torch.float64), ("objective", torch.float64), ("time_penalty", torch.int32),
               ("variance_penalty", torch.float64), ("valid", torch.uint8))


def aggregate(objective, behaviours, n_step, weight=10.0, out=None):
    """simulate's fold over seeds on the device: objective float64 [G, S], behaviours float64 [G, S, D], n_step int32 [G, S]
    (device tensors).  Returns a namespace of device tensors -- behaviours [G, D], objective [G], time_penalty int32 [G],
    variance_penalty [G], valid uint8 [G] -- as aggregated() gives them in numpy; `out=` (such a namespace) is written in
    place.  One kernel on the current stream, no host sync."""
    obj = torch.as_tensor(objective)
    if obj.device.type != "cuda":
        raise ValueError("aggregate() needs device tensors: there is no CPU fallback (aggregated is the numpy twin)")
    dev = obj.device
    if obj.dim() != 2:
        raise ValueError("objective must be [G, S]")
    G, S = obj.shape
    obj = obj.to(torch.float64).contiguous()
    beh = torch.as_tensor(behaviours, device=dev).to(torch.float64).reshape(G, S, -1).contiguous()
    D = beh.shape[2]
    ns = torch.as_tensor(n_step, device=dev).to(torch.int32).reshape(G, S).contiguous()
    shapes = {"behaviours": (G, D), "objective": (G,), "time_penalty": (G,), "variance_penalty": (G,), "valid": (G,)}
    if out is None:
        out = SimpleNamespace(**{k: torch.empty(shapes[k], dtype=dt, device=dev) for k, dt in _AGG_FIELDS})
    else:
        for k, dt in _AGG_FIELDS:
            t = getattr(out, k, None)
            if t is None or t.dtype != dt or tuple(t.shape) != shapes[k] or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"out.{k} must be contiguous {dt} {list(shapes[k])} on {dev}")
    with torch.cuda.device(dev):
        _check(_lib.lib().pcgrl_evo_aggregate(G, S, D, float(weight), obj.data_ptr(), beh.data_ptr(), ns.data_ptr(),
                                              out.behaviours.data_ptr(), out.objective.data_ptr(), out.time_penalty.data_ptr(),
                                              out.variance_penalty.data_ptr(), out.valid.data_ptr(),
                                              torch.cuda.current_stream(dev).cuda_stream), "pcgrl_evo_aggregate")
    return out


def evaluator_score(evaluator, names, **evaluate_kwargs):
    """The ready-made `score` of NcaEvolution for the evaluator classes whose evaluate() has a loss: levels ->
    (-evaluate()["loss"], behaviour(levels, names)).  An evaluator without one (the play-through games) needs a score of the
    caller's own; give it an `evaluator` attribute for the diversity bonus."""
    names = [names] if isinstance(names, str) else list(names)

    def score(levels):
        res = evaluator.evaluate(levels, **evaluate_kwargs)
        if "loss" not in res:
            raise TypeError(f"{type(evaluator).__name__}.evaluate() has no loss: write a score of your own")
        return -res["loss"], evaluator.behaviour(levels, names)

    score.evaluator = evaluator
    return score


def mc3d_holey_score(evaluator, names, holes):
    """The ready-made `score` of NcaEvolution for a Mc3dHoleyEvaluator, whose evaluate() and behaviour() take the holes of every
    level: levels [n S, Z, Y, X] -> (-evaluate(levels, holes)["loss"], the statistics `names` as behaviour).  holes is int32
    [2, 3] (all levels) or [S, 2, 3] (per seed: repeated for the n genomes, seeds fastest, as the levels are laid out) --
    the same holes generation(..., holes=) gives the generator."""
    names = [names] if isinstance(names, str) else list(names)
    evaluator.check_names(names)
    h = torch.as_tensor(holes, device=evaluator.device).to(torch.int32)
    if tuple(h.shape) != (2, 3) and (h.dim() != 3 or tuple(h.shape[1:]) != (2, 3)):
        raise ValueError(f"holes must be [2, 3] or [S, 2, 3], got {list(h.shape)}")

    def score(levels):
        hl = h
        if h.dim() == 3:
            S = h.shape[0]
            if levels.shape[0] % S:
                raise ValueError(f"{levels.shape[0]} levels are not a whole number of genomes of {S} seeds")
            hl = h.repeat(levels.shape[0] // S, 1, 1)  # [n S, 2, 3]
        res = evaluator.evaluate(levels, hl)
        beh = torch.zeros((levels.shape[0], len(names)), dtype=torch.float64, device=evaluator.device)
        for j, k in enumerate(names):
            if k != "NONE":
                beh[:, j] = res["stats"][:, evaluator.stat_keys.index(k)]
        return -res["loss"], beh

    score.evaluator = evaluator
    return score


class NcaEvolution:
    """One generation of the reference's NCA evolution on the device: generation() runs archive.ask (or sample) ->
    generator.generate -> score(levels [n S, H, W]) -> (objective [n S], behaviours [n S, D]) -> aggregate -> diversity(group=S)
    where the score's evaluator has it (no 3-D evaluator has: there is no 3-D diversity kernel, so the bonus of a 3-D
    generation is None) -> archive.add, all enqueued on the current stream with no host sync.  The buffers of the
    library calls are allocated at the first call of a given (n, S) and reused, so a later generation allocates nothing in
    the library and the whole call can be captured in a HIP graph (the evaluators' own outputs come from torch's allocator)."""

    def __init__(self, generator, score, archive, weight=10.0):
        if generator.n_params != archive.n_params:
            raise ValueError(f"the generator's genomes have {generator.n_params} weights, the archive's {archive.n_params}")
        self.generator, self.score, self.archive, self.weight = generator, score, archive, float(weight)
        self._buf = {}

    def _buffers(self, n, S):
        key = (n, S)
        if key not in self._buf:
            a, dims = self.archive, tuple(self.generator.map_shape)
            dev, D = a.device, len(a.dims)
            self._buf[key] = SimpleNamespace(
                genomes=torch.empty((n, a.n_params), dtype=torch.float32, device=dev),
                parent=torch.empty(n, dtype=torch.int32, device=dev),
                gen=SimpleNamespace(levels=torch.empty((n, S) + dims, dtype=torch.uint8, device=dev),
                                    n_step=torch.empty((n, S), dtype=torch.int32, device=dev), frames=None),
                agg=SimpleNamespace(behaviours=torch.empty((n, D), dtype=torch.float64, device=dev),
                                    objective=torch.empty(n, dtype=torch.float64, device=dev),
                                    time_penalty=torch.empty(n, dtype=torch.int32, device=dev),
                                    variance_penalty=torch.empty(n, dtype=torch.float64, device=dev),
                                    valid=torch.empty(n, dtype=torch.uint8, device=dev)))
        return self._buf[key]

    def generation(self, init_states, n, seed, sigma=0.1, first=False, mean=None, holes=None):
        """n children (first=True: samples around `mean`), each rolled out on the S init_states uint8 [S, H, W] (or
        [n, S, H, W]; with a 3-D generator [S, Z, Y, X] or [n, S, Z, Y, X]), scored, folded over its seeds and inserted.
        `holes` (a holey 3-D generator's: [2, 3] or [S, 2, 3]) is passed through to generate().
        Returns a namespace: added (the add result), aggregate,
        diversity_bonus (float64 [n], or None -- reported, not added to the objective, as in the reference), genomes,
        parent_cell (None for a first generation), levels and n_step.  The tensors are reused by the next call."""
        n = int(n)
        init = torch.as_tensor(init_states, device=self.archive.device)
        dims = tuple(self.generator.map_shape)
        S = init.shape[-len(dims) - 1]
        b = self._buffers(n, S)
        if first:
            self.archive.sample(n, seed=seed, sigma=sigma, mean=mean, out=b.genomes)
        else:
            self.archive.ask(n, seed=seed, sigma=sigma, out=(b.genomes, b.parent))
        gen = self.generator.generate(b.genomes, init, out=b.gen, **({} if holes is None else {"holes": holes}))
        levels = gen.levels.view((n * S,) + dims)
        objective, behaviours = self.score(levels)
        agg = aggregate(objective.reshape(n, S), behaviours.reshape(n, S, -1), gen.n_step, weight=self.weight, out=b.agg)
        bonus = None
        evaluator = getattr(self.score, "evaluator", None)
        if evaluator is not None and hasattr(evaluator, "diversity") and S > 1:
            bonus = evaluator.diversity(levels, group=S).diversity_bonus
        added = self.archive.add(b.genomes, agg.objective, agg.behaviours)
        return SimpleNamespace(added=added, aggregate=agg, diversity_bonus=bonus, genomes=b.genomes,
                               parent_cell=None if first else b.parent, levels=gen.levels, n_step=gen.n_step)
