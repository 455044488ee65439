"""The quality-diversity grid archive on the device (include/pcgrl_amd_archive.h, csrc/archive/pcgrl_archive.h, DESIGN.md section
35): a MAP-Elites grid that places a batch of levels by their behaviour vectors, keeps the best of each cell, and hands out the
next generation -- parents drawn from the occupied cells, mutated -- without a host copy.  It closes the reference's evolution
loop (evo/evolve.py:1341-1355, :1426-1434; evo/optimizer.py:70-90; evo/models.py:582-587) around the evaluators of this
package: evaluate() -> behaviour() -> add() -> ask() never leaves the device.

The reference's archive classes are pyribs' and qdpy's, which are not part of it.  The rules here are this project's own,
written down in the header and restated one candidate at a time in tests/archive_rules.py; the kernels equal that restatement
bit for bit.  No parity with pyribs' placement at the last bin edge is claimed: pass `cells=` to place by a rule of your own.
The draws of ask() are a counter-based stream on the splitmix64 finaliser, published here as numpy twins (placed_cells,
sampled_parents, mutated) that the device equals bit for bit; torch's rand / randint streams are not reproduced.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib

MEASURE_NAMES = ("emptiness", "entropy", "symmetry", "symmetry-horizontal", "symmetry-vertical", "co-occurance")
MAX_AXES, MAX_CELLS, MAX_MAP_BYTES, MAX_TILES = 4, 1 << 20, 4096, 256
_GOLDEN, _CHILD, _SALT = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, 0x8CB92BA72F3D8DD7
_M64 = (1 << 64) - 1


# ---- the numpy twins: the same functions the device computes -------------------------------------------------------------

def _mix64(z):
    """splitmix64 finaliser on a uint64 array (wrapping)"""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _u01(z):
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def _base(seed, draw):
    return _mix64(np.uint64(((int(seed) & _M64) + (int(draw) & _M64) * _GOLDEN) & _M64))


def placed_cells(behaviours, dims, bounds):
    """The cell of each behaviour vector: float64 [n, D] -> int32 [n], -1 for a vector with a NaN.  Per axis, in float64:
    b = min(max(x, lo), hi); i = int(((b - lo) / (hi - lo)) * dims); i = min(i, dims - 1); the C-order flat index."""
    x = np.asarray(behaviours, dtype=np.float64)
    dims = [int(d) for d in dims]
    x = x.reshape(-1, len(dims))
    cell = np.zeros(len(x), dtype=np.int64)
    bad = np.isnan(x).any(axis=1)
    for j, d in enumerate(dims):
        lo, hi = np.float64(bounds[j][0]), np.float64(bounds[j][1])
        with np.errstate(invalid="ignore"):
            b = np.minimum(np.maximum(np.where(bad, lo, x[:, j]), lo), hi)
            i = (((b - lo) / (hi - lo)) * np.float64(d)).astype(np.int64)
        cell = cell * d + np.minimum(i, d - 1)
    return np.where(bad, -1, cell).astype(np.int32)


def sampled_parents(seed, draw, n, n_occupied):
    """The parent of each of n children at draw counter `draw`: int64 [n] indices into the occupied cells in ascending cell
    order, uniform with replacement."""
    if int(n_occupied) < 1:
        raise ValueError("no occupied cell to draw from")
    c = np.arange(int(n), dtype=np.uint64)
    with np.errstate(over="ignore"):
        r = _mix64(_base(seed, draw) ^ (c * np.uint64(_CHILD) + np.uint64(_SALT)))
    return np.minimum((_u01(r) * np.float64(int(n_occupied))).astype(np.int64), int(n_occupied) - 1)


def mutated(parent_maps, seed, draw, rate, n_tiles):
    """The children of parent_maps uint8 [n, ...] (row c the map of child c's parent) at draw counter `draw`: every byte mutates
    with probability `rate` to (t + 1 + r) % T, r uniform in [0, T - 2]; T == 1 mutates nothing."""
    p = np.ascontiguousarray(parent_maps, dtype=np.uint8)
    n, T = p.shape[0], int(n_tiles)
    flat = p.reshape(n, -1)
    if T <= 1 or flat.size == 0:
        return p.copy()
    c = np.arange(n, dtype=np.uint64)[:, None]
    k = np.arange(flat.shape[1], dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        cb = _mix64(_base(seed, draw) ^ (c * np.uint64(_CHILD) + np.uint64((2 * _SALT) & _M64)))
        q = _mix64(cb + (k + np.uint64(1)) * np.uint64(_GOLDEN))
    hit = _u01(q) < np.float64(rate)
    r = (_u01(_mix64(q ^ np.uint64(_SALT))) * np.float64(T - 1)).astype(np.int64)
    out = np.where(hit, (flat.astype(np.int64) + 1 + r) % T, flat).astype(np.uint8)
    return out.reshape(p.shape)


# ---- the device archive -----------------------------------------------------------------------------------------------------

def _check(rc, what):
    if rc != 0:
        msg = _lib.lib().pcgrl_archive_last_error().decode()
        raise (ValueError if rc == 1 else RuntimeError)(f"{what}: PCGRL_{_lib.ERRORS.get(rc, rc)}: {msg}")


class DeviceGridArchive:
    """A grid of prod(dims) cells over `bounds` ((lo, hi) per behaviour axis), one elite per cell: its objective, behaviours
    and map (uint8, map_shape, tile ids below n_tiles) in device memory.  Everything but stats(), elites(), check_errors()
    and load_state_dict() only enqueues kernels on the current stream of `device`: no host sync, no allocation inside the
    library, so add() + ask() can be captured in one HIP graph (give `out=` to ask and keep the inputs' storage)."""

    def __init__(self, dims, bounds, map_shape, n_tiles, device="cuda:0"):
        self.dims = tuple(int(d) for d in ([dims] if np.isscalar(dims) else dims))
        bounds = [tuple(float(v) for v in b) for b in bounds]
        if len(bounds) != len(self.dims):
            raise ValueError(f"{len(self.dims)} dims but {len(bounds)} bounds")
        self.bounds = tuple(bounds)
        self.map_shape = tuple(int(s) for s in ([map_shape] if np.isscalar(map_shape) else map_shape))
        self.map_bytes = int(np.prod(self.map_shape)) if self.map_shape else 0
        self.n_tiles = int(n_tiles)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("DeviceGridArchive needs a cuda device: there is no CPU fallback")
        self._L = _lib.lib()
        D = len(self.dims)
        self._h = None
        h = C.c_void_p()
        index = self.device.index if self.device.index is not None else 0
        _check(self._L.pcgrl_archive_create(
            D, (C.c_int32 * max(D, 1))(*self.dims), (C.c_double * max(D, 1))(*[b[0] for b in bounds]),
            (C.c_double * max(D, 1))(*[b[1] for b in bounds]), self.map_bytes, self.n_tiles, index, C.byref(h)),
            "pcgrl_archive_create")
        self._h = h
        self.n_cells = int(np.prod(self.dims))

    # -- plumbing
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _handle(self):
        if self._h is None:
            raise RuntimeError("DeviceGridArchive is closed")
        return self._h

    def _f64(self, x, shape):
        t = torch.as_tensor(x, device=self.device)
        if t.dtype != torch.float64:
            t = t.to(torch.float64)
        t = t.reshape(shape).contiguous()
        return t

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._L.pcgrl_archive_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter shutdown
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def state_bytes(self):
        return int(self._L.pcgrl_archive_state_bytes(self._handle()))

    # -- insertion
    def add(self, grids, objectives, behaviours=None, cells=None):
        """Inserts n candidates: grids uint8 [n, *map_shape] (any alignment), objectives [n], and behaviours [n, D] or cells
        int32 [n] (with cells the placement is skipped; behaviours, when also given, are stored with the elite).  The archive
        afterwards equals inserting them one at a time in batch order, each taking its cell if it is empty or its objective
        is strictly greater than the occupant's.  Returns device tensors: status uint8 [n] (0 not the cell's final winner, 1
        replaced an occupant, 2 took an empty cell, 3 refused: a NaN or a cell out of range -- check_errors() raises), cell
        int32 [n] (-1 when refused), counts int32 [4] (new, improved, refused, occupied after)."""
        h = self._handle()
        if behaviours is None and cells is None:
            raise ValueError("add() needs behaviours or cells")
        g = torch.as_tensor(grids, device=self.device)
        if g.dtype != torch.uint8:
            g = g.to(torch.uint8)
        if g.dim() == len(self.map_shape):
            g = g.unsqueeze(0)
        if tuple(g.shape[1:]) != self.map_shape:
            raise ValueError(f"grids must have shape [n]{list(self.map_shape)}, got {list(g.shape)}")
        g = g.contiguous()
        n = g.shape[0]
        if n < 1:
            raise ValueError("no candidates to add")
        obj = self._f64(objectives, (-1,))
        if obj.shape[0] != n:
            raise ValueError(f"{n} grids but {obj.shape[0]} objectives")
        beh = cel = None
        if behaviours is not None:
            beh = self._f64(behaviours, (-1, len(self.dims)))
            if beh.shape[0] != n:
                raise ValueError(f"{n} grids but {beh.shape[0]} behaviour vectors")
        if cells is not None:
            cel = torch.as_tensor(cells, device=self.device).to(torch.int32).reshape(-1).contiguous()
            if cel.shape[0] != n:
                raise ValueError(f"{n} grids but {cel.shape[0]} cells")
        out = SimpleNamespace(status=torch.empty(n, dtype=torch.uint8, device=self.device),
                              cell=torch.empty(n, dtype=torch.int32, device=self.device),
                              counts=torch.empty(4, dtype=torch.int32, device=self.device))
        with torch.cuda.device(self.device):
            _check(self._L.pcgrl_archive_add(h, n, g.data_ptr(), obj.data_ptr(), beh.data_ptr() if beh is not None else None,
                                             cel.data_ptr() if cel is not None else None, out.status.data_ptr(),
                                             out.cell.data_ptr(), out.counts.data_ptr(), self._stream()), "pcgrl_archive_add")
        return out

    def cell_of(self, behaviours):
        """The placement alone: int32 [n] on the device, -1 for a vector with a NaN (placed_cells is its numpy twin)."""
        beh = self._f64(behaviours, (-1, len(self.dims)))
        n = beh.shape[0]
        out = torch.empty(n, dtype=torch.int32, device=self.device)
        if n:
            with torch.cuda.device(self.device):
                _check(self._L.pcgrl_archive_cells(self._handle(), n, beh.data_ptr(), out.data_ptr(), self._stream()),
                       "pcgrl_archive_cells")
        return out

    # -- selection and mutation
    def ask(self, n, seed=0, rate=0.01, out=None):
        """n children: each draws its parent uniformly, with replacement, from the occupied cells and mutates every cell of its
        copy of the parent's map with probability `rate` (the reference's 0.01) to another tile.  Returns (grids uint8
        [n, *map_shape], parent_cell int32 [n]) on the device; `out=` (such a pair, or the grids alone) is written in place.
        The device's draw counter advances by one per call, so a captured ask draws fresh children at every replay:
        sampled_parents / mutated at that counter are the numpy twins.  On an empty archive nothing is written and
        check_errors() raises."""
        n = int(n)
        if n < 1:
            raise ValueError("ask() needs n >= 1")
        grids = parent = None
        if out is not None:
            grids, parent = out if isinstance(out, (tuple, list)) else (out, None)
        if grids is None:
            grids = torch.empty((n,) + self.map_shape, dtype=torch.uint8, device=self.device)
        if parent is None:
            parent = torch.empty(n, dtype=torch.int32, device=self.device)
        if (grids.dtype != torch.uint8 or tuple(grids.shape) != (n,) + self.map_shape or not grids.is_contiguous()
                or grids.device != self.device):
            raise ValueError(f"out grids must be contiguous uint8 [{n}]{list(self.map_shape)} on {self.device}")
        if parent.dtype != torch.int32 or tuple(parent.shape) != (n,) or not parent.is_contiguous() or parent.device != self.device:
            raise ValueError(f"out parent_cell must be contiguous int32 [{n}] on {self.device}")
        with torch.cuda.device(self.device):
            _check(self._L.pcgrl_archive_ask(self._handle(), n, int(seed) & _M64, float(rate), grids.data_ptr(),
                                             parent.data_ptr(), self._stream()), "pcgrl_archive_ask")
        return grids, parent

    # -- reading
    def stats(self, sync=True):
        """The occupied count, the maximum and minimum objective (exact) and the sum of the objectives over the occupied cells
        (float64, in the scan kernel's own fixed order).  sync=False: the float64 [4] device tensor (count, max, min, sum) with
        no host sync.  An empty archive has max -inf and min +inf."""
        t = torch.empty(4, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _check(self._L.pcgrl_archive_stats(self._handle(), t.data_ptr(), self._stream()), "pcgrl_archive_stats")
        if not sync:
            return t
        v = t.cpu().tolist()
        return SimpleNamespace(count=int(v[0]), max=v[1], min=v[2], sum=v[3], coverage=int(v[0]) / self.n_cells)

    def elites(self):
        """The elites in ascending cell order: cells int32 [k], objectives float64 [k], behaviours float64 [k, D], grids uint8
        [k, *map_shape].  Synchronises (k is read back)."""
        k = self.stats().count
        D = len(self.dims)
        out = SimpleNamespace(cells=torch.empty(k, dtype=torch.int32, device=self.device),
                              objectives=torch.empty(k, dtype=torch.float64, device=self.device),
                              behaviours=torch.empty((k, D), dtype=torch.float64, device=self.device),
                              grids=torch.empty((k,) + self.map_shape, dtype=torch.uint8, device=self.device))
        if k:
            with torch.cuda.device(self.device):
                _check(self._L.pcgrl_archive_elites(self._handle(), k, out.cells.data_ptr(), out.objectives.data_ptr(),
                                                    out.behaviours.data_ptr(), out.grids.data_ptr(), self._stream()),
                       "pcgrl_archive_elites")
        return out

    def dense(self):
        """Every cell, occupied or not, as views of one exported image: objectives float64 [cells], behaviours float64
        [cells, D], occupied uint8 [cells], grids uint8 [cells, *map_shape].  No host sync."""
        img = self.state_dict()["image"]
        n, D, L = self.n_cells, len(self.dims), self.map_bytes
        LP = (L + 15) // 16 * 16
        at = [_lib.PCGRL_ARCHIVE_HEADER_BYTES]
        for size in (n * 8, n * D * 8, n * LP):
            at.append(at[-1] + (size + 15) // 16 * 16)
        return SimpleNamespace(objectives=img[at[0]:at[0] + n * 8].view(torch.float64),
                               behaviours=img[at[1]:at[1] + n * D * 8].view(torch.float64).reshape(n, D),
                               grids=img[at[2]:at[2] + n * LP].reshape(n, LP)[:, :L].reshape((n,) + self.map_shape),
                               occupied=img[at[3]:at[3] + n])

    def check_errors(self):
        """Raises if a candidate was refused by add() (ValueError) or ask() met an empty archive (RuntimeError) since the last
        check.  Synchronises the current stream."""
        with torch.cuda.device(self.device):
            bits = self._L.pcgrl_archive_poll_error(self._handle(), self._stream())
        if bits < 0:
            raise RuntimeError("pcgrl_archive_poll_error: " + self._L.pcgrl_archive_last_error().decode())
        msgs = []
        if bits & 1:
            msgs.append("a candidate was refused (a NaN objective or behaviour, or a cell outside the grid): status 3")
        if bits & 2:
            msgs.append("ask() on an empty archive wrote nothing")
        if msgs:
            raise (RuntimeError if bits & 2 else ValueError)("archive: " + "; ".join(msgs))

    # -- the image
    def state_dict(self):
        """The whole archive as one uint8 device tensor (header: D, dims, bounds, L, T, the draw counter, a version) plus the
        shape in plain Python.  No host sync."""
        img = torch.empty(self.state_bytes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _check(self._L.pcgrl_archive_export(self._handle(), img.data_ptr(), self._stream()), "pcgrl_archive_export")
        return {"image": img, "dims": self.dims, "bounds": self.bounds, "map_shape": self.map_shape, "n_tiles": self.n_tiles}

    def load_state_dict(self, state):
        """Restores an image of state_dict().  An image of another D, dims, bounds, map length, tile count or version is refused
        (ValueError) before anything is overwritten."""
        img = torch.as_tensor(state["image"] if isinstance(state, dict) else state)
        if img.dtype != torch.uint8 or img.dim() != 1 or img.numel() < _lib.PCGRL_ARCHIVE_HEADER_BYTES:
            raise ValueError("not an archive image")
        header = img[:_lib.PCGRL_ARCHIVE_HEADER_BYTES].cpu().numpy().tobytes()
        img = img.to(self.device).contiguous()
        buf = C.create_string_buffer(header, len(header))
        with torch.cuda.device(self.device):
            _check(self._L.pcgrl_archive_import(self._handle(), img.data_ptr(), img.numel(), buf, self._stream()), "pcgrl_archive_import")
            img.record_stream(torch.cuda.current_stream(self.device))


def archive_for(evaluator_or_env, names, bins=100, device=None):
    """The archive the reference's loop builds for the behaviour characteristics `names` (evo/evolve.py:1341-1355, :1421-1434):
    `bins` cells per axis; the bounds of a statistic are the problem's cond_bounds and those of the six measure names are
    (0.0, 1.0); map_shape and n_tiles are the evaluator's.  Takes a LodeRunnerEvaluator, SmbEvaluator,
    MicrostructureEvaluator, DDaveEvaluator, MDungeonEvaluator, a 2-D VecPcgrlEnv, or a Mc3dHoleyEvaluator (its map is the
    Z * Y * X bytes of the interior; its behaviour() takes statistic names only)."""
    from .ddave import DDaveEvaluator
    from .loderunner import LodeRunnerEvaluator
    from .mc3d_holey import Mc3dHoleyEvaluator
    from .mdungeon import MDungeonEvaluator
    from .microstructure import MicrostructureEvaluator
    from .smb import SmbEvaluator
    from .vec_env import VecPcgrlEnv
    e = evaluator_or_env
    known = (LodeRunnerEvaluator, SmbEvaluator, MicrostructureEvaluator, DDaveEvaluator, MDungeonEvaluator, VecPcgrlEnv,
             Mc3dHoleyEvaluator)
    if not isinstance(e, known):
        raise TypeError(f"archive_for takes one of {[k.__name__ for k in known]}, not {type(e).__name__}: it needs the "
                        "problem's cond_bounds, map_shape and tiles")
    if isinstance(e, Mc3dHoleyEvaluator):
        names = [names] if isinstance(names, str) else list(names)
        e.check_names(names)
    elif len(e.map_shape) != 2:
        raise NotImplementedError(f"archive_for: maps of shape {tuple(e.map_shape)} -- the measures and behaviour() exist for "
                                  "2-D maps only")
    return DeviceGridArchive(*archive_shape(e.spec, names, bins), e.map_shape, e.spec.n_tiles,
                             device=e.device if device is None else device)


def archive_shape(spec, names, bins=100):
    """(dims, bounds) of archive_for: no device needed."""
    names = [names] if isinstance(names, str) else list(names)
    bc_bounds = dict(spec.cond_bounds)
    bc_bounds.update({k: (0.0, 1.0) for k in MEASURE_NAMES})
    for bc_name in names:
        if bc_name not in bc_bounds:
            raise Exception(f"Behavior characteristic / measure `{bc_name}` not found in self.bc_bounds."
                            "You probably need to specify the lower/upper bounds of this measure in prob.cond_bounds.")
    return [int(bins)] * len(names), [tuple(float(v) for v in bc_bounds[k]) for k in names]
