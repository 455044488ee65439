"""The quality-diversity grid archive, restated one candidate at a time in plain numpy (include/pcgrl_amd_archive.h, DESIGN.md
section 35).  This file is the pin: the kernels equal it bit for bit.  It shares no code with control_pcgrl_amd/archive.py.

  place(x, dims, bounds)       the cell of one behaviour vector (None with a NaN in it)
  SeqArchive                   the archive: insert(map, objective, behaviours | cell) one candidate at a time
  SeqArchive.add(...)          a batch inserted in batch order, and the batch statuses derived from that
  batch_rule(...)              the per-cell statement of the same (max, lowest index, strict against the occupant)
  placement_values(...)        the values the placement tests use on one axis
"""
import math

import numpy as np

BOUNDS = [(0.0, 1.0), (0.0, 95.0), (-2.5, 7.0)]
DIMS = [1, 3, 100]


def placement_values(lo, hi, dims):
    """lo, hi, both nextafter neighbours of each, values outside, +-inf and every bin edge (shared with the GPU tests)"""
    lo, hi = np.float64(lo), np.float64(hi)
    v = [lo, hi, np.nextafter(lo, -np.inf), np.nextafter(lo, np.inf), np.nextafter(hi, -np.inf), np.nextafter(hi, np.inf),
         lo - 1.0, lo - 1e300, hi + 1.0, hi + 1e300, -np.inf, np.inf]
    v += [lo + np.float64(k) * (hi - lo) / np.float64(dims) for k in range(dims + 1)]
    return np.array(v, np.float64)


def place_axis(x, lo, hi, dims):
    """b = min(max(x, lo), hi); i = int(((b - lo) / (hi - lo)) * dims); i = min(i, dims - 1) -- in float64, each operation
    rounded once"""
    x, lo, hi = np.float64(x), np.float64(lo), np.float64(hi)
    b = lo if x < lo else x
    b = hi if b > hi else b
    i = int(np.float64(np.float64(np.float64(b - lo) / np.float64(hi - lo)) * np.float64(dims)))
    return min(i, int(dims) - 1)


def place(x, dims, bounds):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if np.isnan(x).any():
        return None
    cell = 0
    for j, d in enumerate(dims):
        cell = cell * int(d) + place_axis(x[j], bounds[j][0], bounds[j][1], d)
    return cell


class SeqArchive:
    def __init__(self, dims, bounds, map_shape):
        self.dims = [int(d) for d in dims]
        self.bounds = [(float(a), float(b)) for a, b in bounds]
        self.cells = int(np.prod(self.dims))
        self.map_shape = tuple(map_shape)
        self.obj = np.zeros(self.cells, np.float64)
        self.beh = np.zeros((self.cells, len(self.dims)), np.float64)
        self.flag = np.zeros(self.cells, np.uint8)
        self.maps = np.zeros((self.cells,) + self.map_shape, np.uint8)

    def copy(self):
        c = SeqArchive(self.dims, self.bounds, self.map_shape)
        c.obj, c.beh, c.flag, c.maps = self.obj.copy(), self.beh.copy(), self.flag.copy(), self.maps.copy()
        return c

    def cell_of(self, objective, behaviours=None, cell=None):
        """the cell of a candidate, None when it is refused"""
        if math.isnan(float(objective)):
            return None
        if behaviours is not None and np.isnan(np.asarray(behaviours, np.float64)).any():
            return None
        if cell is not None:
            return int(cell) if 0 <= int(cell) < self.cells else None
        return place(behaviours, self.dims, self.bounds)

    def insert(self, grid, objective, behaviours=None, cell=None):
        """'take the cell if it is empty or the candidate's objective is strictly greater than the occupant's'.  Returns
        (cell or None, took: 0 no, 1 replaced an occupant, 2 took an empty cell)"""
        c = self.cell_of(objective, behaviours, cell)
        if c is None:
            return None, 0
        o = np.float64(objective)
        if self.flag[c] and not (o > self.obj[c]):  # (-0.0 > 0.0 is False, and so is 0.0 > -0.0)
            return c, 0
        took = 1 if self.flag[c] else 2
        self.obj[c] = o
        self.beh[c] = 0.0 if behaviours is None else np.asarray(behaviours, np.float64)
        self.flag[c] = 1
        self.maps[c] = np.asarray(grid, np.uint8).reshape(self.map_shape)
        return c, took

    def add(self, grids, objectives, behaviours=None, cells=None):
        """The batch, one at a time in batch order.  status: 3 refused; for the last candidate that took a cell 2 when the cell
        was empty BEFORE the batch, else 1; 0 for everything else (a candidate that took the cell and lost it again in the same
        batch is not the cell's final winner).  counts: new, improved, refused, occupied after."""
        n = len(objectives)
        before = self.flag.copy()
        status, cell, last = np.zeros(n, np.uint8), np.full(n, -1, np.int32), {}
        for i in range(n):
            c, took = self.insert(grids[i], objectives[i], None if behaviours is None else behaviours[i],
                                  None if cells is None else cells[i])
            if c is None:
                status[i] = 3
                continue
            cell[i] = c
            if took:
                last[c] = i
        for c, i in last.items():
            status[i] = 1 if before[c] else 2
        counts = np.array([(status == 2).sum(), (status == 1).sum(), (status == 3).sum(), self.flag.sum()], np.int32)
        return status, cell, counts

    def occupied(self):
        return np.flatnonzero(self.flag).astype(np.int32)

    def stats(self):
        occ = self.occupied()
        o = self.obj[occ]
        if len(occ) == 0:
            return 0, -math.inf, math.inf, 0.0
        return len(occ), float(o.max()), float(o.min()), math.fsum(o.tolist())


def batch_rule(occupied, occupant, cells, objectives):
    """The per-cell statement: for the candidates (cells[i], objectives[i]) -- cells[i] None when refused -- against the
    occupants {cell: objective}, the winner of each cell: the maximum objective wins, among equal maxima the lowest batch
    index, and only when the cell is empty or the maximum is strictly greater than the occupant's.  Returns {cell: index}."""
    best = {}
    for i, (c, o) in enumerate(zip(cells, objectives)):
        if c is None:
            continue
        if c not in best or o > objectives[best[c]]:
            best[c] = i
    return {c: i for c, i in best.items() if not occupied.get(c, False) or objectives[i] > occupant[c]}
