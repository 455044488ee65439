"""The 3-D NCA level generator on the device (include/pcgrl_amd_nca3d.h, csrc/nca3d/pcgrl_nca3d.h): the
roll-out of the reference's `--model NCA3D` (evo/models.py:180-219) under `--representation cellular3D` (plain) and
`cellular3Dholey` (holey; evo/evolve.py:347-361, :1003-1106) for G genomes x S seeds in one launch.  The net
Conv3d(T, 32, 3, pad 1) -> relu -> Conv3d(32, 32, 1) -> relu -> Conv3d(32, T, 1) -> sigmoid reads the one-hot map, the per-cell
first argmax is the whole next map, and that repeats until the map stops changing or n_steps steps are up.

Maps are uint8 [D0, D1, D2] (each axis 3..16) in the axis order Mc3dHoleyEvaluator takes them (Z, Y, X); kernel index
(k0, k1, k2) runs along those axes.  plain: nothing outside the map is read.  holey: the net reads the bordered map
[D0 + 2, D1 + 2, D2 + 2] -- the border holds border_tile, the four cells of the two holes empty_tile -- and only the interior is
updated, compared and handed out; border and holes never change.

As in nca.py the arithmetic is stated, and the numpy twins below ARE the statement (the kernel equals them bit for bit):
float32, every multiply and add rounded on its own, nca.sigmoid32 and the first index of the largest sigmoid, layers 2 and 3
in ascending input-channel order from the bias.  LAYER 1 IS SUMMED BY TAP, NOT BY TILE: from b1[o], for (k0, k1, k2) ascending,
the tap adds w1[o, c, k0, k1, k2] of the tile c it lies on.  (The 2-D generator sums by (tile, ky, kx); a 3-D genome's logits
are therefore not the 2-D rule along one more axis.)
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .mc3d_holey import hole_ok
from .nca import HIDDEN, MAX_STEPS, MAX_TILES, MIN_TILES, sigmoid32

MIN_AXIS, MAX_AXIS = 3, 16
ERR_TILE, ERR_NONFINITE, ERR_HOLE = 1, 2, 4
NO_TAP = 255  # the ring of a plain map: no tile, so no tap


def n_params(n_tiles):
    """P = 864 T + 32 + 1056 + 33 T: 2882 for T = 2, 5573 for T = 5, 8264 for T = 8."""
    T = int(n_tiles)
    return 27 * T * HIDDEN + HIDDEN + HIDDEN * HIDDEN + HIDDEN + T * HIDDEN + T


def _tiles_of(n_weights):
    return next((t for t in range(MIN_TILES, MAX_TILES + 1) if n_params(t) == int(n_weights)), None)


# ---- the numpy twins: the same functions the device computes ---------------------------------------------------------------

def unpack_weights(w, n_tiles):
    """A flat genome -> namespace w1 [32, T, 3, 3, 3], b1 [32], w2 [32, 32], b2 [32], w3 [T, 32], b3 [T] (float32 views, in the
    order of the reference's get_init_weights)."""
    T = int(n_tiles)
    w = np.asarray(w, dtype=np.float32)
    if w.ndim != 1 or w.shape[0] != n_params(T):
        raise ValueError(f"a 3-D genome for {T} tiles has {n_params(T)} weights, got an array of shape {list(w.shape)}")
    at, out = 0, {}
    for name, shape in (("w1", (HIDDEN, T, 3, 3, 3)), ("b1", (HIDDEN,)), ("w2", (HIDDEN, HIDDEN)), ("b2", (HIDDEN,)),
                        ("w3", (T, HIDDEN)), ("b3", (T,))):
        size = int(np.prod(shape))
        out[name] = w[at:at + size].reshape(shape)
        at += size
    return SimpleNamespace(**out)


def bordered(grid, holes, border_tile=1, empty_tile=0):
    """The map the holey net reads: grid uint8 [..., D0, D1, D2] inside a one-cell border of border_tile, with the foot cells
    holes[..., k, :] = (z, y, x) (bordered coordinates; int [2, 3] for all maps or [..., 2, 3]) and the heads at z + 1 set to
    empty_tile, as HoleyRepresentation3D.dig_holes sets them.  A hole that mc3d_holey.hole_ok rejects raises ValueError."""
    g = np.asarray(grid, dtype=np.uint8)
    if g.ndim < 3:
        raise ValueError("grid must be [..., D0, D1, D2]")
    lead, shape = g.shape[:-3], g.shape[-3:]
    h = np.broadcast_to(np.asarray(holes, dtype=np.int64), lead + (2, 3)).reshape((-1, 2, 3))
    out = np.full(lead + tuple(s + 2 for s in shape), border_tile, dtype=np.uint8)
    out[..., 1:-1, 1:-1, 1:-1] = g
    flat = out.reshape((-1,) + out.shape[-3:])
    for n in range(flat.shape[0]):
        for z, y, x in h[n]:
            if not hole_ok((z, y, x), shape):
                raise ValueError(f"the hole with foot {(int(z), int(y), int(x))} is not on a side face of a {shape} map")
            flat[n, z, y, x] = flat[n, z + 1, y, x] = empty_tile
    return out


def _relu(acc):
    return np.where(acc < 0, np.float32(0), acc)  # (a NaN stays a NaN)


def _stepped_image(w, image):
    """the step on an image with its ring: (next interior, logits) of image uint8 [..., D0 + 2, D1 + 2, D2 + 2]"""
    T = w.w3.shape[0]
    lead = image.shape[:-3]
    D0, D1, D2 = (s - 2 for s in image.shape[-3:])
    f32 = np.float32
    cell = (1, 1, 1)
    with np.errstate(over="ignore", invalid="ignore"):
        # layer 1: acc = b1[o]; for k0, k1, k2 in order: a tap that lies on a tile c adds w1[o, c, k0, k1, k2]
        acc = np.broadcast_to(w.b1.reshape((HIDDEN,) + cell), lead + (HIDDEN, D0, D1, D2)).astype(f32)
        for k0 in range(3):
            for k1 in range(3):
                for k2 in range(3):
                    tile = image[..., k0:k0 + D0, k1:k1 + D1, k2:k2 + D2]
                    hit = tile < T
                    add = np.moveaxis(w.w1[:, :, k0, k1, k2].T[np.where(hit, tile, 0)], -1, -4)  # [..., 32, D0, D1, D2]
                    acc = np.where(hit[..., None, :, :, :], acc + add, acc)
        h = _relu(acc)
        # layers 2 and 3: acc = b[o]; for c: acc = acc + (w[o, c] * h[c])
        acc = np.broadcast_to(w.b2.reshape((HIDDEN,) + cell), lead + (HIDDEN, D0, D1, D2)).astype(f32)
        for c in range(HIDDEN):
            acc = acc + (w.w2[:, c].reshape((HIDDEN,) + cell) * h[..., c:c + 1, :, :, :])
        h = _relu(acc)
        acc = np.broadcast_to(w.b3.reshape((T,) + cell), lead + (T, D0, D1, D2)).astype(f32)
        for c in range(HIDDEN):
            acc = acc + (w.w3[:, c].reshape((T,) + cell) * h[..., c:c + 1, :, :, :])
    assert acc.dtype == f32
    nxt = np.argmax(np.nan_to_num(sigmoid32(acc), nan=-1.0), axis=-4).astype(np.uint8)  # (the first index of the maximum)
    return nxt, acc


def stepped(w, grid, holes=None, n_tiles=None, border_tile=1, empty_tile=0):
    """One step of the maps `grid` uint8 [..., D0, D1, D2] (tiles below T) under the genome `w` (flat, or unpacked): returns
    (next uint8 [..., D0, D1, D2], logits float32 [..., T, D0, D1, D2]).  holes=None is the plain mode; with holes (int [2, 3]
    or [..., 2, 3]) the net reads bordered(grid, holes) and the interior alone is updated."""
    if not hasattr(w, "w1"):
        if n_tiles is None:
            raise ValueError("stepped() needs n_tiles with a flat genome")
        w = unpack_weights(w, n_tiles)
    g = np.asarray(grid, dtype=np.uint8)
    if holes is None:
        image = np.full(g.shape[:-3] + tuple(s + 2 for s in g.shape[-3:]), NO_TAP, dtype=np.uint8)
        image[..., 1:-1, 1:-1, 1:-1] = g
    else:
        image = bordered(g, holes, border_tile, empty_tile)
    return _stepped_image(w, image)


def generated(weights, init_states, holes=None, n_steps=10, n_tiles=None, border_tile=1, empty_tile=0):
    """The roll-out of every (genome, seed): weights float32 [G, P], init_states uint8 [S, D0, D1, D2] (shared) or
    [G, S, D0, D1, D2], holes None (plain) or int [2, 3] (all seeds) or [S, 2, 3].  Returns the fields of
    Nca3dGenerator.generate in numpy -- levels uint8 [G, S, D0, D1, D2], n_step int32 [G, S] (simulate's time_penalty; -1 for a
    refused pair, whose level is its init map), frames uint8 [G, S, n_steps, D0, D1, D2] (the map after every step, rows past
    the end holding the final map) -- and error_bits, the OR over the pairs of 1 (an init tile >= T), 2 (a non-finite logit)
    and 4 (a hole that hole_ok rejects)."""
    weights = np.asarray(weights, dtype=np.float32)
    if weights.ndim != 2:
        raise ValueError("weights must be [G, P]")
    G = weights.shape[0]
    init = np.asarray(init_states, dtype=np.uint8)
    if init.ndim == 4:
        init = np.broadcast_to(init, (G,) + init.shape)
    if init.ndim != 5 or init.shape[0] != G:
        raise ValueError("init_states must be [S, D0, D1, D2] or [G, S, D0, D1, D2]")
    n_steps = int(n_steps)
    if not 1 <= n_steps <= MAX_STEPS:
        raise ValueError(f"n_steps must be in [1, {MAX_STEPS}]")
    if n_tiles is None:
        n_tiles = _tiles_of(weights.shape[1])
        if n_tiles is None:
            raise ValueError(f"no tile count in [{MIN_TILES}, {MAX_TILES}] has 3-D genomes of {weights.shape[1]} weights")
    T = int(n_tiles)
    _, S = init.shape[:2]
    shape = init.shape[2:]
    bits = 0
    bad_hole = np.zeros(S, dtype=bool)
    if holes is not None:
        if not (0 <= int(border_tile) < T and 0 <= int(empty_tile) < T):
            raise ValueError(f"border_tile and empty_tile must be tiles below {T}")
        holes = np.asarray(holes, dtype=np.int64)
        if holes.shape not in ((2, 3), (S, 2, 3)):
            raise ValueError(f"holes must be [2, 3] or [{S}, 2, 3], got {list(holes.shape)}")
        holes = np.broadcast_to(holes, (S, 2, 3))
        bad_hole = np.array([not (hole_ok(h[0], shape) and hole_ok(h[1], shape)) for h in holes])
        bits |= ERR_HOLE if bad_hole.any() else 0
    levels = np.array(init, dtype=np.uint8)
    n_step = np.full((G, S), -1, dtype=np.int32)
    frames = np.repeat(levels[:, :, None], n_steps, axis=2)
    for g in range(G):
        w = unpack_weights(weights[g], T)
        bad_tile = (init[g] >= T).any(axis=(1, 2, 3))
        bits |= ERR_TILE if bad_tile.any() else 0
        live = np.flatnonzero(~bad_tile & ~bad_hole)  # the seeds still rolling
        cur = init[g][live].copy()
        for step in range(n_steps):
            if live.size == 0:
                break
            nxt, logits = stepped(w, cur, None if holes is None else holes[live], border_tile=border_tile,
                                  empty_tile=empty_tile)
            bad = ~np.isfinite(logits).all(axis=(1, 2, 3, 4))
            if bad.any():  # refused: the init map, -1, every frame the init map
                bits |= ERR_NONFINITE
                for s in live[bad]:
                    frames[g, s] = init[g, s]
                live, cur, nxt = live[~bad], cur[~bad], nxt[~bad]
            change = (nxt != cur).any(axis=(1, 2, 3))
            frames[g, live, step:] = nxt[:, None]
            done = ~change | (step >= n_steps - 1)
            levels[g, live[done]] = nxt[done]
            n_step[g, live[done]] = step
            live, cur = live[~done], nxt[~done]
    return SimpleNamespace(levels=levels, n_step=n_step, frames=frames, error_bits=bits)


# ---- the device generator -----------------------------------------------------------------------------------------------------

def _check(rc, what):
    if rc != 0:
        msg = _lib.lib().pcgrl_nca3d_last_error().decode()
        exc = ValueError if rc == 1 else (NotImplementedError if rc == 2 else RuntimeError)
        raise exc(f"{what}: PCGRL_{_lib.ERRORS.get(rc, rc)}: {msg}")


class Nca3dGenerator:
    """The roll-outs of G genomes x S seeds on maps of `map_shape` (D0, D1, D2 in 3..16; the Z, Y, X of Mc3dHoleyEvaluator) with
    n_tiles in 2..8 tile types; holey=True reads the bordered map with the holes given to generate().  generate() only enqueues
    one kernel on the current stream of `device`: no host sync and no allocation inside the library, so with `out=` it can be
    captured in a HIP graph together with the evaluator."""

    def __init__(self, n_tiles, map_shape, n_steps=10, holey=False, border_tile=1, empty_tile=0, device="cuda:0"):
        self._h = None
        self.map_shape = tuple(int(s) for s in ([map_shape] if np.isscalar(map_shape) else map_shape))
        if len(self.map_shape) != 3:
            raise ValueError(f"Nca3dGenerator: maps of shape {self.map_shape} -- 2-D maps are NcaGenerator's")
        self.n_tiles = int(n_tiles)
        self.n_steps = int(n_steps)
        if not 1 <= self.n_steps <= MAX_STEPS:
            raise ValueError(f"n_steps must be in [1, {MAX_STEPS}], got {self.n_steps}")
        self.holey, self.border_tile, self.empty_tile = bool(holey), int(border_tile), int(empty_tile)
        if self.holey and not (0 <= self.border_tile < self.n_tiles and 0 <= self.empty_tile < self.n_tiles):
            raise ValueError(f"border_tile and empty_tile must be tiles below {self.n_tiles}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("Nca3dGenerator needs a cuda device: there is no CPU fallback (nca3d.generated is the numpy twin)")
        self._L = _lib.lib()
        h = C.c_void_p()
        index = self.device.index if self.device.index is not None else 0
        _check(self._L.pcgrl_nca3d_create(self.n_tiles, *self.map_shape, index, C.byref(h)), "pcgrl_nca3d_create")
        self._h = h
        self.n_params = n_params(self.n_tiles)

    def _handle(self):
        if self._h is None:
            raise RuntimeError("Nca3dGenerator is closed")
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._L.pcgrl_nca3d_destroy(self._h)
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

    def generate(self, weights, init_states, holes=None, n_steps=None, frames=False, out=None):
        """weights float32 [G, P], init_states uint8 [S, D0, D1, D2] (shared by all genomes) or [G, S, D0, D1, D2] and, for a
        holey generator, holes int32 [2, 3] (all seeds) or [S, 2, 3] -- the entrance and exit foot cells (z, y, x) in bordered
        coordinates -- on the device.  Returns a namespace of device tensors: levels uint8 [G, S, D0, D1, D2] (the final
        interiors), n_step int32 [G, S] (simulate's time_penalty: the steps taken are n_step + 1; -1 for a refused pair, whose
        level is its init map -- check_errors() raises), frames uint8 [G, S, n_steps, D0, D1, D2] or None.  `out=` (such a
        namespace of an earlier call) is written in place."""
        h = self._handle()
        dims = self.map_shape
        n_steps = self.n_steps if n_steps is None else int(n_steps)
        if not 1 <= n_steps <= MAX_STEPS:
            raise ValueError(f"n_steps must be in [1, {MAX_STEPS}], got {n_steps}")
        if self.holey and holes is None:
            raise ValueError("a holey generator needs holes ([2, 3] or [S, 2, 3])")
        if not self.holey and holes is not None:
            raise ValueError("a plain generator takes no holes: make it with holey=True")
        w = torch.as_tensor(weights, device=self.device)
        if w.dtype != torch.float32:
            raise ValueError(f"weights must be float32, got {w.dtype}")
        if w.dim() != 2 or w.shape[1] != self.n_params:
            raise ValueError(f"weights must be [G, {self.n_params}] for {self.n_tiles} tiles (864 T + 32 + 1056 + 33 T), got "
                             f"{list(w.shape)}")
        w = w.contiguous()
        G = w.shape[0]
        init = torch.as_tensor(init_states, device=self.device)
        if init.dtype != torch.uint8:
            init = init.to(torch.uint8)
        if init.dim() not in (4, 5) or tuple(init.shape[-3:]) != dims or (init.dim() == 5 and init.shape[0] != G):
            raise ValueError(f"init_states must be [S, {dims[0]}, {dims[1]}, {dims[2]}] or [{G}, S, {dims[0]}, {dims[1]}, "
                             f"{dims[2]}], got {list(init.shape)}")
        init = init.contiguous()
        S = init.shape[-4]
        if G < 1 or S < 1:
            raise ValueError("generate() needs at least one genome and one seed")
        hp = None
        if holes is not None:
            hp = torch.as_tensor(holes, device=self.device)
            if hp.dtype != torch.int32:
                hp = hp.to(torch.int32)
            if tuple(hp.shape) not in ((2, 3), (S, 2, 3)):
                raise ValueError(f"holes must be [2, 3] or [{S}, 2, 3], got {list(hp.shape)}")
            hp = hp.contiguous()
        if out is None:
            out = SimpleNamespace(levels=torch.empty((G, S) + dims, dtype=torch.uint8, device=self.device),
                                  n_step=torch.empty((G, S), dtype=torch.int32, device=self.device),
                                  frames=(torch.empty((G, S, n_steps) + dims, dtype=torch.uint8, device=self.device)
                                          if frames else None))
        else:
            want = [("levels", (G, S) + dims, torch.uint8), ("n_step", (G, S), torch.int32)]
            if frames:
                want.append(("frames", (G, S, n_steps) + dims, torch.uint8))
            for name, shape, dtype in want:
                t = getattr(out, name, None)
                if (t is None or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()
                        or t.device != self.device):
                    raise ValueError(f"out.{name} must be contiguous {dtype} {list(shape)} on {self.device}")
        fr = out.frames if frames else None
        with torch.cuda.device(self.device):
            _check(self._L.pcgrl_nca3d_generate(h, G, S, w.data_ptr(), init.data_ptr(), int(init.dim() == 5),
                                                hp.data_ptr() if hp is not None else None,
                                                int(hp is not None and hp.dim() == 3), self.border_tile, self.empty_tile,
                                                n_steps, out.levels.data_ptr(), out.n_step.data_ptr(),
                                                fr.data_ptr() if fr is not None else None,
                                                torch.cuda.current_stream(self.device).cuda_stream), "pcgrl_nca3d_generate")
        return out

    def poll_errors(self):
        """The error bits since the last poll (1 an init tile >= T, 2 a non-finite logit, 4 a refused hole), cleared.
        Synchronises."""
        with torch.cuda.device(self.device):
            bits = self._L.pcgrl_nca3d_poll_error(self._handle(), torch.cuda.current_stream(self.device).cuda_stream)
        if bits < 0:
            raise RuntimeError("pcgrl_nca3d_poll_error: " + self._L.pcgrl_nca3d_last_error().decode())
        return int(bits)

    def check_errors(self):
        """Raises ValueError if a pair was refused since the last check (its n_step is -1).  Synchronises."""
        bits = self.poll_errors()
        msgs = []
        if bits & ERR_TILE:
            msgs.append(f"an init map holds a tile >= {self.n_tiles}")
        if bits & ERR_NONFINITE:
            msgs.append("a genome gave a non-finite logit")
        if bits & ERR_HOLE:
            msgs.append("a hole is not on a side face of the map")
        if msgs:
            raise ValueError("nca3d: " + "; ".join(msgs) + ": the pair's level is its init map and its n_step is -1")


def generator3d_for(evaluator, n_steps=10, device=None):
    """The holey generator for the levels of a Mc3dHoleyEvaluator: its tile count and map shape, DIRT as the border and AIR in
    the holes."""
    e = evaluator
    spec, shape = getattr(e, "spec", None), getattr(e, "map_shape", None)
    if spec is None or shape is None or not hasattr(spec, "n_tiles") or len(tuple(shape)) != 3:
        raise TypeError(f"generator3d_for takes a Mc3dHoleyEvaluator, not {type(e).__name__}: it needs a 3-D map_shape and "
                        "spec.n_tiles")
    tiles = list(spec.tile_types)
    return Nca3dGenerator(spec.n_tiles, tuple(shape), n_steps=n_steps, holey=True, border_tile=tiles.index("DIRT"),
                          empty_tile=tiles.index("AIR"), device=e.device if device is None else device)
