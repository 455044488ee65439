"""A plain high-precision statement of the 3-D NCA generator's step (control_pcgrl_amd/nca3d.py), both
modes, with the recorder's exemption and a genome maker.  nca3d.unpack_weights (the genome's layout) is all that is taken from
the twin; the bordered map is built here on its own.  No GPU.

  logits64   one step's logits in float64: one-hot, zero padding, a cross-correlation by np.einsum in numpy's own order; with
             holes the net reads the bordered map and the interior's logits are returned
  exempt     the recorder's rule of DESIGN 38.2: where the float64 argmax is not the answer whatever the float32 order
  tap_order_layer1, tile_order_layer1   layer 1 summed in float32 in the two orders, for the genome that tells them apart
"""
import numpy as np

from control_pcgrl_amd import nca3d

F32 = np.float32
MARGIN, MAGNITUDE = 1e-3, 8.0  # the recorder's exemption


def genomes(rng, G, T, scale=1.0):
    """random genomes of about the reference's orthogonal init's size: unit-norm rows, small biases"""
    out = np.empty((G, nca3d.n_params(T)), np.float32)
    for g in range(G):
        w = nca3d.unpack_weights(out[g], T)
        for m, fan in ((w.w1, 27 * T), (w.w2, 32), (w.w3, 32)):
            m[...] = rng.normal(0, 1.0 / np.sqrt(fan), m.shape) * 2.0
        for b in (w.b1, w.b2, w.b3):
            b[...] = rng.normal(0, 0.1, b.shape)
    return out * np.float32(scale)


def seeds(rng, lead, shape, T):
    return rng.integers(0, T, size=tuple(lead) + tuple(shape)).astype(np.uint8)


def bordered64(grid, holes, border_tile=1, empty_tile=0):
    """the bordered map of one interior [D0, D1, D2], written out: the border, then foot and head of each hole"""
    g = np.asarray(grid)
    out = np.full(tuple(s + 2 for s in g.shape), border_tile, dtype=np.int64)
    out[1:-1, 1:-1, 1:-1] = g
    for z, y, x in np.asarray(holes):
        out[z, y, x] = empty_tile
        out[z + 1, y, x] = empty_tile
    return out


def logits64(w, grid, T, holes=None, border_tile=1, empty_tile=0):
    """The logits of one step of ONE map `grid` uint8 [D0, D1, D2] under the flat genome `w`: float64 [T, D0, D1, D2] (the
    interior's, in holey mode)."""
    p = nca3d.unpack_weights(w, T)
    g = np.asarray(grid).astype(np.int64) if holes is None else bordered64(grid, holes, border_tile, empty_tile)
    onehot = (g[None] == np.arange(T).reshape((T, 1, 1, 1))).astype(np.float64)
    padded = np.pad(onehot, [(0, 0), (1, 1), (1, 1), (1, 1)])
    windows = np.lib.stride_tricks.sliding_window_view(padded, (3, 3, 3), axis=(-3, -2, -1))  # [T, D0, D1, D2, 3, 3, 3]
    f64 = np.float64
    col = (-1, 1, 1, 1)
    a = np.einsum("ocijk,cdhwijk->odhw", p.w1.astype(f64), windows) + p.b1.astype(f64).reshape(col)
    a = np.einsum("oc,cdhw->odhw", p.w2.astype(f64), np.maximum(a, 0.0)) + p.b2.astype(f64).reshape(col)
    a = np.einsum("oc,cdhw->odhw", p.w3.astype(f64), np.maximum(a, 0.0)) + p.b3.astype(f64).reshape(col)
    return a if holes is None else a[:, 1:-1, 1:-1, 1:-1]


def exempt(l64):
    """bool [D0, D1, D2]: the top-two margin is below 1e-3 or a magnitude is above 8."""
    top = np.sort(l64, axis=-4)
    return ((top[..., -1, :, :, :] - top[..., -2, :, :, :]) < MARGIN) | (np.abs(l64) > MAGNITUDE).any(axis=-4)


def _layer1_f32(p, grid, order):
    """h1's pre-activation [32, D0, D1, D2] of a plain map in float32, the taps added in `order` (a list of (c, k0, k1, k2))"""
    g = np.asarray(grid)
    D0, D1, D2 = g.shape
    pad = np.full((D0 + 2, D1 + 2, D2 + 2), 255, np.uint8)
    pad[1:-1, 1:-1, 1:-1] = g
    acc = np.broadcast_to(p.b1.reshape((-1, 1, 1, 1)), (32, D0, D1, D2)).astype(F32)
    for c, k0, k1, k2 in order:
        hit = pad[k0:k0 + D0, k1:k1 + D1, k2:k2 + D2] == c
        acc = np.where(hit[None], acc + p.w1[:, c, k0, k1, k2].reshape((-1, 1, 1, 1)), acc)
    assert acc.dtype == F32
    return acc


def tap_order_layer1(w, grid, T):
    taps = [(k0, k1, k2) for k0 in range(3) for k1 in range(3) for k2 in range(3)]
    return _layer1_f32(nca3d.unpack_weights(w, T), grid, [(c, *k) for k in taps for c in range(T)])


def tile_order_layer1(w, grid, T):
    taps = [(k0, k1, k2) for k0 in range(3) for k1 in range(3) for k2 in range(3)]
    return _layer1_f32(nca3d.unpack_weights(w, T), grid, [(c, *k) for c in range(T) for k in taps])


def order_genome(T=2):
    """A genome whose layer-1 sum depends on the order: hidden unit 0 has 2^24 at tap (0, 0, 0) of tile 1, -2^24 at tap
    (1, 1, 1) of tile 1 and 1 at tap (2, 2, 2) of tile 0.  At the centre of order_map(), by tap: (2^24 - 2^24) + 1 = 1; by
    (tile, tap): tile 0's 1 first, (1 + 2^24) = 2^24 in float32 (the 1 is absorbed), then - 2^24 = 0.  Unit 0 is carried to
    logit 1 by l2 and l3, and logit 0 is 0.5 everywhere: the centre becomes tile 1 under tap order and tile 0 under the other."""
    g = np.zeros(nca3d.n_params(T), np.float32)
    w = nca3d.unpack_weights(g, T)
    w.w1[0, 1, 0, 0, 0] = 2.0 ** 24
    w.w1[0, 1, 1, 1, 1] = -(2.0 ** 24)
    w.w1[0, 0, 2, 2, 2] = 1.0
    w.w2[0, 0] = 1.0
    w.w3[1, 0] = 1.0
    w.b3[0] = 0.5
    return g


def order_map():
    """3 x 3 x 3 of tile 0 with tile 1 at the corner (0, 0, 0) and at the centre: the centre cell sees all three weights"""
    m = np.zeros((3, 3, 3), np.uint8)
    m[0, 0, 0] = m[1, 1, 1] = 1
    return m
