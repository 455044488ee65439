"""A plain high-precision statement of the NCA generator's step and pick (control_pcgrl_amd/nca.py),
for the tile counts that have no recorded reference roll-out, and the probe set that puts exact logits in front of the pick.
nca.unpack_weights (the genome's layout) is all that is taken from the twin.  No GPU.

  logits64    one step's logits in float64: one-hot, zero padding, a cross-correlation by np.einsum in numpy's own order
  exempt      the recorder's rule of DESIGN 38.2: where the float64 argmax is not the answer whatever the float32 order
  sigmoid_cr32  the correctly rounded float32 sigmoid, by `decimal` at 60 digits
  pick_ref    the first index of the largest sigmoid_cr32
  bias_genomes, probe_vectors  genomes whose logits are exactly l3.bias, and the vectors to put there
"""
import decimal
import functools
from types import SimpleNamespace

import numpy as np

from control_pcgrl_amd import nca

F32 = np.float32
UP, DOWN = F32(np.inf), F32(-np.inf)
MARGIN, MAGNITUDE = 1e-3, 8.0  # the recorder's exemption
GAP_FLOOR = 2.0 ** -40         # below this relative gap a float32 midpoint is beyond what float64 resolves


def genomes(rng, G, T, scale=1.0):
    """random genomes of about the reference's orthogonal init's size: unit-norm rows, small biases"""
    out = np.empty((G, nca.n_params(T)), np.float32)
    for g in range(G):
        w = nca.unpack_weights(out[g], T)
        for m, fan in ((w.w1, 9 * T), (w.w2, 32), (w.w3, 32)):
            m[...] = rng.normal(0, 1.0 / np.sqrt(fan), m.shape) * 2.0
        for b in (w.b1, w.b2, w.b3):
            b[...] = rng.normal(0, 0.1, b.shape)
    return out * np.float32(scale)


def seeds(rng, lead, shape, T):
    return rng.integers(0, T, size=tuple(lead) + tuple(shape)).astype(np.uint8)


# ---- the step in float64 ----------------------------------------------------------------------------------------------------

def logits64(w, grid, T):
    """The logits of one step of the maps `grid` uint8 [..., H, W] under the flat genome `w`: float64 [..., T, H, W]."""
    p = nca.unpack_weights(w, T)
    g = np.asarray(grid)
    H, W = g.shape[-2:]
    onehot = (g[..., None, :, :] == np.arange(T).reshape((T, 1, 1))).astype(np.float64)
    padded = np.pad(onehot, [(0, 0)] * (onehot.ndim - 2) + [(1, 1), (1, 1)])
    windows = np.lib.stride_tricks.sliding_window_view(padded, (3, 3), axis=(-2, -1))  # [..., T, H, W, 3, 3]
    assert windows.shape[-5:] == (T, H, W, 3, 3)
    f64 = np.float64
    a = np.einsum("ocyx,...chwyx->...ohw", p.w1.astype(f64), windows) + p.b1.astype(f64).reshape((-1, 1, 1))
    a = np.einsum("oc,...chw->...ohw", p.w2.astype(f64), np.maximum(a, 0.0)) + p.b2.astype(f64).reshape((-1, 1, 1))
    return np.einsum("oc,...chw->...ohw", p.w3.astype(f64), np.maximum(a, 0.0)) + p.b3.astype(f64).reshape((-1, 1, 1))


def exempt(l64):
    """bool [..., H, W]: the top-two margin is below 1e-3 or a magnitude is above 8.  Elsewhere the sigmoids are far from
    saturation and apart by thousands of float32 spacings, so the float64 argmax is the answer."""
    top = np.sort(l64, axis=-3)
    return ((top[..., -1, :, :] - top[..., -2, :, :]) < MARGIN) | (np.abs(l64) > MAGNITUDE).any(axis=-3)


# ---- the pick, correctly rounded ----------------------------------------------------------------------------------------------

_CTX = decimal.Context(prec=60)


@functools.lru_cache(maxsize=None)
def _cr32(x):
    """(the float32 nearest 1 / (1 + exp(-x)), the relative gap between the nearest and the runner-up) of a Python float that
    holds a float32.  Beyond +-200 the answer is 1 or 0 with room to spare (the float32 range ends at 2^-149 = e^-103.3)."""
    if x != x:
        return F32(np.nan), 1.0
    if abs(x) > 200.0:
        return F32(1.0 if x > 0 else 0.0), 1.0
    D = decimal.Decimal
    s = _CTX.divide(D(1), _CTX.add(D(1), _CTX.exp(_CTX.minus(D(x)))))
    c = F32(float(s))  # rounded twice (to float64, then to float32): hence the neighbours
    ranked = sorted((abs(_CTX.subtract(D(float(v)), s)), float(v))
                    for v in {float(c), float(np.nextafter(c, DOWN)), float(np.nextafter(c, UP))})
    return F32(ranked[0][1]), float(_CTX.divide(_CTX.subtract(ranked[1][0], ranked[0][0]), s))


def sigmoid_cr32(x):
    """(the correctly rounded float32 sigmoid of the float32 values x, the relative gap (d2 - d1) / sigmoid between the
    distances of the runner-up and of the nearest float32): arrays of x's shape."""
    x = np.asarray(x, dtype=F32)
    pairs = [_cr32(float(v)) for v in x.ravel()]
    return (np.array([p[0] for p in pairs], F32).reshape(x.shape), np.array([p[1] for p in pairs], np.float64).reshape(x.shape))


def pick_ref(vec):
    """(the first index of the largest correctly rounded sigmoid, the smallest gap among the channels): vec float32 [..., T]"""
    s, gap = sigmoid_cr32(vec)
    return np.argmax(s, axis=-1), gap.min(axis=-1)


def kernel_pick(vec, lmax_guard=True):
    """The pick as csrc/nca/pcgrl_nca.h organises it, in numpy with the twin's sigmoid32: j = the first argmax of the logits,
    and an i < j wins if it is not skipped by `lmax - l > 1 and l < 12 and lmax > -87` (float32) and its sigmoid equals
    j's.  Returns (pick [N], skipped bool [N, T]: the channels below j that the shortcut leaves out).  lmax_guard=False drops
    the third condition: the probe set has to tell the two apart (test_probe_set_discriminates)."""
    v = np.asarray(vec, dtype=F32)
    j = np.argmax(v, axis=-1)
    lmax = np.take_along_axis(v, j[:, None], axis=-1)
    below = np.arange(v.shape[-1])[None, :] < j[:, None]
    cannot_tie = ((lmax - v) > F32(1.0)) & (v < F32(12.0)) & ((lmax > F32(-87.0)) | (not lmax_guard))
    s = nca.sigmoid32(v)
    wins = below & ~cannot_tie & (s == np.take_along_axis(s, j[:, None], axis=-1))
    return np.where(wins.any(axis=-1), np.argmax(wins, axis=-1), j), below & cannot_tie


def bias_genomes(vectors, T):
    """Genomes that are zero but for l3.bias = vectors[g]: every cell's logits are exactly that vector."""
    v = np.asarray(vectors, dtype=F32)
    assert v.ndim == 2 and v.shape[1] == T
    out = np.zeros((len(v), nca.n_params(T)), F32)
    out[:, nca.n_params(T) - T:] = v
    return out


# ---- the probe set ------------------------------------------------------------------------------------------------------------

def _step(x, n):
    """x moved by n float32 spacings (n of either sign)"""
    x = np.array(x, dtype=F32)
    for _ in range(abs(int(n))):
        x = np.nextafter(x, UP if n > 0 else DOWN)
    return x


def probe_vectors(T, rng):
    """The logit vectors put in front of the pick: a namespace of vectors float32 [N, T], family [N] (str), lo / hi int [N]
    (the indices of the two logits a pair family is about, lo < hi; -1 for the several-ties family) and edge [N] (which of
    the shortcut's thresholds an edge probe sits at: 0 `lmax - l > 1`, 1 `l < 12`, 2 `lmax > -87`; -1 elsewhere).

    A pair (a, b) has a <= b with a at the lower index, so the lower index is the answer exactly when the sigmoids tie.  At
    T > 2 the other slots hold logits below a by 1.5 to 4.5; a pair that may tie at sigmoid 0 sits at indices 0 and 1, so that
    no filler below it takes the tie."""
    pairs = []  # (family, a, b, edge)

    def add(family, a, b, edge=-1):
        for u, v in zip(np.atleast_1d(np.asarray(a, F32)), np.atleast_1d(np.asarray(b, F32))):
            assert u <= v
            pairs.append((family, u, v, edge))

    # adjacent floats
    x = np.concatenate([rng.uniform(-105, 18, 260), rng.normal(0, 2, 200), -np.logspace(-3, 2.02, 115)]).astype(F32)
    add("adjacent", x, np.nextafter(x, UP))
    for ulps in (2, 4, 16):
        x = rng.normal(0, 1, 20).astype(F32)
        add("adjacent", x, [_step(v, ulps) for v in x])
    # the shortcut's edges: each threshold from one float32 below to one above, the other two conditions held or not
    for l in np.concatenate([rng.uniform(-80, 10.5, 40), rng.uniform(-86, -84, 10), [-0.5, 0.0, 10.75]]).astype(F32):
        top = F32(l + F32(1.0))
        add("edge", [l] * 5, [_step(top, n) for n in (-2, -1, 0, 1, 2)], 0)
    for gap in (0.25, 1.0, 1.5, 3.0, 5.4, 6.0):
        for n in (-1, 0, 1):
            l = _step(12.0, n)
            add("edge", l, F32(l + F32(gap)), 1)
    for gap in (0.0, 0.5, 1.0, 1.25, 2.0, 8.0, 16.5, 17.5):
        for n in (-1, 0, 1):
            top = _step(-87.0, n)
            add("edge", F32(top - F32(gap)), top, 2)
    # the denormal band: a rival 0..3 spacings below; rivals more than 1 below that still share the float32 denormal;
    # both at or below -104 (sigmoid exactly 0), near and far
    top = rng.uniform(-104, -87, 320).astype(F32)
    add("denormal", [_step(v, -int(n)) for v, n in zip(top, rng.integers(0, 4, len(top)))], top)
    l = rng.uniform(-103.97, -103.88, 80).astype(F32)  # sigmoid in (0.5, 0.55) of 2^-149; e^(1.0005..1.05) times it is below 1.5
    add("denormal", l, (l.astype(np.float64) + rng.uniform(1.0005, 1.05, len(l))).astype(F32))
    top = rng.uniform(-103.5, -96, 80).astype(F32)  # a few denormal spacings up: rivals 1.0005..1.2 below rarely tie
    add("denormal", (top.astype(np.float64) - rng.uniform(1.0005, 1.2, len(top))).astype(F32), top)
    top = -rng.uniform(104, 140, 80).astype(F32)
    add("zero", (top.astype(np.float64) - rng.uniform(0, 30, len(top))).astype(F32), top)
    add("zero", [-1e30, -np.finfo(F32).max, -105.0, -104.0], [-104.0, -200.0, -104.0, -104.0])
    # the plateau at 1, and the two zeros
    l = rng.uniform(17.4, 60, 80).astype(F32)
    add("plateau", l, (l.astype(np.float64) + rng.uniform(0, 40, len(l))).astype(F32))
    add("plateau", [17.4, 17.4, 1e30, 88.0], [17.4, 1e30, np.finfo(F32).max, 89.5])
    add("zeros", [-0.0, 0.0], [0.0, 0.0])
    zeros = len(pairs)  # the last two are (-0.0, 0.0) and (0.0, 0.0): the second becomes (0.0, -0.0) below

    N = len(pairs)
    vectors = np.empty((N, T), F32)
    lo, hi = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for n, (_, a, b, _) in enumerate(pairs):
        i, j = (0, 1) if T == 2 or a <= -100 else sorted(rng.choice(T, 2, replace=False).tolist())
        vectors[n] = (np.float64(a) - rng.uniform(1.5, 4.5, T)).astype(F32)
        vectors[n, i], vectors[n, j], lo[n], hi[n] = a, b, i, j
    vectors[zeros - 1, hi[zeros - 1]] = F32(-0.0)
    family = [p[0] for p in pairs]
    edge = [p[3] for p in pairs]

    # several ties (T > 2): the maximum at j, a true tie at i1 < j, a near-miss at i0 < i1, a tie above j, the rest far below
    extra = []
    if T > 2:
        for top in np.concatenate([rng.normal(0, 2, 60), rng.uniform(-103, -88, 40), rng.uniform(17.4, 30, 20),
                                   rng.uniform(8, 17, 40)]).astype(F32):
            s = nca.sigmoid32(top)
            tie = top  # up to eight spacings down while the sigmoid stays the same, and the float32 below that
            for _ in range(8):
                if nca.sigmoid32(np.nextafter(tie, DOWN)) != s:
                    break
                tie = np.nextafter(tie, DOWN)
            miss = np.nextafter(tie, DOWN)
            v = (np.float64(top) - rng.uniform(1.5, 4.5, T)).astype(F32)
            j = int(rng.integers(1, T))
            v[j] = top
            if j >= 2:
                i1 = int(rng.integers(1, j))
                v[i1] = tie
                v[int(rng.integers(0, i1))] = miss
            elif rng.random() < 0.5:
                v[0] = tie
            if j + 1 < T:
                v[int(rng.integers(j + 1, T))] = top
            extra.append(v)
        for c in (0.0, -3.25, 9.5, 20.0, -95.0, -120.0):
            extra.append(np.full(T, c, F32))
    if extra:
        vectors = np.concatenate([vectors, np.stack(extra)])
        family += ["several"] * len(extra)
        edge += [-1] * len(extra)
        lo = np.concatenate([lo, np.full(len(extra), -1)])
        hi = np.concatenate([hi, np.full(len(extra), -1)])
    return SimpleNamespace(vectors=vectors, family=np.array(family), lo=lo, hi=hi, edge=np.array(edge))

