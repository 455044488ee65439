"""The NCA level generator on the device (include/pcgrl_amd_nca.h, csrc/nca/pcgrl_nca.h): the roll-out
of the reference's default generator -- `--model NCA --representation cellular`, evo/models.py:62-116 and the `simulate` loop of
evo/evolve.py:944-1290 -- for G genomes x S seeds in one launch.  A genome is the flat float32 vector of get_init_weights /
set_weights (evo/models.py:900-957); its net Conv2d(T, 32, 3, pad 1) -> relu -> Conv2d(32, 32, 1) -> relu -> Conv2d(32, T, 1)
-> sigmoid reads the one-hot map, the per-cell argmax is the whole next map, and that repeats until the map stops changing or
n_steps steps are up.

The dynamics are chaotic, so the arithmetic is stated, not left to a library: float32, every multiply and add rounded on its
own, a fixed summation order, and a float32 sigmoid `sigmoid32` defined with + - * / in float64 only.  The numpy twins below
ARE that statement (sigmoid32, unpack_weights, stepped, generated) and the kernel equals them bit for bit.  torch's conv2d sums
in another order and its sigmoid differs in the last bit, so no parity with torch is claimed beyond the recorded fixtures
(tests/golden/nca): every cell whose answer does not hang on torch's last bit is reproduced.
"""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib

HIDDEN = 32
MIN_TILES, MAX_TILES, MAX_SIDE, MAX_STEPS = 2, 8, 64, 1024
ERR_TILE, ERR_NONFINITE = 1, 2
_LOG2E = 1.4426950408889634
_LN2_HI = 6.93147180369123816490e-01
_LN2_LO = 1.90821492927058770002e-10
_INV_FACT = [1.0 / math.factorial(n) for n in range(14)]


def n_params(n_tiles):
    """P = 288 T + 32 + 1056 + 33 T: 1730 for T = 2, 3656 for T = 8."""
    T = int(n_tiles)
    return 9 * T * HIDDEN + HIDDEN + HIDDEN * HIDDEN + HIDDEN + T * HIDDEN + T


# ---- the numpy twins: the same functions the device computes ---------------------------------------------------------------

def sigmoid32(x):
    """This project's float32 sigmoid: float32 in, float32 out, every step one float64 + - * / (or an exact scaling).
    a = min(|x|, 104); z = -a; k = rint(z * log2(e)); r = (z - k * ln2_hi) - k * ln2_lo; p = the degree-13 Taylor polynomial
    of exp(r) by Horner; t = p * 2^k; s = 1 / (1 + t) for x >= 0, else t / (1 + t); the result is s rounded to float32.
    NaN gives NaN."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        a = np.minimum(np.abs(x), 104.0)
        z = -a
        k = np.rint(z * _LOG2E)
        r = (z - k * _LN2_HI) - k * _LN2_LO
        p = np.full_like(r, _INV_FACT[13])
        for n in range(12, -1, -1):
            p = p * r + _INV_FACT[n]
        t = np.ldexp(p, np.where(np.isnan(k), 0, k).astype(np.int32))
        s = np.where(x >= 0, 1.0, t) / (1.0 + t)
    return s.astype(np.float32)


def unpack_weights(w, n_tiles):
    """A flat genome -> namespace w1 [32, T, 3, 3], b1 [32], w2 [32, 32], b2 [32], w3 [T, 32], b3 [T] (float32 views, in the
    order of the reference's get_init_weights)."""
    T = int(n_tiles)
    w = np.asarray(w, dtype=np.float32)
    if w.ndim != 1 or w.shape[0] != n_params(T):
        raise ValueError(f"a genome for {T} tiles has {n_params(T)} weights, got an array of shape {list(w.shape)}")
    at, out = 0, {}
    for name, shape in (("w1", (HIDDEN, T, 3, 3)), ("b1", (HIDDEN,)), ("w2", (HIDDEN, HIDDEN)), ("b2", (HIDDEN,)),
                        ("w3", (T, HIDDEN)), ("b3", (T,))):
        size = int(np.prod(shape))
        out[name] = w[at:at + size].reshape(shape)
        at += size
    return SimpleNamespace(**out)


def _relu(acc):
    return np.where(acc < 0, np.float32(0), acc)  # (a NaN stays a NaN)


def stepped(w, grid, n_tiles=None):
    """One step of the maps `grid` uint8 [..., H, W] (tiles below T) under the genome `w` (flat, or unpacked): returns
    (next uint8 [..., H, W], logits float32 [..., T, H, W]).  The next tile of a cell is the first index at which
    sigmoid32(logit) is largest."""
    if not hasattr(w, "w1"):
        if n_tiles is None:
            raise ValueError("stepped() needs n_tiles with a flat genome")
        w = unpack_weights(w, n_tiles)
    T = w.w3.shape[0]
    g = np.asarray(grid, dtype=np.uint8)
    H, W = g.shape[-2:]
    lead = g.shape[:-2]
    f32 = np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        # layer 1: acc = b1[o]; for c, ky, kx in order: a tap inside the map that holds tile c adds w1[o, c, ky, kx]
        pad = np.full(lead + (H + 2, W + 2), 255, dtype=np.uint8)
        pad[..., 1:H + 1, 1:W + 1] = g
        acc = np.broadcast_to(w.b1.reshape((HIDDEN, 1, 1)), lead + (HIDDEN, H, W)).astype(f32)
        for c in range(T):
            for ky in range(3):
                for kx in range(3):
                    hit = (pad[..., ky:ky + H, kx:kx + W] == c)[..., None, :, :]
                    acc = np.where(hit, acc + w.w1[:, c, ky, kx].reshape((HIDDEN, 1, 1)), acc)
        h = _relu(acc)
        # layers 2 and 3: acc = b[o]; for c: acc = acc + (w[o, c] * h[c])
        acc = np.broadcast_to(w.b2.reshape((HIDDEN, 1, 1)), lead + (HIDDEN, H, W)).astype(f32)
        for c in range(HIDDEN):
            acc = acc + (w.w2[:, c].reshape((HIDDEN, 1, 1)) * h[..., c:c + 1, :, :])
        h = _relu(acc)
        acc = np.broadcast_to(w.b3.reshape((T, 1, 1)), lead + (T, H, W)).astype(f32)
        for c in range(HIDDEN):
            acc = acc + (w.w3[:, c].reshape((T, 1, 1)) * h[..., c:c + 1, :, :])
    assert acc.dtype == f32
    nxt = np.argmax(np.nan_to_num(sigmoid32(acc), nan=-1.0), axis=-3).astype(np.uint8)  # (the first index of the maximum)
    return nxt, acc


def generated(weights, init_states, n_steps=10, n_tiles=None):
    """The roll-out of every (genome, seed): weights float32 [G, P], init_states uint8 [S, H, W] (shared) or [G, S, H, W].
    Returns the fields of NcaGenerator.generate in numpy -- levels uint8 [G, S, H, W], n_step int32 [G, S] (simulate's
    time_penalty; -1 for a refused pair, whose level is its init map), frames uint8 [G, S, n_steps, H, W] (the map after every
    step, rows past the end holding the final map) -- and error_bits, the OR over the pairs of 1 (an init tile >= T) and 2 (a
    non-finite logit)."""
    weights = np.asarray(weights, dtype=np.float32)
    if weights.ndim != 2:
        raise ValueError("weights must be [G, P]")
    G = weights.shape[0]
    init = np.asarray(init_states, dtype=np.uint8)
    if init.ndim == 3:
        init = np.broadcast_to(init, (G,) + init.shape)
    if init.ndim != 4 or init.shape[0] != G:
        raise ValueError("init_states must be [S, H, W] or [G, S, H, W]")
    n_steps = int(n_steps)
    if not 1 <= n_steps <= MAX_STEPS:
        raise ValueError(f"n_steps must be in [1, {MAX_STEPS}]")
    if n_tiles is None:
        n_tiles = next((t for t in range(MIN_TILES, MAX_TILES + 1) if n_params(t) == weights.shape[1]), None)
        if n_tiles is None:
            raise ValueError(f"no tile count in [{MIN_TILES}, {MAX_TILES}] has genomes of {weights.shape[1]} weights")
    T = int(n_tiles)
    _, S, H, W = init.shape
    levels = np.array(init, dtype=np.uint8)
    n_step = np.full((G, S), -1, dtype=np.int32)
    frames = np.repeat(levels[:, :, None], n_steps, axis=2)
    bits = 0
    for g in range(G):
        w = unpack_weights(weights[g], T)
        bad_tile = (init[g] >= T).any(axis=(1, 2))
        bits |= ERR_TILE if bad_tile.any() else 0
        live = np.flatnonzero(~bad_tile)  # the seeds still rolling
        cur = init[g][live].copy()
        for step in range(n_steps):
            if live.size == 0:
                break
            nxt, logits = stepped(w, cur)
            bad = ~np.isfinite(logits).all(axis=(1, 2, 3))
            if bad.any():  # refused: the init map, -1, every frame the init map
                bits |= ERR_NONFINITE
                for s in live[bad]:
                    frames[g, s] = init[g, s]
                live, cur, nxt = live[~bad], cur[~bad], nxt[~bad]
            change = (nxt != cur).any(axis=(1, 2))
            frames[g, live, step:] = nxt[:, None]
            done = ~change | (step >= n_steps - 1)
            levels[g, live[done]] = nxt[done]
            n_step[g, live[done]] = step
            live, cur = live[~done], nxt[~done]
    return SimpleNamespace(levels=levels, n_step=n_step, frames=frames, error_bits=bits)


# ---- the device generator -----------------------------------------------------------------------------------------------------

def _check(rc, what):
    if rc != 0:
        msg = _lib.lib().pcgrl_nca_last_error().decode()
        exc = ValueError if rc == 1 else (NotImplementedError if rc == 2 else RuntimeError)
        raise exc(f"{what}: PCGRL_{_lib.ERRORS.get(rc, rc)}: {msg}")


class NcaGenerator:
    """The roll-outs of G genomes x S seeds on maps of `map_shape` (H, W in 1..64) with n_tiles in 2..8 tile types.
    generate() only enqueues one kernel on the current stream of `device`: no host sync and no allocation inside the library, so
    with `out=` it can be captured in a HIP graph together with the evaluators."""

    def __init__(self, n_tiles, map_shape, n_steps=10, device="cuda:0", n_aux_chan=0):
        self._h = None
        if int(n_aux_chan) > 0:
            raise NotImplementedError("NcaGenerator: auxiliary channels (n_aux_chan > 0) are not built -- the auxiliary state "
                                      "would have to be an input for a roll-out to be testable step by step")
        self.map_shape = tuple(int(s) for s in ([map_shape] if np.isscalar(map_shape) else map_shape))
        if len(self.map_shape) != 2:
            raise NotImplementedError(f"NcaGenerator: maps of shape {self.map_shape} -- the 3-D generator (NCA3D) is not built")
        self.n_tiles = int(n_tiles)
        self.n_steps = int(n_steps)
        if not 1 <= self.n_steps <= MAX_STEPS:
            raise ValueError(f"n_steps must be in [1, {MAX_STEPS}], got {self.n_steps}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("NcaGenerator needs a cuda device: there is no CPU fallback (nca.generated is the numpy twin)")
        self._L = _lib.lib()
        h = C.c_void_p()
        index = self.device.index if self.device.index is not None else 0
        _check(self._L.pcgrl_nca_create(self.n_tiles, self.map_shape[0], self.map_shape[1], index, C.byref(h)),
               "pcgrl_nca_create")
        self._h = h
        self.n_params = n_params(self.n_tiles)

    def _handle(self):
        if self._h is None:
            raise RuntimeError("NcaGenerator is closed")
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._L.pcgrl_nca_destroy(self._h)
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

    def generate(self, weights, init_states, n_steps=None, frames=False, out=None):
        """weights float32 [G, P] and init_states uint8 [S, H, W] (shared by all genomes) or [G, S, H, W], on the device.
        Returns a namespace of device tensors: levels uint8 [G, S, H, W] (the final maps), n_step int32 [G, S] (simulate's
        time_penalty: the steps taken are n_step + 1; -1 for a refused pair, whose level is its init map -- check_errors()
        raises), frames uint8 [G, S, n_steps, H, W] or None.  `out=` (such a namespace of an earlier call) is written in place.
        """
        h = self._handle()
        H, W = self.map_shape
        n_steps = self.n_steps if n_steps is None else int(n_steps)
        if not 1 <= n_steps <= MAX_STEPS:
            raise ValueError(f"n_steps must be in [1, {MAX_STEPS}], got {n_steps}")
        w = torch.as_tensor(weights, device=self.device)
        if w.dtype != torch.float32:
            raise ValueError(f"weights must be float32, got {w.dtype}")
        if w.dim() != 2 or w.shape[1] != self.n_params:
            raise ValueError(f"weights must be [G, {self.n_params}] for {self.n_tiles} tiles (288 T + 32 + 1056 + 33 T), got "
                             f"{list(w.shape)}")
        w = w.contiguous()
        G = w.shape[0]
        init = torch.as_tensor(init_states, device=self.device)
        if init.dtype != torch.uint8:
            init = init.to(torch.uint8)
        if init.dim() not in (3, 4) or tuple(init.shape[-2:]) != (H, W) or (init.dim() == 4 and init.shape[0] != G):
            raise ValueError(f"init_states must be [S, {H}, {W}] or [{G}, S, {H}, {W}], got {list(init.shape)}")
        init = init.contiguous()
        S = init.shape[-3]
        if G < 1 or S < 1:
            raise ValueError("generate() needs at least one genome and one seed")
        if out is None:
            out = SimpleNamespace(levels=torch.empty((G, S, H, W), dtype=torch.uint8, device=self.device),
                                  n_step=torch.empty((G, S), dtype=torch.int32, device=self.device),
                                  frames=(torch.empty((G, S, n_steps, H, W), dtype=torch.uint8, device=self.device)
                                          if frames else None))
        else:
            want = [("levels", (G, S, H, W), torch.uint8), ("n_step", (G, S), torch.int32)]
            if frames:
                want.append(("frames", (G, S, n_steps, H, W), torch.uint8))
            for name, shape, dtype in want:
                t = getattr(out, name, None)
                if (t is None or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()
                        or t.device != self.device):
                    raise ValueError(f"out.{name} must be contiguous {dtype} {list(shape)} on {self.device}")
        fr = out.frames if frames else None
        with torch.cuda.device(self.device):
            _check(self._L.pcgrl_nca_generate(h, G, S, w.data_ptr(), init.data_ptr(), int(init.dim() == 4), n_steps,
                                              out.levels.data_ptr(), out.n_step.data_ptr(),
                                              fr.data_ptr() if fr is not None else None,
                                              torch.cuda.current_stream(self.device).cuda_stream), "pcgrl_nca_generate")
        return out

    def poll_errors(self):
        """The error bits since the last poll (1 an init tile >= T, 2 a non-finite logit), cleared.  Synchronises."""
        with torch.cuda.device(self.device):
            bits = self._L.pcgrl_nca_poll_error(self._handle(), torch.cuda.current_stream(self.device).cuda_stream)
        if bits < 0:
            raise RuntimeError("pcgrl_nca_poll_error: " + self._L.pcgrl_nca_last_error().decode())
        return int(bits)

    def check_errors(self):
        """Raises ValueError if a pair was refused since the last check (its n_step is -1).  Synchronises."""
        bits = self.poll_errors()
        msgs = []
        if bits & ERR_TILE:
            msgs.append(f"an init map holds a tile >= {self.n_tiles}")
        if bits & ERR_NONFINITE:
            msgs.append("a genome gave a non-finite logit")
        if msgs:
            raise ValueError("nca: " + "; ".join(msgs) + ": the pair's level is its init map and its n_step is -1")


def generator_for(evaluator_or_env, n_steps=10, device=None):
    """The generator for the maps of an evaluator or a 2-D VecPcgrlEnv: its tile count and map shape, as archive_for takes
    them."""
    e = evaluator_or_env
    spec, shape = getattr(e, "spec", None), getattr(e, "map_shape", None)
    if spec is None or shape is None or not hasattr(spec, "n_tiles"):
        raise TypeError(f"generator_for takes an evaluator or a VecPcgrlEnv, not {type(e).__name__}: it needs map_shape and "
                        "spec.n_tiles")
    return NcaGenerator(spec.n_tiles, tuple(shape), n_steps=n_steps, device=e.device if device is None else device)
