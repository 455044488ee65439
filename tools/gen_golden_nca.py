"""NCA generator roll-outs, recorded from the REFERENCE's own NCA class on torch-CPU -> tests/golden/nca/*.npz (data only).

    python tools/gen_golden_nca.py     # needs the reference tree; well under a minute

evo/models.py is imported as it stands; its third-party imports (cv2, einops, neat, pytorch_neat, qdpy, graphviz) and the
attention module it never uses here are stubbed in sys.modules.  The genomes are made by the class's own orthogonal init under
a fixed torch.manual_seed and by 0, 5 and 10 calls of its mutate(); their flat vectors are get_init_weights's.  A trajectory is
the `simulate` loop of evo/evolve.py for the cellular representation, written out: the one-hot map (the reference's
get_one_hot_map) through the net, CARepresentation.update's argmax as the whole next map, until the map stops changing or
n_step reaches n_steps - 1.

torch sums a convolution in an order of its own and its float32 sigmoid differs from this project's in the last bit, so a cell
whose answer hangs on that is marked EXEMPT: the logits of the step, recomputed here in float64, have a top-two margin below
1e-3 or a magnitude above 8.  A trajectory with no exempt cell at any step is CLEAN.  The script draws seeds, keeping every clean
trajectory and the first 16 of the others, until every tile
count has at least 16 clean trajectories, some ending early (n_step < 9) and some running all steps, and fails if more than
2 % of the recorded cells of a tile count are exempt.

Layout of a file (N trajectories of n genomes on H x W maps with T tiles):
  weights float32 [n, P]            get_init_weights per genome;  n_mutations int32 [n]
  l1_weight [n, 32, T, 3, 3], l1_bias [n, 32], l2_weight [n, 32, 32], l2_bias [n, 32], l3_weight [n, T, 32], l3_bias [n, T]
  genome int32 [N], init uint8 [N, H, W], frames uint8 [N, n_steps, H, W] (rows past the end hold the final map),
  n_step int32 [N], exempt bool [N, n_steps, H, W] (cell of the map BEFORE the step's update), clean bool [N],
  n_tiles, n_steps int32
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle", "ref_shim")):
    if p not in sys.path:
        sys.path.insert(0, p)
from install import REFERENCE_ROOT, _Inert  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "nca")
N_STEPS = 10
MARGIN, MAGNITUDE, CAP = 1e-3, 8.0, 0.02


def reference_models():
    """evo/models.py with its third-party imports stubbed (nothing of it is written out)"""
    import torch  # noqa: F401
    for name in ("cv2", "einops", "neat", "pytorch_neat", "pytorch_neat.cppn", "qdpy", "graphviz", "cbam"):
        m = _Inert(name)  # every attribute a harmless class
        m.__path__ = []
        sys.modules.setdefault(name, m)
    sys.modules["qdpy"].phenotype = _Inert("qdpy.phenotype")  # (a base class is taken from it)
    sys.dont_write_bytecode = True  # the reference tree is read-only
    sys.path.insert(0, os.path.join(REFERENCE_ROOT, "control_pcgrl", "evo"))
    import models
    import utils
    return models, utils


def logits64(state, grid, T):
    """the net in float64 on one map: [T, H, W]"""
    w1, b1, w2, b2, w3, b3 = (np.asarray(state[k], dtype=np.float64) for k in ("w1", "b1", "w2", "b2", "w3", "b3"))
    H, W = grid.shape
    pad = np.zeros((T, H + 2, W + 2))
    pad[:, 1:H + 1, 1:W + 1] = (np.arange(T)[:, None, None] == grid[None]).astype(np.float64)
    acc = np.broadcast_to(b1[:, None, None], (32, H, W)).copy()
    for ky in range(3):
        for kx in range(3):
            acc += np.einsum("oc,chw->ohw", w1[:, :, ky, kx], pad[:, ky:ky + H, kx:kx + W])
    h = np.maximum(acc, 0)
    h = np.maximum(np.einsum("oc,chw->ohw", w2, h) + b2[:, None, None], 0)
    return np.einsum("oc,chw->ohw", w3, h) + b3[:, None, None]


def exempt_cells(state, grid, T):
    lg = np.sort(logits64(state, grid, T), axis=0)
    return ((lg[-1] - lg[-2]) < MARGIN) | (np.abs(lg).max(axis=0) > MAGNITUDE)


def rollout(th, model, utils, state, init, T):
    """the simulate loop for the cellular representation"""
    frames = np.empty((N_STEPS,) + init.shape, dtype=np.uint8)
    exempt = np.zeros((N_STEPS,) + init.shape, dtype=bool)
    int_map = init.astype(np.int64)
    obs = utils.get_one_hot_map(int_map, T)
    n_step, done = 0, False
    while not done:
        exempt[n_step] = exempt_cells(state, int_map, T)
        action, done = model(th.unsqueeze(th.Tensor(obs), 0))
        action = action[0].numpy()
        next_map = action.argmax(axis=0)  # CARepresentation.update
        change = np.any(next_map != int_map)
        int_map = next_map
        obs = utils.get_one_hot_map(int_map, T)
        frames[n_step:] = int_map
        done = done or not change or n_step >= N_STEPS - 1
        if not done:
            n_step += 1
    return frames, n_step, exempt


def genomes(th, models, T, seed, mutations):
    th.manual_seed(seed)
    out = []
    for m in mutations:
        model = models.NCA(T, T)
        models.set_nograd(model)
        for _ in range(m):
            model.mutate()
        w = np.asarray(models.get_init_weights(model, init=False), dtype=np.float32)
        state = {"w1": model.l1.weight.detach().numpy().copy(), "b1": model.l1.bias.detach().numpy().copy(),
                 "w2": model.l2.weight.detach().numpy().reshape(32, 32).copy(), "b2": model.l2.bias.detach().numpy().copy(),
                 "w3": model.l3.weight.detach().numpy().reshape(T, 32).copy(), "b3": model.l3.bias.detach().numpy().copy()}
        out.append((model, w, state, m))
    return out


def record(th, models, utils, T, shape, seed, mutations, want_clean, max_rounds=400, keep_other=16):
    rng = np.random.default_rng(seed)
    gs = genomes(th, models, T, seed, mutations)
    rows = []
    for rnd in range(max_rounds):
        for gi, (model, _, state, _) in enumerate(gs):
            init = rng.integers(0, T, size=shape).astype(np.uint8)
            frames, n_step, exempt = rollout(th, model, utils, state, init, T)
            row = (gi, init, frames, n_step, exempt, not exempt.any())
            if row[5] or sum(not r[5] for r in rows) < keep_other:  # every clean trajectory, the first few of the others
                rows.append(row)
        clean = [r for r in rows if r[5]]
        early = sum(r[3] < N_STEPS - 1 for r in clean)
        if len(clean) >= want_clean and (want_clean < 4 or (early > 0 and early < len(clean))):
            break
    else:
        raise AssertionError(f"T={T}: {len(clean)} clean trajectories ({early} early) after {max_rounds} rounds")
    ex = np.stack([r[4] for r in rows])
    share = ex.mean()
    assert share <= CAP, f"T={T}: {share:.4f} of the recorded cells are exempt"
    z = {"weights": np.stack([g[1] for g in gs]), "n_mutations": np.array([g[3] for g in gs], np.int32),
         "genome": np.array([r[0] for r in rows], np.int32), "init": np.stack([r[1] for r in rows]),
         "frames": np.stack([r[2] for r in rows]), "n_step": np.array([r[3] for r in rows], np.int32), "exempt": ex,
         "clean": np.array([r[5] for r in rows]), "n_tiles": np.int32(T), "n_steps": np.int32(N_STEPS)}
    for key, name in (("w1", "l1_weight"), ("b1", "l1_bias"), ("w2", "l2_weight"), ("b2", "l2_bias"), ("w3", "l3_weight"),
                      ("b3", "l3_bias")):
        z[name] = np.stack([g[2][key] for g in gs]).astype(np.float32)
    print(f"T={T} {shape}: {len(rows)} trajectories, {int(z['clean'].sum())} clean ({early} early), exempt share {share:.4%}",
          flush=True)
    return z


def main():
    import torch as th
    models, utils = reference_models()
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for T, shape, seed, mutations, want in ((2, (16, 16), 2002, (0, 0, 5, 5, 10, 10), 16),
                                            (8, (16, 16), 2008, (0, 0, 5, 5, 10, 10), 16),
                                            (3, (5, 7), 2003, (5,), 3)):
        z = record(th, models, utils, T, shape, seed, mutations, want)
        path = os.path.join(OUT, f"nca_T{T}_{shape[0]}x{shape[1]}.npz")
        np.savez_compressed(path, **z)
        total += os.path.getsize(path)
        print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes", flush=True)
    assert total < 900 * 1024, total


if __name__ == "__main__":
    main()
