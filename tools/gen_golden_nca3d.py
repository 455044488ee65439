"""3-D NCA generator roll-outs, recorded from the REFERENCE's own NCA3D class on torch-CPU -> tests/golden/nca3d/*.npz (data
only), as tools/gen_golden_nca.py records the 2-D ones.

    python tools/gen_golden_nca3d.py [NAME ...]   # needs the reference tree; about twenty minutes for all eight files, most of
                                                  # it the walk over torch seeds for the 7 x 7 x 7 ones; NAME: those files alone

evo/models.py is imported under the stubs of gen_golden_nca.py.  The genomes are made by the class's own init under a fixed
torch.manual_seed and by 0, 2 and 5 calls of its mutate(); their flat vectors are get_init_weights's.  A trajectory is the
`simulate` loop of evo/evolve.py:1003-1106 written out for both representations:
  plain  (cellular3D)       the one-hot map through the net, CARepresentation.update's argmax as the whole next map
  holey  (cellular3Dholey)  the one-hot BORDERED map (the border DIRT = 1, foot and head of both holes AIR = 0, as
                            HoleyRepresentation3D.dig_holes sets them) through the net, cut_border_action_3d, the argmax as the
                            next interior; the change test is on the interior
until the map stops changing or n_step reaches n_steps - 1.  The holes of a holey file are fixed_holes(shape) and one pair of
all_holes(shape) with its entrance on each of the four side faces.

A cell whose answer hangs on torch's summation order or on the last bit of its sigmoid is EXEMPT: the logits of the
step, recomputed here in float64 on the map before the step, have a top-two margin below 1e-3 or a magnitude above 8.  A
trajectory with no exempt cell at any step is CLEAN.  A file holds few genomes (a T = 5 genome alone is 22 KB, and it is stored
flat and by layer), so that it stays below 100 KB.  Per file the script tries torch seeds in order and takes the first under
which the drawn trajectories hold at least 8 clean ones, some ending early (n_step < 9) and some running all ten steps, and
at most 2 % exempt cells; it keeps up to 8 clean ones of either kind and the first four of the others.  A seed is given up
after 12 rounds without a clean trajectory and after 20 with one kind only.  Everything is seeded and the zip members carry a
fixed date: a rerun is byte-identical.

Layout of a file (N trajectories of n genomes on D0 x D1 x D2 maps with T tiles):
  weights float32 [n, P]            get_init_weights per genome;  n_mutations int32 [n]
  l1_weight [n, 32, T, 3, 3, 3], l1_bias [n, 32], l2_weight [n, 32, 32], l2_bias [n, 32], l3_weight [n, T, 32], l3_bias [n, T]
  genome int32 [N], init uint8 [N, D0, D1, D2], frames uint8 [N, n_steps, D0, D1, D2] (interiors; rows past the end hold the
  final map), n_step int32 [N], exempt bool [N, n_steps, D0, D1, D2] (cell of the map BEFORE the step's update), clean bool [N],
  holey bool, hole_pairs int32 [K, 2, 3] (foot cells (z, y, x), bordered; K = 0 in a plain file), hole int32 [N] (the pair of
  a trajectory; 0 in a plain file), n_tiles, n_steps, torch_seed int32
"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from gen_golden_nca import reference_models  # noqa: E402
from control_pcgrl_amd.mc3d_holey import all_holes, fixed_holes  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "nca3d")
N_STEPS = 10
MARGIN, MAGNITUDE, CAP, MAX_BYTES = 1e-3, 8.0, 0.02, 100 * 1024
BORDER, EMPTY = 1, 0
WANT, KEEP_OTHER = 8, 4


def bordered(grid, holes):
    out = np.full(tuple(s + 2 for s in grid.shape), BORDER, dtype=np.int64)
    out[1:-1, 1:-1, 1:-1] = grid
    for z, y, x in holes:
        out[z, y, x] = out[z + 1, y, x] = EMPTY
    return out


def logits64(state, grid, T):
    """the net in float64 on one map (zero padding): [T, D0, D1, D2]"""
    w1, b1, w2, b2, w3, b3 = (np.asarray(state[k], dtype=np.float64) for k in ("w1", "b1", "w2", "b2", "w3", "b3"))
    D0, D1, D2 = grid.shape
    pad = np.zeros((T, D0 + 2, D1 + 2, D2 + 2))
    pad[:, 1:-1, 1:-1, 1:-1] = (np.arange(T)[:, None, None, None] == grid[None]).astype(np.float64)
    acc = np.broadcast_to(b1[:, None, None, None], (32, D0, D1, D2)).copy()
    for k0 in range(3):
        for k1 in range(3):
            for k2 in range(3):
                acc += np.einsum("oc,cdhw->odhw", w1[:, :, k0, k1, k2], pad[:, k0:k0 + D0, k1:k1 + D1, k2:k2 + D2])
    h = np.maximum(acc, 0)
    h = np.maximum(np.einsum("oc,cdhw->odhw", w2, h) + b2[:, None, None, None], 0)
    return np.einsum("oc,cdhw->odhw", w3, h) + b3[:, None, None, None]


def exempt_cells(state, seen, T, holey):
    lg = logits64(state, seen, T)
    if holey:
        lg = lg[:, 1:-1, 1:-1, 1:-1]
    lg = np.sort(lg, axis=0)
    return ((lg[-1] - lg[-2]) < MARGIN) | (np.abs(lg).max(axis=0) > MAGNITUDE)


def rollout(th, model, utils, state, init, T, holes):
    """the simulate loop; holes None is cellular3D, else cellular3Dholey"""
    holey = holes is not None
    frames = np.empty((N_STEPS,) + init.shape, dtype=np.uint8)
    exempt = np.zeros((N_STEPS,) + init.shape, dtype=bool)
    int_map = init.astype(np.int64)
    n_step, done = 0, False
    while not done:
        seen = bordered(int_map, holes) if holey else int_map  # env._get_rep_map()
        obs = utils.get_one_hot_map(seen, T)
        exempt[n_step] = exempt_cells(state, seen, T, holey)
        action, done = model(th.unsqueeze(th.Tensor(obs), 0))
        action = action[0].numpy()
        if holey:
            action = action[:, 1:-1, 1:-1, 1:-1]  # cut_border_action_3d
        next_map = action.argmax(axis=0)  # CARepresentation.update
        change = np.any(next_map != int_map)
        int_map = next_map
        frames[n_step:] = int_map
        done = done or not change or n_step >= N_STEPS - 1
        if not done:
            n_step += 1
    return frames, n_step, exempt


def genomes(th, models, T, seed, mutations):
    th.manual_seed(seed)
    out = []
    for m in mutations:
        model = models.NCA3D(T, T)
        models.set_nograd(model)
        for _ in range(m):
            model.mutate()
        w = np.asarray(models.get_init_weights(model, init=False), dtype=np.float32)
        state = {"w1": model.l1.weight.detach().numpy().copy(), "b1": model.l1.bias.detach().numpy().copy(),
                 "w2": model.l2.weight.detach().numpy().reshape(32, 32).copy(), "b2": model.l2.bias.detach().numpy().copy(),
                 "w3": model.l3.weight.detach().numpy().reshape(T, 32).copy(), "b3": model.l3.bias.detach().numpy().copy()}
        out.append((model, w, state, m))
    return out


def hole_pairs(shape):
    """fixed_holes and, from all_holes, the first pair whose entrance is on each side face: x = 0, x = X + 1, y = 0, y = Y + 1"""
    Z, Y, X = shape
    pairs = all_holes(shape)
    ent = pairs[:, 0]
    faces = (ent[:, 2] == 0, ent[:, 2] == X + 1, ent[:, 1] == 0, ent[:, 1] == Y + 1)
    picked = [pairs[np.flatnonzero(f)[len(np.flatnonzero(f)) // 3]] for f in faces]  # a third of the way into each face's run
    return np.stack([fixed_holes(shape)] + picked).astype(np.int32)


def draw(th, models, utils, T, shape, holey, torch_seed, mutations, rounds):
    """the trajectories under one torch seed, or None if they miss what the file asks for"""
    rng = np.random.default_rng(torch_seed)
    gs = genomes(th, models, T, torch_seed, mutations)
    pairs = hole_pairs(shape) if holey else np.zeros((0, 2, 3), np.int32)
    rows, n_drawn = [], 0
    kept = {"early": 0, "full": 0, "other": 0}
    ex_cells = all_cells = 0
    for rnd in range(rounds):
        for gi, (model, _, state, _) in enumerate(gs):
            init = rng.integers(0, T, size=shape).astype(np.uint8)
            hi = n_drawn % len(pairs) if holey else 0
            n_drawn += 1
            frames, n_step, exempt = rollout(th, model, utils, state, init, T, pairs[hi] if holey else None)
            clean = not exempt.any()
            kind = ("early" if n_step < N_STEPS - 1 else "full") if clean else "other"
            if kept[kind] < (WANT if clean else KEEP_OTHER):
                kept[kind] += 1
                rows.append((gi, init, frames, n_step, exempt, clean, hi))
                ex_cells += int(exempt.sum())
                all_cells += exempt.size
        if kept["early"] + kept["full"] >= WANT and kept["early"] > 0 and kept["full"] > 0:
            break
        if rnd == 11 and kept["early"] + kept["full"] == 0:  # (a genome set that is exempt somewhere on every seed)
            return None, f"kept {kept} after 12 rounds"
        if rnd == 19 and (kept["early"] == 0 or kept["full"] == 0):  # (a genome set of one kind)
            return None, f"kept {kept} after 20 rounds"
    else:
        return None, f"kept {kept}"
    share = ex_cells / all_cells
    if share > CAP:
        return None, f"exempt share {share:.4f}"
    z = {"weights": np.stack([g[1] for g in gs]), "n_mutations": np.array([g[3] for g in gs], np.int32),
         "genome": np.array([r[0] for r in rows], np.int32), "init": np.stack([r[1] for r in rows]),
         "frames": np.stack([r[2] for r in rows]), "n_step": np.array([r[3] for r in rows], np.int32),
         "exempt": np.stack([r[4] for r in rows]), "clean": np.array([r[5] for r in rows]),
         "holey": np.bool_(holey), "hole_pairs": pairs, "hole": np.array([r[6] for r in rows], np.int32),
         "n_tiles": np.int32(T), "n_steps": np.int32(N_STEPS), "torch_seed": np.int32(torch_seed)}
    for key, name in (("w1", "l1_weight"), ("b1", "l1_bias"), ("w2", "l2_weight"), ("b2", "l2_bias"), ("w3", "l3_weight"),
                      ("b3", "l3_bias")):
        z[name] = np.stack([g[2][key] for g in gs]).astype(np.float32)
    return z, f"{len(rows)} trajectories, kept {kept}, exempt share {share:.4%}"


def save(path, z):
    """np.savez_compressed with fixed member dates, so that a rerun is byte-identical"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as f:
        for name in sorted(z):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(z[name]), allow_pickle=False)
            f.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED)


# (name, T, shape, holey, mutations of the file's genomes, first torch seed)
FILES = [("nca3d_T2_3x3x3_plain", 2, (3, 3, 3), False, (0, 2, 5), 3002),
         ("nca3d_T2_5x4x3_holey", 2, (5, 4, 3), True, (0, 2, 5), 3012),
         ("nca3d_T5_3x4x5_plain_m0", 5, (3, 4, 5), False, (0,), 3050),
         ("nca3d_T5_3x4x5_plain_m2", 5, (3, 4, 5), False, (2,), 3052),
         ("nca3d_T5_3x4x5_plain_m5", 5, (3, 4, 5), False, (5,), 3055),
         ("nca3d_T5_7x7x7_holey_m0", 5, (7, 7, 7), True, (0,), 9070),
         ("nca3d_T5_7x7x7_holey_m2", 5, (7, 7, 7), True, (2,), 3072),
         ("nca3d_T5_7x7x7_holey_m5", 5, (7, 7, 7), True, (5,), 3075)]


def main():
    import torch as th
    models, utils = reference_models()
    os.makedirs(OUT, exist_ok=True)
    for name, T, shape, holey, mutations, first_seed in FILES:
        if len(sys.argv) > 1 and name not in sys.argv[1:]:  # (one file alone: python tools/gen_golden_nca3d.py NAME)
            continue
        for torch_seed in range(first_seed, first_seed + 100000, 100):
            z, note = draw(th, models, utils, T, shape, holey, torch_seed, mutations, rounds=40)
            print(f"{name} torch seed {torch_seed}: {note}", flush=True)
            if z is not None:
                break
        else:
            raise AssertionError(f"{name}: no torch seed gave the trajectories asked for")
        path = os.path.join(OUT, name + ".npz")
        save(path, z)
        size = os.path.getsize(path)
        print(f"{os.path.basename(path)}: {size} bytes", flush=True)
        assert size <= MAX_BYTES, (path, size)


if __name__ == "__main__":
    main()
