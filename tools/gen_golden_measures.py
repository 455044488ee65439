"""Level measures and pairwise Hamming diversity, recorded from the REFERENCE's own functions on the CPU
-> tests/golden/measures/{binary,sokoban,zelda}_<H>x<W>.npz (data only; sokoban's largest shape is 62 x 62, the engine's limit).

    python tools/gen_golden_measures.py     # needs the reference tree; about a minute

The reference's modules cannot be imported (evo/evolve.py pulls in ribs, qdpy, skimage, ...), so its own TEXT is evaluated at
generation time and only results are written:
  * evo/evolve.py and rl/evaluate_ctrl.py are parsed with `ast`;
  * the definitions of get_entropy, get_counts, get_emptiness, get_hor_sym, get_ver_sym, get_sym, get_co and div_calc are
    compiled into a namespace holding np, reduce, mul, ENV3D = False, CONTINUOUS = False;
  * the two assignments to diversity_bonus inside simulate (the sum over pairs / (N * N - 1), then the 10 * ... / (width *
    height) scaling) are compiled and run with final_levels, N_INIT_STATES, width, height;
  * env is a stub with env.unwrapped._prob._width / ._height and a ._prob dict of T entries.

Layout of a file (n maps of one problem and shape; the first `n_hand` are hand-built, `names` says which):
  grids uint8 [n, H, W]
  ref_emptiness, ref_entropy, ref_sym_hor, ref_sym_ver, ref_sym, ref_co  float64 [n]; ref_tile_fractions float64 [n, T]
  counts int32 [n, T], match int32 [n, 3]     the integers (tests/measures_numpy.py), whose float forms equal the ref_* above
  div_K int32 [c], div_G int32 [c], div_off int32 [c + 1], div_idx int32 [total]: diversity case i is the maps
      grids[div_idx[div_off[i]:div_off[i + 1]]] in div_G[i] consecutive groups of div_K[i]
  div_ref_score, div_ref_bonus float64 [sum G]    div_calc / diversity_bonus per group, cases and groups in order
  div_sum int64 [sum G], div_nearest, div_nearest_idx int32 [total]

The script fails unless the set tells the rules apart (check_worth): a non-wrapping co-occurance, a W * H // 2 divisor, a
K (K - 1) bonus denominator, a per-bit distance, a highest-index tie-break and a leak across a group boundary must each fail
at least one fixture.
"""
import ast
import os
import sys
from functools import reduce
from operator import mul
from types import SimpleNamespace as NS

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle", "ref_shim")):
    if p not in sys.path:
        sys.path.insert(0, p)
import measures_numpy as mn  # noqa: E402
from install import REFERENCE_ROOT  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "measures")
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (2, 7), (7, 11), (8, 8), (16, 16), (12, 40), (64, 64)]
# the engine's sokoban takes maps up to 62 x 62 (the solver's level is the map plus its border): its largest shape stands in
LARGEST = {"sokoban": (62, 62)}
N_RANDOM = {(64, 64): 20, (62, 62): 20, (12, 40): 32}  # default 48
GROUPS = [(2, 1), (2, 3), (3, 1), (3, 3), (5, 1), (5, 3), (64, 1), (64, 3), (65, 1), (65, 3), (130, 1), (130, 3)]
BC_FUNCS = ("get_entropy", "get_counts", "get_emptiness", "get_hor_sym", "get_ver_sym", "get_sym", "get_co")


def reference_functions():
    """the reference's own definitions, compiled from its text (nothing of it is written out)"""
    ns = {"np": np, "reduce": reduce, "mul": mul, "ENV3D": False, "CONTINUOUS": False}
    evolve = os.path.join(REFERENCE_ROOT, "control_pcgrl", "evo", "evolve.py")
    tree = ast.parse(open(evolve).read())
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in BC_FUNCS]
    assert {d.name for d in defs} == set(BC_FUNCS)
    exec(compile(ast.Module(body=defs, type_ignores=[]), evolve, "exec"), ns)
    ctrl = os.path.join(REFERENCE_ROOT, "control_pcgrl", "rl", "evaluate_ctrl.py")
    defs = [n for n in ast.parse(open(ctrl).read()).body if isinstance(n, ast.FunctionDef) and n.name == "div_calc"]
    assert len(defs) == 1
    exec(compile(ast.Module(body=defs, type_ignores=[]), ctrl, "exec"), ns)
    # the two assignments to diversity_bonus inside simulate (the `= None` of the else branch is not one of them)
    (simulate,) = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "simulate"]
    assigns = [n for n in ast.walk(simulate) if isinstance(n, ast.Assign) and len(n.targets) == 1
               and isinstance(n.targets[0], ast.Name) and n.targets[0].id == "diversity_bonus"
               and not (isinstance(n.value, ast.Constant) and n.value.value is None)]
    assigns.sort(key=lambda n: n.lineno)
    assert len(assigns) == 2, [n.lineno for n in assigns]
    bonus_code = compile(ast.Module(body=assigns, type_ignores=[]), evolve, "exec")

    def diversity_bonus(levels, width, height):
        loc = {"np": np, "final_levels": levels, "N_INIT_STATES": len(levels), "width": width, "height": height}
        exec(bonus_code, loc)
        return loc["diversity_bonus"]

    ns["diversity_bonus"] = diversity_bonus
    return ns


def stub_env(T, H, W):
    return NS(unwrapped=NS(_prob=NS(_width=W, _height=H, _prob={i: 1.0 / T for i in range(T)})))


def hand_maps(T, shape, rng):
    H, W = shape
    n = H * W
    maps, names = [], []

    def add(name, g):
        maps.append(np.asarray(g, dtype=np.uint8).reshape(shape))
        names.append(name)

    for t in sorted({0, 1, T - 1}):
        add(f"all-{t}", np.full(shape, t))
    # symmetric both ways: a random quarter mirrored (odd sizes keep a free middle row / column)
    q = rng.integers(0, T, size=((H + 1) // 2, (W + 1) // 2))
    top = np.concatenate([q, q[:, ::-1][:, W % 2:]], axis=1)
    add("symmetric", np.concatenate([top, top[::-1][H % 2:]], axis=0))
    add("equal-counts", np.arange(n) % T)  # as equal as n allows
    add("equal-counts-shuffled", rng.permutation(np.arange(n) % T))
    base = rng.integers(0, T, size=shape)
    add("base", base)
    last = base.copy()
    last[-1, -1] = (last[-1, -1] + 1) % T
    add("base-last-cell", last)  # differs from "base" in the very last cell only
    add("base-copy", base)  # identical maps: distance 0, a nearest tie
    if T == 8:
        add("all-7", np.full(shape, 7))  # against all-0: three differing bits per cell, distance 1 per cell
    add("rows", np.arange(H)[:, None] % T + np.zeros(shape, dtype=int))
    add("columns", np.arange(W)[None, :] % T + np.zeros(shape, dtype=int))
    add("checker", np.add.outer(np.arange(H), np.arange(W)) % 2)
    return maps, names


def random_maps(T, shape, count, rng):
    maps = []
    for i in range(count):
        kind = i % 3
        if kind == 0:
            g = rng.integers(0, T, size=shape)
        elif kind == 1:  # skewed tile frequencies
            pr = rng.dirichlet(np.full(T, 0.5))
            g = rng.choice(T, size=shape, p=pr)
        else:  # a few cells away from an earlier map: near neighbours
            g = maps[rng.integers(0, len(maps))].copy()
            for _ in range(int(rng.integers(1, 4))):
                g[rng.integers(0, shape[0]), rng.integers(0, shape[1])] = rng.integers(0, T)
        maps.append(np.asarray(g, dtype=np.uint8))
    return maps


def group_indices(n_maps, K, G, names, rng):
    """G * K indices into the file's maps.  Every group gets a map whose exact copy sits in the NEXT group and (where the pool
    allows) nowhere in its own, so that a leak across a group boundary changes `nearest`; ties come from repeated maps."""
    idx = np.empty((G, K), dtype=np.int32)
    for g in range(G):
        idx[g] = rng.choice(n_maps, size=K, replace=n_maps < K)
    if K <= 5:  # the small groups also hold the hand-built pairs
        base, last, copy = names.index("base"), names.index("base-last-cell"), names.index("base-copy")
        idx[0, :min(K, 3)] = [base, last, copy][:min(K, 3)]
    for g in range(G - 1):
        idx[g + 1, 0] = idx[g, K - 1]
    return idx.reshape(-1)


def generate(problem, shape, ref, seed):
    T = mn.N_TILES[problem]
    H, W = shape
    n = H * W
    rng = np.random.default_rng(seed)
    maps, names = hand_maps(T, shape, rng)
    n_hand = len(maps)
    maps += random_maps(T, shape, N_RANDOM.get(shape, 48), rng)
    names += ["random"] * (len(maps) - n_hand)
    grids = np.stack(maps)
    env = stub_env(T, H, W)
    out = {"grids": grids, "n_hand": np.int32(n_hand), "names": np.array(names)}
    ints = [g.astype(np.int64) for g in grids]  # the reference's int_map
    out["ref_emptiness"] = np.array([ref["get_emptiness"](g, env) for g in ints], dtype=np.float64)
    out["ref_entropy"] = np.array([ref["get_entropy"](g, env) for g in ints], dtype=np.float64)
    out["ref_sym_hor"] = np.array([ref["get_hor_sym"](g, env) for g in ints], dtype=np.float64)
    out["ref_sym_ver"] = np.array([ref["get_ver_sym"](g, env) for g in ints], dtype=np.float64)
    out["ref_sym"] = np.array([ref["get_sym"](g, env) for g in ints], dtype=np.float64)
    out["ref_co"] = np.array([ref["get_co"](g, env) for g in ints], dtype=np.float64)
    out["ref_tile_fractions"] = np.array([ref["get_counts"](g, env) for g in ints], dtype=np.float64)
    out["counts"] = mn.counts(grids, T)
    out["match"] = mn.matches(grids, T)
    # the integers' float forms ARE the reference's answers
    bc = mn.bc_from_integers(out["counts"], out["match"], H, W, T)
    for key, name in (("emptiness", "ref_emptiness"), ("entropy", "ref_entropy"), ("symmetry-horizontal", "ref_sym_hor"),
                      ("symmetry-vertical", "ref_sym_ver"), ("symmetry", "ref_sym"), ("co-occurance", "ref_co")):
        assert np.array_equal(bc[key], out[name]), (problem, shape, key)
    assert np.array_equal(mn.tile_fractions(out["counts"], n), out["ref_tile_fractions"])
    Ks, Gs, off, idx_all, score, bonus, S_all, near_all, nidx_all = [], [], [0], [], [], [], [], [], []
    for K, G in GROUPS:
        idx = group_indices(len(grids), K, G, names, rng)
        sel = grids[idx]
        for g in range(G):
            levels = [m.astype(np.int64) for m in sel[g * K:(g + 1) * K]]
            score.append(ref["div_calc"](levels))
            bonus.append(ref["diversity_bonus"](levels, W, H))
        S, near, nidx, _ = mn.diversity(sel, T, K)
        assert all(int(s) == mn.hamming_sum(sel[g * K:(g + 1) * K], T) for g, s in enumerate(S))  # the histogram identity
        Ks.append(K)
        Gs.append(G)
        off.append(off[-1] + len(idx))
        idx_all.append(idx)
        S_all.append(S)
        near_all.append(near)
        nidx_all.append(nidx)
    out.update(div_K=np.array(Ks, np.int32), div_G=np.array(Gs, np.int32), div_off=np.array(off, np.int32),
               div_idx=np.concatenate(idx_all), div_ref_score=np.array(score, np.float64),
               div_ref_bonus=np.array(bonus, np.float64), div_sum=np.concatenate(S_all),
               div_nearest=np.concatenate(near_all), div_nearest_idx=np.concatenate(nidx_all))
    # ... and the sums' float forms are the reference's
    gi = 0
    for c, (K, G) in enumerate(GROUPS):
        S = out["div_sum"][gi:gi + G]
        assert np.array_equal(mn.div_score(S, K, n), out["div_ref_score"][gi:gi + G]), (problem, shape, K)
        assert np.array_equal(mn.diversity_bonus(S, K, n), out["div_ref_bonus"][gi:gi + G]), (problem, shape, K)
        gi += G
    return out


def check_worth(files):
    """every wrong rule fails at least one fixture"""
    fails = dict.fromkeys(("co-wrap", "sym-divisor", "bonus-denominator", "per-bit", "tie-break", "group-leak"), 0)
    for (problem, shape), z in files.items():
        T = mn.N_TILES[problem]
        H, W = shape
        n = H * W
        fails["co-wrap"] += not np.array_equal(mn.matches(z["grids"], T, wrap=False)[:, 2], z["match"][:, 2])
        bad = mn.bc_from_integers(z["counts"], z["match"], H, W, T, sym_divisor=max(1, W * H // 2))
        fails["sym-divisor"] += not np.array_equal(bad["symmetry-horizontal"], z["ref_sym_hor"])
        gi = 0
        for c in range(len(z["div_K"])):
            K, G = int(z["div_K"][c]), int(z["div_G"][c])
            sel = z["grids"][z["div_idx"][z["div_off"][c]:z["div_off"][c + 1]]]
            S = z["div_sum"][gi:gi + G]
            fails["bonus-denominator"] += not np.array_equal(mn.diversity_bonus(S, K, n, denominator=K * (K - 1)),
                                                             z["div_ref_bonus"][gi:gi + G])
            want_near = z["div_nearest"][z["div_off"][c]:z["div_off"][c + 1]]
            want_idx = z["div_nearest_idx"][z["div_off"][c]:z["div_off"][c + 1]]
            if K <= 65:
                for g in range(G):
                    d_bits = mn.pairwise(sel[g * K:(g + 1) * K], T, per_bit=True)
                    fails["per-bit"] += int(d_bits.sum(dtype=np.int64)) != int(S[g])
                    d = mn.pairwise(sel[g * K:(g + 1) * K], T)
                    fails["tie-break"] += not np.array_equal(mn.nearest(d, lowest=False)[1], want_idx[g * K:(g + 1) * K])
                if G > 1:  # one group of everything: what a kernel that ignores the boundaries would see
                    leak = mn.nearest(mn.pairwise(sel, T))[0]
                    fails["group-leak"] += not np.array_equal(leak, want_near)
            gi += G
    print("fixtures failed by each wrong rule:", fails)
    missing = [k for k, v in fails.items() if v == 0]
    assert not missing, f"the fixture set does not tell these rules apart: {missing}"


def main():
    ref = reference_functions()
    os.makedirs(OUT, exist_ok=True)
    files, total = {}, 0
    for pi, problem in enumerate(sorted(mn.N_TILES)):
        for si, shape in enumerate(SHAPES):
            shape = LARGEST.get(problem, shape) if shape == (64, 64) else shape
            z = generate(problem, shape, ref, seed=1000 * pi + si)
            files[(problem, shape)] = z
            path = os.path.join(OUT, f"{problem}_{shape[0]}x{shape[1]}.npz")
            np.savez_compressed(path, **z)
            total += os.path.getsize(path)
            print(f"{os.path.basename(path)}: {len(z['grids'])} maps, {os.path.getsize(path)} bytes", flush=True)
    check_worth(files)
    assert total < 900 * 1024, total
    print("total", total, "bytes")


if __name__ == "__main__":
    main()
