#!/usr/bin/env python3
"""A CPU model of the path sweeps of the binary 16x16 step kernel (csrc/step16/): how many trips of six BFS levels the
simulate waves of a launch run, and what that costs for a given price of a trip and of a sweep.  numpy only, no GPU.

  python tools/step16_chain_model.py [--overhead 90] [--fixed 380] [--envs 4096] [--launches 12] [--seed 0]

Setup.  Maps are iid uniform binary 16x16 (True = passable); in half of the envs one cell is flipped: the stationary state
of the headline workload under uniform random actions.  An env whose map changed re-sweeps the component(s) K that touch the
edited cell (component_fars16): the pieces of K in row-major order of their first cell, a level-synchronous BFS from that
cell each, the far cell being the first cell in row-major order of the last level; isolated cells need no sweep.  Then one
more sweep (the second sweep) from the new far cells -- from all far cells of the map when the edit touched a component that
held the longest path -- gives the path length.  A sweep of L levels takes L // 6 + 1 trips.  The four envs of a wave run in
lockstep: sweep i of the wave runs as many trips as its longest i-th piece needs (an env without an i-th piece idles), and a
wave in which no map changed sweeps nothing.

Costing.  A sweep costs trips * (144 + overhead) + fixed cycles: 144 for the 36 level instructions, `overhead` for the
trip's control, `fixed` for the sweep's header and wrap-up.  Printed: the cost of the slowest wave of a launch (mean over
the launches) and of the mean wave.

Simplification: which of several components that tie for the longest path the kernel's `best` mask marks depends on the
history; the model takes an edit to hit `best` when it touches ANY of them."""
import argparse
import json

import numpy as np

H = W = 16
LEVELS_PER_TRIP = 6
LEVEL_CYCLES = 144  # the 36 level instructions of a trip (the phase table's cycles over the trips run)


def neighbours(f):
    p = np.zeros((len(f), H + 2, W + 2), bool)
    p[:, 1:-1, 1:-1] = f
    return p[:, :-2, 1:-1] | p[:, 2:, 1:-1] | p[:, 1:-1, :-2] | p[:, 1:-1, 2:]


def first_rowmajor(x):
    """the first cell of x in row-major order per env (nothing where x is empty)"""
    flat = x.reshape(len(x), -1)
    out = np.zeros_like(flat)
    has = flat.any(axis=1)
    out[has, flat.argmax(axis=1)[has]] = True
    return out.reshape(x.shape)


def sweep(src, avail):
    """level-synchronous BFS per env -> (levels [n], last non-empty level [n, 16, 16] (the sources where levels == 0), reached)"""
    front = src & avail
    reached, last = front.copy(), front.copy()
    levels = np.zeros(len(src), np.int64)
    while True:
        front = neighbours(front) & avail & ~reached
        alive = front.any(axis=(1, 2))
        if not alive.any():
            return levels, last, reached
        levels += alive
        last[alive] = front[alive]
        reached |= front


def first_sweeps(cells):
    """component_fars16 on `cells` [n, 16, 16].  Returns (fars [n, 16, 16], pieces): pieces is a list over sweep rounds of
    (has [n] bool, first cell [n] flat index, far cell [n] flat index, levels [n]) -- round i holds every env's i-th piece"""
    fars = cells & ~neighbours(cells)
    remaining = cells & ~fars
    pieces = []
    while remaining.any():
        has = remaining.any(axis=(1, 2))
        seed = first_rowmajor(remaining)
        levels, last, reached = sweep(seed, remaining)
        far = first_rowmajor(last) & has[:, None, None]
        fars |= far
        pieces.append((has, seed.reshape(len(cells), -1).argmax(1), far.reshape(len(cells), -1).argmax(1), np.where(has, levels, 0)))
        remaining &= ~reached
    return fars, pieces


def second_sweep_levels(passable, fars):
    """per cell the level of the BFS from its component's far cell (-1: not reached)"""
    level = np.full(passable.shape, -1, np.int64)
    front = fars & passable
    k = 0
    while front.any():
        level[front] = k
        front = neighbours(front) & passable & (level < 0)
        k += 1
    return level


def trips_of(levels):
    return levels // LEVELS_PER_TRIP + 1


def launch(n, rng):
    """one launch of n envs -> (first [rounds, n] trips of each env's i-th first sweep (0: none), second [n] trips of the
    second sweep, changed [n])"""
    old = rng.random((n, H, W)) < 0.5
    changed = rng.random(n) < 0.5
    x = np.zeros((n, H, W), bool)
    x[np.arange(n), rng.integers(0, H, n), rng.integers(0, W, n)] = True
    x &= changed[:, None, None]
    new = old ^ x
    became = (x & new).any(axis=(1, 2))
    K = sweep(x, np.where(became[:, None, None], new, old))[2]
    K &= ~(x & ~became[:, None, None])
    touched = K | x
    # the state before the edit: far cells of every component, the longest second sweep and the components that reach it
    fars_old, _ = first_sweeps(old)
    lev_old = second_sweep_levels(old, fars_old)
    longest = lev_old.max(axis=(1, 2)).clip(min=0)
    best = sweep(lev_old == longest[:, None, None], old)[2] & (longest > 0)[:, None, None]
    hit = (best & touched).any(axis=(1, 2))
    newfars, pieces = first_sweeps(K)
    first = np.zeros((len(pieces), n), np.int64)
    for i, (has, _, _, levels) in enumerate(pieces):
        first[i] = np.where(has, trips_of(levels), 0)
    fars = (fars_old & ~touched) | newfars
    src = np.where(hit[:, None, None], fars, newfars)
    second = np.where(changed, trips_of(sweep(src, new)[0]), 0)
    return first, second, changed


def wave_trips(first, second, changed, envs_per_wave=4):
    """lockstep: per wave the trips of every sweep it runs -> (trips [waves], sweeps [waves])"""
    n = len(changed)
    assert n % envs_per_wave == 0
    w = n // envs_per_wave
    any_change = changed.reshape(w, envs_per_wave).any(1)
    f = first.reshape(len(first), w, envs_per_wave).max(2)  # [rounds, waves]; a round the wave runs has >= 1 trip
    s = np.where(any_change, second.reshape(w, envs_per_wave).max(1).clip(min=1), 0)
    return f.sum(0) + s, (f > 0).sum(0) + any_change


def cost(trips, sweeps, overhead, fixed):
    return trips * (LEVEL_CYCLES + overhead) + sweeps * fixed


def run(envs, launches, seed, overhead, fixed):
    rng = np.random.default_rng(seed)
    slowest, mean, n_sweeps = [], [], []
    for _ in range(launches):
        trips, sweeps = wave_trips(*launch(envs, rng))
        c = cost(trips, sweeps, overhead, fixed)
        i = int(c.argmax())
        slowest.append(float(c[i]))
        mean.append(float(c.mean()))
        n_sweeps.append(float(sweeps[i]))
    return {"envs": envs, "launches": launches, "overhead": overhead, "fixed": fixed,
            "slowest_wave_cycles": float(np.mean(slowest)), "mean_wave_cycles": float(np.mean(mean)),
            "slowest_wave_sweeps": float(np.mean(n_sweeps))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--overhead", type=float, default=90.0, help="cycles of a trip beyond its 36 level instructions")
    ap.add_argument("--fixed", type=float, default=380.0, help="cycles of a sweep's header and wrap-up")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    print(json.dumps(run(a.envs, a.launches, a.seed, a.overhead, a.fixed)))


if __name__ == "__main__":
    main()
