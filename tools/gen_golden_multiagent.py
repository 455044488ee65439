"""Multi-agent turtle episodes recorded from the REFERENCE on the CPU (through oracle/ref_env.py: make_reference_env with
cfg.multiagent.n_agents = A and cfg.show_agents) -> tests/golden/multiagent/<name>.npz.  Data only.

    python tools/gen_golden_multiagent.py        # needs the reference tree; about a minute

The reference is driven the way RLlib drives it: an agent gets no action after it has reported done, and the episode is over
when every agent has.  Every sub-step is one MultiAgentWrapper.step({agent_i: a}) -- the wrapper's own loop over a round's dict
does exactly that, one agent after the other -- so that the state after EACH sub-step can be written down.

Layout of a file (S sub-steps, E resets, R rounds; A agents, map H x W, window OH x OW, C channels):
  meta_*                 problem, shape, n_agents, show_agents, seed, change_percentage (-1: none)
  actions     int8  [R, A]   what the driver offered in round r: -1 = the agent is absent (a done agent is skipped anyway)
  round_reset uint8 [R]      1: the round ended the episode and a reset followed
  sub_round   int32 [S], sub_agent int8 [S]
  map_crc     uint32 [S]     crc32 of the uint8 map after the sub-step; pos int8 [S, A, 2] all positions (row, col)
  stats       int32 [S, n_stats], reward float64 [S], done uint8 [S], iteration / changes int32 [S]
  obs_crc     uint32 [S]     crc32 of the agent's uint8 observation
  full_idx    int32 [K], full_obs uint8 [K, OH, OW, C], full_map uint8 [K, H, W]   a few sub-steps in full
  reset_map   uint8 [E, H, W], reset_pos int8 [E, A, 2], reset_stats int32 [E, n_stats], reset_obs uint8 [E, A, OH, OW, C]

The script FAILS unless the set shows, in the reference alone: a round in which one agent is done and another is not; two agents
on one cell with show_agents; an edit that changes what another agent sees next; a negative and a positive reward in one round;
an episode ended by max_changes; a zelda sub-step with path-length > 0; the kept 32-bit half alternating over four resets.
"""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import pcgrl_oracle as po  # noqa: E402  (the order of the statistics)
import ref_env  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "multiagent")
N_FULL = 6

# name: problem, shape, agents, show_agents, change_percentage, episodes, seed, policy
#   policy "random": moves and edits, "absent": the same with agents left out of some rounds, "sweep": agent 0 clears the map
#   cell by cell and then places a player, a key and a door next to each other (zelda: path-length > 0), the others mostly absent
CASES = {
    "binary_8x8_a2": ("binary", (8, 8), 2, False, None, 4, 11, "random"),
    "binary_8x8_a2_show": ("binary", (8, 8), 2, True, 0.2, 4, 12, "random"),
    "binary_8x8_a8_show": ("binary", (8, 8), 8, True, 0.3, 1, 13, "random"),
    "binary_5x7_a3_show": ("binary", (5, 7), 3, True, None, 2, 14, "random"),
    "binary_5x7_a3_absent": ("binary", (5, 7), 3, False, None, 2, 15, "absent"),
    "binary_16x16_a1": ("binary", (16, 16), 1, False, 0.1, 1, 16, "random"),
    "binary_16x16_a3_show": ("binary", (16, 16), 3, True, 0.05, 2, 17, "random"),
    "binary_20x24_a2_show": ("binary", (20, 24), 2, True, 0.02, 1, 18, "random"),
    "binary_40x16_a3": ("binary", (40, 16), 3, False, 0.02, 1, 19, "random"),
    "binary_12x40_a2_show": ("binary", (12, 40), 2, True, 0.02, 1, 20, "absent"),
    "binary_40x48_a2": ("binary", (40, 48), 2, False, 0.005, 1, 21, "random"),
    "binary_1x2_a3_show": ("binary", (1, 2), 3, True, None, 4, 22, "random"),
    "binary_2x2_a4": ("binary", (2, 2), 4, False, None, 4, 23, "random"),
    "zelda_8x8_a2_show": ("zelda", (8, 8), 2, True, 0.3, 4, 31, "random"),
    "zelda_5x7_a3": ("zelda", (5, 7), 3, False, None, 2, 32, "absent"),
    "zelda_5x7_a2_sweep_show": ("zelda", (5, 7), 2, True, None, 1, 33, "sweep"),
    "zelda_16x16_a1": ("zelda", (16, 16), 1, False, 0.05, 1, 34, "random"),
    "zelda_16x16_a2_show": ("zelda", (16, 16), 2, True, 0.05, 2, 35, "random"),
    "zelda_20x24_a3": ("zelda", (20, 24), 3, False, 0.02, 1, 36, "random"),
    "zelda_40x16_a2_show": ("zelda", (40, 16), 2, True, 0.02, 1, 37, "random"),
    "zelda_12x40_a3_show": ("zelda", (12, 40), 3, True, 0.02, 1, 38, "random"),
    "zelda_40x48_a2_show": ("zelda", (40, 48), 2, True, 0.005, 1, 39, "random"),
}


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.uint8).tobytes()) & 0xFFFFFFFF


def sweep_actions(shape, start, nt):
    """agent 0's script: to the top-left corner, a serpentine that empties every cell, then player, key, door in a row"""
    h, w = shape
    acts = [0] * start[0] + [2] * start[1]
    r, c = 0, 0
    for r in range(h):
        cols = range(w) if r % 2 == 0 else range(w - 1, -1, -1)
        for k, c in enumerate(cols):
            acts.append(4 + 0)
            if k + 1 < w:
                acts.append(3 if r % 2 == 0 else 2)
        if r + 1 < h:
            acts.append(1)
    back = 2 if c > 1 else 3  # along the last row, away from the edge it ended at
    acts += [4 + 2, back, 4 + 3, back, 4 + 4]
    return acts


def record(name, problem, shape, A, show, cp, episodes, seed, policy):
    cfg = ref_env.make_cfg(problem, "turtle", shape, change_percentage=cp)
    cfg.multiagent.n_agents = A
    cfg.show_agents = bool(show)
    env = ref_env.make_reference_env(cfg, seed=seed)
    u = env.unwrapped
    keys = po.STAT_KEYS[problem]
    nt = po.N_TILES[problem]
    rng = np.random.default_rng(1000 + seed)
    agents = [f"agent_{i}" for i in range(A)]
    rec = {k: [] for k in ("actions", "round_reset", "sub_round", "sub_agent", "map_crc", "pos", "stats", "reward", "done",
                           "iteration", "changes", "obs_crc", "reset_map", "reset_pos", "reset_stats", "reset_obs")}
    fulls = []  # (sub-step index, obs, map)
    spare = []  # the bit generator's kept half after every reset
    seen = dict(split_done=False, shared_cell=False, seen_edit=False, both_signs=False, by_changes=False, zelda_path=False)

    def the_map():
        return np.array(u._rep.unwrapped._map, dtype=np.uint8)

    def positions():
        return np.array(u._rep.agent_positions, dtype=np.int8).reshape(A, 2)

    def stats_row():
        return np.array([int(u._rep_stats[k]) for k in keys], np.int32)

    pending = {}  # agent -> (cell, tile) of the latest edit by ANOTHER agent that it has not observed yet
    rnd = 0
    for ep in range(episodes):
        obs, _ = env.reset()
        st = u._rep.unwrapped._random.bit_generator.state
        spare.append((int(st["has_uint32"]), int(st["uinteger"])))
        rec["reset_map"].append(the_map())
        rec["reset_pos"].append(positions())
        rec["reset_stats"].append(stats_row())
        rec["reset_obs"].append(np.stack([obs[k] for k in agents]).astype(np.uint8))
        done = [False] * A
        pending.clear()
        script = sweep_actions(shape, positions()[0], nt) if policy == "sweep" else None
        while not all(done):
            offered = np.full(A, -1, np.int8)
            for i in range(A):
                if policy == "sweep":
                    if i == 0:
                        offered[i] = script.pop(0) if script else int(rng.integers(0, 4))
                    elif rng.random() < 0.15:
                        offered[i] = int(rng.integers(0, 4))
                elif policy == "absent" and rng.random() < 0.3:
                    continue
                else:
                    offered[i] = int(rng.integers(0, 4)) if rng.random() < 0.5 else 4 + int(rng.integers(0, nt))
            rews = []
            for i in range(A):
                if offered[i] < 0 or done[i]:
                    continue
                before = the_map()
                o, r, d, _, _ = env.step({agents[i]: int(offered[i])})
                ob = o[agents[i]].astype(np.uint8)
                m, ps = the_map(), positions()
                s = len(rec["sub_round"])
                rec["sub_round"].append(rnd)
                rec["sub_agent"].append(i)
                rec["map_crc"].append(crc(m))
                rec["pos"].append(ps)
                rec["stats"].append(stats_row())
                rec["reward"].append(float(r[agents[i]]))
                rec["done"].append(int(bool(d[agents[i]])))
                rec["iteration"].append(int(u._iteration))
                rec["changes"].append(int(u._changes))
                rec["obs_crc"].append(crc(ob))
                done[i] = bool(d[agents[i]])
                rews.append(float(r[agents[i]]))
                fulls.append((s, ob, m))
                if show and len({tuple(p) for p in ps.tolist()}) < A:
                    seen["shared_cell"] = True
                # an edit by another agent since this agent's last observation: its cell must lie inside this agent's window and
                # show the new tile there, which the observation before the edit did not
                if i in pending:
                    (er, ec), tile, old = pending.pop(i)
                    y, x = er - (ps[i][0] - ob.shape[0] // 2), ec - (ps[i][1] - ob.shape[1] // 2)
                    if 0 <= y < ob.shape[0] and 0 <= x < ob.shape[1] and m[er, ec] == tile and ob[y, x, 1 + tile] == 1 and old != tile:
                        seen["seen_edit"] = True
                if (before != m).any():
                    (cell,) = np.argwhere(before != m)
                    for j in range(A):
                        if j != i and not done[j]:
                            pending[j] = ((int(cell[0]), int(cell[1])), int(m[tuple(cell)]), int(before[tuple(cell)]))
                if problem == "zelda" and int(u._rep_stats["path-length"]) > 0:
                    seen["zelda_path"] = True
                if done[i] and u._max_changes is not None and u._changes > u._max_changes and u._iteration <= u._max_iterations:
                    seen["by_changes"] = True
            if any(done) and not all(done):
                seen["split_done"] = True
            if any(x < 0 for x in rews) and any(x > 0 for x in rews):
                seen["both_signs"] = True
            rec["actions"].append(offered)
            rec["round_reset"].append(1 if all(done) else 0)
            rnd += 1
    env.close() if hasattr(env, "close") else None
    S = len(rec["sub_round"])
    # in full: the first and the last sub-step and a few in between (always some with an edit before them)
    keep = sorted(set(np.linspace(0, S - 1, N_FULL).astype(int).tolist()))
    out = dict(
        meta_problem=problem, meta_shape=np.array(shape, np.int32), meta_n_agents=A, meta_show_agents=int(show), meta_seed=seed,
        meta_change_percentage=-1.0 if cp is None else float(cp),
        actions=np.array(rec["actions"], np.int8).reshape(-1, A), round_reset=np.array(rec["round_reset"], np.uint8),
        sub_round=np.array(rec["sub_round"], np.int32), sub_agent=np.array(rec["sub_agent"], np.int8),
        map_crc=np.array(rec["map_crc"], np.uint32), pos=np.array(rec["pos"], np.int8).reshape(S, A, 2),
        stats=np.array(rec["stats"], np.int32).reshape(S, len(keys)), reward=np.array(rec["reward"], np.float64),
        done=np.array(rec["done"], np.uint8), iteration=np.array(rec["iteration"], np.int32),
        changes=np.array(rec["changes"], np.int32), obs_crc=np.array(rec["obs_crc"], np.uint32),
        full_idx=np.array(keep, np.int32), full_obs=np.stack([fulls[s][1] for s in keep]),
        full_map=np.stack([fulls[s][2] for s in keep]),
        reset_map=np.stack(rec["reset_map"]), reset_pos=np.stack(rec["reset_pos"]), reset_stats=np.stack(rec["reset_stats"]),
        reset_obs=np.stack(rec["reset_obs"]), spare=np.array(spare, np.uint64))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    return seen, spare, S


def main():
    assert ref_env.available(), "the reference tree is needed"
    os.makedirs(OUT, exist_ok=True)
    total = dict(split_done=False, shared_cell=False, seen_edit=False, both_signs=False, by_changes=False, zelda_path=False)
    alternates = False
    for name, case in CASES.items():
        seen, spare, S = record(name, *case)
        for k, v in seen.items():
            total[k] = total[k] or v
        flags = [h for h, _ in spare]
        if case[2] == 2 and len(flags) >= 4 and flags[:4] in ([1, 0, 1, 0], [0, 1, 0, 1]):
            alternates = True
        size = os.path.getsize(os.path.join(OUT, name + ".npz"))
        print(f"{name}: {S} sub-steps, {size} bytes, spare flags {flags}, {[k for k, v in seen.items() if v]}", flush=True)
    missing = [k for k, v in total.items() if not v] + ([] if alternates else ["alternating spare half"])
    assert not missing, f"the set does not show: {missing}"
    print("ok: the set shows", sorted(total), "and the alternating spare half")


if __name__ == "__main__":
    main()
