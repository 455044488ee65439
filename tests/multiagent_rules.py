"""The rules of multi-agent turtle stepping (include/pcgrl_amd_multiagent.h) stated in numpy: what the reference's
MultiAgentWrapper over MultiAgentTurtleRepresentation, optionally under ShowAgentRepresentation, does (wrappers.py:697-736,
reps/wrappers.py:189-231, :616-651, pcgrl_env.py:158-188, :267-342, control_wrappers.py:216-244, :318-345).  The statistics come
from the CPU oracle (pcgrl_oracle.stats_for_grids) and the targets from pcgrl_oracle.make_config; everything else is here.
Test infrastructure only."""
import numpy as np

import pcgrl_oracle as po

DIRS = ((-1, 0), (1, 0), (0, -1), (0, 1))  # turtle_rep.py: on (row, col), clamped


class Half32:
    """PCG64's next_uint32 (numpy/random/src/pcg64/pcg64.h): a 64-bit draw serves two 32-bit requests, the low half first;
    the other half is kept -- also from one reset to the next."""

    def __init__(self, bitgen):
        self.bitgen, self.has, self.val = bitgen, 0, 0

    def next32(self):
        if self.has:
            self.has = 0
            return self.val
        n = int(self.bitgen.random_raw())
        self.has, self.val = 1, n >> 32
        return n & 0xFFFFFFFF

    def bounded(self, r):
        """a draw from [0, r]: Lemire's method on 32-bit draws; r == 0 draws nothing"""
        if r == 0:
            return 0
        ex = r + 1
        m = self.next32() * ex
        if (m & 0xFFFFFFFF) < ex:
            threshold = ((1 << 32) - ex) % ex
            while (m & 0xFFFFFFFF) < threshold:
                m = self.next32() * ex
        return m >> 32


def choice_without_replacement(h32, n, size):
    """Generator.choice(n, size=(size,), replace=False) for n <= 10000: Floyd's algorithm, then a shuffle"""
    idx, taken = [], set()
    for j in range(n - size, n):
        v = h32.bounded(j)
        if v in taken:
            v = j
        taken.add(v)
        idx.append(v)
    for i in range(size - 1, 0, -1):
        j = h32.bounded(i)
        idx[i], idx[j] = idx[j], idx[i]
    return idx


def spawn_cells(h32, n_cells, n_agents):
    """the cells (row-major indices) the agents of one reset start on"""
    if n_cells < n_agents:  # the spawn list becomes n_agents copies of cell 0
        choice_without_replacement(h32, n_agents, n_agents)
        return [0] * n_agents
    return choice_without_replacement(h32, n_cells, n_agents)


class MultiAgentRules:
    """One env.  reset() / step(actions) return what the engine returns for it; `actions` holds one entry per agent, -1 for
    an absent one.  An agent that has reported done takes no sub-step either (RLlib gives it no action any more)."""

    def __init__(self, problem, map_shape, n_agents, show_agents=False, seed=0, obs_window=None, max_board_scans=3,
                 change_percentage=None):
        self.problem, self.shape, self.A, self.show = problem, tuple(int(s) for s in map_shape), int(n_agents), bool(show_agents)
        self.cfg = po.make_config(problem, "turtle", self.shape, obs_window=obs_window, max_board_scans=max_board_scans,
                                  change_percentage=change_percentage)
        self.nt, self.ns = po.N_TILES[problem], self.cfg.n_stats
        self.window = (self.cfg.obs_window[0], self.cfg.obs_window[1])
        self.seed(seed)
        self.episodes = []  # (return, length, final stats) of every finished episode

    def seed(self, seed):
        # envs/pcgrl_env.py:142-146: the same seed for the representation's and the problem's generator
        self.rep_bits = np.random.PCG64(np.random.SeedSequence(int(seed)))
        self.rep_rng = np.random.Generator(self.rep_bits)
        self.prob_rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence(int(seed))))
        self.h32 = Half32(self.rep_bits)

    # -- pieces ----------------------------------------------------------------------------------------------------------
    def stats_of(self, grid):
        if not hasattr(self, "_stats_cfg"):  # (pcgrl_oracle.stats_for_grids with the config built once)
            self._stats_cfg = po.make_config(self.problem, "narrow", self.shape)
        g = np.ascontiguousarray(grid, dtype=np.uint8)
        out = np.empty((1, self.ns), np.int32)
        po.lib().orc_stats_for_grids_mt(po.C.byref(self._stats_cfg), 1, g.ctypes.data, out.ctypes.data, 1)
        return out[0]

    def loss(self, st):
        c, total = self.cfg, 0.0
        for k in range(self.ns):
            if c.has_trg[k]:
                v = float(st[k])
                d = c.trg_lo[k] - v if v < c.trg_lo[k] else (v - c.trg_hi[k] if v > c.trg_hi[k] else 0.0)
                total += -d * c.weights[k]
        return total

    def observation(self, i):
        """agent i's window: channel 0 out of bounds, 1 + tile, and with show_agents the occupancy plane behind them"""
        (H, W), (OH, OW) = self.shape, self.window
        C = self.nt + 1 + (1 if self.show else 0)
        rows = self.pos[i][0] - OH // 2 + np.arange(OH)[:, None]
        cols = self.pos[i][1] - OW // 2 + np.arange(OW)[None, :]
        inside = (rows >= 0) & (rows < H) & (cols >= 0) & (cols < W)
        r, c = np.clip(rows, 0, H - 1), np.clip(cols, 0, W - 1)
        channel = np.where(inside, 1 + self.grid[r, c].astype(np.int64), 0)  # Cropped: map + 1, zero pad
        obs = (channel[..., None] == np.arange(C)[None, None, :]).astype(np.uint8)
        if self.show:
            occ = np.zeros(self.shape, np.uint8)
            for p in self.pos:
                occ[tuple(p)] = 1
            obs[..., C - 1] = np.where(inside, occ[r, c], 0)
        return obs

    # -- the env ---------------------------------------------------------------------------------------------------------
    def reset(self, grid=None, pos=None):
        """a new map and the spawn draw, or an injected map with injected positions (which draw nothing)"""
        H, W = self.shape
        if grid is not None:
            self.grid = np.array(grid, np.uint8).reshape(self.shape).copy()
            self.pos = [[int(p[0]), int(p[1])] for p in pos]
        else:
            probs = self.prob_rng.random(size=self.nt)  # pcgrl_env.py:158-163
            total = 0.0
            for p in probs:
                total += p
            p = [v / total for v in probs]  # helper.py get_int_prob
            self.rep_rng.random(), self.rep_rng.random()  # turtle_rep.py:41-44: the wrapped turtle's own, unused position
            self.grid = self.rep_rng.choice(self.nt, size=self.shape, p=p).astype(np.uint8)
            if self.problem == "binary":
                self.prob_rng.random()  # binary_prob.py:139-143
            self.pos = [list(divmod(c, W)) for c in spawn_cells(self.h32, H * W, self.A)]
        self.iteration = self.changes = 0
        self.done = [False] * self.A
        self.stats = self.stats_of(self.grid)
        self.last_stats = [self.stats.copy() for _ in range(self.A)]
        self.last_loss = self.loss(self.stats)
        self.ep_return = 0.0
        return np.stack([self.observation(i) for i in range(self.A)])

    def step(self, actions, auto_reset=False):
        """one round.  Returns (obs, reward, done, stats, done_all, bad): obs[i] is None where the engine leaves the row
        unwritten; with auto_reset a finished round returns the new episode's first observations."""
        H, W = self.shape
        obs, rew, bad = [None] * self.A, np.zeros(self.A), False
        stats = np.zeros((self.A, self.ns), np.int32)
        for i in range(self.A):
            a = int(actions[i])
            if a == -1 or self.done[i]:
                stats[i] = self.last_stats[i]
                continue
            self.iteration += 1
            r, c = self.pos[i]
            if 0 <= a < 4:
                self.pos[i] = [min(max(r + DIRS[a][0], 0), H - 1), min(max(c + DIRS[a][1], 0), W - 1)]
            elif 4 <= a < 4 + self.nt:
                if self.grid[r, c] != a - 4:
                    self.grid[r, c] = a - 4
                    self.changes += 1
                    self.stats = self.stats_of(self.grid)
            else:
                bad = True  # edits nothing, raises the error bit; the sub-step still counts
            loss = self.loss(self.stats)
            rew[i] = loss - self.last_loss
            self.last_loss = loss
            self.ep_return += rew[i]
            self.done[i] = bool(self.iteration > self.cfg.max_iterations
                                or (self.cfg.max_changes >= 0 and self.changes > self.cfg.max_changes))
            self.last_stats[i] = self.stats.copy()
            stats[i] = self.stats
            obs[i] = self.observation(i)
        done = np.array(self.done)
        done_all = bool(done.all())
        if done_all and auto_reset:
            self.episodes.append((self.ep_return, self.iteration, self.stats.copy()))
            obs = list(self.reset())
        return obs, rew, done, stats, done_all, bad


# -- the recorded reference episodes (tools/gen_golden_multiagent.py -> tests/golden/multiagent/) --------------------------
def crc(a):
    import zlib
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.uint8).tobytes()) & 0xFFFFFFFF


def fixture_kwargs(z):
    cp = float(z["meta_change_percentage"])
    return dict(problem=str(z["meta_problem"]), map_shape=tuple(int(v) for v in z["meta_shape"]), n_agents=int(z["meta_n_agents"]),
                show_agents=bool(int(z["meta_show_agents"])), change_percentage=None if cp < 0 else cp)


def fixture_rounds(z):
    """per round: (the actions offered, the indices of the sub-steps it made in agent order, whether a reset followed)"""
    sub_round = z["sub_round"]
    for r, acts in enumerate(z["actions"]):
        yield acts.astype(np.int32), np.nonzero(sub_round == r)[0], bool(z["round_reset"][r])


def replay_fixture(z, rules):
    """`rules` (a fresh MultiAgentRules of the file's seed) through the whole file: everything the file holds, bit for bit"""
    A, full = rules.A, {int(s): k for k, s in enumerate(z["full_idx"])}
    ep = 0

    def check_reset(obs):
        assert np.array_equal(rules.grid, z["reset_map"][ep]), ("reset map", ep)
        assert np.array_equal(np.array(rules.pos), z["reset_pos"][ep]), ("reset positions", ep)
        assert np.array_equal(rules.stats, z["reset_stats"][ep]), ("reset stats", ep)
        assert np.array_equal(obs, z["reset_obs"][ep]), ("reset observations", ep)
        assert (rules.h32.has, rules.h32.val if rules.h32.has else 0) == (int(z["spare"][ep][0]),
                                                                          int(z["spare"][ep][1]) if rules.h32.has else 0), ep

    check_reset(rules.reset())
    for acts, subs, reset_after in fixture_rounds(z):
        # sub-step by sub-step, so that the map and the positions after each are seen: a round of one agent at a time
        k = 0
        for i in range(A):
            if acts[i] == -1 or rules.done[i]:
                continue
            s = int(subs[k])
            k += 1
            assert int(z["sub_agent"][s]) == i, s
            one = np.full(A, -1, np.int32)
            one[i] = acts[i]
            obs, rew, done, stats, _, bad = rules.step(one)
            assert not bad
            assert crc(rules.grid) == int(z["map_crc"][s]), ("map", s)
            assert np.array_equal(np.array(rules.pos), z["pos"][s]), ("positions", s)
            assert np.array_equal(stats[i], z["stats"][s]), ("stats", s)
            assert rew[i] == z["reward"][s], ("reward", s, rew[i], z["reward"][s])
            assert int(done[i]) == int(z["done"][s]), ("done", s)
            assert (rules.iteration, rules.changes) == (int(z["iteration"][s]), int(z["changes"][s])), ("counters", s)
            assert crc(obs[i]) == int(z["obs_crc"][s]), ("observation", s)
            if s in full:
                assert np.array_equal(obs[i], z["full_obs"][full[s]]) and np.array_equal(rules.grid, z["full_map"][full[s]]), s
        assert k == len(subs)
        assert all(rules.done) == reset_after
        if reset_after and ep + 1 < len(z["reset_map"]):
            ep += 1
            check_reset(rules.reset())
