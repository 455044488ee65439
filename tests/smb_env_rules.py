"""The Super Mario Bros environment in plain Python on top of tests/smb_rules.py: what make_env(cfg) of the reference does for
smb + narrow / turtle (file:line references are relative to the reference's control_pcgrl/).  Test
infrastructure: the fixtures under tests/golden/smb_env pin these rules to the reference, and the GPU tests pin the step kernel
to these rules.

    reset   envs/pcgrl_env.py:158-188: seven doubles of the problem stream are the tile probabilities (normalised by
            helper.py get_int_prob); turtle draws its start (int(u * H), int(u * W)) from the representation stream before the
            map (reps/turtle_rep.py:31-44); the map is H * W doubles of that stream through searchsorted(cdf, u, 'right')
            (Generator.choice); both streams are PCG64(SeedSequence(seed)) and continue from one episode to the next.
    narrow  reps/narrow_rep.py:89-102: update k writes the cell the position points at and then moves to cell (k - 1) mod H*W,
            so cell 0 is written by updates 1 and 2.
    turtle  reps/turtle_rep.py:87-107: actions 0..3 move by DIRS, clamped; actions 4..10 write tile a - 4.
    step    pcgrl_env.py:267-342, control_wrappers.py:216-244: the statistics are recomputed only when the written tile differs.
    search  the two exact shortcuts of the device are stated as a count: `searches` goes up at a reset and at an edit that
            changes the cell's solidity (smb_rules.BLOCKING) -- every other edit keeps the play statistics it had.
"""
import numpy as np

import smb_rules as R

DIRS = ((-1, 0), (1, 0), (0, -1), (0, 1))  # turtle_rep.py:14, on (row, col)
N_TILES = 7


def is_solid(t):
    return int(t) in R.BLOCKING


class SmbEnvRules:
    def __init__(self, representation, shape, seed=None, obs_window=None, weights=None, max_board_scans=3,
                 change_percentage=None, solver_power=10000):
        assert representation in ("narrow", "turtle")
        self.rep = representation
        self.shape = (int(shape[0]), int(shape[1]))
        H, W = self.shape
        self.window = tuple(obs_window) if obs_window is not None else (2 * H, 2 * W)
        self.weights = dict(R.DEFAULT_WEIGHTS if weights is None else weights)
        self.power = int(solver_power)
        self.max_iterations = H * W * max_board_scans + 1  # pcgrl_env.py:241
        self.max_changes = None if change_percentage is None else max(int(change_percentage * H * W), 1)  # :235-239
        self.num_actions = N_TILES if representation == "narrow" else 4 + N_TILES
        self.searches = 0
        if seed is not None:
            self.seed(seed)

    def seed(self, seed):
        self.prob_rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence(int(seed))))
        self.rep_rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence(int(seed))))

    # -- pieces ----------------------------------------------------------------------------------------------------------
    def observation(self):
        """Cropped + OneHotEncoding (wrappers.py:407-437): channel 0 outside the map, 1 + tile inside"""
        (H, W), (OH, OW) = self.shape, self.window
        rows = self.pos[0] - OH // 2 + np.arange(OH)[:, None]
        cols = self.pos[1] - OW // 2 + np.arange(OW)[None, :]
        inside = (rows >= 0) & (rows < H) & (cols >= 0) & (cols < W)
        r, c = np.clip(rows, 0, H - 1), np.clip(cols, 0, W - 1)
        channel = np.where(inside, 1 + self.grid[r, c].astype(np.int64), 0)
        return (channel[..., None] == np.arange(N_TILES + 1)[None, None, :]).astype(np.uint8)

    def _evaluate(self):
        self.searches += 1
        self.stats, self.rec = R.get_stats(self.grid, self.power)

    def loss(self):
        return R.loss(self.stats, self.weights)

    # -- the env ---------------------------------------------------------------------------------------------------------
    def reset(self, grid=None, pos=None):
        """a drawn map, or an injected one (which draws nothing, as VecPcgrlEnv.reset(init_grids=...)); always a search"""
        H, W = self.shape
        if grid is not None:
            self.grid = np.array(grid, np.uint8).reshape(self.shape).copy()
            self.pos = [0, 0] if (pos is None or self.rep == "narrow") else [int(pos[0]), int(pos[1])]
        else:
            probs = self.prob_rng.random(size=N_TILES)
            total = 0.0
            for p in probs:
                total += p
            p = [v / total for v in probs]
            self.pos = [0, 0]
            if self.rep == "turtle":
                self.pos = [int(self.rep_rng.random() * H), int(self.rep_rng.random() * W)]
            self.grid = self.rep_rng.choice(N_TILES, size=self.shape, p=p).astype(np.uint8)
        self.n_step = 0
        self.iteration = self.changes = 0
        self._evaluate()
        self.last_loss = self.loss()
        self.ep_return = 0.0
        return self.observation()

    def step(self, action, auto_reset=False):
        """-> (obs, reward, done, info): info has "changed", "searched", and with auto_reset at an episode end the finished
        episode's "final_stats"; the observation is then the new episode's first."""
        H, W = self.shape
        a = int(action)
        assert 0 <= a < self.num_actions
        self.iteration += 1
        changed = searched = False
        tile = None
        if self.rep == "narrow":
            tile = a
        elif a < 4:
            self.pos = [min(max(self.pos[0] + DIRS[a][0], 0), H - 1), min(max(self.pos[1] + DIRS[a][1], 0), W - 1)]
        else:
            tile = a - 4
        if tile is not None:
            old = int(self.grid[self.pos[0], self.pos[1]])
            changed = old != tile
            self.grid[self.pos[0], self.pos[1]] = tile
            if changed:
                self.changes += 1
                if is_solid(old) != is_solid(tile):
                    searched = True
                    self._evaluate()
                else:  # the level of the play-through is the same: only the five map statistics move
                    self.stats = R.map_stats(self.grid) + self.stats[5:]
        if self.rep == "narrow":
            self.pos = list(divmod(self.n_step % (H * W), W))
            self.n_step += 1
        loss = self.loss()
        reward = loss - self.last_loss
        self.last_loss = loss
        self.ep_return += reward
        done = self.iteration > self.max_iterations
        if self.max_changes is not None:
            done = done or self.changes > self.max_changes
        info = {"changed": changed, "searched": searched, "stats": list(self.stats), "iteration": self.iteration,
                "changes": self.changes, "pos": list(self.pos)}
        if done and auto_reset:
            info["final_stats"] = list(self.stats)
            info["ep_return"] = self.ep_return
            obs = self.reset()
        else:
            obs = self.observation()
        return obs, reward, done, info
