"""Trained-like maps for the step kernels (numpy only; a helper, not collected): corridor families for any H x W, a driver
that morphs every env of a batch from one family to the next through the actions of its representation, scripted single-cell
edits (cut, re-open, fill, bridge, far cell) and the coverage figures the tests assert.  Everything here reads maps and
positions from the CPU oracle's get_state(), never from the engine: tests/test_structured_maps_cpu.py runs it on the oracle
alone, tests/test_gpu_structured_steps.py with the engine alongside.

The step kernels keep the far cell of every component and the last frontier of the sweep that gave the current path-length
(csrc/pcgrl_kernels2d.h, INCREMENTAL UPDATE); which of their branches a step takes is decided by the map's structure --
splits, merges, the maximum passing to another component, ties, sweeps of many trips -- and uniform random actions hardly
ever build such maps.  Cells are (row, col); binary: 0 empty, 1 solid; zelda: tests/paths_numpy.py's tile ids, 5..7 enemies."""
import os

import numpy as np

import paths_numpy as pn

EMPTY, SOLID, PLAYER, KEY, DOOR = pn.EMPTY, pn.SOLID, pn.PLAYER, pn.KEY, pn.DOOR
ENEMIES = (5, 6, 7)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "paths", "structured")
REW_TOL = 1e-6  # the suite's: float32 reward outputs against the oracle's float64


# ---- map families ---------------------------------------------------------------------------------------------------------------
def snake_h(h, w):
    """every other row empty, joined at alternating ends: one corridor from (0, 0)"""
    g = np.ones((h, w), np.uint8)
    g[0::2] = EMPTY
    for k, r in enumerate(range(1, h - 1, 2)):
        g[r, w - 1 if k % 2 == 0 else 0] = EMPTY
    return g


def snake_v(h, w):
    return np.ascontiguousarray(snake_h(w, h).T)


def spiral(h, w):
    """one corridor from (0, 0) inwards, a wall between its arms"""
    g = np.ones((h, w), np.uint8)
    r = c = d = 0
    g[0, 0] = EMPTY
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))

    def free(rr, cc, fr, fc):  # (rr, cc) can be carved coming from (fr, fc): solid, and no other empty neighbour
        if not (0 <= rr < h and 0 <= cc < w) or g[rr, cc] == EMPTY:
            return False
        return all(not (0 <= rr + a < h and 0 <= cc + b < w) or g[rr + a, cc + b] == SOLID or (rr + a, cc + b) == (fr, fc)
                   for a, b in dirs)

    while True:
        for turn in (0, 1):
            dr, dc = dirs[(d + turn) % 4]
            if free(r + dr, c + dc, r, c):
                d = (d + turn) % 4
                r, c = r + dr, c + dc
                g[r, c] = EMPTY
                break
        else:
            return g


def comb(h, w):
    """a spine along row 0 and a tooth down every other column"""
    g = np.ones((h, w), np.uint8)
    g[0] = EMPTY
    g[:, 0::2] = EMPTY
    return g


def _half(h):
    k = (h - 1) // 2
    return max(1, k - 1 if k % 2 == 0 else k)  # odd: the half's last row is an empty one, next to the separating wall


def tie_pair(h, w):
    """two corridors of equal length, one wall row between them: a tie for the maximum"""
    k = _half(h)
    g = np.ones((h, w), np.uint8)
    g[:k] = snake_h(k, w)
    g[k + 1:2 * k + 1] = snake_h(k, w)
    return g


def off_by_one(h, w):
    """the tie pair with the lower corridor one cell shorter"""
    g = tie_pair(h, w)
    k = _half(h)
    r, c = order_from(g, (k + 1, 0))[-1]
    g[r, c] = SOLID
    return g


def ring(h, w):
    g = np.ones((h, w), np.uint8)
    g[0] = g[-1] = EMPTY
    g[:, 0] = g[:, -1] = EMPTY
    return g


def checkerboard(h, w):
    """the maximum number of one-cell regions"""
    return ((np.add.outer(np.arange(h), np.arange(w)) % 2) == 1).astype(np.uint8)


def all_empty(h, w):
    return np.zeros((h, w), np.uint8)


def all_solid(h, w):
    return np.ones((h, w), np.uint8)


FAMILIES = {"snake_h": snake_h, "snake_v": snake_v, "spiral": spiral, "comb": comb, "tie": tie_pair, "off_by_one": off_by_one,
            "ring": ring, "checker": checkerboard, "empty": all_empty, "solid": all_solid}
_cache = {}


def family(name, shape):
    """the (read-only) map of a family; "golden<k>": the recorded binary map with the k-th longest path, where the folder of
    reference-recorded structured maps has this shape (else the horizontal snake)"""
    key = (name, tuple(shape))
    if key not in _cache:
        if name.startswith("golden"):
            path = os.path.join(GOLDEN, f"binary_{shape[0]}x{shape[1]}.npz")
            if os.path.exists(path):
                z = np.load(path)
                g = z["grids"][np.argsort(-z["L"], kind="stable")[int(name[6:])]].astype(np.uint8)
            else:
                g = snake_h(*shape)
        else:
            g = FAMILIES[name](*shape)
        g.setflags(write=False)
        _cache[key] = g
    return _cache[key]


def order_from(grid, start):
    """the cells of start's component (passable: not solid) by BFS distance from `start`; along a corridor, its order"""
    d = pn.bfs(grid != SOLID, tuple(start))
    cells = np.argwhere(d >= 0)
    return [tuple(int(v) for v in c) for c in cells[np.argsort(d[d >= 0], kind="stable")]]


def far_cell(grid):
    """the far cell of the first component: the first farthest cell (row-major) from its first cell"""
    first = tuple(int(v) for v in np.argwhere(grid == EMPTY)[0])
    d = pn.bfs(grid == EMPTY, first)
    return tuple(int(v) for v in divmod(int(np.argmax(d)), grid.shape[1]))


# the schedule of targets; envs of a batch start at different points of it.  Long corridors dominate, so that most compared
# steps run sweeps of many trips; checkerboard, empty and solid put the many-regions, one-region and no-region maps between them.
SCHEDULE = ("snake_h", "tie", "snake_v", "golden0", "checker", "spiral", "off_by_one", "empty", "comb", "tie", "golden1",
            "solid", "snake_h", "off_by_one", "ring", "spiral")
# zelda: layouts, and phases that keep the layout: "key" moves the key between the corridor's first cell and its third (the scan
# passes through a map without a key one way and with two keys the other), "walled" cuts the player off
ZELDA_SCHEDULE = ("snake_h", "key", "ladder", "empty", "key", "snake_h", "walled", "snake_h", "comb", "snake_h")


def zelda_spots(shape):
    """(key cells a and b, player, door) of a shape: the key at the first cell of the horizontal snake (b: two cells on), the
    player at the snake's other end, the door in a pocket of the wall next to the snake's middle cell"""
    h, w = shape
    g = snake_h(h, w)
    order = order_from(g, (0, 0))
    mr, mc = order[len(order) // 2]
    door = next((r, c) for r, c in ((mr + 1, mc), (mr - 1, mc), (mr, mc + 1), (mr, mc - 1))
                if 0 <= r < h and 0 <= c < w and g[r, c] == SOLID)
    return order[0], order[2], order[-1], door


def zelda_layout(name, shape):
    """binary layout of a zelda phase: "ladder" is the snake with every connector row opened at both ends (two routes)"""
    if name == "ladder":
        g = snake_h(*shape).copy()
        g[1:shape[0] - 1:2, 0] = g[1:shape[0] - 1:2, -1] = EMPTY
        return g
    return family(name, shape)


# ---- the morph driver -----------------------------------------------------------------------------------------------------------
class Morph:
    """Per env a target map and the next action towards it.

    narrow: the target's tile at the current position (the position scans the board, narrow_rep.py:137; writes that change
    nothing are the non-changing steps).  turtle: the target's tile where the cell differs, else the next move of a
    boustrophedon walk (even rows rightwards, odd rows leftwards, down at a row's end, back up from the last row).  wide: one
    differing cell per step -- the first in row-major order, the last, or a seeded-random one, alternating between phases --
    and a write that changes nothing once none differs.

    A phase lasts at most `budget` steps.  The target is the family's map on the cells the representation reaches within the
    budget (narrow: the first budget - 2 cells of the scan; turtle: the rows the walk finishes, writes counted; wide: the first
    budget - 2 differing cells) and the current map elsewhere, so every phase can be completed: `missed` counts those that
    were not.  due() names the envs whose phase is over; begin() gives them their next target and returns the maps and
    positions for the masked reset that restarts them (their current maps, position (0, 0)): the reset zeroes the counters,
    which keeps episodes from ending mid-morph and restarts narrow's scan."""

    def __init__(self, problem, rep, shape, n, budget, seed=0, schedule=None):
        self.problem, self.rep, self.shape, self.n, self.budget = problem, rep, tuple(shape), n, int(budget)
        self.schedule = schedule or (ZELDA_SCHEDULE if problem == "zelda" else SCHEDULE)
        self.nt = 2 if problem == "binary" else 8
        self.rng = np.random.default_rng(seed)
        self.k = np.arange(n) % len(self.schedule)  # the next phase of every env
        self.target = np.zeros((n,) + self.shape, np.uint8)
        self.age = np.zeros(n, np.int64)
        self.vdir = np.ones(n, np.int64)
        self.mode = np.zeros(n, np.int64)
        self.phases = self.completed = self.missed = 0
        self.started = False
        if problem == "zelda":
            self.key_a, self.key_b, self.player, self.door = zelda_spots(shape)
            self.key = [self.key_a] * n

    # -- maps --
    def _zelda(self, i, layout, enemies=True):
        """the zelda map of a binary layout: the env's key, the player and the door on it, up to three enemies on passable
        cells of the top rows"""
        g = np.array(layout, np.uint8)
        if enemies:
            cells = np.argwhere(g[:max(2, self.shape[0] // 4)] == EMPTY)
            for r, c in cells[self.rng.permutation(len(cells))[:int(self.rng.integers(0, 4))]]:
                g[r, c] = ENEMIES[int(self.rng.integers(3))]
        g[self.key_a] = g[self.key_b] = EMPTY
        g[self.key[i]], g[self.player], g[self.door] = KEY, PLAYER, DOOR
        return g

    def start_maps(self):
        """the maps every env starts from: the family before its first target, whole"""
        maps = np.zeros((self.n,) + self.shape, np.uint8)
        for i in range(self.n):
            name = self.schedule[(self.k[i] - 1) % len(self.schedule)]
            if name == "checker" and self.shape[0] * self.shape[1] > 2048:
                name = "comb"  # (a whole checkerboard of this size costs the oracle 10 ms a step; as a target it is reached in part)
            if self.problem == "zelda":
                maps[i] = self._zelda(i, zelda_layout("snake_h" if name in ("key", "walled") else name, self.shape))
            else:
                maps[i] = family(name, self.shape)
        return maps

    def _wanted(self, i, cur):
        name = self.schedule[self.k[i] % len(self.schedule)]
        if self.problem == "binary":
            return np.array(family(name, self.shape))
        if name == "key":
            self.key[i] = self.key_b if self.key[i] == self.key_a else self.key_a
            g = cur.copy()
            g[self.key_a] = g[self.key_b] = EMPTY
            g[self.key[i]] = KEY
            return g
        if name == "walled":  # solid on the player's neighbours; on a board the phase cannot cross, a solid row it can reach
            g, (pr, pc), (h, w) = cur.copy(), self.player, self.shape
            keep = np.isin(g, (KEY, DOOR, PLAYER))
            for r, c in ((pr - 1, pc), (pr + 1, pc), (pr, pc - 1), (pr, pc + 1)):
                if 0 <= r < h and 0 <= c < w and not keep[r, c]:
                    g[r, c] = SOLID
            rows = self._reach_rows(cur, cur)
            if rows < h:
                cut = max(0, rows // 2 - 1)
                g[cut] = np.where(keep[cut], g[cut], SOLID)
            return g
        return self._zelda(i, zelda_layout(name, self.shape))

    def _reach_rows(self, cur, want):
        """rows a phase can finish (turtle: a row costs its moves and its differing cells)"""
        h, w = self.shape
        if self.rep == "narrow":
            return min(h, (self.budget - 2) // w)
        cost = np.cumsum(w + (cur != want).sum(axis=1))
        return int(np.searchsorted(cost, self.budget - 2, side="right"))

    def _limit(self, cur, want):
        """`want` on the cells the phase reaches, `cur` elsewhere"""
        h, w = self.shape
        out = cur.copy()
        if self.rep == "narrow":
            m = min(h * w, self.budget - 2)
            out.reshape(-1)[:m] = want.reshape(-1)[:m]
        elif self.rep == "turtle":
            rows = self._reach_rows(cur, want)
            out[:rows] = want[:rows]
        else:
            diff = np.flatnonzero(cur != want)[:self.budget - 2]
            out.reshape(-1)[diff] = want.reshape(-1)[diff]
        return out

    # -- phases --
    def due(self, grids):
        """bool [n]: envs whose phase is over (target reached, or the budget spent); everyone before the first begin()"""
        if not self.started:
            return np.ones(self.n, bool)
        reached = (grids == self.target).all(axis=(1, 2))
        spent = self.age >= self.budget
        self.completed += int(reached.sum())
        self.missed += int((spent & ~reached).sum())
        return reached | spent

    def begin(self, grids, mask):
        """next targets for the envs of `mask`; -> (init_grids [n, H, W], init_pos [n, 2]) for reset(mask=mask, ...)"""
        init = np.array(grids, np.uint8).reshape((self.n,) + self.shape)
        if not self.started:
            init, self.started = self.start_maps(), True
        for i in np.flatnonzero(mask):
            self.target[i] = self._limit(init[i], self._wanted(i, init[i]))
            self.mode[i] = (self.k[i] // len(self.schedule) + self.k[i]) % 3
            self.k[i] += 1
            self.phases += 1
        self.age[mask] = 0
        self.vdir[mask] = 1
        return init, np.zeros((self.n, 2), np.int32)

    def actions(self, grids, pos):
        """int32 [n]: the next action of every env, from the oracle's maps [n, H, W] and positions [n, >= 2]"""
        n, (h, w), idx = self.n, self.shape, np.arange(self.n)
        r, c = pos[:, 0].astype(np.int64), pos[:, 1].astype(np.int64)
        self.age += 1
        if self.rep == "narrow":
            return self.target[idx, r, c].astype(np.int32)
        if self.rep == "turtle":
            cur, want = grids[idx, r, c], self.target[idx, r, c]
            place = cur != want
            right = r % 2 == 0
            at_end = np.where(right, c == w - 1, c == 0)
            nr = r + self.vdir
            flip = at_end & ~place & ((nr < 0) | (nr >= h))
            self.vdir = np.where(flip, -self.vdir, self.vdir)
            move = np.where(at_end, np.where(self.vdir > 0, 1, 0), np.where(right, 3, 2))
            return np.where(place, 4 + want.astype(np.int64), move).astype(np.int32)
        diff = (grids != self.target).reshape(n, -1)
        first = diff.argmax(axis=1)
        last = h * w - 1 - diff[:, ::-1].argmax(axis=1)
        rand = (self.rng.random(diff.shape) * diff).argmax(axis=1)
        cell = np.where(diff.any(axis=1), np.choose(self.mode, (first, last, rand)), 0)
        return wide_action(cell // w, cell % w, self.target.reshape(n, -1)[idx, cell], w, self.nt)


def wide_action(r, c, tile, w, nt):
    """the wide action that sets cell (r, c): the flat index over (y, x, tile) whose write lands on map[x, y] (square maps)"""
    return ((np.asarray(c, np.int64) * w + r) * nt + tile).astype(np.int32)


# ---- scripted single-cell edits -------------------------------------------------------------------------------------------------
def edit_scripts(shape):
    """-> [(name, start map, [(row, col, tile), ...])]: each list applies its edits and then undoes them, and is run in a loop"""
    h, w = shape
    out = []
    snake = snake_h(h, w)
    order = order_from(snake, (0, 0))

    def there_and_back(edits, back):
        return edits + [(r, c, back) for r, c, _ in reversed(edits)]

    for name, cell in (("cut_middle", order[len(order) // 2]), ("cut_far_end", order[-1]), ("cut_first", order[0])):
        out.append((name, snake, there_and_back([cell + (SOLID,)], EMPTY)))
    # fill the upper (longer) corridor from its end until the lower one holds the maximum, and a few cells more
    pair = off_by_one(h, w)
    upper = order_from(pair, (0, 0))
    out.append(("fill_max", pair, there_and_back([cell + (SOLID,) for cell in upper[::-1][:min(6, len(upper) - 1)]], EMPTY)))
    out.append(("bridge", tie_pair(h, w), there_and_back([(_half(h), w // 2, EMPTY)], SOLID)))
    for name in ("comb", "ring"):  # (the far cell where it is neither the corridor's end nor a corner of the scan)
        g = FAMILIES[name](h, w)
        out.append(("far_cell_" + name, g, there_and_back([far_cell(g) + (SOLID,)], EMPTY)))
    return out


class Script:
    """env i runs edit script i % len(scripts) in a loop: wide sets the cell, turtle walks to it (rows first) and places"""

    def __init__(self, rep, shape, n, nt=2):
        self.rep, self.shape, self.n, self.nt = rep, tuple(shape), n, nt
        self.scripts = edit_scripts(shape)
        self.edits = [self.scripts[i % len(self.scripts)][2] for i in range(n)]
        self.at = np.zeros(n, np.int64)

    def start_maps(self):
        return np.stack([self.scripts[i % len(self.scripts)][1] for i in range(self.n)]).astype(np.uint8)

    def actions(self, grids, pos):
        a = np.zeros(self.n, np.int32)
        for i in range(self.n):
            r, c, t = self.edits[i][self.at[i] % len(self.edits[i])]
            if self.rep == "wide":
                a[i] = wide_action(r, c, t, self.shape[1], self.nt)
                self.at[i] += 1
            elif pos[i, 0] != r:
                a[i] = 1 if pos[i, 0] < r else 0
            elif pos[i, 1] != c:
                a[i] = 3 if pos[i, 1] < c else 2
            else:
                a[i] = 4 + t
                self.at[i] += 1
        return a


# ---- coverage -------------------------------------------------------------------------------------------------------------------
class Coverage:
    """what the compared steps covered, from the ORACLE's statistics before and after each step and the tile it placed"""

    def __init__(self, problem, shape):
        self.problem, self.shape = problem, tuple(shape)
        self.reg, self.path = (0, 1) if problem == "binary" else (4, 6)
        self.pairs = self.long = self.alive = self.enemy = self.max_path = 0
        self.split = self.merge = self.handover = self.unchanged = 0
        self.threshold = 61 * shape[0] * shape[1] / 256  # 61: the longest path of 102 400 random binary-narrow 16 x 16 steps

    def add(self, before, after, tile, changed):
        """statistics [n, n_stats] before and after a step, the tile [n] it placed (-1: a move) and whether the map changed"""
        rb, ra, pb, pa = before[:, self.reg], after[:, self.reg], before[:, self.path], after[:, self.path]
        self.pairs += len(after)
        self.long += int((pa > self.threshold).sum())
        self.alive += int((pa > 0).sum())
        self.max_path = max(self.max_path, int(pa.max()))
        self.split += int(((ra > rb) & (tile == SOLID)).sum())
        self.merge += int(((ra < rb) & (tile == EMPTY)).sum())
        self.handover += int(((pa < pb - 1) & (ra >= rb)).sum())
        self.unchanged += int((~changed).sum())
        if self.problem == "zelda":
            self.enemy += int((after[:, 5] > 0).sum())

    def figures(self):
        return {k: getattr(self, k) for k in ("pairs", "long", "alive", "enemy", "max_path", "split", "merge", "handover", "unchanged")}

    def check_floors(self, events=True):
        """the floors of DESIGN.md section 2 ("trained-like maps"); a schedule that misses one is changed, not the floor"""
        h, w = self.shape
        f = self.figures()
        if self.problem == "binary":
            assert self.max_path >= 0.45 * h * w, f
            assert 3 * self.long >= self.pairs, f
            if events:
                assert min(self.split, self.merge, self.handover) >= 20, f
        else:
            assert 2 * self.alive >= self.pairs and 4 * self.enemy >= self.pairs and self.max_path >= h * w / 4, f
        return f


def placed_tile(rep, actions, nt):
    """the tile an action writes, -1 for a turtle move"""
    a = np.asarray(actions, np.int64)
    return a if rep == "narrow" else np.where(a >= 4, a - 4, -1) if rep == "turtle" else a % nt


# ---- the loop: the oracle alone, or the engine held against it at every step ----------------------------------------------------
def oracle_state(orc):
    st = orc.get_state()
    return st, st["grids"].reshape((orc.n,) + tuple(orc.map_shape)), st["pos"]


def compare_state(env, orc, what):
    n, st, ost = orc.n, env.get_state(), orc.get_state()
    assert np.array_equal(st.grids.cpu().numpy().reshape(n, -1), ost["grids"]), f"grids {what}"
    if orc.representation != "wide":
        assert np.array_equal(st.pos.cpu().numpy()[:, :2], ost["pos"][:, :2]), f"pos {what}"
    for key in ("iteration", "changes", "stats", "last_loss"):
        assert np.array_equal(getattr(st, key).cpu().numpy(), ost[key]), f"{key} {what}"
    if orc.representation == "narrow":
        assert np.array_equal(st.n_step.cpu().numpy(), ost["n_step"]), f"n_step {what}"
    assert np.allclose(st.ep_return.cpu().numpy(), ost["ep_return"], atol=REW_TOL), f"ep_return {what}"


def compare_obs(env, obs, oobs, what):
    if env.obs_format == "codes":  # the code is the index of the one-hot channel; and back through the library's own expansion
        from control_pcgrl_amd.vec_env import codes_to_onehot
        assert np.array_equal(obs.cpu().numpy()[..., 0], oobs.argmax(axis=-1)), f"codes {what}"
        assert np.array_equal(codes_to_onehot(obs, env).cpu().numpy(), oobs), f"codes expanded {what}"
    else:
        assert np.array_equal(obs.cpu().numpy(), oobs), f"obs {what}"


def engine_step(env, a, want_obs=True):
    """env.step; want_obs False: pcgrl_step with d_obs = NULL (the env's observation buffer keeps its last contents)"""
    if want_obs:
        return env.step(a)
    from control_pcgrl_amd import _lib
    p = env._ptrs
    _lib.check(env._L.pcgrl_step(env._h, env._actions(a).data_ptr(), 0, None, p[1], p[2], p[3], env._stream()), "pcgrl_step")
    return env._step_out


def run(orc, driver, steps, env=None, cov=None, sync=10, obs_every=40, null_obs=False, record=None, what=""):
    """`steps` steps of `driver` on the oracle, and on `env` (a VecPcgrlEnv without auto-reset) when given: statistics, done and
    reward of every step are compared, the observation and the whole state every `obs_every` steps, after every restart and at
    the end.  Every `sync` steps the envs whose phase is over are restarted by a masked reset(init_grids, init_pos) (sync 0, or a
    driver without phases: no restarts).  null_obs: the engine steps without an observation output except where one is compared.
    record: a list that receives ("reset", mask, grids, pos) and ("step", actions, reward, done, stats) entries."""
    if env is not None:
        import torch
    nt = 2 if orc.problem == "binary" else 8
    for t in range(steps):
        st, grids, pos = oracle_state(orc)
        if sync and hasattr(driver, "due") and t % sync == 0:
            due = driver.due(grids)
            if due.any():
                init_grids, init_pos = driver.begin(grids, due)
                mask = due.astype(np.uint8)
                oobs = orc.reset(mask=mask, init_grids=init_grids, init_pos=init_pos)
                if record is not None:
                    record.append(("reset", mask, init_grids.copy(), init_pos.copy()))
                if env is not None:
                    obs, _ = env.reset(mask=mask, init_grids=init_grids, init_pos=init_pos)
                    compare_obs(env, obs, oobs, f"{what} restart @ {t}")
                    compare_state(env, orc, f"{what} restart @ {t}")
                st, grids, pos = oracle_state(orc)
        a = driver.actions(grids, pos)
        want = t % obs_every == obs_every - 1 or t == steps - 1
        oobs, orew, odone, ostats = orc.step(a, auto_reset=False, want_obs=want)
        if cov is not None:
            cov.add(st["stats"], ostats, placed_tile(orc.representation, a, nt), orc.get_state()["changes"] != st["changes"])
        if record is not None:
            record.append(("step", a.copy(), orew, odone, ostats))
        if env is not None:
            obs, rew, done, _, info = engine_step(env, torch.as_tensor(a).to(env.device), want or not null_obs)
            stats = info["stats"].cpu().numpy()
            bad = np.nonzero((stats != ostats).any(axis=1))[0]
            assert bad.size == 0, (f"{what} stats @ step {t}: {bad.size} envs differ, first {bad[:4]}: engine {stats[bad[:4]].tolist()} "
                                   f"oracle {ostats[bad[:4]].tolist()}")
            assert np.max(np.abs(rew.cpu().numpy().astype(np.float64) - orew)) <= REW_TOL, f"{what} reward @ {t}"
            assert np.array_equal(done.cpu().numpy(), odone), f"{what} done @ {t}"
            if want:
                compare_obs(env, obs, oobs, f"{what} @ {t}")
                compare_state(env, orc, f"{what} @ {t}")
    if env is not None:
        env.check_errors()


# (shape, representation) forms of the step kernels: lanes per env / row-mask bits 8/32, 16/32 (the compile-time 16 x 16
# kernels), 32/32, 64/32, 32/64, 64/64 and the 64 x 64 maps of the reference's binary_bigger; per form the batch, the steps of
# a test and the budget of a phase (narrow: a scan of the board where it fits; wide: fewer differing cells than the budget)
FORMS = {
    ((8, 8), "turtle"): dict(n=128, steps=450, budget=150),
    ((16, 16), "narrow"): dict(n=128, steps=540, budget=260),
    ((16, 16), "turtle"): dict(n=128, steps=600, budget=300),
    ((16, 16), "wide"): dict(n=128, steps=450, budget=150),
    ((20, 24), "narrow"): dict(n=96, steps=600, budget=300),
    ((40, 16), "narrow"): dict(n=96, steps=600, budget=300),
    ((12, 40), "narrow"): dict(n=96, steps=600, budget=300),
    ((40, 48), "narrow"): dict(n=64, steps=600, budget=300),
    ((40, 48), "turtle"): dict(n=64, steps=600, budget=300),
    ((64, 64), "wide"): dict(n=64, steps=300, budget=150),
}
ZELDA_FORMS = [((16, 16), "turtle"), ((20, 24), "narrow"), ((12, 40), "narrow"), ((40, 48), "turtle")]
SCRIPT_FORMS = [((8, 8), "turtle"), ((16, 16), "wide"), ((16, 16), "turtle"), ((40, 48), "turtle"), ((64, 64), "wide")]


def form_id(problem, shape, rep):
    return f"{problem}-{shape[0]}x{shape[1]}-{rep}"


def make_oracle(problem, rep, shape, n, **kw):
    import pcgrl_oracle as po
    return po.OracleVecEnv(problem, rep, shape, n, seeds=300 + np.arange(n), threads=8, change_percentage=1.0, **kw)


def script_steps(shape, rep):
    """steps of a scripted-edit run: wide needs one per edit; the turtle walks to the farthest cell and back"""
    return 300 if rep == "wide" else max(300, min(600, 6 * (shape[0] + shape[1])))


def start_script(orc, driver, env=None):
    """both sides from the scripts' start maps, position (0, 0)"""
    maps, pos = driver.start_maps(), np.zeros((orc.n, 2), np.int32)
    oobs = orc.reset(init_grids=maps, init_pos=pos)
    if env is not None:
        obs, _ = env.reset(init_grids=maps, init_pos=pos)
        compare_obs(env, obs, oobs, "script start")


# ---- calls that could leave the cached masks stale ----------------------------------------------------------------------------
STALE_KINDS = ("update", "state_dict", "set_state", "inject")
STALE_FORMS = [("binary", (16, 16), "narrow"), ("binary", (16, 16), "wide"), ("binary", (12, 40), "narrow"),
               ("binary", (40, 48), "turtle")]


def stale_scenario(kind, problem, shape, rep, make_env=None):
    """150 steps of the morph, one of the calls below, 50 more steps; with make_env (-> a fresh engine of this config) the engine
    is held against the oracle throughout, without it the oracle runs alone.  -> the Coverage of the steps.
    update: five update() calls of the morph's own actions without refresh_stats(), then steps (the next changing step
    recomputes from scratch); the statistics stay the stale ones in between, as the reference's do.
    state_dict: all envs restarted at step 100 and a snapshot taken; at step 150 the whole state goes into a second engine
    (which has stepped random maps before), then the snapshot of step 100 into every third env of it.
    set_state: every other env gets its neighbour's map through pcgrl_set_state.
    inject: one env of every four (one per wave of the 16-lane kernels) is handed a vertical snake by a masked reset; its
    wave neighbours keep their cached masks and go on."""
    form = FORMS[(shape, rep)]
    n, what = form["n"], f"{kind} {form_id(problem, shape, rep)}"
    orc, driver, cov = make_oracle(problem, rep, shape, n), Morph(problem, rep, shape, n, form["budget"], seed=4), Coverage(problem, shape)
    env = make_env() if make_env else None
    if env is not None:
        import torch

        def dev(a):
            return torch.as_tensor(a).to(env.device)
    run(orc, driver, 100, env=env, cov=cov, what=what)
    if kind == "state_dict":  # restart everyone: the snapshot then is a state the oracle can be put back into
        _, grids, pos = oracle_state(orc)
        old_grids, old_pos = grids.copy(), pos[:, :2].copy()
        orc.reset(init_grids=old_grids, init_pos=old_pos)
        driver.age[:] = 0
        if env is not None:
            env.reset(init_grids=old_grids, init_pos=old_pos)
            old = env.state_dict()
    run(orc, driver, 50, env=env, cov=cov, sync=0, what=what)  # (no restarts: the phases go on)
    _, grids, pos = oracle_state(orc)
    mask = np.ones(n, np.uint8)
    if kind == "update":
        for k in range(5):
            a = driver.actions(grids, pos)
            oobs = orc.update(a)
            if env is not None:
                compare_obs(env, env.update(dev(a)), oobs, f"{what} update {k}")
            _, grids, pos = oracle_state(orc)
    elif kind == "state_dict":
        mask = (np.arange(n) % 3 == 0).astype(np.uint8)
        if env is not None:
            other = make_env()
            other.reset()
            gen = torch.Generator().manual_seed(5)
            for _ in range(3):
                other.step(dev(torch.randint(0, other.num_actions, (n,), dtype=torch.int32, generator=gen)))
            other.load_state_dict(env.state_dict())
            compare_state(other, orc, what + " full")
            env.close()
            env = other
            env.load_state_dict(old, mask=mask)
        orc.reset(mask=mask, init_grids=old_grids, init_pos=old_pos)
    elif kind == "set_state":
        mask = (np.arange(n) % 2 == 0).astype(np.uint8)
        new = np.roll(grids, -1, axis=0)
        if env is not None:
            env.load_state_dict({"grids": dev(new), "pos": dev(pos), "counters": torch.zeros((n, 4), dtype=torch.int32),
                                 "ep_return": torch.zeros(n, dtype=torch.float64), "rng": env.get_rng_state()}, mask=mask)
        orc.reset(mask=mask, init_grids=new, init_pos=pos[:, :2])
    else:
        mask = (np.arange(n) % 4 == 1).astype(np.uint8)
        new = np.broadcast_to(family("snake_v", shape), grids.shape).copy()
        oobs = orc.reset(mask=mask, init_grids=new, init_pos=pos[:, :2])
        if env is not None:
            compare_obs(env, env.reset(mask=mask, init_grids=new, init_pos=pos[:, :2])[0], oobs, what)
    if kind != "update":
        driver.age[mask != 0] = 0
    if env is not None:  # (after update: statistics included, both sides still hold those of the map before)
        compare_state(env, orc, what + " after the call")
    run(orc, driver, 50, env=env, cov=cov, sync=0, obs_every=25, what=what + " afterwards")
    if env is not None:
        env.close()
    return cov


# the other runs of tests/test_gpu_structured_steps.py: (problem, shape, rep, batch, steps, sync, seed)
BIG_BATCH = [("binary", (16, 16), rep, 1027, 300, 10, 2) for rep in ("narrow", "turtle", "wide")]
ROLLOUTS = [((16, 16), "narrow", 1), ((16, 16), "narrow", 2), ((16, 16), "turtle", 1), ((16, 16), "wide", 2),
            ((20, 24), "narrow", -1), ((40, 48), "turtle", -1)]  # (shape, rep, pcgrl_set_rollout_form)
ROLLOUT_STEPS, ROLLOUT_SYNC, ROLLOUT_SEED = 300, 50, 3
CODES = [("binary", (16, 16), "narrow"), ("zelda", (16, 16), "turtle"), ("binary", (40, 48), "narrow"), ("zelda", (40, 48), "turtle")]
CODES_STEPS, CODES_SEED = 300, 6
