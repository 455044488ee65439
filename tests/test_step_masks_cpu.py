"""tests/step_masks_numpy.py proved on the CPU: a numpy model of the single-cell update of csrc/pcgrl_kernels2d.h
(binary_stats_update with the PREFLOOD hand-over) keeps every rule over random and scripted edit sequences and agrees with the
oracle's statistics at every step, and each of four wrong variants of it is reported -- never later than a comparison of the
statistics alone notices it, and sooner for the `best` and PREFLOOD variants (the figures are printed; DESIGN.md section 34
records them).

A fifth variant is BENIGN: `l >= path_len` instead of `l > path_len` (a component that draws with the maximum takes `best`
over) changes no statistic and breaks no rule -- `best` then marks another of the components that attain the maximum.  Both
are correct updates, which is why `best` has rules and no exact formula (test_the_benign_variant...)."""
import numpy as np
import pytest

import pcgrl_oracle as po
import step_masks_numpy as sm
import structured_maps as maps

VARIANTS = ("best_not_refreshed", "hit_without_x", "fars_cleared_on_K_only", "preflood_kept_across_a_move")
STEPS, N_ENVS, DENSITIES = 200, 12, (0.3, 0.5, 0.7)


def cells_to_words(cells):
    return (cells.astype(np.uint32) << np.arange(sm.W, dtype=np.uint32)).sum(axis=2).astype(np.uint32)


class Model:
    """n envs: map, position, regions / path-length, the fars / best masks and the PREFLOOD plane, updated as the kernels do"""

    def __init__(self, grids, pos, rep, variant=None, use_pre=True):
        self.g, self.pos = np.array(grids, np.uint8), np.array(pos, np.int64)[:, :2]
        self.rep, self.variant, self.use_pre = rep, variant, use_pre
        self.n, self.n_step = len(self.g), np.zeros(len(self.g), np.int64)
        self.fars = sm.component_fars(self.g == 0)  # binary_stats_full
        self.len, last, _ = sm.bfs(self.fars, self.g == 0)
        self.best = last & (self.len > 0)[:, None, None]
        self.reg = self.fars.sum(axis=(1, 2))
        self.pre_valid, self.pre = np.zeros(self.n, bool), np.zeros_like(self.fars)

    def edit(self, r, c, tile):
        """binary_stats_update after writing tile [n] (-1: nothing) to the cells (r [n], c [n])"""
        idx = np.arange(self.n)
        p_old, x = self.g == 0, np.zeros_like(self.fars)
        x[idx, r, c] = (tile >= 0) & (self.g[idx, r, c] != tile)
        self.g[idx, r, c] = np.where(tile >= 0, tile, self.g[idx, r, c])
        p_new = self.g == 0
        edited, became = x.any(axis=(1, 2)), (x & p_new).any(axis=(1, 2))
        K = sm.flood(x, np.where(became[:, None, None], p_new, p_old))
        have_pre = self.pre_valid & self.use_pre
        K = np.where(have_pre[:, None, None], self.pre & edited[:, None, None], K)
        K &= ~(x & ~became[:, None, None])
        touched = K | x
        hit = (self.best & (K if self.variant == "hit_without_x" else touched)).any(axis=(1, 2))
        newfars = sm.component_fars(K)
        self.fars = (self.fars & ~(K if self.variant == "fars_cleared_on_K_only" else touched)) | newfars
        l, b, _ = sm.bfs(np.where(hit[:, None, None], self.fars, newfars), p_new)  # the second sweep
        b &= (l > 0)[:, None, None]
        more = l >= self.len if self.variant == "l >= path_len" else l > self.len
        take = edited & (hit | more)
        self.reg = np.where(edited, self.fars.sum(axis=(1, 2)), self.reg)
        self.len = np.where(take, l, self.len)
        if self.variant == "best_not_refreshed":
            take &= hit
        self.best = np.where(take[:, None, None], b, self.best)
        return edited

    def step(self, action):
        """one narrow / turtle step with an observation: the edit at `pos`, the move, the PREFLOOD plane of the new `pos`"""
        r, c = self.pos[:, 0].copy(), self.pos[:, 1].copy()
        tile = action if self.rep == "narrow" else np.where(action >= 4, action - 4, -1)
        edited = self.edit(r, c, tile)
        if self.rep == "narrow":
            idx = self.n_step % (sm.H * sm.W)
            self.pos = np.stack([idx // sm.W, idx % sm.W], axis=1)
            self.n_step += 1
        else:
            d = np.array([(-1, 0), (1, 0), (0, -1), (0, 1), (0, 0), (0, 0)])[action]
            self.pos = np.clip(self.pos + d, 0, sm.H - 1)
        fresh = sm.expected_preflood(self.g, self.pos)
        keep = self.pre_valid & ~edited if self.variant == "preflood_kept_across_a_move" else np.zeros(self.n, bool)
        self.pre = np.where(keep[:, None, None], self.pre, fresh)
        self.pre_valid[:] = True

    def planes(self):
        pre = cells_to_words(self.pre) | np.where(self.pre_valid, sm.PRE_VALID, np.uint32(0))[:, None]
        return np.stack([cells_to_words(self.g != 0), cells_to_words(self.fars), cells_to_words(self.best), pre], axis=1)

    def broken(self):
        """per env: the first broken rule, or None"""
        return sm.masks_violations(self.g, self.pos, self.planes(), np.stack([self.reg, self.len], axis=1))

    def stats_wrong(self):
        """per env: do regions / path-length differ from the oracle's, computed from scratch?"""
        return (po.stats_for_grids("binary", np.ascontiguousarray(self.g)) != np.stack([self.reg, self.len], axis=1)).any(axis=1)


def random_model(rep, density, seed, variant=None, **kw):
    rng = np.random.default_rng(seed)
    grids = (rng.random((N_ENVS, sm.H, sm.W)) < density).astype(np.uint8)
    pos = np.zeros((N_ENVS, 2), np.int64) if rep == "narrow" else rng.integers(0, sm.H, (N_ENVS, 2))
    return Model(grids, pos, rep, variant, **kw), rng


def random_actions(rep, rng):
    """narrow: a tile; turtle: half moves, half tiles (a uniform turtle edits a third of the time)"""
    if rep == "narrow":
        return rng.integers(0, 2, N_ENVS)
    return np.where(rng.random(N_ENVS) < 0.5, rng.integers(0, 4, N_ENVS), rng.integers(4, 6, N_ENVS))


def run_random(rep, density, seed, variant=None, steps=STEPS, **kw):
    """-> per env the first step (1-based) at which the checker / the statistics report the model, 0 = never"""
    m, rng = random_model(rep, density, seed, variant, **kw)
    assert not any(m.broken()) and not m.stats_wrong().any(), "start"
    by_rules, by_stats = np.zeros(N_ENVS, np.int64), np.zeros(N_ENVS, np.int64)
    for t in range(1, steps + 1):
        m.step(random_actions(rep, rng))
        bad = np.array([b is not None for b in m.broken()])
        by_rules[(by_rules == 0) & bad] = t
        by_stats[(by_stats == 0) & m.stats_wrong()] = t
    return by_rules, by_stats


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("rep", ["narrow", "turtle"])
def test_the_model_keeps_every_rule_on_random_edits(rep, density):
    """with the PREFLOOD hand-over (as step16_kernel / step_kernel with an observation) and without it (the in-kernel flood)"""
    for use_pre, steps in ((True, 100), (False, 50)):
        by_rules, by_stats = run_random(rep, density, seed=11, use_pre=use_pre, steps=steps)
        assert not by_rules.any() and not by_stats.any(), (use_pre, by_rules, by_stats)


@pytest.mark.parametrize("rep", ["turtle", "wide"])
def test_the_model_keeps_every_rule_on_the_scripted_edits(rep):
    """structured_maps.Script on 16 x 16: cuts, fills up to a tie, a bridge between tied components, far cells off the corners"""
    n = len(maps.edit_scripts((sm.H, sm.W)))
    driver = maps.Script(rep, (sm.H, sm.W), n)
    m = Model(driver.start_maps(), np.zeros((n, 2), np.int64), rep)
    edits = 0
    for t in range(maps.script_steps((sm.H, sm.W), rep)):
        a = driver.actions(m.g, m.pos)
        if rep == "turtle":
            edits += int((a >= 4).sum())
            m.step(a)
        else:  # wide: the action names the cell (structured_maps.wide_action), no PREFLOOD plane
            cell, tile = a // 2, a % 2
            edits += int(m.edit(cell % sm.W, cell // sm.W, tile).sum())
        assert not any(m.broken()), (t, m.broken())
        assert not m.stats_wrong().any(), t
    assert edits >= 4 * n


RUNS = (("narrow", 1), ("turtle", 2))  # (representation, seed) of the runs the variants and the true model are put through


def test_every_wrong_variant_is_reported_and_no_later_than_by_its_statistics(capsys):
    """the figures printed here are records, not thresholds: a variant must be reported, that is all"""
    lines = []
    for variant in VARIANTS:
        reported = 0
        for rep, seed in RUNS:
            rules, stats = run_random(rep, 0.5, seed, variant)
            reported += int((rules > 0).sum())
            # a wrong statistic is a broken rule (regions == popcount(fars), path-length == the longest second sweep)
            assert ((rules > 0) & (rules <= stats))[stats > 0].all(), (variant, rep, rules, stats)
            hit, late, both = rules[rules > 0], stats[stats > 0], (rules > 0) & (stats > 0)
            line = f"{variant:28s} {rep:6s} rules: {len(hit):2d}/{N_ENVS} envs"
            if len(hit):
                line += f", first after {hit.min()}, median {int(np.median(hit))}"
            line += f" | statistics only: {len(late):2d}/{N_ENVS} envs"
            if len(late):
                line += f", first after {late.min()}, median {int(np.median(late))}, median delay {int(np.median((stats - rules)[both]))}"
            lines.append(line)
        assert reported > 0, variant
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_the_true_model_is_reported_on_none_of_those_runs():
    for rep, seed in RUNS:
        by_rules, by_stats = run_random(rep, 0.5, seed)
        assert not by_rules.any() and not by_stats.any(), (rep, seed, by_rules, by_stats)


def test_the_benign_variant_changes_neither_statistics_nor_rules_but_best():
    """`l >= path_len`: the reason `best` has no exact formula"""
    differs = 0
    for rep in ("narrow", "turtle"):
        a, rng = random_model(rep, 0.5, 3)
        b, _ = random_model(rep, 0.5, 3, "l >= path_len")
        for t in range(STEPS // 2):
            act = random_actions(rep, rng)
            a.step(act), b.step(act)
            assert not any(b.broken()) and not b.stats_wrong().any(), (rep, t, b.broken())
            assert np.array_equal(a.fars, b.fars) and np.array_equal(a.len, b.len)
            differs += int((a.best != b.best).any())
    assert differs > 0, "the tie never arose: choose another seed"


def test_the_checker_reads_words_and_images_as_laid_out():
    m, _ = random_model("narrow", 0.5, 5)
    m.step(np.zeros(N_ENVS, np.int64))
    planes = m.planes()
    image = np.zeros(sm.STATE_HDR_BYTES + 2 * N_ENVS * 256, np.uint8)
    image[:8] = np.frombuffer(np.uint64(sm.STATE_MAGIC).tobytes(), np.uint8)
    image[16:20] = np.frombuffer(np.int32(N_ENVS).tobytes(), np.uint8)
    image[sm.STATE_HDR_BYTES:sm.STATE_HDR_BYTES + planes.nbytes] = np.frombuffer(planes.tobytes(), np.uint8)
    image[sm.STATE_HDR_BYTES + planes.nbytes + sm.ENV_RECORD_BYTES * 3 + sm.FLAGS_AT] = sm.ENV_STATS_DIRTY
    assert np.array_equal(sm.planes_of(image, N_ENVS, m.g), planes)
    assert sm.flags_of(image, N_ENVS).tolist() == [0, 0, 0, 1] + [0] * (N_ENVS - 4)
    with pytest.raises(AssertionError, match="plane 0"):
        sm.planes_of(image, N_ENVS, 1 - m.g)
    with pytest.raises(AssertionError, match="n_envs"):
        sm.planes_of(image, N_ENVS + 1)
    # the PREFLOOD plane's either-or: a mix of valid and non-valid rows, stray bits, a valid plane of another cell
    for i in range(N_ENVS):
        assert sm.preflood_violation(m.g[i], m.pos[i], planes[i, 3]) is None
        assert sm.preflood_violation(m.g[i], m.pos[i], np.zeros(16, np.uint32)) is None
    mixed = planes[0, 3].copy(); mixed[7] &= ~sm.PRE_VALID
    assert "neither" in sm.preflood_violation(m.g[0], m.pos[0], mixed)
    stray = planes[0, 3].copy(); stray[2] |= np.uint32(1 << 20)
    assert "neither" in sm.preflood_violation(m.g[0], m.pos[0], stray)
    other = np.full(16, sm.PRE_VALID, np.uint32)  # valid and empty: no cell's component (the cell itself always belongs)
    assert "not the component" in sm.preflood_violation(m.g[0], m.pos[0], other)
    # best: each rule by hand on a corridor of four cells next to an isolated one
    g = np.ones((1, sm.H, sm.W), np.uint8); g[0, 0, :4] = 0; g[0, 5, 5] = 0
    fars = sm.expected_fars(g)
    assert sorted(zip(*np.nonzero(fars[0]))) == [(0, 3), (5, 5)]
    end = np.zeros_like(fars); end[0, 0, 0] = True
    assert sm.best_violation(g, fars, end, [3]) is None
    solid, iso = np.zeros_like(fars), np.zeros_like(fars)
    solid[0, 9, 9], iso[0, 5, 5] = True, True
    assert "solid" in sm.best_violation(g, fars, solid, [3])
    assert "non-empty" in sm.best_violation(g, fars, np.zeros_like(fars), [3])
    assert "non-empty" in sm.best_violation(g, fars, end, [0])
    assert "second sweep" in sm.best_violation(g, fars, iso, [3])
    assert "second sweep" in sm.best_violation(g, fars, end, [2])
