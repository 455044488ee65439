"""The level measures and the pairwise Hamming diversity (include/pcgrl_amd_measures.h) stated in plain numpy: our own
statement of the reference's rules, citing its lines.  The kernels are checked against this file, and this file against the
fixtures recorded from the reference's own functions (tools/gen_golden_measures.py -> tests/golden/measures/).

Integers first (what the kernels produce), then the float64 forms made from them in the reference's order of operations."""
import numpy as np

N_TILES = {"binary": 2, "zelda": 8, "sokoban": 5}
BC_NAMES = ("emptiness", "entropy", "symmetry", "symmetry-horizontal", "symmetry-vertical", "co-occurance")


def n_planes(T):
    return int(np.ceil(np.log2(T)))


def mask_ids(grids, T):
    """tile ids as the engine keeps them: the low ceil(log2 T) bits"""
    return np.asarray(grids, dtype=np.uint8) & np.uint8((1 << n_planes(T)) - 1)


# ---------------------------------------------------------------------------------------------------------- integers
def counts(grids, T):
    """int32 [n, T]: cells per tile (evolve.py:441, :462, :494)"""
    g = mask_ids(grids, T).reshape(len(grids), -1)
    return np.stack([(g == t).sum(1) for t in range(T)], axis=1).astype(np.int32)


def matches(grids, T, wrap=True):
    """int32 [n, 3]: horizontal matches (evolve.py:512-527: the top H // 2 rows against the bottom H // 2 flipped, the middle
    row of an odd H left out), vertical matches (:545-560, the same over columns), co-occurance matches (:585-590: the four
    np.roll comparisons, which wrap around).  wrap=False is the wrong, non-wrapping rule, for the fixtures' self-check."""
    g = mask_ids(grids, T)
    n, H, W = g.shape
    hor = (g[:, :H // 2] == g[:, ::-1][:, :H // 2]).reshape(n, -1).sum(1)
    ver = (g[:, :, :W // 2] == g[:, :, ::-1][:, :, :W // 2]).reshape(n, -1).sum(1)
    if wrap:
        co = sum((np.roll(g, s, axis=ax) == g).reshape(n, -1).sum(1) for ax in (1, 2) for s in (1, -1))
    else:
        co = 2 * ((g[:, 1:] == g[:, :-1]).reshape(n, -1).sum(1) + (g[:, :, 1:] == g[:, :, :-1]).reshape(n, -1).sum(1))
    return np.stack([hor, ver, co], axis=1).astype(np.int32)


def pairwise(grids, T, per_bit=False):
    """int32 [K, K]: cells whose tiles differ (evaluate_ctrl.py:43 np.sum(a != b)); one cell counts once.  per_bit=True is the
    wrong rule that counts differing id bits, for the fixtures' self-check."""
    g = mask_ids(grids, T).reshape(len(grids), -1)
    if per_bit:
        x = g[:, None] ^ g[None]
        return sum(((x >> b) & 1).sum(-1) for b in range(8)).astype(np.int32)
    return (g[:, None] != g[None]).sum(-1).astype(np.int32)


def hamming_sum(grids, T):
    """S over all ordered pairs of one group by the per-cell histogram identity: a cell where tile t occurs count_t times among
    the K maps has K^2 - sum_t count_t^2 ordered pairs that differ.  int64; no K x K matrix."""
    g = mask_ids(grids, T).reshape(len(grids), -1)
    K, n = g.shape
    sq = np.zeros(n, dtype=np.int64)
    for t in range(1 << n_planes(T)):
        c = (g == t).sum(0).astype(np.int64)
        sq += c * c
    return int(np.int64(K) * K * n - sq.sum())


def nearest(d, lowest=True):
    """(nearest distance, its index) per row of a K x K distance matrix, the diagonal excluded; the lowest index on ties
    (lowest=False: the highest, the wrong rule, for the fixtures' self-check)"""
    K = len(d)
    dd = d.astype(np.int64) + np.where(np.eye(K, dtype=bool), np.int64(1) << 40, 0)
    if lowest:
        idx = dd.argmin(1)
    else:
        idx = K - 1 - dd[:, ::-1].argmin(1)
    return dd[np.arange(K), idx].astype(np.int32), idx.astype(np.int32)


def diversity(grids, T, group):
    """per consecutive group of `group` maps: S int64 [G], nearest / nearest_idx int32 [n], pairwise int32 [G, K, K]"""
    n, K = len(grids), group
    assert K >= 2 and n % K == 0
    S, near, idx, mats = [], [], [], []
    for g in range(n // K):
        d = pairwise(grids[g * K:(g + 1) * K], T)
        a, b = nearest(d)
        S.append(int(d.sum(dtype=np.int64)))
        near.append(a)
        idx.append(b)
        mats.append(d)
    return np.array(S, dtype=np.int64), np.concatenate(near), np.concatenate(idx), np.stack(mats)


# ------------------------------------------------------------------------------------------------------- float64 forms
def entropy_table(n, T):
    """tab[c] = (c / n) * ln(c / n), c = 0 .. n (tab[0] unused), then get_entropy's max_val (evolve.py:436) -- scalar numpy
    operations, as get_entropy performs them (evolve.py:441-444)"""
    tab = np.zeros(n + 2, dtype=np.float64)
    for c in range(1, n + 1):
        p = np.int64(c) / n
        tab[c] = p * np.log(p)
    tab[n + 1] = -(1 / T) * np.log(1 / T) * T
    return tab


def entropy(cnt, n, T, tab=None):
    """get_entropy (evolve.py:423-446) from the counts: float64 [n_maps]"""
    tab = entropy_table(n, T) if tab is None else tab
    out = np.zeros(len(cnt), dtype=np.float64)
    for i, row in enumerate(cnt):
        e = 0.0
        for t in range(T):
            if row[t] != 0:
                e -= tab[row[t]]
        out[i] = e / tab[n + 1]
    return out


def bc_from_integers(cnt, mat, H, W, T, sym_divisor=None):
    """the float64 forms under get_bc's names (evolve.py:606-635) from counts int32 [n, T] and matches int32 [n, 3]"""
    n = H * W
    half = W * H / 2 if sym_divisor is None else sym_divisor  # a float: evolve.py:507, :540
    hor = mat[:, 0].astype(np.float64) / half
    ver = mat[:, 1].astype(np.float64) / half
    return {"emptiness": cnt[:, 0].astype(np.float64) / n,  # evolve.py:494
            "entropy": entropy(cnt, n, T),
            "symmetry-horizontal": hor, "symmetry-vertical": ver,
            "symmetry": (ver + hor) / 2.0,  # evolve.py:575
            "co-occurance": mat[:, 2].astype(np.float64) / (n * 4)}  # evolve.py:584-592


def tile_fractions(cnt, n):
    return cnt.astype(np.float64) / n  # get_counts, evolve.py:461-464


def div_score(S, K, n):
    """div_calc (evaluate_ctrl.py:42-48): S / (K (K - 1)), then / n"""
    return np.asarray(S, dtype=np.int64) / (K * (K - 1)) / n


def diversity_bonus(S, K, n, denominator=None):
    """evolve.py:1236-1244: S / (K * K - 1) -- not K (K - 1) --, then 10 * that / n"""
    den = K * K - 1 if denominator is None else denominator
    return 10 * (np.asarray(S, dtype=np.int64) / den) / n
