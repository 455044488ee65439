"""tools/step16_chain_model.py (the CPU model of the 16x16 step kernel's sweep trips) on a small batch: its piece order and
far cells are those of tests/step_masks_numpy.py's rules on the same maps, and its costing is the stated formula.  No GPU."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import step16_chain_model as model  # noqa: E402
import step_masks_numpy as rules  # noqa: E402


def _maps(n, seed, density=0.5):
    return np.random.default_rng(seed).random((n, 16, 16)) < density


def test_piece_order_and_far_cells_are_the_rules():
    for seed, density in ((1, 0.5), (2, 0.65), (3, 0.8)):
        cells = _maps(24, seed, density)
        fars, pieces = model.first_sweeps(cells)
        assert np.array_equal(fars, rules.component_fars(cells))
        assert len(pieces) >= 2
        remaining = cells & ~(cells & ~rules.neighbours(cells))  # isolated cells are their own far cells: no sweep
        prev = np.full(len(cells), -1)
        for has, first, far, levels in pieces:
            assert np.array_equal(has, remaining.any(axis=(1, 2)))
            seed_cell = rules.first_rowmajor(remaining)
            want_levels, last, reached = rules.bfs(seed_cell, remaining)
            flat = lambda x: x.reshape(len(x), -1).argmax(1)  # noqa: E731
            assert np.array_equal(first[has], flat(seed_cell)[has])
            assert (first[has] > prev[has]).all(), "pieces come in row-major order of their first cell"
            assert np.array_equal(far[has], flat(rules.first_rowmajor(last))[has])
            assert np.array_equal(levels[has], want_levels[has]) and (levels[has] >= 1).all() and not levels[~has].any()
            prev = np.where(has, first, prev)
            remaining &= ~reached
        assert not remaining.any()


def test_second_sweep_levels_are_the_rules():
    cells = _maps(16, 5)
    fars, _ = model.first_sweeps(cells)
    assert np.array_equal(model.second_sweep_levels(cells, fars), rules.second_sweeps(cells, fars))


def test_trips_lockstep_and_costing():
    assert model.trips_of(np.array([0, 5, 6, 11, 12, 40])).tolist() == [1, 1, 2, 2, 3, 7]
    # two waves: in the first the envs' first pieces need 1, 3, 0, 2 trips and their second pieces 0, 1, 0, 4; nothing changed
    # in the second wave
    first = np.array([[1, 3, 0, 2, 0, 0, 0, 0], [0, 1, 0, 4, 0, 0, 0, 0]])
    second = np.array([2, 5, 0, 1, 0, 0, 0, 0])
    changed = np.array([1, 1, 0, 1, 0, 0, 0, 0], bool)
    trips, sweeps = model.wave_trips(first, second, changed)
    assert trips.tolist() == [3 + 4 + 5, 0] and sweeps.tolist() == [3, 0]
    assert model.cost(trips, sweeps, 90, 380).tolist() == [12 * 234 + 3 * 380, 0]


def test_a_small_run(capsys, monkeypatch):
    base = model.run(64, 2, 0, 90.0, 380.0)
    assert base["slowest_wave_cycles"] >= base["mean_wave_cycles"] > 0 and base["slowest_wave_sweeps"] >= 2
    # the same maps (same seed) under cheaper trips and a cheaper fixed part
    assert model.run(64, 2, 0, 45.0, 380.0)["slowest_wave_cycles"] < base["slowest_wave_cycles"]
    assert model.run(64, 2, 0, 90.0, 270.0)["mean_wave_cycles"] < base["mean_wave_cycles"]
    monkeypatch.setattr(sys, "argv", ["step16_chain_model.py", "--envs", "64", "--launches", "2"])
    model.main()
    assert json.loads(capsys.readouterr().out) == base
