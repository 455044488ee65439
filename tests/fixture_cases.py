"""The cases of the GPU tests that run a level family's golden fixtures (tests/golden/<family>/): every file with the evaluator's
max_levels as the test always had it (max_levels None, the id the file's name), and once more with a max_levels that is smaller
than the file's number of levels and does not divide it, so that the batch runs as several launches with a shorter last one
against the same recorded answers.  LevelEvaluator._launch (control_pcgrl_amd/evaluator.py) is the one place that slices a
batch's outputs per launch."""
import os

import numpy as np


def split_at(n):
    """a max_levels below n that does not divide it: 3 where that holds, else the first of 4, 5, 7, 2 (None for n <= 2)"""
    return next((m for m in (3, 4, 5, 7, 2) if m < n and n % m), None)


def fixture_cases(files):
    """(cases, ids) for pytest.mark.parametrize("path,max_levels", cases, ids=ids)"""
    cases, ids = [], []
    for f in files:
        name = os.path.basename(f)[:-4]
        cases.append((f, None))
        ids.append(name)
        m = split_at(len(np.load(f)["grids"]))
        if m is not None:  # (a file of two levels has no such number)
            cases.append((f, m))
            ids.append(f"{name}-max_levels{m}")
    return cases, ids
