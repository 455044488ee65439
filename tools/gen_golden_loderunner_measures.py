"""Level measures and pairwise Hamming diversity of Lode Runner maps, recorded from the REFERENCE's own functions on the CPU
-> tests/golden/loderunner_measures/lr_<H>x<W>.npz (data only).

    python tools/gen_golden_loderunner_measures.py     # needs the reference tree; about a minute

Everything is tools/gen_golden_measures.py's: the reference's definitions compiled from its text at generation time
(reference_functions), the env stub, the hand-built maps, the random maps, the diversity cases, the file layout (that file's
docstring has it) and check_worth.  What differs is T = 8 (envs/probs/loderunner_prob.py:46) and the shapes: the corners of
what the Lode Runner evaluator takes (1..16 rows x 1..32 columns) and the cases they bring -- a single cell, one row, one and
two columns, odd sizes, a partly empty 64-cell chunk, the stock 8 x 12 and the largest map (eight full chunks).

Every file stays at or below the size of the largest file under tests/golden/measures/ (38 390 bytes).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_measures as gm  # noqa: E402

OUT = os.path.join(gm.ROOT, "tests", "golden", "loderunner_measures")
SHAPES = [(1, 1), (2, 1), (1, 2), (1, 32), (16, 1), (5, 7), (8, 12), (15, 31), (16, 32)]
MAX_FILE_BYTES = 38390
T = 8


def main():
    gm.mn.N_TILES.setdefault("loderunner", T)  # (the rules take any T; the table only names the engine's problems)
    ref = gm.reference_functions()
    os.makedirs(OUT, exist_ok=True)
    files = {}
    for si, shape in enumerate(SHAPES):
        z = gm.generate("loderunner", shape, ref, seed=9000 + si)
        assert z["grids"].max() < T and z["counts"].shape[1] == T
        files[("loderunner", shape)] = z
        path = os.path.join(OUT, f"lr_{shape[0]}x{shape[1]}.npz")
        np.savez_compressed(path, **z)
        size = os.path.getsize(path)
        print(f"{os.path.basename(path)}: {len(z['grids'])} maps, {size} bytes", flush=True)
        assert size <= MAX_FILE_BYTES, (path, size)
    gm.check_worth(files)


if __name__ == "__main__":
    main()
