"""Level measures and pairwise Hamming diversity of Super Mario Bros maps, recorded from the REFERENCE's own functions on the
CPU -> tests/golden/smb_measures/smb_<H>x<W>.npz (data only).

    python tools/gen_golden_smb_measures.py     # needs the reference tree; about a minute

Everything is tools/gen_golden_measures.py's: the reference's definitions compiled from its text at generation time
(reference_functions), the env stub, the hand-built maps, the random maps, the diversity cases, the file layout (that file's
docstring has it) and check_worth.  What differs is T = 7 (envs/probs/smb/smb_prob.py:12) and the shapes: the corners of what
the SMB evaluator takes (4..16 rows x 1..128 columns) and the cases the 2-D kernel never met -- one and two columns, odd sizes,
rows longer than a 64-cell chunk, the stock 16 x 116 and the largest map.

Every file stays at or below the size of the largest file under tests/golden/measures/ (38 390 bytes); the number of random
maps per shape is chosen for that.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_measures as gm  # noqa: E402

OUT = os.path.join(gm.ROOT, "tests", "golden", "smb_measures")
SHAPES = [(4, 1), (4, 2), (5, 7), (4, 65), (15, 127), (16, 116), (16, 128)]
N_RANDOM = {(15, 127): 20, (16, 116): 20, (16, 128): 20}  # default 48, as gen_golden_measures
MAX_FILE_BYTES = 38390
T = 7


def main():
    gm.mn.N_TILES.setdefault("smb", T)  # (the rules take any T; the table only names the engine's problems)
    gm.N_RANDOM.update(N_RANDOM)
    ref = gm.reference_functions()
    os.makedirs(OUT, exist_ok=True)
    files = {}
    for si, shape in enumerate(SHAPES):
        z = gm.generate("smb", shape, ref, seed=7000 + si)
        assert z["grids"].max() < T and z["counts"].shape[1] == T
        files[("smb", shape)] = z
        path = os.path.join(OUT, f"smb_{shape[0]}x{shape[1]}.npz")
        np.savez_compressed(path, **z)
        size = os.path.getsize(path)
        print(f"{os.path.basename(path)}: {len(z['grids'])} maps, {size} bytes", flush=True)
        assert size <= MAX_FILE_BYTES, (path, size)
    gm.check_worth(files)


if __name__ == "__main__":
    main()
