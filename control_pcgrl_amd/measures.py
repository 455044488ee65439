"""The Python side of the measure / pack step and the pairwise Hamming step, written once: the entropy table, the result
namespaces and their views (include/pcgrl_amd_measures.h, pcgrl_amd_smb_measures.h, pcgrl_amd_loderunner_measures.h; DESIGN.md
sections 16, 24, 27, 29).  VecPcgrlEnv, SmbMeasures (for SmbVecEnv) and evaluator.py's LevelEvaluator, the base of the level
evaluators, mix it in; each keeps its choice of C entry point, its T and its checks of the grids
argument.  file:line references are relative to the reference's control_pcgrl/ directory.
"""
from contextlib import nullcontext
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib


class MeasuresMixin:
    """A user class has device, _L, _stream() and _meas_dims() -> (cells per map, T).  An entry point `fn` (a function of _L)
    comes with the arguments that stand before its output pointers (`head`: the handle, or H, W, n, grids, ...); the stream
    goes last."""

    _entropy_tab = None  # built at the first measures(entropy=True)
    _meas_set_device = True  # the entry points that take no handle launch on the current device

    def _entropy_table(self):
        """tab[c] = (c / n) * ln(c / n) for c = 0 .. n, then get_entropy's max_val (evolve.py:436) for the class's T: built once
        on the host with numpy's scalar log -- the very operations of get_entropy (evolve.py:441-444) -- and uploaded at first
        use"""
        if self._entropy_tab is None:
            n, T = self._meas_dims()
            tab = np.zeros(n + 2, dtype=np.float64)
            for c in range(1, n + 1):
                p = np.int64(c) / n
                tab[c] = p * np.log(p)
            tab[n + 1] = -(1 / T) * np.log(1 / T) * T
            self._entropy_tab = torch.from_numpy(tab).to(self.device)
        return self._entropy_tab

    def _measures_result(self, fn, head, n, entropy):
        dev, T = self.device, self._meas_dims()[1]
        out = SimpleNamespace(counts=torch.empty((n, T), dtype=torch.int32, device=dev),
                              match=torch.empty((n, 3), dtype=torch.int32, device=dev),
                              forms=torch.empty((n, 5 + T), dtype=torch.float64, device=dev),
                              entropy=torch.empty(n, dtype=torch.float64, device=dev) if entropy else None)
        ent = out.entropy.data_ptr() if entropy else None
        tab = self._entropy_table().data_ptr() if entropy else None
        with torch.cuda.device(dev) if self._meas_set_device else nullcontext():
            _lib.check(fn(*head, out.counts.data_ptr(), out.match.data_ptr(), out.forms.data_ptr(), ent, tab, self._stream()),
                       fn.__name__)
        # the float64 forms come from the kernel (correctly rounded divisions in the reference's order; torch's division by
        # a scalar multiplies by its reciprocal, which is an ulp off now and then): views of its rows
        f = out.forms
        out.tile_fractions = f[:, 5:]  # get_counts (evolve.py:461-464)
        out.bc = {"emptiness": f[:, 0], "symmetry-horizontal": f[:, 1], "symmetry-vertical": f[:, 2], "symmetry": f[:, 3],
                  "co-occurance": f[:, 4]}
        if entropy:
            out.bc["entropy"] = out.entropy
        out.emptiness = out.bc["emptiness"]
        return out

    def _diversity_result(self, fn, head, n, group, pairwise, scratch_bytes):
        """scratch_bytes: what the entry point family's *_diversity_scratch_bytes gives for the n maps"""
        K = n if group is None else int(group)
        dev = self.device
        if K < 2 or n % K:
            raise ValueError(f"diversity: group = {K} must be at least 2 and divide the {n} maps")
        G = n // K
        scratch = torch.empty(max(1, int(scratch_bytes) // 8), dtype=torch.int64, device=dev)
        out = SimpleNamespace(hamming_sum=torch.empty(G, dtype=torch.int64, device=dev),
                              scores=torch.empty((G, 2), dtype=torch.float64, device=dev),
                              nearest=torch.empty(n, dtype=torch.int32, device=dev),
                              nearest_idx=torch.empty(n, dtype=torch.int32, device=dev),
                              pairwise=torch.empty((G, K, K), dtype=torch.int32, device=dev) if pairwise else None)
        pw = out.pairwise.data_ptr() if pairwise else None
        with torch.cuda.device(dev) if self._meas_set_device else nullcontext():
            _lib.check(fn(*head, K, scratch.data_ptr(), out.hamming_sum.data_ptr(), out.scores.data_ptr(), out.nearest.data_ptr(),
                          out.nearest_idx.data_ptr(), pw, self._stream()), fn.__name__)
        out.div_score = out.scores[:, 0]  # div_calc (evaluate_ctrl.py:42-48)
        out.diversity_bonus = out.scores[:, 1]  # evolve.py:1236-1244: N * N - 1, not N * (N - 1)
        return out
