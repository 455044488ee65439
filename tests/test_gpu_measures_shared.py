"""The measure / pack step is written once (csrc/measures/pcgrl_measures_wave.h, one host path, control_pcgrl_amd/measures.py):
the same bytes through the three families of entry points -- a zelda VecPcgrlEnv's *_for_grids (T = 8), LodeRunnerEvaluator
(T = 8) and SmbEvaluator (T = 7) -- give the same answers bit for bit, also when the batch is a view one byte into a larger
buffer.  Ids 0..6, so every id is a counted tile of all three."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
N, K = 64, 8
DIV_FIELDS = ("hamming_sum", "nearest", "nearest_idx", "scores", "pairwise")


def _results(shape, grids):
    from control_pcgrl_amd import LodeRunnerEvaluator, SmbEvaluator, VecPcgrlEnv
    zelda = VecPcgrlEnv("zelda", "narrow", shape, 2)
    lr, smb = LodeRunnerEvaluator(shape, DEV), SmbEvaluator(shape, DEV, max_levels=1)
    meas = (zelda.measures_for_grids(grids), lr.measures(grids), smb.measures(grids))
    div = (zelda.diversity_for_grids(grids, group=K, pairwise=True), lr.diversity(grids, group=K, pairwise=True),
           smb.diversity(grids, group=K, pairwise=True))
    torch.cuda.synchronize()
    return meas, div


@pytest.mark.parametrize("shape", [(8, 12), (5, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "one-byte-in"])
def test_three_entry_point_families_agree(shape, offset):
    H, W = shape
    rng = np.random.default_rng(1000 * H + W)
    maps = rng.integers(0, 7, size=(N, H, W), dtype=np.uint8)
    buf = torch.zeros(N * H * W + 64, dtype=torch.uint8, device=DEV)
    grids = buf[offset:offset + N * H * W].view(N, H, W)
    grids.copy_(torch.as_tensor(maps))
    assert grids.data_ptr() == buf.data_ptr() + offset and grids.is_contiguous()
    (mz, ml, ms), (dz, dl, ds) = _results(shape, grids)
    # T = 8 twice: everything
    for key in ("counts", "match", "forms", "entropy"):
        assert torch.equal(getattr(mz, key), getattr(ml, key)), key
    # T = 7: the matches, the counts of the seven tiles, the five forms (the fractions follow the counts; the entropy's
    # maximum is ln 7, not ln 8)
    assert torch.equal(ms.match, ml.match)
    assert torch.equal(ms.counts, ml.counts[:, :7]) and int(ml.counts[:, 7].sum()) == 0
    assert torch.equal(ms.forms[:, :5], ml.forms[:, :5])
    for key in DIV_FIELDS:
        assert torch.equal(getattr(dz, key), getattr(dl, key)), key
        assert torch.equal(getattr(ds, key), getattr(dl, key)), key
    # ... and they are the answers: the integers against plain numpy on the host's copy
    assert np.array_equal(ml.counts.cpu().numpy(), np.stack([(maps == t).sum((1, 2)) for t in range(8)], 1))
    g = maps.reshape(N // K, K, H * W)
    pair = (g[:, :, None, :] != g[:, None, :, :]).sum(-1)
    assert np.array_equal(dl.pairwise.cpu().numpy(), pair)
    assert np.array_equal(dl.hamming_sum.cpu().numpy(), pair.sum((1, 2)))
