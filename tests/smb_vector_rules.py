"""The float32 image SmbVectorEnv hands out, in numpy (include/pcgrl_amd_smb_vector.h).  Test
infrastructure: tests/test_smb_vector_cpu.py pins this statement to the plain-Python rules of tests/smb_env_rules.py, and the GPU
tests compare the hand-out kernel with it bit for bit.

    image     float32 [oh][ow][2K + 8].  Channels 0 .. 2K-1: the env's 2K control values, each broadcast over the window -- the
              planes come first (control_wrappers.py:189-214).  Channel 2K: 1.0 outside the map.  Channel 2K + 1 + tile: 1.0
              inside.  Everything else 0.0.
    centring  window row i, column j shows map cell (pos[0] - oh // 2 + i, pos[1] - ow // 2 + j) (wrappers.py:407-437).
"""
import numpy as np

N_TILES = 7


def f32_image(grid, pos, window, ctrl=()):
    grid = np.asarray(grid)
    (H, W), (OH, OW) = grid.shape, (int(window[0]), int(window[1]))
    ctrl = np.asarray(ctrl, np.float32).reshape(-1)
    K2 = ctrl.size
    rows = int(pos[0]) - OH // 2 + np.arange(OH)[:, None]  # the map cell window cell (i, j) shows
    cols = int(pos[1]) - OW // 2 + np.arange(OW)[None, :]
    inside = (rows >= 0) & (rows < H) & (cols >= 0) & (cols < W)
    channel = np.where(inside, 1 + grid[np.clip(rows, 0, H - 1), np.clip(cols, 0, W - 1)].astype(np.int64), 0)
    out = np.zeros((OH, OW, K2 + N_TILES + 1), np.float32)
    out[:, :, :K2] = ctrl
    out[:, :, K2:] = channel[..., None] == np.arange(N_TILES + 1)
    return out


def f32_images(grids, pos, window, ctrl=None):
    """the batch: grids [N][H][W], pos [N][2], ctrl [N][2K] or None"""
    return np.stack([f32_image(g, p, window, () if ctrl is None else ctrl[i]) for i, (g, p) in enumerate(zip(grids, pos))])


def alignment_case(n_ctrl, window):
    """which of the kernel's three store cases a shape is: C = 2K + 8 is a multiple of 4 floats for even K only, and then an
    env's run of oh * ow * C floats is one of 16 bytes; for odd K it is one only when oh * ow is even"""
    if n_ctrl % 2 == 0:
        return "Keven"
    return "Kodd-cells-even" if (int(window[0]) * int(window[1])) % 2 == 0 else "Kodd-cells-odd"
