"""Controllable generation for the Super Mario Bros environment in plain Python on top of tests/smb_env_rules.py: what
ControlWrapper(ctrl_metrics=cfg.controls) of the reference adds (file:line references are relative to the
reference's control_pcgrl/).  Test infrastructure: the fixtures under tests/golden/smb_ctrl pin these rules to the reference, and
the GPU tests pin the kernels to these rules.

    targets   every env has active targets for all nine statistics; they start as the frozen static ones.  set_trgs only queues
              (control_wrappers.py:167-168: the queue is REPLACED); the queue is applied at the next reset, before the new
              level's loss (:174-187), and replaces the targets of the metrics it names only.
    loss      :318-345: a scalar t gives -|t - val| * w, a tuple (lo, hi) gives -min|arange(lo, hi) - val| * w, which for a
              whole-number lo is the distance to [lo, lo + ceil(hi - lo) - 1].  The engine's sum is specified: the terms in
              STAT_KEYS order, each -(d) * w rounded to double, then added.
    ctrl obs  :189-214: per control (trg / range, metric / range), range = |cond_bounds[1] - cond_bounds[0]|; a tuple target
              shows the midpoint of the RAW tuple.
    resample  the engine's own stream: trg_resampled(seed, env, c, j, lo_j, hi_j) of csrc/pcgrl_kernels2d.h with the env's draw
              counter c, which advances at every reset of that env; the draw replaces whatever was queued.
"""
import math

import smb_env_rules as E
import smb_rules as R

# frozen at the stock 16 x 116 (smb_prob.py:16-26 before smb_ctrl_prob.py:8-36)
COND_BOUNDS = {"dist-floor": (0, 1856), "disjoint-tubes": (0, 1856), "enemies": (0, 1856), "empty": (0, 116), "noise": (0, 1856),
               "jumps": (0, 116), "jumps-dist": (0, 1856), "dist-win": (0, 116), "sol-length": (0, 348.0)}
_M = (1 << 64) - 1


def interval(trg):
    """the zero-loss interval of a target, both ends included"""
    if isinstance(trg, tuple):
        lo, hi = trg
        assert float(lo) == int(lo), "a tuple target's grid starts at a whole number"
        n = int(math.ceil(hi - lo))
        assert n >= 1
        return float(lo), float(lo + n - 1)
    return float(trg), float(trg)


def shown(trg):
    """what the control observation shows for a target (control_wrappers.py:203-204)"""
    return (trg[0] + trg[1]) / 2 if isinstance(trg, tuple) else float(trg)


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & _M
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & _M
    return z ^ (z >> 31)


def trg_resampled(seed, env, c, j, lo, hi):
    """the c-th resampled target of env `env`'s control j under `seed`: uniform in [lo, hi) with a 53-bit u"""
    a = mix64(((seed & _M) + (c & 0xFFFFFFFF) * 0x9e3779b97f4a7c15) & _M)
    b = ((env & 0xFFFFFFFF) * 0xd1b54a32d192ed03 + (j + 1) * 0x8cb92ba72f3d8dd7) & _M
    u = float(mix64(a ^ b) >> 11) * (1.0 / 9007199254740992.0)
    return u * (float(hi) - float(lo)) + float(lo)


class SmbCtrlRules(E.SmbEnvRules):
    def __init__(self, representation, shape, controls, env_index=0, **kw):
        super().__init__(representation, shape, **kw)
        self.controls = list(controls)
        assert all(k in R.STAT_KEYS for k in self.controls) and len(set(self.controls)) == len(self.controls)
        self.trg = {k: interval(R.STATIC_TRGS[k]) for k in R.STAT_KEYS}  # active (lo, hi)
        self.shown = {k: shown(R.STATIC_TRGS[k]) for k in self.controls}
        self.ranges = {k: abs(COND_BOUNDS[k][1] - COND_BOUNDS[k][0]) for k in self.controls}
        self.queue = None
        self.resampling = None  # seed
        self.draws = 0
        self.env_index = int(env_index)

    def set_trgs(self, trgs):
        assert all(k in self.controls for k in trgs)
        self.queue = dict(trgs)

    def set_resampling(self, enable, seed=0):
        self.resampling = int(seed) if enable else None

    def take(self):
        """what a reset does before the new level's loss"""
        if self.resampling is not None:
            for j, k in enumerate(self.controls):
                t = trg_resampled(self.resampling, self.env_index, self.draws, j, *COND_BOUNDS[k])
                self.trg[k], self.shown[k] = (t, t), t
            self.draws += 1
        elif self.queue is not None:
            for k, v in self.queue.items():
                self.trg[k], self.shown[k] = interval(v), shown(v)
        self.queue = None

    def loss(self):
        total = 0.0
        for k, v in zip(R.STAT_KEYS, self.stats):
            lo, hi = self.trg[k]
            v = float(v)
            d = lo - v if v < lo else (v - hi if v > hi else 0.0)
            term = -d * float(self.weights[k])
            total = total + term
        return total

    def reset(self, grid=None, pos=None):
        self.take()
        return super().reset(grid, pos)

    def ctrl_obs(self):
        """[2K] doubles: per control (target / range, metric / range)"""
        out = []
        for k in self.controls:
            out += [self.shown[k] / self.ranges[k], float(self.stats[R.STAT_KEYS.index(k)]) / self.ranges[k]]
        return out
