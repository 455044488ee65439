"""The launch rules of asynchronous Super Mario Bros stepping (include/pcgrl_amd_smb_ready.h) in plain
Python, on top of tests/smb_env_rules.py and smb_rules.play, which returns both passes' iteration counts.  Test infrastructure:
the CPU tests replay the fixtures of tests/golden/smb_env through these rules, and the GPU tests pin the kernels to them.

A search of a level takes T = it1 + it2 iterations.  A launch gives the env B iterations, spent in order on whatever the env
searches in that launch; a search ends in the launch in which its T-th iteration runs.

    idle                the env consumes its action; a step whose edit changes a cell's solidity searches.  Finished -> the step
                        completes (EMITTED); else the env holds a pending step (BUSY) and its committed state is the one before.
    pending step        the search resumes; finished -> the step completes, else BUSY.
    a completed step    that ended the episode under auto_reset draws the next episode in the same launch and starts its search
                        with the rest of B; unfinished -> pending statistics, EMITTED | BUSY.
    pending statistics  the search resumes and no action is taken; finished -> 0, once; else BUSY.
    reset               abandons what was in flight and searches the new level within the reset launch; unfinished -> pending
                        statistics.
    bad action          taken by an idle env: nothing changes, reward 0, EMITTED, and the error is remembered.
"""
import copy

import smb_env_rules as E

EMITTED, BUSY = 1, 2  # PCGRL_ENV_EMITTED, PCGRL_ENV_BUSY
IDLE, PENDING_STEP, PENDING_STATS = 0, 1, 2


def search_length(rules):
    """T of the search the rules ran last"""
    return int(rules.rec["it1"]) + int(rules.rec["it2"])


class SmbReadyRules:
    """One env.  `env` (an SmbEnvRules) is the state ahead: it has taken every consumed action.  `committed` is what get_state
    shows: a copy taken before a pending step, else `env` itself (for pending statistics with the statistics, the loss and the
    search count of before: committed_stats)."""

    env_class = E.SmbEnvRules  # (a test may put a subclass here, one that remembers evaluations for instance)

    def __init__(self, *args, **kw):
        self.env = self.env_class(*args, **kw)
        self.mode, self.remaining = IDLE, 0
        self.before = None       # the rules before a pending step
        self.result = None       # what the pending step emits once its search is over
        self.stale = None        # (stats, last_loss) shown while the statistics are pending
        self.error = False
        self.iterations = 0      # every iteration run, abandoned searches included
        self.max_per_launch = 0
        self.committed_searches = 0
        self.launches = 0

    # -- what the device shows ---------------------------------------------------------------------------------------------
    def busy(self):
        return self.mode != IDLE

    def committed(self):
        """the rules whose grid, pos, iteration and changes get_state shows"""
        return self.before if self.mode == PENDING_STEP else self.env

    def committed_stats(self):
        if self.mode == PENDING_STATS:
            return list(self.stale[0]), self.stale[1]
        c = self.committed()
        return list(c.stats), c.last_loss

    def observation(self):
        """the env's row of d_obs after a launch: of the step in flight for a busy env"""
        return self.env.observation()

    # -- pieces ------------------------------------------------------------------------------------------------------------
    def _spend(self, left):
        use = min(left, self.remaining)
        self.remaining -= use
        self.iterations += use
        self._spent += use
        return left - use

    def _begin(self, left, grid=None, pos=None, keep_stale=False):
        """a new episode (self.env.reset) and its search with what the launch has left; -> the launch's BUSY bit"""
        if not keep_stale:  # what get_state shows until the new level's statistics arrive
            self.stale = (list(self.env.stats), self.env.last_loss) if hasattr(self.env, "stats") else ([0] * 9, 0.0)
        self.env.reset(grid, pos)
        self.remaining = search_length(self.env)
        self._spend(left)
        if self.remaining > 0:
            self.mode = PENDING_STATS
            return BUSY
        self.mode = IDLE
        self.committed_searches += 1
        return 0

    def _end_launch(self):
        self.max_per_launch = max(self.max_per_launch, self._spent)

    # -- launches ----------------------------------------------------------------------------------------------------------
    def reset(self, budget, grid=None, pos=None):
        """a reset launch that selects this env -> busy.  Whatever was in flight is abandoned: a pending step leaves no trace (the
        env is the one of before it), pending statistics never arrive."""
        self._spent = 0
        keep_stale = self.mode == PENDING_STATS
        if self.mode == PENDING_STEP:
            self.env = self.before
        self.before = self.result = None
        self.mode, self.remaining = IDLE, 0
        status = self._begin(int(budget), grid, pos, keep_stale)
        self._end_launch()
        return bool(status & BUSY)

    def launch(self, action, budget, auto_reset=True):
        """a step_ready launch -> (status, emitted): emitted is None or a dict with obs (the row the launch wrote), reward, done,
        stats, pos, iteration, changes -- the values SmbEnvRules.step returns, of the finished episode where the step ended one
        (but obs and pos of the new episode then)"""
        self.launches += 1
        self._spent = 0
        left = int(budget)
        if self.mode == PENDING_STATS:
            left = self._spend(left)
            if self.remaining == 0:
                self.mode = IDLE
                self.committed_searches += 1
            self._end_launch()
            return (BUSY if self.mode != IDLE else 0), None
        if self.mode == IDLE:
            a = int(action)
            if not 0 <= a < self.env.num_actions:
                self.error = True
                return EMITTED, dict(obs=self.env.observation(), reward=0.0, done=False, stats=list(self.env.stats),
                                     pos=list(self.env.pos), iteration=self.env.iteration, changes=self.env.changes, bad=True)
            self.before = copy.deepcopy(self.env)
            _, reward, done, info = self.env.step(a, auto_reset=False)
            self.result = dict(reward=reward, done=done, stats=list(info["stats"]), pos=list(info["pos"]),
                               iteration=info["iteration"], changes=info["changes"], searched=info["searched"])
            self.remaining = search_length(self.env) if info["searched"] else 0
            self.mode = PENDING_STEP
        # a pending step, fresh or resumed
        left = self._spend(left)
        if self.remaining > 0:
            self._end_launch()
            return BUSY, None
        out, self.result, self.before = self.result, None, None
        self.committed_searches += int(out.pop("searched"))
        self.mode = IDLE
        status = EMITTED
        if out["done"] and auto_reset:
            status |= self._begin(left)
            out["pos"] = list(self.env.pos)  # as the fixtures record it: the new episode's start
        out["obs"] = self.env.observation()
        self._end_launch()
        return status, out
