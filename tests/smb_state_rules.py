"""Checkpoint and restore of Super Mario Bros environments (include/pcgrl_amd_smb_state.h) in plain Python,
on top of tests/smb_env_rules.py and tests/smb_ready_rules.py.  Test infrastructure: the CPU tests check these rules against
themselves (a restored run equals the uninterrupted one), and the GPU tests pin pcgrl_smb_state_export / _import to them launch
by launch.

    image     export(rules) -> what the device's image holds of one env: the COMMITTED env (map, position, counters, statistics,
              last_loss, return, both streams), the counters of searches and iterations, the mode and the pending action.
    in flight a parked search is not in the image.  The iterations it had spent are taken off the exported total, because
    restart   an imported busy env plays its search again from iteration 0: a pending step keeps its action, pending statistics
              keep the fresh level, and `remaining` is the search's whole length again.  A search is a function of the map and
              solver_power, so every emitted transition equals the uninterrupted run's; only the launch it comes in is later.
    modes     an env without a budget (SmbEnvRules) cannot finish a parked search: import_ refuses a busy image for it.
"""
import copy

import smb_env_rules as E
import smb_ready_rules as RR

IDLE, PENDING_STEP, PENDING_STATS = RR.IDLE, RR.PENDING_STEP, RR.PENDING_STATS


class SmbReadyStateRules(RR.SmbReadyRules):
    """SmbReadyRules that remember the action a pending step consumed: the image carries it"""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.action = 0

    def launch(self, action, budget, auto_reset=True):
        if self.mode == IDLE:
            self.action = int(action)
        return super().launch(action, budget, auto_reset)


def in_flight(r):
    """the iterations a busy env's parked search has spent"""
    if r.mode == IDLE:
        return 0
    return RR.search_length(r.env) - r.remaining


def export(r):
    """the image's row of one env: r is an SmbEnvRules (always idle) or an SmbReadyStateRules"""
    if isinstance(r, E.SmbEnvRules):
        return dict(env=copy.deepcopy(r), mode=IDLE, action=0, stale=None, searches=r.searches, iterations=None,
                    max_per_launch=None)
    stale = (list(r.stale[0]), r.stale[1]) if r.mode == PENDING_STATS else None
    return dict(env=copy.deepcopy(r.committed()), mode=r.mode, action=r.action if r.mode == PENDING_STEP else 0, stale=stale,
                searches=r.committed_searches, iterations=r.iterations - in_flight(r), max_per_launch=r.max_per_launch)


def _overwrite(target, source):
    """target becomes a copy of source and keeps its class (a test's subclass that remembers evaluations, for instance)"""
    target.__dict__.clear()
    target.__dict__.update(copy.deepcopy(source.__dict__))


def import_(r, image):
    """r continues as the image's env.  Whatever r had in flight is abandoned."""
    if isinstance(r, E.SmbEnvRules):
        if image["mode"] != IDLE:
            raise NotImplementedError("a busy row into an env without a solver budget")
        _overwrite(r, image["env"])
        r.searches = image["searches"]  # (of a ready image: the searches whose result was committed)
        return
    _overwrite(r.env, image["env"])
    r.before = r.result = r.stale = None
    r.mode, r.remaining = image["mode"], 0
    r.committed_searches = image["searches"]
    r.env.searches = image["searches"]
    if image["iterations"] is not None:  # (an image of an env without a budget counts no launches)
        r.iterations, r.max_per_launch = image["iterations"], image["max_per_launch"]
    if image["mode"] == PENDING_STEP:  # the step is taken again, and its search runs from iteration 0
        r.action = image["action"]
        r.before = copy.deepcopy(r.env)
        _, reward, done, info = r.env.step(r.action, auto_reset=False)
        assert info["searched"], "only a step that searches can be pending"
        r.result = dict(reward=reward, done=done, stats=list(info["stats"]), pos=list(info["pos"]),
                        iteration=info["iteration"], changes=info["changes"], searched=True)
        r.remaining = RR.search_length(r.env)
    elif image["mode"] == PENDING_STATS:  # the fresh level's search runs from iteration 0
        r.stale = (list(image["stale"][0]), image["stale"][1])
        r.env.searches += 1  # (the env ahead has evaluated the level; the count is committed when the search is over)
        r.remaining = RR.search_length(r.env)
