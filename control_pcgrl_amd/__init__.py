"""control_pcgrl_amd -- MI355X-native batched PCGRL environment engine (host side).

Drop-in for the reference's env hot path only (control_pcgrl/rl/envs.py:make_env and what it builds):
  make_env(cfg)            single-env adapter with the reference's reset()/step() tuple shapes
  make_vec_env(cfg, n)     batched engine: torch tensors in/out, one HIP launch per step for all envs
  VecPcgrlEnv              the batched env class
  MultiAgentVecEnv         cfg.multiagent.n_agents != 0: A turtle agents on one map, a round per launch (binary, zelda)
  PcgrlVectorEnv           the same batch behind ray.rllib's VectorEnv call shape (vector_step / reset_at ...)
  SmbEvaluator             Super Mario Bros levels: the nine statistics, the loss and the A* play-through of a batch of maps
                           in one launch (smb_spec() has the problem's tables)
  SmbVecEnv                cfg.task.problem == "smb": Mario envs stepped on the device (narrow, turtle), one launch per step
                           -- or per K steps: rollout(), with given actions or actions drawn on the device
  SmbReadyVecEnv           the same with cfg.task.solver_budget: a bounded, resumable play-through per launch and a status byte
                           (both take cfg.controls / controls=[...]: per-env targets, queue_targets, ctrl_obs, resampling)
  SmbVectorEnv             the same envs behind the VectorEnv call shape, the float32 Box image written once by a kernel of
                           its own; make_vector_env(cfg, n) picks SmbVectorEnv or PcgrlVectorEnv by problem
  LodeRunnerEvaluator      Lode Runner levels: the five statistics, the loss and the per-gold record of the gold searches of a
                           batch of maps in one launch (loderunner_spec() has the problem's tables); measures(), diversity()
                           and behaviour(): the behaviour vector under the names of LODERUNNER_BC_NAMES; routes(): the cells
                           and moves of both A* paths of every counted gold, the tour behind path-length
  MicrostructureEvaluator  microstructure levels (two-phase maps up to 64 x 64): path-length, tortuosity, the loss and the
                           per-region record of a batch of maps in one launch (microstructure_spec() has the problem's
                           tables); measures(), diversity() and behaviour() under the names of MICROSTRUCTURE_BC_NAMES
  DDaveEvaluator           Dangerous Dave levels: the eleven statistics, the four-stage solver play-through (A* at balance 1,
                           0.5 and 0, then BFS) and the returned action list of a batch of maps in one launch; reward() and
                           episode_over() of the problem (ddave_spec() has its tables); measures(), diversity() and
                           behaviour() under the names of DDAVE_BC_NAMES
  MDungeonEvaluator        MiniDungeon levels: the eleven statistics, the four-stage solver play-through (health, potions,
                           treasures, goblins and ogres; A* at balance 1, 0.5 and 0, then BFS) and the returned move list of a
                           batch of maps in one launch; reward() and episode_over() of the problem (mdungeon_spec() has its
                           tables); measures(), diversity() and behaviour() under the names of MDUNGEON_BC_NAMES
  Mc3dHoleyEvaluator       3-D holey dungeon and maze levels (an entrance and an exit dug into the border of a cube): the
                           statistics, the loss and the routes under the player physics of the 3-D maze (walk, step down,
                           step up, a jump over a gap) of a batch of levels in one launch (mc3d_holey_spec() has the tables);
                           behaviour() under the statistics' names
  DeviceGridArchive        the quality-diversity grid archive on the device: add() places a batch by its behaviour vectors
                           and keeps each cell's best, ask() draws parents from the occupied cells and mutates them, with no
                           host copy; archive_for(evaluator, names) builds the one the reference's loop would
  NcaGenerator             the NCA level generator (the reference's default `--model NCA --representation cellular`): G
                           genomes x S seeds rolled out to their final maps in one launch, bit for bit the numpy twins of
                           control_pcgrl_amd.nca; generator_for(evaluator_or_env) builds the one for an evaluator's maps
  Nca3dGenerator           the 3-D NCA level generator (`--model NCA3D`, cellular3D and cellular3Dholey): the same for maps of
                           3..16 cells an axis, plain or reading the bordered map with its holes, bit for bit the numpy twins
                           of control_pcgrl_amd.nca3d; generator3d_for(evaluator) builds the holey one for a
                           Mc3dHoleyEvaluator, and mc3d_holey_score() is its score in NcaEvolution
  GenomeArchive            the same archive with a genome (float32 [P]) as the elite: ask() hands out Gaussian children with
                           stated arithmetic, sample() the first generation; aggregate() is simulate's fold over a genome's
                           seeds; NcaEvolution chains ask -> generate -> score -> aggregate -> add with no host sync
                           (control_pcgrl_amd.evo has the numpy twins)
  obs_format="codes"       any of them hands out the tile-code observation (one byte per cell); codes_to_onehot()
                           restores the one-hot image on the device
The compute lives in csrc/libpcgrl_amd.so (hand-written HIP for gfx950) behind the C ABI of
include/pcgrl_amd.h; this package fails loudly if that library is missing -- there is no CPU fallback.
"""
from .problems import PROBLEMS, REPRESENTATIONS, ProblemSpec, problem_spec  # noqa: F401
from .vec_env import OBS_FORMATS, SubBatchedVecEnv, VecPcgrlEnv, codes_to_onehot, flatten_wide_action, make_vec_env  # noqa: F401
from .envs import make_env, PcgrlGymEnv  # noqa: F401
from .rllib_env import PcgrlVectorEnv  # noqa: F401
from .multiagent import MultiAgentGymEnv, MultiAgentVecEnv  # noqa: F401
from .dist import EpisodeStatsReducer, shard_env_range  # noqa: F401
from .smb import SmbEvaluator, smb_spec  # noqa: F401
from .smb_env import SmbGymEnv, SmbVecEnv  # noqa: F401
from .smb_ready import SmbReadyVecEnv  # noqa: F401
from .smb_rllib import SmbVectorEnv, make_vector_env  # noqa: F401
from .loderunner import LODERUNNER_BC_NAMES, LodeRunnerEvaluator, loderunner_spec  # noqa: F401
from .microstructure import MICROSTRUCTURE_BC_NAMES, MicrostructureEvaluator, microstructure_spec  # noqa: F401
from .ddave import DDAVE_BC_NAMES, DDaveEvaluator, ddave_spec  # noqa: F401
from .mdungeon import MDUNGEON_BC_NAMES, MDungeonEvaluator, mdungeon_spec  # noqa: F401
from .mc3d_holey import Mc3dHoleyEvaluator, all_holes, fixed_holes, mc3d_holey_spec  # noqa: F401
from .archive import DeviceGridArchive, archive_for  # noqa: F401
from . import nca  # noqa: F401
from .nca import NcaGenerator, generator_for  # noqa: F401
from . import nca3d  # noqa: F401
from .nca3d import Nca3dGenerator, generator3d_for  # noqa: F401

__version__ = "0.7.0"  # csrc/pcgrl_engine.hip pcgrl_version() carries the same number

# The evolution layer (evo.py) is imported at first use, so that importing the package for the env engine alone does what it
# did before that layer existed: `from control_pcgrl_amd import GenomeArchive` and `control_pcgrl_amd.evo` work as usual.
_EVO_EXPORTS = ("GenomeArchive", "NcaEvolution", "aggregate", "evaluator_score", "genome_archive_for", "mc3d_holey_score")


def __getattr__(name):
    if name == "evo" or name in _EVO_EXPORTS:
        import importlib
        module = importlib.import_module(".evo", __name__)
        return module if name == "evo" else getattr(module, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def __dir__():
    return sorted(list(globals()) + ["evo"] + list(_EVO_EXPORTS))
