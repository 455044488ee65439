"""ctypes binding of csrc/libpcgrl_amd.so (the C ABI of include/pcgrl_amd.h).  No fallback: a missing or
stale library is an error."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libpcgrl_amd.so")


def _csrc_files(ext):
    """the files of that extension under csrc/, relative with forward slashes, sorted; build directories (_obj*) left out"""
    found = []
    for root, dirs, files in os.walk(CSRC):
        dirs[:] = [d for d in dirs if not d.startswith("_obj")]
        found += [os.path.relpath(os.path.join(root, f), CSRC).replace(os.sep, "/") for f in files if f.endswith(ext)]
    return sorted(found)


# translation units (compiled in parallel, see csrc/pcgrl_dispatch.h) and the headers they depend on: every file under csrc/
UNITS = _csrc_files(".hip")
HEADERS = _csrc_files(".h")
SOURCES = UNITS + HEADERS


def _include(name):
    return os.path.join(os.path.dirname(_HERE), "include", name)


HEADER = _include("pcgrl_amd.h")
CODES_HEADER = _include("pcgrl_amd_codes.h")
ASYNC3D_HEADER = _include("pcgrl_amd_async3d.h")
PATHS_HEADER = _include("pcgrl_amd_paths.h")
SOLUTIONS_HEADER = _include("pcgrl_amd_solutions.h")
MULTIAGENT_HEADER = _include("pcgrl_amd_multiagent.h")
MEASURES_HEADER = _include("pcgrl_amd_measures.h")
SMB_HEADER = _include("pcgrl_amd_smb.h")
SMB_ENV_HEADER = _include("pcgrl_amd_smb_env.h")
SMB_READY_HEADER = _include("pcgrl_amd_smb_ready.h")
SMB_STATE_HEADER = _include("pcgrl_amd_smb_state.h")
SMB_ROLLOUT_HEADER = _include("pcgrl_amd_smb_rollout.h")
SMB_CTRL_HEADER = _include("pcgrl_amd_smb_ctrl.h")
SMB_VECTOR_HEADER = _include("pcgrl_amd_smb_vector.h")
SMB_MEASURES_HEADER = _include("pcgrl_amd_smb_measures.h")
LODERUNNER_HEADER = _include("pcgrl_amd_loderunner.h")
LODERUNNER_MEASURES_HEADER = _include("pcgrl_amd_loderunner_measures.h")
LODERUNNER_ROUTES_HEADER = _include("pcgrl_amd_loderunner_routes.h")
MICROSTRUCTURE_HEADER = _include("pcgrl_amd_microstructure.h")
DDAVE_HEADER = _include("pcgrl_amd_ddave.h")
MDUNGEON_HEADER = _include("pcgrl_amd_mdungeon.h")
ARCHIVE_HEADER = _include("pcgrl_amd_archive.h")
MC3D_HOLEY_HEADER = _include("pcgrl_amd_mc3d_holey.h")
NCA_HEADER = _include("pcgrl_amd_nca.h")
NCA3D_HEADER = _include("pcgrl_amd_nca3d.h")
EVO_HEADER = _include("pcgrl_amd_evo.h")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-falign-loops=32", "-fPIC"]

PCGRL_MAX_STATS = 8
ERRORS = {1: "EINVAL", 2: "EUNSUPPORTED", 3: "EHIP", 4: "EACTION", 5: "ESTALE"}


class PcgrlConfig(C.Structure):
    _fields_ = [
        ("problem", C.c_int32), ("representation", C.c_int32), ("ndim", C.c_int32),
        ("dims", C.c_int32 * 3), ("obs_window", C.c_int32 * 3),
        ("max_iterations", C.c_int32), ("max_changes", C.c_int32), ("n_stats", C.c_int32),
        ("has_trg", C.c_int32 * PCGRL_MAX_STATS), ("weights", C.c_double * PCGRL_MAX_STATS),
        ("trg_lo", C.c_double * PCGRL_MAX_STATS), ("trg_hi", C.c_double * PCGRL_MAX_STATS),
        ("solver_power", C.c_int32),
        ("n_ctrl", C.c_int32), ("ctrl_idx", C.c_int32 * PCGRL_MAX_STATS), ("ctrl_range", C.c_double * PCGRL_MAX_STATS),
        ("act_window", C.c_int32 * 3), ("static_tiles", C.c_int32), ("n_static_walls", C.c_int32),
        ("static_eval", C.c_int32), ("static_prob", C.c_double),
    ]


SYMBOLS = {
    # name: (restype, argtypes)
    "pcgrl_create": (C.c_int, [C.POINTER(PcgrlConfig), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "pcgrl_destroy": (None, [C.c_void_p]),
    "pcgrl_seed": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pcgrl_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_step_seq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p]),
    "pcgrl_step_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_rollout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_rollout_is_one_launch": (C.c_int32, [C.c_void_p]),
    "pcgrl_set_rollout_form": (C.c_int, [C.c_void_p, C.c_int32]),
    "pcgrl_rollout_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_queue_targets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_ctrl_observe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_set_target_resampling": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p]),
    "pcgrl_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_refresh_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_observe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_get_static": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_set_static": (C.c_int, [C.c_void_p, C.c_double, C.c_int32, C.c_int32]),
    "pcgrl_obs_bytes": (C.c_int64, [C.c_void_p]),
    "pcgrl_obs_shape": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32 * 4), C.POINTER(C.c_int32)]),
    "pcgrl_get_state": (C.c_int, [C.c_void_p] + [C.c_void_p] * 7),
    "pcgrl_get_last_episode": (C.c_int, [C.c_void_p] + [C.c_void_p] * 5),
    "pcgrl_stats_for_grids": (C.c_int, [C.POINTER(PcgrlConfig), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                        C.c_void_p]),
    "pcgrl_stats_for_grids_h": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_stats_poll_error": (C.c_int, [C.POINTER(PcgrlConfig), C.c_int32]),
    "pcgrl_stats_cache_clear": (None, []),
    "pcgrl_reduce_episodes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "pcgrl_set_state": (C.c_int, [C.c_void_p] + [C.c_void_p] * 6),
    "pcgrl_state_bytes": (C.c_int64, [C.c_void_p]),
    "pcgrl_export_state": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "pcgrl_import_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "pcgrl_get_rng_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_set_rng_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_poll_error": (C.c_int, [C.c_void_p]),
    "pcgrl_sample_actions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "pcgrl_num_actions": (C.c_int32, [C.c_void_p]),
    "pcgrl_set_solver_budget": (C.c_int, [C.c_void_p, C.c_int32]),
    "pcgrl_get_solver_budget": (C.c_int32, [C.c_void_p]),
    "pcgrl_step_ready": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "pcgrl_env_busy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_reserve_solver_pool": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "pcgrl_solver_pool_slots": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "pcgrl_copy_to_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "pcgrl_stream_synchronize": (C.c_int, [C.c_void_p]),
    "pcgrl_graph_upload": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pcgrl_debug_counters": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "pcgrl_last_error": (C.c_char_p, []),
    "pcgrl_version": (C.c_char_p, []),
}

# include/pcgrl_amd_codes.h: the tile-code observation form
CODES_SYMBOLS = {
    "pcgrl_codes_shape": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32 * 4), C.POINTER(C.c_int32)]),
    "pcgrl_codes_bytes": (C.c_int64, [C.c_void_p]),
    "pcgrl_observe_codes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_onehot_to_codes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "pcgrl_step_ready_codes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 7),
}

# include/pcgrl_amd_async3d.h: asynchronous stepping of the 3-D maze (the entry points themselves are pcgrl_amd.h's)
ASYNC3D_SYMBOLS = {
    "pcgrl_park_bytes_per_env": (C.c_int64, [C.c_void_p]),
}

# include/pcgrl_amd_paths.h: solution paths of binary / zelda maps
PATHS_SYMBOLS = {
    "pcgrl_path_capacity": (C.c_int32, [C.c_void_p]),
    "pcgrl_paths": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_paths_for_grids": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
}

# include/pcgrl_amd_solutions.h: sokoban solutions (the move list behind sol-length)
SOLUTIONS_SYMBOLS = {
    "pcgrl_solution_capacity": (C.c_int32, [C.c_void_p]),
    "pcgrl_solutions": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_solutions_for_grids": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
}

# include/pcgrl_amd_multiagent.h: multi-agent turtle stepping (binary, zelda)
MULTIAGENT_SYMBOLS = {
    "pcgrl_ma_attach": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "pcgrl_ma_attached": (C.c_int32, [C.c_void_p]),
    "pcgrl_ma_obs_shape": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32 * 4), C.POINTER(C.c_int32)]),
    "pcgrl_ma_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_ma_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 6),
    "pcgrl_ma_observe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_ma_get_state": (C.c_int, [C.c_void_p] + [C.c_void_p] * 4),
    "pcgrl_ma_set_state": (C.c_int, [C.c_void_p] + [C.c_void_p] * 5),
}

# include/pcgrl_amd_measures.h: level measures and pairwise Hamming diversity of 2-D maps
MEASURES_SYMBOLS = {
    "pcgrl_measures_tiles": (C.c_int32, [C.c_void_p]),
    "pcgrl_measures": (C.c_int, [C.c_void_p] + [C.c_void_p] * 6),
    "pcgrl_measures_for_grids": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 7),
    "pcgrl_diversity_scratch_bytes": (C.c_size_t, [C.c_void_p, C.c_int32]),
    "pcgrl_diversity": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 7),
    "pcgrl_diversity_for_grids": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 7),
}

# include/pcgrl_amd_smb.h: Super Mario Bros levels (statistics, loss and A* play-through; no engine handle)
PCGRL_SMB_STATS = 9


class PcgrlSmbConfig(C.Structure):
    _fields_ = [
        ("h", C.c_int32), ("w", C.c_int32), ("solver_power", C.c_int32), ("has_trg", C.c_int32 * PCGRL_SMB_STATS),
        ("weight", C.c_double * PCGRL_SMB_STATS), ("trg_lo", C.c_double * PCGRL_SMB_STATS),
        ("trg_hi", C.c_double * PCGRL_SMB_STATS),
    ]


SMB_SYMBOLS = {
    "pcgrl_smb_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "pcgrl_smb_evaluate": (C.c_int, [C.POINTER(PcgrlSmbConfig), C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                     C.c_int32] + [C.c_void_p] * 8),
}


# include/pcgrl_amd_smb_env.h: stepping Super Mario Bros environments (narrow, turtle; a handle of its own)
class PcgrlSmbEnvConfig(C.Structure):
    _fields_ = [
        ("h", C.c_int32), ("w", C.c_int32), ("representation", C.c_int32), ("obs_window", C.c_int32 * 2),
        ("max_iterations", C.c_int32), ("max_changes", C.c_int32), ("solver_power", C.c_int32), ("n_envs", C.c_int32),
        ("has_trg", C.c_int32 * PCGRL_SMB_STATS), ("weight", C.c_double * PCGRL_SMB_STATS),
        ("trg_lo", C.c_double * PCGRL_SMB_STATS), ("trg_hi", C.c_double * PCGRL_SMB_STATS),
    ]


SMB_ENV_SYMBOLS = {
    "pcgrl_smb_env_workspace_bytes": (C.c_int64, [C.POINTER(PcgrlSmbEnvConfig)]),
    "pcgrl_smb_env_obs_bytes": (C.c_int64, [C.POINTER(PcgrlSmbEnvConfig)]),
    "pcgrl_smb_env_create": (C.c_int, [C.POINTER(PcgrlSmbEnvConfig), C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]),
    "pcgrl_smb_env_destroy": (None, [C.c_void_p]),
    "pcgrl_smb_env_seed": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pcgrl_smb_env_reset": (C.c_int, [C.c_void_p] + [C.c_void_p] * 5),
    "pcgrl_smb_env_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 6),
    "pcgrl_smb_env_observe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_smb_env_get_state": (C.c_int, [C.c_void_p] + [C.c_void_p] * 8),
    "pcgrl_smb_env_get_last_episode": (C.c_int, [C.c_void_p] + [C.c_void_p] * 5),
    "pcgrl_smb_env_poll_error": (C.c_int, [C.c_void_p]),
}

# include/pcgrl_amd_smb_ready.h: the same envs under a solver budget (a resumable play-through; works on an smb env handle)
SMB_READY_SYMBOLS = {
    "pcgrl_smb_ready_set_budget": (C.c_int, [C.c_void_p, C.c_int32]),
    "pcgrl_smb_ready_get_budget": (C.c_int32, [C.c_void_p]),
    "pcgrl_smb_ready_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 7),
    "pcgrl_smb_ready_busy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_smb_ready_park_bytes": (C.c_int64, [C.POINTER(PcgrlSmbEnvConfig)]),
}

# include/pcgrl_amd_smb_state.h: checkpoint and restore of those envs (the image, the portable form, the RNG streams)
SMB_STATE_SYMBOLS = {
    "pcgrl_smb_state_bytes": (C.c_int64, [C.c_void_p]),
    "pcgrl_smb_state_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_smb_state_import": (C.c_int, [C.c_void_p] + [C.c_void_p] * 4),
    "pcgrl_smb_state_set": (C.c_int, [C.c_void_p] + [C.c_void_p] * 6),
    "pcgrl_smb_state_get_rng": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_smb_state_set_rng": (C.c_int, [C.c_void_p] + [C.c_void_p] * 3),
}

# include/pcgrl_amd_smb_rollout.h: K steps of those envs in one launch, and actions drawn on the device
SMB_ROLLOUT_SYMBOLS = {
    "pcgrl_smb_env_rollout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
                              + [C.c_void_p] * 10),
    "pcgrl_smb_env_sample_actions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "pcgrl_smb_env_num_actions": (C.c_int32, [C.c_void_p]),
}

# include/pcgrl_amd_smb_ctrl.h: controllable generation for those envs (per-env targets, the control observation, resampling)
SMB_CTRL_SYMBOLS = {
    "pcgrl_smb_ctrl_attach": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 4),
    "pcgrl_smb_ctrl_count": (C.c_int32, [C.c_void_p]),
    "pcgrl_smb_ctrl_queue": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 5),
    "pcgrl_smb_ctrl_observe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_smb_ctrl_set_resampling": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcgrl_smb_ctrl_get": (C.c_int, [C.c_void_p] + [C.c_void_p] * 5),
}

# include/pcgrl_amd_smb_vector.h: the float32 hand-out of those envs (RLlib's Box form, control planes in front)
SMB_VECTOR_SYMBOLS = {
    "pcgrl_smb_env_obs_f32_bytes": (C.c_int64, [C.c_void_p]),
    "pcgrl_smb_env_observe_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
}

# include/pcgrl_amd_smb_measures.h: level measures and pairwise Hamming diversity of smb maps (caller maps, or an env handle's)
SMB_MEASURES_SYMBOLS = {
    "pcgrl_smb_measures_for_grids": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 7),
    "pcgrl_smb_diversity_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "pcgrl_smb_diversity_for_grids": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 7),
    "pcgrl_smb_env_measures": (C.c_int, [C.c_void_p] + [C.c_void_p] * 6),
    "pcgrl_smb_env_diversity": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 7),
}

# include/pcgrl_amd_loderunner.h: Lode Runner levels (statistics, win score and gold searches; no engine handle)
PCGRL_LODERUNNER_STATS = 5


class PcgrlLoderunnerConfig(C.Structure):
    _fields_ = [
        ("h", C.c_int32), ("w", C.c_int32), ("has_trg", C.c_int32 * PCGRL_LODERUNNER_STATS),
        ("weight", C.c_double * PCGRL_LODERUNNER_STATS), ("trg_lo", C.c_double * PCGRL_LODERUNNER_STATS),
        ("trg_hi", C.c_double * PCGRL_LODERUNNER_STATS),
    ]


LODERUNNER_SYMBOLS = {
    "pcgrl_loderunner_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "pcgrl_loderunner_evaluate": (C.c_int, [C.POINTER(PcgrlLoderunnerConfig), C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                            C.c_int32] + [C.c_void_p] * 7),
}

# include/pcgrl_amd_loderunner_measures.h: level measures and pairwise Hamming diversity of Lode Runner maps (caller maps)
LODERUNNER_MEASURES_SYMBOLS = {
    "pcgrl_loderunner_measures_for_grids": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 7),
    "pcgrl_loderunner_diversity_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "pcgrl_loderunner_diversity_for_grids": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
                                             + [C.c_void_p] * 7),
}

# include/pcgrl_amd_loderunner_routes.h: the routes behind a Lode Runner level's path-length (the evaluation and the cell lists)
LODERUNNER_ROUTES_SYMBOLS = {
    "pcgrl_loderunner_routes": (C.c_int, [C.POINTER(PcgrlLoderunnerConfig), C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_int32, C.c_int32] + [C.c_void_p] * 12),
}

# include/pcgrl_amd_microstructure.h: microstructure levels (path-length, tortuosity and the per-region record; the level
# measures and pairwise Hamming diversity of such maps; no engine handle, no workspace)
PCGRL_MICROSTRUCTURE_STATS = 2


class PcgrlMicrostructureConfig(C.Structure):
    _fields_ = [
        ("h", C.c_int32), ("w", C.c_int32), ("has_trg", C.c_int32 * PCGRL_MICROSTRUCTURE_STATS),
        ("weight", C.c_double * PCGRL_MICROSTRUCTURE_STATS), ("trg_lo", C.c_double * PCGRL_MICROSTRUCTURE_STATS),
        ("trg_hi", C.c_double * PCGRL_MICROSTRUCTURE_STATS),
    ]


MICROSTRUCTURE_SYMBOLS = {
    "pcgrl_microstructure_evaluate": (C.c_int, [C.POINTER(PcgrlMicrostructureConfig), C.c_int32, C.c_void_p, C.c_int32]
                                      + [C.c_void_p] * 7),
    "pcgrl_microstructure_measures_for_grids": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 7),
    "pcgrl_microstructure_diversity_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "pcgrl_microstructure_diversity_for_grids": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
                                                 + [C.c_void_p] * 7),
}

# include/pcgrl_amd_ddave.h: Dangerous Dave levels (statistics and the four-stage play-through; the level measures and pairwise
# Hamming diversity of such maps; no engine handle)
PCGRL_DDAVE_STATS = 11
PCGRL_DDAVE_WEIGHTS = 10
PCGRL_DDAVE_PLAY = 12


class PcgrlDdaveConfig(C.Structure):
    _fields_ = [
        ("h", C.c_int32), ("w", C.c_int32), ("solver_power", C.c_int32), ("max_diamonds", C.c_int32),
        ("min_spikes", C.c_int32), ("target_jumps", C.c_int32), ("target_solution", C.c_int32),
        ("weight", C.c_double * PCGRL_DDAVE_WEIGHTS),
    ]


DDAVE_SYMBOLS = {
    "pcgrl_ddave_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "pcgrl_ddave_evaluate": (C.c_int, [C.POINTER(PcgrlDdaveConfig), C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
                             + [C.c_void_p] * 6),
    "pcgrl_ddave_measures_for_grids": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 7),
    "pcgrl_ddave_diversity_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "pcgrl_ddave_diversity_for_grids": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 7),
}
# include/pcgrl_amd_mdungeon.h: MiniDungeon levels (statistics and the four-stage play-through; the level measures and pairwise
# Hamming diversity of such maps; no engine handle)
PCGRL_MDUNGEON_STATS = 11
PCGRL_MDUNGEON_WEIGHTS = 9
PCGRL_MDUNGEON_PLAY = 12


class PcgrlMdungeonConfig(C.Structure):
    _fields_ = [
        ("h", C.c_int32), ("w", C.c_int32), ("solver_power", C.c_int32), ("max_enemies", C.c_int32),
        ("max_potions", C.c_int32), ("max_treasures", C.c_int32), ("target_solution", C.c_int32),
        ("target_col_enemies", C.c_double), ("weight", C.c_double * PCGRL_MDUNGEON_WEIGHTS),
    ]


MDUNGEON_SYMBOLS = {
    "pcgrl_mdungeon_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "pcgrl_mdungeon_evaluate": (C.c_int, [C.POINTER(PcgrlMdungeonConfig), C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_int32] + [C.c_void_p] * 6),
    "pcgrl_mdungeon_measures_for_grids": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 7),
    "pcgrl_mdungeon_diversity_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "pcgrl_mdungeon_diversity_for_grids": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
                                           + [C.c_void_p] * 7),
}

# include/pcgrl_amd_archive.h: the quality-diversity grid archive (insert, select, mutate; a handle of its own)
PCGRL_ARCHIVE_MAX_AXES = 4
PCGRL_ARCHIVE_HEADER_BYTES = 128
ARCHIVE_SYMBOLS = {
    "pcgrl_archive_create": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32,
                                       C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "pcgrl_archive_destroy": (None, [C.c_void_p]),
    "pcgrl_archive_add": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 8),
    "pcgrl_archive_cells": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 3),
    "pcgrl_archive_stats": (C.c_int, [C.c_void_p] * 3),
    "pcgrl_archive_elites": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 5),
    "pcgrl_archive_ask": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.c_double] + [C.c_void_p] * 3),
    "pcgrl_archive_state_bytes": (C.c_int64, [C.c_void_p]),
    "pcgrl_archive_export": (C.c_int, [C.c_void_p] * 3),
    "pcgrl_archive_import": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "pcgrl_archive_poll_error": (C.c_int, [C.c_void_p] * 2),
    "pcgrl_archive_last_error": (C.c_char_p, []),
}

# include/pcgrl_amd_mc3d_holey.h: 3-D holey dungeon and maze levels (statistics, loss and routes; no engine handle)
PCGRL_MC3D_HOLEY_MAX_STATS = 6
PCGRL_MC3D_HOLEY_PLAY = 12


class PcgrlMc3dHoleyConfig(C.Structure):
    _fields_ = [
        ("problem", C.c_int32), ("z", C.c_int32), ("y", C.c_int32), ("x", C.c_int32),
        ("weight", C.c_double * PCGRL_MC3D_HOLEY_MAX_STATS), ("trg_lo", C.c_double * PCGRL_MC3D_HOLEY_MAX_STATS),
        ("trg_hi", C.c_double * PCGRL_MC3D_HOLEY_MAX_STATS),
    ]


MC3D_HOLEY_SYMBOLS = {
    "pcgrl_mc3d_holey_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "pcgrl_mc3d_holey_evaluate": (C.c_int, [C.POINTER(PcgrlMc3dHoleyConfig), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int64, C.c_int32] + [C.c_void_p] * 12),
}

# include/pcgrl_amd_nca.h: the NCA level generator (genomes x seeds rolled out in one launch; a handle of its own)
NCA_SYMBOLS = {
    "pcgrl_nca_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "pcgrl_nca_destroy": (None, [C.c_void_p]),
    "pcgrl_nca_generate": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
                           + [C.c_void_p] * 4),
    "pcgrl_nca_poll_error": (C.c_int, [C.c_void_p] * 2),
    "pcgrl_nca_last_error": (C.c_char_p, []),
}

# include/pcgrl_amd_nca3d.h: the 3-D NCA level generator, plain and holey (a handle of its own)
NCA3D_SYMBOLS = {
    "pcgrl_nca3d_create": (C.c_int, [C.c_int32] * 5 + [C.POINTER(C.c_void_p)]),
    "pcgrl_nca3d_destroy": (None, [C.c_void_p]),
    "pcgrl_nca3d_generate": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
                             + [C.c_int32] * 4 + [C.c_void_p] * 4),
    "pcgrl_nca3d_poll_error": (C.c_int, [C.c_void_p] * 2),
    "pcgrl_nca3d_last_error": (C.c_char_p, []),
}

# include/pcgrl_amd_evo.h: NCA evolution (genome archives on the archive's handle, Gaussian children, simulate's fold over seeds;
# the kernels are csrc/evo/pcgrl_evo.h, compiled into the archive's unit so that the insertion is written once)
PCGRL_EVO_MAX_PARAMS = 16384
PCGRL_EVO_MAX_SEEDS = 128
PCGRL_EVO_MAX_BEHAVIOURS = 4
EVO_SYMBOLS = {
    "pcgrl_archive_create_genomes": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                               C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "pcgrl_archive_ask_genomes": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.c_float] + [C.c_void_p] * 3),
    "pcgrl_archive_sample_genomes": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.c_float] + [C.c_void_p] * 3),
    "pcgrl_evo_aggregate": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_double] + [C.c_void_p] * 9),
}


# The C ABI, one entry per public header: (file under include/, its symbol table).  build() watches these headers and lib()
# binds these tables; tests/test_abi_table_cpu.py holds each header's declarations against its table.
ABI = [("pcgrl_amd.h", SYMBOLS),
       ("pcgrl_amd_codes.h", CODES_SYMBOLS),
       ("pcgrl_amd_async3d.h", ASYNC3D_SYMBOLS),
       ("pcgrl_amd_paths.h", PATHS_SYMBOLS),
       ("pcgrl_amd_solutions.h", SOLUTIONS_SYMBOLS),
       ("pcgrl_amd_multiagent.h", MULTIAGENT_SYMBOLS),
       ("pcgrl_amd_measures.h", MEASURES_SYMBOLS),
       ("pcgrl_amd_smb.h", SMB_SYMBOLS),
       ("pcgrl_amd_smb_env.h", SMB_ENV_SYMBOLS),
       ("pcgrl_amd_smb_ready.h", SMB_READY_SYMBOLS),
       ("pcgrl_amd_smb_state.h", SMB_STATE_SYMBOLS),
       ("pcgrl_amd_smb_rollout.h", SMB_ROLLOUT_SYMBOLS),
       ("pcgrl_amd_smb_ctrl.h", SMB_CTRL_SYMBOLS),
       ("pcgrl_amd_smb_vector.h", SMB_VECTOR_SYMBOLS),
       ("pcgrl_amd_smb_measures.h", SMB_MEASURES_SYMBOLS),
       ("pcgrl_amd_loderunner.h", LODERUNNER_SYMBOLS),
       ("pcgrl_amd_loderunner_measures.h", LODERUNNER_MEASURES_SYMBOLS),
       ("pcgrl_amd_loderunner_routes.h", LODERUNNER_ROUTES_SYMBOLS),
       ("pcgrl_amd_microstructure.h", MICROSTRUCTURE_SYMBOLS),
       ("pcgrl_amd_ddave.h", DDAVE_SYMBOLS),
       ("pcgrl_amd_mdungeon.h", MDUNGEON_SYMBOLS),
       ("pcgrl_amd_archive.h", ARCHIVE_SYMBOLS),
       ("pcgrl_amd_mc3d_holey.h", MC3D_HOLEY_SYMBOLS),
       ("pcgrl_amd_nca.h", NCA_SYMBOLS),
       ("pcgrl_amd_nca3d.h", NCA3D_SYMBOLS),
       ("pcgrl_amd_evo.h", EVO_SYMBOLS)]
ABI_HEADERS = [_include(name) for name, _ in ABI]


def build(force=False, verbose=False, out=None, defines=(), jobs=None):
    """hipcc --offload-arch=gfx950 (cross-compiles without a GPU), one object per translation unit, compiled in
    parallel, then linked into the shared library.  Rebuilds when a source is newer than the library.
    `out` / `defines`: development builds (tools/phase_timing.py, tools/wave_trace.py)."""
    out = out or LIB_PATH
    srcs = [os.path.join(CSRC, s) for s in SOURCES] + ABI_HEADERS
    if (not force and os.path.exists(out)
            and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in srcs if os.path.exists(s))):
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    tag = "".join(sorted(d.replace("=", "_") for d in defines))
    objdir = os.path.join(CSRC, "_obj" + ("_" + tag if tag else ""))
    os.makedirs(objdir, exist_ok=True)
    hdr_time = max(os.path.getmtime(h) for h in [os.path.join(CSRC, h) for h in HEADERS] + ABI_HEADERS)
    jobs_todo, objs = [], []
    for u in UNITS:
        obj = os.path.join(objdir, os.path.basename(u).replace(".hip", ".o"))
        objs.append(obj)
        if (force or not os.path.exists(obj)
                or os.path.getmtime(obj) < max(hdr_time, os.path.getmtime(os.path.join(CSRC, u)))):
            jobs_todo.append([hipcc] + HIPCC_FLAGS + ["-D" + d for d in defines] + ["-c", os.path.join(CSRC, u), "-o", obj])
    if jobs_todo:
        from concurrent.futures import ThreadPoolExecutor

        def run(cmd):
            if verbose:
                print(" ".join(cmd), flush=True)
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)

        with ThreadPoolExecutor(max_workers=jobs or min(len(jobs_todo), os.cpu_count() or 1)) as ex:
            list(ex.map(run, jobs_todo))
    cmd = [hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", out] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return out


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH) and os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
            build()  # in-tree build of the HIP extension (never a CPU fallback)
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; "
                "g.build()' or control_pcgrl_amd._lib.build()).  There is no CPU fallback.")
        # development: another build of the same ABI for A/B timing -- only a file of this package's csrc directory
        override = os.environ.get("PCGRL_LIB")
        if override and os.path.dirname(os.path.realpath(override)) != os.path.realpath(CSRC):
            raise RuntimeError(f"PCGRL_LIB={override}: only libraries inside {CSRC} are loaded")
        L = C.CDLL(override or LIB_PATH)
        for name, (res, args) in [item for _, table in ABI for item in table.items()]:
            if override and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().pcgrl_last_error().decode()
        exc = ValueError if rc in (1, 4) else (NotImplementedError if rc == 2 else RuntimeError)
        raise exc(f"{what}: PCGRL_{ERRORS.get(rc, rc)}: {msg}")
