"""ctypes binding of libaz_engine.so (include/az_engine.h).

This module is the only place the Python host layer touches the C-ABI.  It fails loudly when
the HIP library is missing or no GPU is present: there is no CPU fallback for the path.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AZ_ENGINE_LIB") or os.path.join(_HERE, "libaz_engine.so")   # override: experiment builds

STATE_DICT_ORDER = [
    "conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias",
    "policy_conv.weight", "policy_conv.bias", "policy_fc.weight", "policy_fc.bias",
    "value_conv.weight", "value_conv.bias", "value_fc1.weight", "value_fc1.bias",
    "value_fc2.weight", "value_fc2.bias",
]

AZ_EVAL_NET, AZ_EVAL_SYNTHETIC = 0, 1
AZ_RES_NONE, AZ_RES_X, AZ_RES_O, AZ_RES_DRAW = 0, 1, 2, 3
AZ_AUG_NONE, AZ_AUG_REFERENCE4, AZ_AUG_DIHEDRAL8 = 1, 4, 8
AZ_MODEL_PLAIN, AZ_MODEL_RESNET = 0, 1
AZ_TRUNK_F32, AZ_TRUNK_BF16X3, AZ_TRUNK_F16X2 = 0, 1, 2
AZ_MAX_SIMULATIONS, AZ_DEEP_MAX_SIMULATIONS = 1024, 65534      # az_create | az_create_deep
REUSE_MAX_SIMULATIONS = 1023                                   # az_set_subtree_reuse

EXPORTS = [
    "az_create", "az_create_deep", "az_destroy", "az_last_error", "az_load_weights", "az_load_weights_resnet", "az_net_eval", "az_search", "az_search_batch", "az_search_callback", "az_selfplay",
    "az_selfplay_begin", "az_selfplay_step", "az_selfplay_end", "az_selfplay_games", "az_selfplay_records", "az_selfplay_clear", "az_record_bytes", "az_selfplay_pack", "az_examples_from_packed",
    "az_examples_gather", "az_arena", "az_rules_replay", "az_rng_selfplay_tape", "az_rng_uniforms", "az_set_profiling", "az_set_subtree_reuse", "az_get_counters", "az_get_lanes", "az_get_persistent", "az_set_virtual_loss", "az_set_eval_cache",
    "az_set_trunk_mode", "az_get_trunk_mode", "az_set_leaf_symmetry", "az_emul_split",
    "az_set_start_positions", "az_get_start_positions",
    "az_set_resign", "az_get_resign", "az_selfplay_values", "az_selfplay_pack_values", "az_selfplay_resign_info",
    "az_resign_mix", "az_resign_exempt",
    "az_set_playout_cap", "az_get_playout_cap", "az_playout_cap_full", "az_selfplay_sims", "az_selfplay_export_count",
    "az_set_forced_playouts", "az_get_forced_playouts", "az_forced_prune",
    "az_set_selection", "az_get_selection", "az_selection_tables",
    "az_set_candidates", "az_get_candidates", "az_candidate_mask",
    "az_set_gumbel", "az_get_gumbel", "az_gumbel_schedule", "az_gumbel_target", "az_gumbel_vmix", "az_rng_selfplay_tape_gumbel",
    "az_set_external_evaluator", "az_get_external_evaluator", "az_ext_capacity", "az_ext_stats",
    "az_set_solver", "az_get_solver", "az_last_proof", "az_selfplay_proofs", "az_solver_counts", "az_solver_stops",
    "az_set_win_rule", "az_get_win_rule", "az_rules_winner",
    "az_set_threat_search", "az_get_threat_search", "az_threat_batch", "az_threat_solve", "az_selfplay_threats", "az_threat_stats",
    "az_set_rng", "az_get_rng", "az_rng_philox4x32", "az_rng_log", "az_rng_exp", "az_rng_philox_tape", "az_rng_philox_tape_device",
    "az_set_delta_eval", "az_get_delta_eval", "az_delta_max_tiles", "az_delta_stats", "az_net_eval_delta", "az_delta_lists", "az_delta_lists_full",
    "az_delta_changed",
    "az_dist_unique_id", "az_dist_init", "az_dist_rank", "az_dist_world", "az_dist_counts", "az_dist_gather_records",
    "az_dist_allreduce_sum", "az_dist_broadcast",
]
AZ_DIST_ID_BYTES = 128


class AzError(RuntimeError):
    pass


class az_config(C.Structure):
    _fields_ = [("board_size", C.c_int32), ("win_length", C.c_int32), ("num_simulations", C.c_int32),
                ("slots", C.c_int32), ("c_puct", C.c_double), ("dirichlet_alpha", C.c_double),
                ("dirichlet_weight", C.c_double), ("eval_kind", C.c_int32), ("device", C.c_int32),
                ("log_table", C.POINTER(C.c_float)), ("model", C.c_int32), ("engines", C.c_int32)]


class az_selfplay_args(C.Structure):
    _fields_ = [("seed0", C.c_uint64), ("num_games", C.c_int32), ("max_plies", C.c_int32),
                ("temperature_table", C.POINTER(C.c_double)), ("noise_tape", C.POINTER(C.c_double)),
                ("u_tape", C.POINTER(C.c_double)), ("tape_stride", C.c_int64)]


class az_counters(C.Structure):
    _fields_ = [("games", C.c_int64), ("plies", C.c_int64), ("records", C.c_int64), ("simulations", C.c_int64),
                ("expansions", C.c_int64), ("root_evals", C.c_int64), ("terminal_hits", C.c_int64),
                ("depth_sum", C.c_int64), ("steps", C.c_int64), ("seconds", C.c_double), ("nn_seconds", C.c_double),
                ("trunk_seconds", C.c_double), ("trunk_launches", C.c_int64), ("trunk_boards", C.c_int64),
                ("step_seconds", C.c_double), ("duplicate_leaves", C.c_int64), ("cache_lookups", C.c_int64),
                ("cache_hits", C.c_int64), ("tape_wait_seconds", C.c_double), ("tape_threads", C.c_int64),
                ("host_cpus", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class az_arena_args(C.Structure):
    _fields_ = [("seed0", C.c_uint64), ("num_games", C.c_int32), ("temperature_table", C.POINTER(C.c_double)),
                ("u_tape", C.POINTER(C.c_double))]


class az_arena_result(C.Structure):
    _fields_ = [("wins", C.c_int32), ("losses", C.c_int32), ("draws", C.c_int32), ("total", C.c_int32),
                ("win_rate", C.c_double)]


_EVAL_BATCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int)


class az_ext_evaluator(C.Structure):
    _fields_ = [("planes_dev", C.c_void_p), ("policy_dev", C.c_void_p), ("value_dev", C.c_void_p),
                ("capacity", C.c_int32), ("fn", _EVAL_BATCH_FN), ("user", C.c_void_p)]


_LIB = None


def build(force=False):
    """Compile the HIP engine in-tree (hipcc --offload-arch=gfx950); cross-compiles without a GPU."""
    src_dir = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(src_dir, f) for f in os.listdir(src_dir) if f.endswith((".hip", ".h", ".cpp"))]
    srcs.append(os.path.join(os.path.dirname(_HERE), "include", "az_engine.h"))
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        if not os.path.exists("/opt/rocm/bin/hipcc") and os.path.exists(LIB_PATH):
            return LIB_PATH
        subprocess.check_call(["make", "-C", src_dir], stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise AzError(f"{LIB_PATH} is missing: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        # torch ships its own libamdhip64.so.7; load it FIRST so that this library binds to the same HIP
        # runtime (same soname) -- two runtimes in one process cannot both own the GPU.
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for the pure C-ABI user
            pass
        L = C.CDLL(LIB_PATH)
        L.az_last_error.restype = C.c_char_p
        L.az_last_error.argtypes = [C.c_void_p]
        L.az_create.argtypes = [C.POINTER(az_config), C.POINTER(C.c_void_p)]
        L.az_create_deep.argtypes = [C.POINTER(az_config), C.POINTER(C.c_void_p)]
        L.az_destroy.argtypes = [C.c_void_p]
        L.az_destroy.restype = None
        L.az_record_bytes.restype = C.c_int64
        L.az_record_bytes.argtypes = [C.c_void_p]
        L.az_rng_selfplay_tape.argtypes = [C.c_uint64, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
        L.az_rng_uniforms.argtypes = [C.c_uint64, C.c_int, C.c_void_p]
        L.az_dist_init.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
        L.az_dist_gather_records.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.az_dist_counts.argtypes = [C.c_void_p, C.c_void_p]
        L.az_dist_allreduce_sum.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.az_dist_broadcast.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
        L.az_dist_unique_id.argtypes = [C.c_void_p]
        if hasattr(L, "az_search_batch"):        # an experiment build from older sources (AZ_ENGINE_LIB) may lack it
            L.az_search_batch.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 11
        if hasattr(L, "az_set_start_positions"):
            L.az_set_start_positions.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
            L.az_get_start_positions.argtypes = [C.c_void_p]
        if hasattr(L, "az_set_resign"):
            L.az_set_resign.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int]
            L.az_get_resign.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)]
            L.az_selfplay_values.argtypes = [C.c_void_p, C.c_void_p]
            L.az_selfplay_pack_values.argtypes = [C.c_void_p, C.c_void_p]
            L.az_selfplay_resign_info.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            L.az_resign_mix.argtypes = [C.c_uint32]
            L.az_resign_mix.restype = C.c_uint32
            L.az_resign_exempt.argtypes = [C.c_uint32, C.c_int]
        if hasattr(L, "az_set_playout_cap"):
            L.az_set_playout_cap.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
            L.az_get_playout_cap.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
            L.az_playout_cap_full.argtypes = [C.c_uint32, C.c_int, C.c_int]
            L.az_selfplay_sims.argtypes = [C.c_void_p, C.c_void_p]
            L.az_selfplay_export_count.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        if hasattr(L, "az_set_forced_playouts"):
            L.az_set_forced_playouts.argtypes = [C.c_void_p, C.c_double, C.c_int]
            L.az_get_forced_playouts.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
            L.az_forced_prune.argtypes = [C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.az_forced_prune.restype = C.c_int64
        if hasattr(L, "az_set_selection"):
            L.az_set_selection.argtypes = [C.c_void_p, C.c_int] + [C.c_double] * 4
            L.az_get_selection.argtypes = [C.c_void_p, C.POINTER(C.c_int)] + [C.POINTER(C.c_double)] * 4
            L.az_selection_tables.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
        if hasattr(L, "az_set_candidates"):
            L.az_set_candidates.argtypes = [C.c_void_p, C.c_int]
            L.az_get_candidates.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
            L.az_candidate_mask.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        if hasattr(L, "az_set_gumbel"):
            L.az_set_gumbel.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double]
            L.az_get_gumbel.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]
            L.az_gumbel_schedule.argtypes = [C.c_int, C.c_int, C.c_void_p]
            L.az_gumbel_target.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_double,
                                           C.c_double, C.c_void_p, C.POINTER(C.c_int32)]
            L.az_gumbel_vmix.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]
            L.az_gumbel_vmix.restype = C.c_double
            L.az_rng_selfplay_tape_gumbel.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        if hasattr(L, "az_set_external_evaluator"):
            L.az_set_external_evaluator.argtypes = [C.c_void_p, C.POINTER(az_ext_evaluator)]
            L.az_get_external_evaluator.argtypes = [C.c_void_p]
            L.az_ext_capacity.argtypes = [C.c_void_p]
            L.az_ext_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        if hasattr(L, "az_set_solver"):
            L.az_set_solver.argtypes = [C.c_void_p, C.c_int]
            L.az_get_solver.argtypes = [C.c_void_p]
            L.az_last_proof.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
            L.az_solver_stops.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
            L.az_selfplay_proofs.argtypes = [C.c_void_p, C.c_void_p]
            L.az_solver_counts.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "az_set_win_rule"):
            L.az_set_win_rule.argtypes = [C.c_void_p, C.c_int]
            L.az_get_win_rule.argtypes = [C.c_void_p]
            L.az_rules_winner.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        if hasattr(L, "az_set_threat_search"):
            L.az_set_threat_search.argtypes = [C.c_void_p, C.c_int, C.c_int]
            L.az_get_threat_search.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
            L.az_threat_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
            L.az_threat_solve.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4
            L.az_selfplay_threats.argtypes = [C.c_void_p, C.c_void_p]
            L.az_threat_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_int64)] * 5
        if hasattr(L, "az_set_delta_eval"):
            L.az_set_delta_eval.argtypes = [C.c_void_p, C.c_int]
            L.az_get_delta_eval.argtypes = [C.c_void_p]
            L.az_delta_max_tiles.argtypes = [C.c_void_p, C.c_int]
            L.az_delta_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_int64)] * 4 + [C.c_void_p]
            L.az_net_eval_delta.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7
            L.az_delta_lists.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 5
        if hasattr(L, "az_delta_lists_full"):
            L.az_delta_lists_full.argtypes = [C.c_int] + [C.c_void_p] * 4
        if hasattr(L, "az_delta_changed"):
            L.az_delta_changed.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3
        if hasattr(L, "az_set_rng"):
            L.az_set_rng.argtypes = [C.c_void_p, C.c_int]
            L.az_get_rng.argtypes = [C.c_void_p]
            L.az_rng_philox4x32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            L.az_rng_philox4x32.restype = None
            L.az_rng_log.argtypes = L.az_rng_exp.argtypes = [C.c_double]
            L.az_rng_log.restype = L.az_rng_exp.restype = C.c_double
            L.az_rng_philox_tape.argtypes = [C.c_uint64, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
            L.az_rng_philox_tape_device.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _LIB = L
    return _LIB


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def rng_selfplay_tape(seed, n, alpha=0.3, max_plies=0):
    nn = n * n
    plies = max_plies if 0 < max_plies < nn else nn
    total = sum(nn - m for m in range(plies))
    noise = np.zeros(total, np.float64)
    u = np.zeros(nn, np.float64)
    rc = lib().az_rng_selfplay_tape(int(seed), n, float(alpha), int(max_plies), _p(noise), _p(u))
    if rc:
        raise AzError(f"az_rng_selfplay_tape failed ({rc})")
    return noise, u[:plies]


def dist_unique_id():
    """AZ_DIST_ID_BYTES bytes naming a new RCCL communicator (az_dist_unique_id): create on one rank, hand to all."""
    buf = C.create_string_buffer(AZ_DIST_ID_BYTES)
    rc = lib().az_dist_unique_id(buf)
    if rc:
        raise AzError(f"az_dist_unique_id failed ({rc}): {lib().az_last_error(None).decode()}")
    return buf.raw


def rng_uniforms(seed, count):
    u = np.zeros(count, np.float64)
    rc = lib().az_rng_uniforms(int(seed), int(count), _p(u))
    if rc:
        raise AzError(f"az_rng_uniforms failed ({rc})")
    return u


def resign_mix(key):
    """The 32-bit mix that names the exempt games (az_resign_mix; needs no GPU)."""
    return int(lib().az_resign_mix(int(key) & 0xFFFFFFFF))


def resign_exempt(key, playout_permille):
    """True when the game named key = low 32 bits of seed0 + g plays on whatever its search values (az_resign_exempt)."""
    return bool(lib().az_resign_exempt(int(key) & 0xFFFFFFFF, int(playout_permille)))


def resign_permille(playout):
    """The share of games that play out, as az_set_resign takes it: round(1000 * playout), 0 <= playout <= 1."""
    playout = float(playout)
    if not 0.0 <= playout <= 1.0:
        raise ValueError(f"playout must be a share in [0, 1], got {playout}")
    return int(round(1000 * playout))


def playout_cap_full(key, ply, permille):
    """True when ply `ply` (absolute) of the game named key = low 32 bits of seed0 + g gets the full search under a playout
    cap with `permille` full plies per thousand (az_playout_cap_full; needs no GPU)."""
    return bool(lib().az_playout_cap_full(int(key) & 0xFFFFFFFF, int(ply), int(permille)))


def playout_cap_permille(full):
    """The share of full plies, as az_set_playout_cap takes it: round(1000 * full), 0 <= full <= 1."""
    full = float(full)
    if not 0.0 <= full <= 1.0:
        raise ValueError(f"full must be a share in [0, 1], got {full}")
    return int(round(1000 * full))


FORCED_K_MAX = 16.0                                            # az_set_forced_playouts


def forced_prune(k, c_puct, visits, W, prior):
    """Policy target pruning of one root row (az_forced_prune; needs no GPU): visits int[count], W float64[count] and prior
    float32[count] of the LEGAL children in row-major order -> (pruned counts int32[count], visits removed).  The most visited
    child, the lowest on ties, keeps its count."""
    visits = np.ascontiguousarray(visits, np.int32)
    W = np.ascontiguousarray(W, np.float64)
    prior = np.ascontiguousarray(prior, np.float32)
    if not (visits.ndim == 1 and visits.shape == W.shape == prior.shape):
        raise ValueError("forced_prune takes three one-dimensional arrays of one length")
    out = np.zeros(len(visits), np.int32)
    removed = int(lib().az_forced_prune(float(k), float(c_puct), len(visits), _p(visits), _p(W), _p(prior), _p(out)))
    if removed < 0:
        raise ValueError(f"az_forced_prune refused its arguments (k {k} in (0, {FORCED_K_MAX:g}], counts 0..65534 with at least one visit)")
    return out, removed


# az_set_selection: the keys of the option with their defaults, and the closed range of each (None = no upper bound)
SELECTION_DEFAULTS = dict(fpu=0.2, fpu_root=0.0, cpuct_base=19652.0, cpuct_factor=0.0)
SELECTION_RANGES = dict(fpu=(0.0, 2.0), fpu_root=(0.0, 2.0), cpuct_base=(1.0, None), cpuct_factor=(0.0, 16.0))
SELECTION_MASS_STEPS = 4096


def check_selection(selection):
    """The option as the seams keep it: None (off), or a dict over fpu, fpu_root, cpuct_base and cpuct_factor completed with
    the defaults, every value a finite float inside its range (ValueError otherwise; no engine is touched)."""
    if selection is None or selection is False:
        return None
    if selection is True:
        selection = {}
    if not isinstance(selection, dict) or set(selection) - set(SELECTION_DEFAULTS):
        raise ValueError(f"selection takes a dict over {sorted(SELECTION_DEFAULTS)}, got {selection!r}")
    out = dict(SELECTION_DEFAULTS)
    out.update({k: float(v) for k, v in selection.items()})
    for k, (lo, hi) in SELECTION_RANGES.items():
        if not (np.isfinite(out[k]) and out[k] >= lo and (hi is None or out[k] <= hi)):
            raise ValueError(f"selection {k} must be finite and in [{lo:g}, {'inf' if hi is None else format(hi, 'g')}], got {out[k]}")
    return out


def selection_tables(c_puct, cpuct_base, cpuct_factor, S):
    """The two tables of the selection rule exactly as an engine with S simulations uploads them (az_selection_tables; needs no
    GPU): (cpuct float64[S + 2], mass float64[4097])."""
    cp = np.zeros(int(S) + 2, np.float64)
    mass = np.zeros(SELECTION_MASS_STEPS + 1, np.float64)
    rc = lib().az_selection_tables(float(c_puct), float(cpuct_base), float(cpuct_factor), int(S), _p(cp), _p(mass))
    if rc:
        raise ValueError(f"az_selection_tables refused its arguments (c_puct {c_puct}, cpuct_base {cpuct_base} >= 1, "
                         f"cpuct_factor {cpuct_factor} in [0, 16], S {S} in 1..{AZ_DEEP_MAX_SIMULATIONS})")
    return cp, mass


def check_candidates(candidates):
    """The option as the seams keep it: None (off), or dict(radius=r) with r an int >= 1 (ValueError otherwise; no engine is
    touched -- the upper bound n - 1 is the engine's, which knows the board)."""
    if candidates is None or candidates is False:
        return None
    if not isinstance(candidates, dict) or set(candidates) != {"radius"}:
        raise ValueError(f"candidates takes dict(radius=r), got {candidates!r}")
    r = candidates["radius"]
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 1 <= int(r) <= 14:
        raise ValueError(f"candidates radius must be an int in 1 .. n-1 (at most 14), got {r!r}")
    return dict(radius=int(r))


def candidate_mask(board, n, radius):
    """The candidate set of a position as az_set_candidates defines it (az_candidate_mask; needs no GPU): board uint8[n*n]
    (0 empty, 1 / 2 stones) -> uint8[n*n], 1 for the cells of C.  radius 0 gives the empty cells."""
    b = np.ascontiguousarray(np.asarray(board).reshape(-1), np.uint8)
    if b.size != int(n) * int(n):
        raise ValueError(f"board has {b.size} cells, n*n = {int(n) * int(n)}")
    mask = np.zeros(b.size, np.uint8)
    if lib().az_candidate_mask(int(n), _p(b), int(radius), _p(mask)):
        raise ValueError(f"az_candidate_mask refused its arguments (n {n} in 3..15, radius {radius} in 0..n-1, cells in 0..2)")
    return mask


WIN_RULES = {"freestyle": 0, "exact": 1}                     # az_set_win_rule: AZ_RULE_*


def win_rule_id(rule):
    """AZ_RULE_* of a rule given by name ("freestyle" | "exact"), by number (0 | 1) or as None (the default, freestyle)."""
    if rule is None:
        return 0
    if isinstance(rule, str) and rule in WIN_RULES:
        return WIN_RULES[rule]
    if not isinstance(rule, (str, bool)) and rule in (0, 1):
        return int(rule)
    raise ValueError(f"win rule must be 'freestyle' or 'exact', got {rule!r}")


def win_rule_name(rule):
    return "exact" if win_rule_id(rule) == 1 else "freestyle"


def rules_winner(board, n, k, rule="freestyle"):
    """Full-board scan under a win rule (az_rules_winner; needs no GPU): board uint8[n*n] or [n, n] with 0 empty, 1 X, 2 O ->
    1 / 2 when that colour holds a winning run, 3 for a full board without one, 0 otherwise.  ValueError for a bad argument or
    a board on which both colours hold a winning run."""
    rid = win_rule_id(rule)
    b = np.ascontiguousarray(board, np.uint8).reshape(-1)
    n, k = int(n), int(k)
    if n < 1 or b.size != n * n:
        raise ValueError(f"rules_winner: the board has {b.size} cells, n = {n}")
    rc = int(lib().az_rules_winner(_p(b), n, k, rid))
    if rc < 0:
        raise ValueError(f"az_rules_winner refused its arguments (n {n} in 1..15, k {k} in 1..n, cells 0..2, at most one colour with a winning run)")
    return rc


PROOF_UNKNOWN, PROOF_WIN, PROOF_LOSS, PROOF_DRAW = 0, 1, 2, 3    # az_set_solver: AZ_PROOF_*


def solver_counts(visits, status):
    """The count vector N' the solver makes pi and the move from (az_solver_counts; needs no GPU): visits int[count] and
    status int8[count] (PROOF_*) of the LEGAL children of one root in row-major order -> int32[count]."""
    visits = np.ascontiguousarray(visits, np.int32)
    status = np.ascontiguousarray(status, np.int8)
    if not (visits.ndim == 1 and visits.shape == status.shape):
        raise ValueError("solver_counts takes two one-dimensional arrays of one length")
    out = np.zeros(len(visits), np.int32)
    if lib().az_solver_counts(len(visits), _p(visits), _p(status), _p(out)):
        raise ValueError("az_solver_counts refused its arguments (at least one child, counts >= 0, statuses 0..3)")
    return out


THREAT_MAX_DEPTH = 16                                          # az_set_threat_search: AZ_THREAT_MAX_DEPTH
THREAT_DEFAULTS = dict(max_depth=8, node_budget=256)


def check_threat_search(threat_search, solver=True):
    """None (off) or the checked dict(max_depth, node_budget) of a seam's threat_search option (az_set_threat_search).  True means
    the defaults.  ValueError for unknown keys, values out of range, or without the solver it hands its results to."""
    if not threat_search:
        return None
    cfg = dict(THREAT_DEFAULTS)
    if threat_search is not True:
        unknown = set(threat_search) - set(cfg)
        if unknown:
            raise ValueError(f"threat_search: unknown keys {sorted(unknown)}")
        cfg.update(threat_search)
    cfg = {k: int(v) for k, v in cfg.items()}
    if not 1 <= cfg["max_depth"] <= THREAT_MAX_DEPTH or not 1 <= cfg["node_budget"] <= 65535:
        raise ValueError(f"threat_search: max_depth in 1..{THREAT_MAX_DEPTH} and node_budget in 1..65535, got {cfg}")
    if not solver:
        raise ValueError("threat_search needs solver=True: it hands its results to the solver")
    return cfg


def threat_solve(board, n, k, rule="freestyle", player=1, max_depth=8, node_budget=256):
    """The root threat search of one position on the host (az_threat_solve; needs no GPU): board uint8[n*n] or [n, n] with
    0 empty, 1 X, 2 O and `player` to move -> dict(status, move, depth, nodes, edges int8[n*n]).  status and edges are PROOF_*
    seen from the mover; move = -1 and depth = 0 without a win; the search was exhausted iff nodes > node_budget.  ValueError
    for a bad argument, a full board or a position that is already won."""
    rid = win_rule_id(rule)
    b = np.ascontiguousarray(board, np.uint8).reshape(-1)
    n, k = int(n), int(k)
    if n < 1 or b.size != n * n:
        raise ValueError(f"threat_solve: the board has {b.size} cells, n = {n}")
    mv, dp, nd = (np.zeros(1, np.int32) for _ in range(3))
    edges = np.zeros(n * n, np.int8)
    rc = int(lib().az_threat_solve(_p(b), n, k, rid, int(player), int(max_depth), int(node_budget), _p(mv), _p(dp), _p(nd), _p(edges)))
    if rc < 0:
        raise ValueError("az_threat_solve refused its arguments (n in 1..15, k in 1..n, cells 0..2, player 1 / 2, max_depth in 1..16, "
                         "node_budget in 1..65535, a legal action, no winning run on the board)")
    return dict(status=rc, move=int(mv[0]), depth=int(dp[0]), nodes=int(nd[0]), edges=edges)


GUMBEL_M_MAX = 64                                              # az_set_gumbel: m <= min(n * n, 64)
GUMBEL_DEFAULTS = dict(m=16, c_visit=50.0, c_scale=1.0)


def selfplay_tape_gumbel(seed, n, max_plies=0):
    """One game's tape under the Gumbel root search (az_rng_selfplay_tape_gumbel; needs no GPU): per ply p, n * n - p draws of
    RandomState(seed).gumbel() then one uniform -> (noise, u) in rng_selfplay_tape's layout."""
    nn = n * n
    plies = max_plies if 0 < max_plies < nn else nn
    noise = np.zeros(sum(nn - m for m in range(plies)), np.float64)
    u = np.zeros(nn, np.float64)
    rc = lib().az_rng_selfplay_tape_gumbel(int(seed), n, int(max_plies), _p(noise), _p(u))
    if rc:
        raise AzError(f"az_rng_selfplay_tape_gumbel failed ({rc})")
    return noise, u[:plies]


RNG_MODES = ("numpy", "philox")                                # az_set_rng: AZ_RNG_NUMPY, AZ_RNG_PHILOX
TAPE_KINDS = ("dirichlet", "gumbel")                           # AZ_TAPE_DIRICHLET, AZ_TAPE_GUMBEL


def check_rng(rng):
    """The name of an RNG mode as the seams keep it: "numpy" (None: the default) or "philox"."""
    if rng is None:
        return "numpy"
    if rng not in RNG_MODES:
        raise ValueError(f"rng must be one of {RNG_MODES}, got {rng!r}")
    return rng


def philox4x32(counter, key):
    """Philox4x32-10 of a counter of four and a key of two 32-bit words (az_rng_philox4x32; needs no GPU) -> uint32[4]."""
    c = np.array([int(x) & 0xFFFFFFFF for x in counter], np.uint32)
    k = np.array([int(x) & 0xFFFFFFFF for x in key], np.uint32)
    if c.shape != (4,) or k.shape != (2,):
        raise ValueError("philox4x32: a counter of four words and a key of two")
    out = np.zeros(4, np.uint32)
    lib().az_rng_philox4x32(_p(c), _p(k), _p(out))
    return out


def rng_log(x):
    """The software float64 logarithm of the Philox stream (az_rng_log; needs no GPU)."""
    return float(lib().az_rng_log(float(x)))


def rng_exp(x):
    """The float64 exp of the Philox stream, the engine's az_exp (az_rng_exp; needs no GPU)."""
    return float(lib().az_rng_exp(float(x)))


def philox_tape(seed, n, alpha=0.3, max_plies=0, kind="dirichlet"):
    """One game's tape of the AZ_RNG_PHILOX stream made on the host (az_rng_philox_tape; needs no GPU) -> (noise, u) in
    rng_selfplay_tape's layout.  kind "gumbel": Gumbel(0, 1) draws, the tape of the Gumbel root search."""
    nn = n * n
    plies = max_plies if 0 < max_plies < nn else nn
    noise = np.zeros(sum(nn - m for m in range(plies)), np.float64)
    u = np.zeros(nn, np.float64)
    rc = lib().az_rng_philox_tape(int(seed) & (2 ** 64 - 1), n, float(alpha), int(max_plies), TAPE_KINDS.index(kind), _p(noise), _p(u))
    if rc:
        raise AzError(f"az_rng_philox_tape failed ({rc})")
    return noise, u[:plies]


def gumbel_schedule(k, S):
    """The sequential-halving schedule of k candidates over S simulations (az_gumbel_schedule; needs no GPU): int32[S], entry t =
    the visit count a root child must have to be selectable at simulation t."""
    out = np.zeros(int(S), np.int32)
    if lib().az_gumbel_schedule(int(k), int(S), _p(out)):
        raise ValueError(f"az_gumbel_schedule refused its arguments (k {k} >= 0, S {S} in 1..{AZ_DEEP_MAX_SIMULATIONS})")
    return out


def gumbel_target(logits, g, visits, W, prior, root_value, c_visit=50.0, c_scale=1.0):
    """Move and policy target of one Gumbel root row (az_gumbel_target; needs no GPU): logits float32, g float64, visits int, W
    float64 and prior float32 of the LEGAL children in row-major order, root_value the root's float32 value ->
    (pi float32[count], index of the chosen child)."""
    logits = np.ascontiguousarray(logits, np.float32)
    g = np.ascontiguousarray(g, np.float64)
    visits = np.ascontiguousarray(visits, np.int32)
    W = np.ascontiguousarray(W, np.float64)
    prior = np.ascontiguousarray(prior, np.float32)
    if not (logits.ndim == 1 and logits.shape == g.shape == visits.shape == W.shape == prior.shape):
        raise ValueError("gumbel_target takes five one-dimensional arrays of one length")
    pi = np.zeros(len(visits), np.float32)
    a = C.c_int32(-1)
    rc = lib().az_gumbel_target(len(visits), _p(logits), _p(g), _p(visits), _p(W), _p(prior), C.c_float(float(root_value)),
                                float(c_visit), float(c_scale), _p(pi), C.byref(a))
    if rc:
        raise ValueError("az_gumbel_target refused its arguments (1..225 children, counts 0..65535 with at least one visit, "
                         "c_visit >= 0 and c_scale > 0, finite)")
    return pi, int(a.value)


def gumbel_vmix(visits, W, prior, root_value):
    """v_mix of one Gumbel root row as az_gumbel_target forms it (az_gumbel_vmix; needs no GPU)."""
    visits = np.ascontiguousarray(visits, np.int32)
    W = np.ascontiguousarray(W, np.float64)
    prior = np.ascontiguousarray(prior, np.float32)
    if not (visits.ndim == 1 and visits.shape == W.shape == prior.shape):
        raise ValueError("gumbel_vmix takes three one-dimensional arrays of one length")
    return float(lib().az_gumbel_vmix(len(visits), _p(visits), _p(W), _p(prior), C.c_float(float(root_value))))


class Engine:
    """One engine per GPU (az_create .. az_destroy).  engines = lanes inside the engine (az_config.engines): the slots
    are split over that many HIP streams driven by the library's own host threads; 0 lets the library choose.
    deep=True: az_create_deep, num_simulations up to AZ_DEEP_MAX_SIMULATIONS (tree memory grows with it; see
    include/az_engine.h); up to 1024 simulations the same engine as deep=False."""

    def __init__(self, board_size, win_length, num_simulations, slots, c_puct=2.0, dirichlet_alpha=0.3,
                 dirichlet_weight=0.25, synthetic=False, device=0, log_table=None, model="plain", engines=0, deep=False):
        self.n, self.k, self.S, self.slots = board_size, win_length, num_simulations, slots
        self.deep = bool(deep)
        self.device = int(device)
        if model not in ("plain", "resnet"):
            raise ValueError("model must be 'plain' or 'resnet'")
        self.model = model
        self.nn = board_size * board_size
        self._log_table = None if log_table is None else np.ascontiguousarray(log_table, np.float32)
        if self._log_table is not None and len(self._log_table) < num_simulations + 1:
            raise ValueError("log_table must have num_simulations + 1 entries")
        cfg = az_config(board_size, win_length, num_simulations, slots, c_puct, dirichlet_alpha, dirichlet_weight,
                        AZ_EVAL_SYNTHETIC if synthetic else AZ_EVAL_NET, device,
                        None if self._log_table is None else self._log_table.ctypes.data_as(C.POINTER(C.c_float)),
                        AZ_MODEL_RESNET if model == "resnet" else AZ_MODEL_PLAIN, int(engines))
        self.h = C.c_void_p()
        create = lib().az_create_deep if self.deep else lib().az_create
        rc = create(C.byref(cfg), C.byref(self.h))
        if rc:
            raise AzError(f"{'az_create_deep' if self.deep else 'az_create'} failed ({rc}): {lib().az_last_error(None).decode()}")
        self.record_bytes = int(lib().az_record_bytes(self.h))
        self.last_records = 0
        self._ext_cb = None           # the ctypes callback of the external evaluator: kept alive while the engine holds it
        self._ext_err = []

    def _check(self, rc, what):
        err = self.__dict__.get("_ext_err")
        if err:                       # the external evaluator raised inside the call: its exception, not the engine's code
            ex = err[0]
            del err[:]
            raise ex
        if rc:
            raise AzError(f"{what} failed ({rc}): {lib().az_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            lib().az_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights ----
    def load_weights(self, state_dict, slot=0):
        if self.model == "resnet":
            from .net import fold_resnet_state_dict
            keep = state_dict if isinstance(state_dict, (list, tuple)) else fold_resnet_state_dict(state_dict)
            keep = [np.ascontiguousarray(t, dtype=np.float32) for t in keep]
            arr = (C.c_void_p * 24)(*[t.ctypes.data for t in keep])
            self._check(lib().az_load_weights_resnet(self.h, int(slot), arr), "az_load_weights_resnet")
            return
        keep = []
        for k in STATE_DICT_ORDER:
            t = state_dict[k]
            if hasattr(t, "detach"):
                t = t.detach().cpu().numpy()
            keep.append(np.ascontiguousarray(t, dtype=np.float32))
        arr = (C.c_void_p * 16)(*[t.ctypes.data for t in keep])
        self._check(lib().az_load_weights(self.h, int(slot), arr), "az_load_weights")

    # ---- net ----
    def net_eval(self, boards, players, lasts, slot=0):
        boards = np.ascontiguousarray(boards, np.uint8).reshape(-1, self.nn)
        cnt = boards.shape[0]
        players = np.ascontiguousarray(players, np.uint8).reshape(cnt)
        lasts = np.ascontiguousarray(lasts, np.int16).reshape(cnt)
        logits = np.zeros((cnt, self.nn), np.float32)
        policy = np.zeros((cnt, self.nn), np.float32)
        value = np.zeros(cnt, np.float32)
        self._check(lib().az_net_eval(self.h, int(slot), cnt, _p(boards), _p(players), _p(lasts), _p(logits),
                                      _p(policy), _p(value)), "az_net_eval")
        return logits, policy, value

    # ---- delta evaluation (include/az_engine.h) ----
    def set_delta_eval(self, on):
        """Leaves evaluated as deltas from the ply's root activations where the configuration is eligible (on by default);
        results are bit-identical either way."""
        self._check(lib().az_set_delta_eval(self.h, 1 if on else 0), "az_set_delta_eval")

    def delta_eval(self):
        return lib().az_get_delta_eval(self.h) == 1

    def delta_max_tiles(self, tiles=0):
        """Sets (1 .. 15) and returns the conv3 tile count above which a leaf is evaluated in full; 0 only asks."""
        rc = lib().az_delta_max_tiles(self.h, int(tiles))
        if rc < 0:
            self._check(rc, "az_delta_max_tiles")
        return int(rc)

    def delta_stats(self, by_tiles=False):
        """dict(delta, full, tiles, base) of the last (or open) episode or search call (az_delta_stats); by_tiles: also the
        delta evaluations by conv3 tile count, 16 entries."""
        v = [C.c_int64(0) for _ in range(4)]
        h = np.zeros(16, np.int64)
        self._check(lib().az_delta_stats(self.h, *[C.byref(x) for x in v], _p(h)), "az_delta_stats")
        d = dict(zip(("delta", "full", "tiles", "base"), (int(x.value) for x in v)))
        if by_tiles:
            d["by_tiles"] = h.tolist()
        return d

    def net_eval_delta(self, root, root_player, boards, players, lasts, slot=0):
        """The positions evaluated as deltas from one root position: (logits, policy, value, path) with path[i] = conv3 tiles
        the delta path computed for position i, -1 = evaluated in full (az_net_eval_delta)."""
        root = np.ascontiguousarray(root, np.uint8).reshape(self.nn)
        boards = np.ascontiguousarray(boards, np.uint8).reshape(-1, self.nn)
        cnt = boards.shape[0]
        players = np.ascontiguousarray(players, np.uint8).reshape(cnt)
        lasts = np.ascontiguousarray(lasts, np.int16).reshape(cnt)
        logits = np.zeros((cnt, self.nn), np.float32)
        policy = np.zeros((cnt, self.nn), np.float32)
        value = np.zeros(cnt, np.float32)
        path = np.zeros(cnt, np.int32)
        self._check(lib().az_net_eval_delta(self.h, int(slot), _p(root), int(root_player), cnt, _p(boards), _p(players), _p(lasts),
                                            _p(logits), _p(policy), _p(value), _p(path)), "az_net_eval_delta")
        return logits, policy, value, path

    # ---- single search ----
    def search(self, board, player, last, temperature, noise=None, u=0.5, slot=0):
        board = np.ascontiguousarray(board, np.uint8).reshape(self.nn)
        nz = None if noise is None else np.ascontiguousarray(noise, np.float64)
        if nz is not None and len(nz) != int((board == 0).sum()):
            raise ValueError("noise must have one entry per legal cell")
        pi = np.zeros(self.nn, np.float32); N = np.zeros(self.nn, np.int32)
        W = np.zeros(self.nn, np.float64); P = np.zeros(self.nn, np.float32)
        a = C.c_int32(-1)
        self._check(lib().az_search(self.h, int(slot), _p(board), int(player), int(last), C.c_double(temperature),
                                    _dp(nz), C.c_double(u), _p(pi), C.byref(a), _p(N), _p(W), _p(P)), "az_search")
        self._last_search_batched = False
        return dict(action=int(a.value), pi=pi, N=N, W=W, P=P)

    # ---- many searches at once ----
    def search_batch(self, boards, players, lasts, temperature, noise=None, u=None, slot=0):
        """MCTS.run for every position of a list (az_search_batch): boards [count, n*n] or [count, n, n], players / lasts
        [count], temperature a scalar or [count], noise None or `count` float64 arrays (array i: one entry per legal cell of
        position i), u None (0.5 for every position, like search) or [count].  Position i gets exactly what
        search(boards[i], players[i], lasts[i], temperature[i], noise[i], u[i], slot) returns.
        -> dict(action [count], pi [count, n*n], N, W, P)."""
        nn = self.nn
        boards = np.ascontiguousarray(boards, np.uint8)
        if not ((boards.ndim == 2 and boards.shape[1] == nn) or (boards.ndim == 3 and boards.shape[1:] == (self.n, self.n))):
            raise ValueError(f"boards must be [count, {nn}] or [count, {self.n}, {self.n}], got {boards.shape}")
        cnt = boards.shape[0]
        boards = boards.reshape(cnt, nn)
        players = np.ascontiguousarray(players, np.uint8)
        lasts = np.ascontiguousarray(lasts, np.int16)
        if players.shape != (cnt,) or lasts.shape != (cnt,):
            raise ValueError(f"players and lasts must have one entry per position ({cnt})")
        T = np.asarray(temperature, np.float64)
        if T.ndim == 0:
            T = np.full(cnt, float(T), np.float64)
        if T.shape != (cnt,):
            raise ValueError(f"temperature must be a scalar or have one entry per position ({cnt})")
        T = np.ascontiguousarray(T)
        uu = np.full(cnt, 0.5, np.float64) if u is None else np.ascontiguousarray(u, np.float64)
        if uu.shape != (cnt,):
            raise ValueError(f"u must have one entry per position ({cnt})")
        nz = None
        if noise is not None:
            if len(noise) != cnt:
                raise ValueError(f"noise must have one array per position ({cnt})")
            nz = np.zeros((cnt, nn), np.float64)
            legal = (boards == 0).sum(axis=1)
            for i, row in enumerate(noise):
                row = np.asarray(row, np.float64)
                if row.ndim != 1 or len(row) != int(legal[i]):
                    raise ValueError(f"noise[{i}] must have one entry per legal cell ({int(legal[i])})")
                nz[i, :len(row)] = row
        pi = np.zeros((cnt, nn), np.float32); N = np.zeros((cnt, nn), np.int32)
        W = np.zeros((cnt, nn), np.float64); P = np.zeros((cnt, nn), np.float32)
        a = np.full(cnt, -1, np.int32)
        self._check(lib().az_search_batch(self.h, int(slot), cnt, _p(boards), _p(players), _p(lasts), _p(T), _p(nz), _p(uu),
                                          _p(pi), _p(a), _p(N), _p(W), _p(P)), "az_search_batch")
        self._last_search_batched = True
        return dict(action=a, pi=pi, N=N, W=W, P=P)

    _EVAL_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float))

    def search_callback(self, board, player, last, temperature, fn, noise=None, u=0.5):
        """MCTS.run with the evaluator on the host (az_search_callback): fn(cells uint8[n*n], player, last) -> (policy
        float32[n*n] or [n,n], value).  One host round trip per simulation: the compatibility path for arbitrary
        policy_value_fn callables (mcts.py:87-93)."""
        board = np.ascontiguousarray(board, np.uint8).reshape(self.nn)
        nz = None if noise is None else np.ascontiguousarray(noise, np.float64)
        if nz is not None and len(nz) != int((board == 0).sum()):
            raise ValueError("noise must have one entry per legal cell")
        nn = self.nn
        err = []

        def _cb(user, b, pl, la, pol, val):
            try:
                cells = np.ctypeslib.as_array(b, shape=(nn,)).copy()
                P, v = fn(cells, int(pl), int(la))
                if hasattr(P, "detach"):
                    P = P.detach().cpu().numpy()
                np.ctypeslib.as_array(pol, shape=(nn,))[:] = np.asarray(P, dtype=np.float32).reshape(nn)
                val[0] = float(v)
                return 0
            except Exception as ex:       # nothing may propagate through the C frames
                err.append(ex)
                return 1

        cb = self._EVAL_CB(_cb)
        pi = np.zeros(nn, np.float32); N = np.zeros(nn, np.int32)
        W = np.zeros(nn, np.float64); P = np.zeros(nn, np.float32)
        a = C.c_int32(-1)
        rc = lib().az_search_callback(self.h, _p(board), int(player), int(last), C.c_double(temperature), _dp(nz), C.c_double(u),
                                      cb, None, _p(pi), C.byref(a), _p(N), _p(W), _p(P))
        if err:
            raise err[0]
        self._check(rc, "az_search_callback")
        return dict(action=int(a.value), pi=pi, N=N, W=W, P=P)

    # ---- self-play ----
    def selfplay(self, num_games, seed0=0, max_plies=0, temperature_table=None, noise_tape=None, u_tape=None):
        T = None if temperature_table is None else np.ascontiguousarray(temperature_table, np.float64)
        if T is not None and len(T) < self.nn + 1:
            raise ValueError("temperature_table needs n*n + 1 entries")
        nz = None if noise_tape is None else np.ascontiguousarray(noise_tape, np.float64)
        ut = None if u_tape is None else np.ascontiguousarray(u_tape, np.float64)
        stride = 0 if nz is None else nz.shape[1]
        args = az_selfplay_args(int(seed0), int(num_games), int(max_plies), _dp(T), _dp(nz), _dp(ut), stride)
        c = az_counters()
        self._check(lib().az_selfplay(self.h, C.byref(args), C.byref(c)), "az_selfplay")
        self.last_records = int(c.records)
        self.last_games = int(num_games)
        return c.as_dict()

    def selfplay_begin(self, num_games, seed0=0, max_plies=0, temperature_table=None):
        T = None if temperature_table is None else np.ascontiguousarray(temperature_table, np.float64)
        args = az_selfplay_args(int(seed0), int(num_games), int(max_plies), _dp(T), None, None, 0)
        self._check(lib().az_selfplay_begin(self.h, C.byref(args)), "az_selfplay_begin")
        self.last_games = int(num_games)

    def selfplay_step(self, max_steps=1):
        active = C.c_int32(0)
        c = az_counters()
        self._check(lib().az_selfplay_step(self.h, int(max_steps), C.byref(active), C.byref(c)), "az_selfplay_step")
        return int(active.value), c.as_dict()

    def selfplay_end(self):
        c = az_counters()
        self._check(lib().az_selfplay_end(self.h, C.byref(c)), "az_selfplay_end")
        self.last_records = int(c.records)
        return c.as_dict()

    def games(self):
        nply = np.zeros(self.last_games, np.int32); res = np.zeros(self.last_games, np.int32)
        self._check(lib().az_selfplay_games(self.h, _p(nply), _p(res)), "az_selfplay_games")
        return nply, res

    def records(self):
        R, nn = self.last_records, self.nn
        out = dict(boards=np.zeros((R, nn), np.uint8), movers=np.zeros(R, np.uint8), lasts=np.zeros(R, np.int16),
                   actions=np.zeros(R, np.int16), pis=np.zeros((R, nn), np.float32), visits=np.zeros((R, nn), np.int32),
                   z=np.zeros(R, np.int8))
        self._check(lib().az_selfplay_records(self.h, _p(out["boards"]), _p(out["movers"]), _p(out["lasts"]),
                                              _p(out["actions"]), _p(out["pis"]), _p(out["visits"]), _p(out["z"])),
                    "az_selfplay_records")
        return out

    def clear_episode(self):
        """Forget the last episode (az_selfplay_clear): this engine then contributes no records to the episode-end exchange.
        For a rank that got no games this time."""
        self._check(lib().az_selfplay_clear(self.h), "az_selfplay_clear")
        self.last_records = 0
        self.last_games = 0

    def _torch_sync(self):
        """The engine works on its own non-blocking HIP stream and synchronises it before every call returns; device
        buffers handed in by the caller (torch tensors on the engine's device) must be complete on the caller's side too."""
        import torch
        if torch.cuda.is_available() and torch.cuda.is_initialized():
            torch.cuda.current_stream(self.device).synchronize()

    def pack_into(self, dev_ptr):
        self._torch_sync()
        self._check(lib().az_selfplay_pack(self.h, C.c_void_p(dev_ptr)), "az_selfplay_pack")

    def examples_from_packed(self, packed_ptr, records, aug, states_ptr, pis_ptr, z_ptr):
        self._torch_sync()
        self._check(lib().az_examples_from_packed(self.h, C.c_void_p(packed_ptr), C.c_int64(records), int(aug),
                                                  C.c_void_p(states_ptr), C.c_void_p(pis_ptr), C.c_void_p(z_ptr)),
                    "az_examples_from_packed")

    def examples_gather(self, packed_ptr, idx_ptr, sym_ptr, count, reference_pi, states_ptr, pis_ptr, z_ptr):
        self._torch_sync()
        self._check(lib().az_examples_gather(self.h, C.c_void_p(packed_ptr), C.c_void_p(idx_ptr), C.c_void_p(sym_ptr),
                                             int(count), int(reference_pi), C.c_void_p(states_ptr), C.c_void_p(pis_ptr),
                                             C.c_void_p(z_ptr)), "az_examples_gather")

    # ---- rules ----
    def rules_replay(self, actions):
        """Gomoku rules on the device for whole action lists (az_rules_replay): actions [games][max_len] int16, -1 padded."""
        acts = np.ascontiguousarray(actions, np.int16)
        if acts.ndim == 1:
            acts = acts.reshape(1, -1)
        G, L = acts.shape
        term = np.zeros((G, max(L, 1)), np.uint8); boards = np.zeros((G, self.nn), np.uint8)
        players = np.zeros(G, np.int32); results = np.zeros(G, np.int32); bad = np.zeros(G, np.int32)
        self._check(lib().az_rules_replay(self.h, G, L, _p(acts), _p(term), _p(boards), _p(players), _p(results), _p(bad)),
                    "az_rules_replay")
        return dict(term_before=term[:, :L].astype(bool), boards=boards, players=players, results=results, first_illegal=bad)

    # ---- arena ----
    def arena(self, num_games, seed0=0, temperature_table=None, u_tape=None):
        T = None if temperature_table is None else np.ascontiguousarray(temperature_table, np.float64)
        ut = None if u_tape is None else np.ascontiguousarray(u_tape, np.float64)
        args = az_arena_args(int(seed0), int(num_games), _dp(T), _dp(ut))
        res = az_arena_result()
        results = np.zeros(num_games, np.int32); actions = np.zeros((num_games, self.nn), np.int16)
        nply = np.zeros(num_games, np.int32)
        self._check(lib().az_arena(self.h, C.byref(args), C.byref(res), _p(results), _p(actions), _p(nply)), "az_arena")
        self.last_games = int(num_games)      # the arena is the engine's last episode now: games(), records(), values(), resign_info()
        self.last_records = int(nply.sum())
        return dict(wins=res.wins, losses=res.losses, draws=res.draws, total=res.total, win_rate=res.win_rate,
                    results=results, actions=actions, nply=nply)

    # ---- batched external evaluator ----
    def set_external_evaluator(self, planes_ptr, policy_ptr, value_ptr, capacity, fn):
        """Opt-in: every net evaluation of selfplay*, arena, search and search_batch goes to fn(net, count) -> None
        (az_set_external_evaluator).  planes_ptr / policy_ptr / value_ptr: DEVICE buffers [capacity, 4, n, n], [capacity, n*n]
        and [capacity] of float32 on the engine's GPU, capacity >= ext_capacity().  When fn is called the first `count`
        entries of the planes are complete; when it returns, the same entries of policy and value must be complete in
        device memory (synchronise your stream).  fn runs on the calling thread; an exception it raises ends the engine
        call and is raised again from it.  See include/az_engine.h."""
        if not callable(fn):
            raise TypeError("fn must be callable: fn(net, count) -> None")
        if not (planes_ptr and policy_ptr and value_ptr):
            raise ValueError("planes_ptr, policy_ptr and value_ptr must be device pointers (tensor.data_ptr())")
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError(f"capacity must be positive, got {capacity}")
        err = self.__dict__.setdefault("_ext_err", [])

        def _cb(user, net, count):
            try:
                fn(int(net), int(count))
                return 0
            except Exception as ex:       # nothing may propagate through the C frames
                err.append(ex)
                return 1

        cb = _EVAL_BATCH_FN(_cb)
        ev = az_ext_evaluator(int(planes_ptr), int(policy_ptr), int(value_ptr), capacity, cb, None)
        self._check(lib().az_set_external_evaluator(self.h, C.byref(ev)), "az_set_external_evaluator")
        self._ext_cb = cb

    def clear_external_evaluator(self):
        """Back to the engine's own evaluator (its nets, or the synthetic one)."""
        self._check(lib().az_set_external_evaluator(self.h, None), "az_set_external_evaluator")
        self._ext_cb = None

    def external_evaluator(self):
        return bool(lib().az_get_external_evaluator(self.h))

    def ext_capacity(self):
        """Items a request can hold: slots x leaves per batch; the evaluator's buffers must hold as many."""
        return int(lib().az_ext_capacity(self.h))

    def ext_stats(self):
        """dict(requests, items) of the last (or open) episode / call: calls of the evaluator and items handed out."""
        r, i = C.c_int64(0), C.c_int64(0)
        self._check(lib().az_ext_stats(self.h, C.byref(r), C.byref(i)), "az_ext_stats")
        return dict(requests=int(r.value), items=int(i.value))

    def set_subtree_reuse(self, on):
        """Opt-in: keep the chosen child's subtree for the next ply (mcts.py:17-22 TODO); see include/az_engine.h."""
        self._check(lib().az_set_subtree_reuse(self.h, 1 if on else 0), "az_set_subtree_reuse")

    def set_virtual_loss(self, leaves):
        """Opt-in: virtual-loss batching, `leaves` leaves per search and evaluation batch (mcts.py:17-22 TODO); 1 = the
        reference's sequential loop.  See include/az_engine.h."""
        self._check(lib().az_set_virtual_loss(self.h, int(leaves)), "az_set_virtual_loss")

    def set_eval_cache(self, entries):
        """Opt-in: evaluation cache of `entries` positions in HBM (mcts.py:17,22 TODO), 0 = off; results are bit-identical."""
        self._check(lib().az_set_eval_cache(self.h, C.c_int64(int(entries))), "az_set_eval_cache")

    def set_leaf_symmetry(self, on):
        """Opt-in: every net evaluation of a search sees a pseudo-random dihedral symmetry of the position (SURVEY 8f-2's
        optional half); see include/az_engine.h."""
        self._check(lib().az_set_leaf_symmetry(self.h, 1 if on else 0), "az_set_leaf_symmetry")

    def set_start_positions(self, boards, players, lasts, first=0):
        """Opt-in: later selfplay* / arena games start from these positions instead of the empty board
        (az_set_start_positions): boards [count, n*n] or [count, n, n] cells 0 / 1 X / 2 O, players / lasts [count].  Self-play
        game g starts from position (first + g) % count; arena game g from ((first + g) >> 1) % count, colours exchanged
        for odd g.  Plies stay absolute (stones on the board); records carry the searched plies only."""
        nn = self.nn
        boards = np.ascontiguousarray(boards, np.uint8)
        if not ((boards.ndim == 2 and boards.shape[1] == nn) or (boards.ndim == 3 and boards.shape[1:] == (self.n, self.n))):
            raise ValueError(f"boards must be [count, {nn}] or [count, {self.n}, {self.n}], got {boards.shape}")
        cnt = boards.shape[0]
        if cnt == 0:
            raise ValueError("no positions given (clear_start_positions() goes back to the empty board)")
        boards = boards.reshape(cnt, nn)
        players = np.ascontiguousarray(players, np.uint8)
        lasts = np.ascontiguousarray(lasts, np.int16)
        if players.shape != (cnt,) or lasts.shape != (cnt,):
            raise ValueError(f"players and lasts must have one entry per position ({cnt})")
        self._check(lib().az_set_start_positions(self.h, cnt, _p(boards), _p(players), _p(lasts), int(first)),
                    "az_set_start_positions")

    def clear_start_positions(self):
        self._check(lib().az_set_start_positions(self.h, 0, None, None, None, 0), "az_set_start_positions")

    def start_positions(self):
        """Number of start positions in force, 0 = games start from the empty board."""
        return int(lib().az_get_start_positions(self.h))

    # ---- search value per record, resignation ----
    def set_resign(self, threshold, min_ply=0, playout=0.0):
        """Opt-in: a selfplay* / arena game ends as a loss of the mover once a ply at or after min_ply has a search value
        v < -threshold (v = W / N of the root's most visited cell); a pseudo-random share `playout` of the self-play games,
        named by their seeds, is exempt and plays on.  threshold = 0 switches it off.  See include/az_engine.h."""
        threshold, min_ply = float(threshold), int(min_ply)
        if not 0.0 <= threshold <= 1.0:
            raise ValueError(f"threshold must be 0 (off) or in (0, 1], got {threshold}")
        if min_ply < 0:
            raise ValueError(f"min_ply must be >= 0, got {min_ply}")
        self._check(lib().az_set_resign(self.h, threshold, min_ply, resign_permille(playout)), "az_set_resign")

    def resign(self):
        """The setting in force: dict(threshold, min_ply, playout); threshold 0.0 = off."""
        t, m, p = C.c_double(0.0), C.c_int(0), C.c_int(0)
        self._check(lib().az_get_resign(self.h, C.byref(t), C.byref(m), C.byref(p)), "az_get_resign")
        return dict(threshold=float(t.value), min_ply=int(m.value), playout=int(p.value) / 1000.0)

    def values(self):
        """float32 search value of every record of the last episode, in the order of records() (az_selfplay_values)."""
        v = np.zeros(self.last_records, np.float32)
        self._check(lib().az_selfplay_values(self.h, _p(v)), "az_selfplay_values")
        return v

    def pack_values_into(self, dev_ptr):
        """The same values into a device buffer of last_records floats, in pack_into's order (az_selfplay_pack_values)."""
        self._torch_sync()
        self._check(lib().az_selfplay_pack_values(self.h, C.c_void_p(dev_ptr)), "az_selfplay_pack_values")

    def resign_info(self):
        """(cross_ply int32[games], exempt bool[games]) of the last episode: the first ply whose value crossed the threshold
        (absolute ply, -1 = none), exempt games included (az_selfplay_resign_info)."""
        G = getattr(self, "last_games", 0)
        cross = np.full(G, -1, np.int32); ex = np.zeros(G, np.uint8)
        self._check(lib().az_selfplay_resign_info(self.h, _p(cross), _p(ex)), "az_selfplay_resign_info")
        return cross, ex.astype(bool)

    # ---- playout cap randomisation ----
    def set_playout_cap(self, fast_sims, full=0.25, export_full_only=True):
        """Opt-in: only a pseudo-random share `full` of the self-play plies, named by game seed and ply, gets the full search
        with root noise; the others are searched with fast_sims simulations and no noise.  With export_full_only the packed
        export (pack_into, pack_values_into, the dist_* exchange) carries the records of full plies only.  fast_sims = 0
        switches it off.  See include/az_engine.h."""
        fast_sims = int(fast_sims)
        if fast_sims < 0:
            raise ValueError(f"fast_sims must be 0 (off) or 1..num_simulations, got {fast_sims}")
        self._check(lib().az_set_playout_cap(self.h, fast_sims, playout_cap_permille(full), 1 if export_full_only else 0),
                    "az_set_playout_cap")

    def playout_cap(self):
        """The setting in force: dict(fast_sims, full, export_full_only); fast_sims 0 = off."""
        f, p, x = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(lib().az_get_playout_cap(self.h, C.byref(f), C.byref(p), C.byref(x)), "az_get_playout_cap")
        return dict(fast_sims=int(f.value), full=int(p.value) / 1000.0, export_full_only=bool(x.value))

    # ---- forced playouts and policy target pruning ----
    def set_forced_playouts(self, k, prune=True):
        """Opt-in (KataGo): at every noised root a child is selected regardless of its PUCT value while its visits squared stay
        below k * prior * (simulations so far), and with `prune` pi and the sampled move are made from counts that take those
        visits back unless the search confirmed them.  k = 0 switches it off; KataGo uses 2.  See include/az_engine.h."""
        self._check(lib().az_set_forced_playouts(self.h, float(k), 1 if prune else 0), "az_set_forced_playouts")

    def forced_playouts(self):
        """The setting in force: dict(k, prune); k 0.0 = off."""
        k, p = C.c_double(0.0), C.c_int(0)
        self._check(lib().az_get_forced_playouts(self.h, C.byref(k), C.byref(p)), "az_get_forced_playouts")
        return dict(k=float(k.value), prune=bool(p.value))

    # ---- selection rule ----
    def set_selection(self, fpu=0.2, fpu_root=0.0, cpuct_base=19652.0, cpuct_factor=0.0, on=True):
        """Opt-in: an unvisited child is worth its parent's value less fpu * sqrt(visited prior mass) (fpu_root at the root)
        instead of 0, and c_puct grows with the parent's count, c_puct + cpuct_factor * log((N + cpuct_base + 1) / cpuct_base).
        on=False switches it off.  While it is on every board size runs the lock-step kernels.  See include/az_engine.h."""
        self._check(lib().az_set_selection(self.h, 1 if on else 0, float(fpu), float(fpu_root), float(cpuct_base), float(cpuct_factor)),
                    "az_set_selection")

    def selection(self):
        """The setting: dict(on, fpu, fpu_root, cpuct_base, cpuct_factor); the parameters are the last ones set (az_get_selection)."""
        on = C.c_int(0)
        v = [C.c_double(0.0) for _ in range(4)]
        self._check(lib().az_get_selection(self.h, C.byref(on), *[C.byref(x) for x in v]), "az_get_selection")
        return dict(on=bool(on.value), fpu=float(v[0].value), fpu_root=float(v[1].value), cpuct_base=float(v[2].value),
                    cpuct_factor=float(v[3].value))

    # ---- candidate moves ----
    def set_candidates(self, radius):
        """Opt-in: every search expands, noises and selects only the empty cells within Chebyshev distance `radius` (1 .. n-1) of
        a stone, every cell on an empty board, with the priors normalised over them; 0 switches it off.  While it is on every
        board size runs the lock-step kernels.  See include/az_engine.h."""
        self._check(lib().az_set_candidates(self.h, int(radius)), "az_set_candidates")

    def candidates(self):
        """The radius set, 0 = off (az_get_candidates)."""
        r = C.c_int(0)
        self._check(lib().az_get_candidates(self.h, C.byref(r)), "az_get_candidates")
        return int(r.value)

    # ---- win rule ----
    def set_win_rule(self, rule):
        """Which game is played: "freestyle" (default, the reference's: a run of win_length or more wins) or "exact" (standard
        Gomoku: a maximal run of exactly win_length wins, overlines give nothing).  Holds for every search, self-play, arena and
        rules_replay; refused while start positions are set under the other rule.  See include/az_engine.h."""
        rid = win_rule_id(rule)                                 # ValueError before the engine is touched
        self._check(lib().az_set_win_rule(self.h, rid), "az_set_win_rule")

    def win_rule(self):
        """The rule in force, "freestyle" | "exact" (az_get_win_rule)."""
        return win_rule_name(lib().az_get_win_rule(self.h))

    # ---- MCTS-Solver ----
    def set_solver(self, on=True):
        """Opt-in (Winands et al. 2008): every search keeps proven wins, losses and draws in its tree, propagates them by minimax,
        never samples a refuted move when a better one is known and reports an exact value for a proven root.  See
        include/az_engine.h."""
        self._check(lib().az_set_solver(self.h, 1 if on else 0), "az_set_solver")

    def solver(self):
        """True while the solver is on (az_get_solver)."""
        return lib().az_get_solver(self.h) == 1

    def proofs(self):
        """int8 root status (PROOF_*) of every record of the last episode, in the order of records() (az_selfplay_proofs)."""
        v = np.zeros(self.last_records, np.int8)
        self._check(lib().az_selfplay_proofs(self.h, _p(v)), "az_selfplay_proofs")
        return v

    def last_proof(self):
        """(edges, root) of the last search(): int8[n*n] statuses of the root's edges (0 on occupied cells) and the root's own;
        after search_batch(): int8[count, n*n] and int8[count] (az_last_proof)."""
        cnt = C.c_int32(0)
        self._check(lib().az_last_proof(self.h, 0, None, None, C.byref(cnt)), "az_last_proof")
        cnt = int(cnt.value)
        edges = np.zeros((cnt, self.nn), np.int8); roots = np.zeros(cnt, np.int8)
        self._check(lib().az_last_proof(self.h, cnt, _p(edges), _p(roots), None), "az_last_proof")
        if not getattr(self, "_last_search_batched", False):
            return edges[0], int(roots[0])
        return edges, roots

    def solver_stops(self):
        """Simulations of the last episode / search call that ended on a proven edge (az_solver_stops)."""
        v = C.c_int64(0)
        self._check(lib().az_solver_stops(self.h, C.byref(v)), "az_solver_stops")
        return int(v.value)

    # ---- root threat search ----
    def set_threat_search(self, max_depth=8, node_budget=256):
        """Opt-in: an exact forced-four search (VCF) on every root before the simulations; its proven wins and forced blocks go
        to the solver as premarked root statuses.  max_depth = 0 switches it off.  Needs set_solver(True).  See
        include/az_engine.h."""
        self._check(lib().az_set_threat_search(self.h, int(max_depth), int(node_budget)), "az_set_threat_search")

    def threat_search(self):
        """(max_depth, node_budget) in force, (0, 0) = off (az_get_threat_search)."""
        d, b = C.c_int(0), C.c_int(0)
        self._check(lib().az_get_threat_search(self.h, C.byref(d), C.byref(b)), "az_get_threat_search")
        return int(d.value), int(b.value)

    def threat_batch(self, boards, players, max_depth=8, node_budget=256, outputs=("status", "move", "depth", "nodes", "edges")):
        """The threat search kernel on its own (az_threat_batch): boards uint8[count, n*n] (0 empty, 1 X, 2 O), players
        uint8[count] -> dict of the requested outputs: status int8[count], move / depth / nodes int32[count], edges
        int8[count, n*n]."""
        boards = np.ascontiguousarray(boards, np.uint8).reshape(-1, self.nn) if np.size(boards) else np.zeros((0, self.nn), np.uint8)
        players = np.ascontiguousarray(players, np.uint8).reshape(-1)
        count = len(boards)
        if len(players) != count:
            raise ValueError("threat_batch: one player per board")
        shapes = dict(status=((count,), np.int8), move=((count,), np.int32), depth=((count,), np.int32), nodes=((count,), np.int32),
                      edges=((count, self.nn), np.int8))
        out = {k: np.zeros(*shapes[k]) for k in outputs}
        self._check(lib().az_threat_batch(self.h, count, _p(boards), _p(players), int(max_depth), int(node_budget),
                                          *[_p(out.get(k)) for k in ("status", "move", "depth", "nodes", "edges")]), "az_threat_batch")
        return out

    def threats(self):
        """int8 depth of the threat search's win at every record's root of the last episode, 0 = none, in the order of
        records() (az_selfplay_threats)."""
        v = np.zeros(self.last_records, np.int8)
        self._check(lib().az_selfplay_threats(self.h, _p(v)), "az_selfplay_threats")
        return v

    def threat_stats(self):
        """dict(win_roots, lost_roots, block_roots, exhausted, nodes) of the last (or open) episode or search call (az_threat_stats)."""
        v = [C.c_int64(0) for _ in range(5)]
        self._check(lib().az_threat_stats(self.h, *[C.byref(x) for x in v]), "az_threat_stats")
        return dict(zip(("win_roots", "lost_roots", "block_roots", "exhausted", "nodes"), (int(x.value) for x in v)))

    # ---- Gumbel root search ----
    def set_gumbel(self, m, c_visit=50.0, c_scale=1.0):
        """Opt-in (Danihelka et al. 2022): every noised root samples m Gumbel-top candidates, searches them by sequential halving
        and makes pi = softmax(logits + sigma(completed Q)); the noise tape is read as Gumbel(0, 1) draws.  m = 0 switches it
        off; the paper uses m = 16, c_visit = 50, c_scale = 1.  See include/az_engine.h."""
        self._check(lib().az_set_gumbel(self.h, int(m), float(c_visit), float(c_scale)), "az_set_gumbel")

    def gumbel(self):
        """The setting in force: dict(m, c_visit, c_scale); m 0 = off."""
        m, cv, cs = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        self._check(lib().az_get_gumbel(self.h, C.byref(m), C.byref(cv), C.byref(cs)), "az_get_gumbel")
        return dict(m=int(m.value), c_visit=float(cv.value), c_scale=float(cs.value))

    # ---- device RNG ----
    def set_rng(self, mode):
        """"philox": the engine fills its own tapes on the GPU from the counter-based stream of include/az_engine.h, with no host
        tape thread; "numpy" (the default): numpy's RandomState streams made on the host, the reference's numbers (az_set_rng)."""
        self._check(lib().az_set_rng(self.h, RNG_MODES.index(check_rng(mode))), "az_set_rng")

    def rng(self):
        """The RNG mode in force: "numpy" or "philox" (az_get_rng)."""
        return RNG_MODES[lib().az_get_rng(self.h)]

    def philox_tape_device(self, seed0, games, alpha=0.3, max_plies=0, kind="dirichlet"):
        """The tape kernel on its own (az_rng_philox_tape_device): games seed0 + 0 .. games - 1 on the engine's board ->
        (noise float64[games, tape length], u float64[games, plies]), each row what philox_tape gives for that seed."""
        nn = self.nn
        plies = max_plies if 0 < max_plies < nn else nn
        noise = np.zeros((int(games), sum(nn - m for m in range(plies))), np.float64)
        u = np.zeros((int(games), nn), np.float64)
        self._check(lib().az_rng_philox_tape_device(self.h, int(seed0) & (2 ** 64 - 1), int(games), float(alpha), int(max_plies),
                                                    TAPE_KINDS.index(kind), _p(noise), _p(u)), "az_rng_philox_tape_device")
        return noise, u[:, :plies]

    def sims(self):
        """int32 simulations of every record of the last episode, in the order of records() (az_selfplay_sims)."""
        s = np.zeros(self.last_records, np.int32)
        self._check(lib().az_selfplay_sims(self.h, _p(s)), "az_selfplay_sims")
        return s

    def export_count(self):
        """Records pack_into writes for the last episode: all of them, or the full plies' only (az_selfplay_export_count)."""
        n = C.c_int64(0)
        self._check(lib().az_selfplay_export_count(self.h, C.byref(n)), "az_selfplay_export_count")
        return int(n.value)

    def set_trunk_mode(self, mode):
        """Opt-in: "bf16x3" / "f16x2" = fp32-emulating conv trunks on the 16-bit matrix cores (tolerance instead of
        bit-exactness; f16x2 is the faster one and has float16's range), "f32" = the default canonical float32 trunk.
        See include/az_engine.h."""
        code = {"f32": AZ_TRUNK_F32, "bf16x3": AZ_TRUNK_BF16X3, "f16x2": AZ_TRUNK_F16X2}.get(mode, mode)
        self._check(lib().az_set_trunk_mode(self.h, int(code)), "az_set_trunk_mode")

    def trunk_mode(self):
        return {AZ_TRUNK_BF16X3: "bf16x3", AZ_TRUNK_F16X2: "f16x2"}.get(int(lib().az_get_trunk_mode(self.h)), "f32")

    # ---- multi-GPU exchange inside the library (RCCL on the engine's stream; include/az_engine.h az_dist_*) ----
    def dist_init(self, unique_id, rank, world):
        if len(unique_id) != AZ_DIST_ID_BYTES:
            raise ValueError("unique_id must be AZ_DIST_ID_BYTES bytes (dist_unique_id())")
        self._check(lib().az_dist_init(self.h, C.c_char_p(bytes(unique_id)), int(rank), int(world)), "az_dist_init")

    def dist_rank(self):
        return int(lib().az_dist_rank(self.h))

    def dist_world(self):
        return int(lib().az_dist_world(self.h))

    def dist_counts(self):
        c = np.zeros(self.dist_world(), np.int64)
        self._check(lib().az_dist_counts(self.h, _p(c)), "az_dist_counts")
        return [int(x) for x in c]

    def dist_gather_records(self, dst, dev_ptr):
        """dst = rank that receives every rank's packed records (-1: all ranks); dev_ptr = device buffer (0 where not receiving)."""
        self._torch_sync()
        self._check(lib().az_dist_gather_records(self.h, int(dst), C.c_void_p(dev_ptr or None)), "az_dist_gather_records")

    def dist_allreduce_sum(self, values):
        v = np.ascontiguousarray(values, np.int64).copy()
        self._check(lib().az_dist_allreduce_sum(self.h, _p(v), len(v)), "az_dist_allreduce_sum")
        return [int(x) for x in v]

    def dist_broadcast(self, dev_ptr, nbytes, root=0):
        self._torch_sync()
        self._check(lib().az_dist_broadcast(self.h, C.c_void_p(dev_ptr), C.c_int64(int(nbytes)), int(root)), "az_dist_broadcast")

    def set_profiling(self, on):
        lib().az_set_profiling(self.h, 1 if on else 0)

    def lanes(self):
        """Number of lanes (streams + driver threads) inside the engine, az_config.engines after the library's choice."""
        return int(lib().az_get_lanes(self.h))

    def persistent(self):
        """Games per workgroup of the persistent search kernel in the last / open episode, 0 = lock-step pipeline."""
        return int(lib().az_get_persistent(self.h))

    def counters(self):
        c = az_counters()
        lib().az_get_counters(self.h, C.byref(c))
        return c.as_dict()


class MultiEngine(Engine):
    """An engine with an explicit number of lanes (kept for callers written against the host-thread version: the
    lanes, their streams and their driver threads now live inside the library, az_config.engines)."""

    def __init__(self, board_size, win_length, num_simulations, slots, engines=1, **kw):
        super().__init__(board_size, win_length, num_simulations, slots, engines=max(1, min(int(engines), slots)), **kw)
