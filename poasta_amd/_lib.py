"""ctypes binding of the C ABI in include/poasta_amd.h (libpoasta_amd.so, built in-tree by hipcc).

There is no fallback: if the shared library is missing or cannot be loaded the import of any compute
entry point raises, and on a box without a HIP device every compute call returns POA_ERR_NO_DEVICE.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("POA_LIB_PATH") or os.path.join(_HERE, "libpoasta_amd.so")  # override: A/B runs of two builds
CSRC = os.path.join(_HERE, "csrc")

POA_OK = 0
ERRORS = {-1: "POA_ERR_INVALID_ARG", -2: "POA_ERR_NOT_A_DAG", -3: "POA_ERR_NO_DEVICE", -4: "POA_ERR_HIP",
          -5: "POA_ERR_CAPACITY", -6: "POA_ERR_OUT_OF_MEMORY", -7: "POA_ERR_UNSUPPORTED"}
POA_NONE = 0xFFFFFFFF
FLAG_AMBIGUOUS, FLAG_START_QUIRK, FLAG_REF_PANIC, FLAG_SHORT_QUERY, FLAG_TRUNCATED, FLAG_EMPTY_GRAPH = 1, 2, 4, 8, 16, 32
FLAG_CAPPED = 0x80

# every symbol include/poasta_amd.h declares (checked by tests/test_abi.py)
EXPORTS = ["poa_version", "poa_last_error", "poa_device_count", "poa_graph_create", "poa_graph_destroy",
           "poa_graph_rows", "poa_graph_node_rows", "poa_graph_update", "poa_align_batch", "poa_align_batch_ex", "poa_align_batch_2piece", "poa_align_batch_2piece_ex", "poa_planes_2piece", "poa_release_cache", "poa_batch_create", "poa_batch_run",
           "poa_batch_run_ex",
           "poa_batch_fetch", "poa_batch_stats", "poa_batch_device_results", "poa_batch_fetch_search_counters", "poa_batch_last_layout", "poa_batch_band_info", "poa_batch_band_pair_info", "poa_batch_band_narrow_info", "poa_batch_last_launch", "poa_batch_replay_info", "poa_batch_fetch_planes", "poa_batch_fetch_compact", "poa_batch_destroy",
           "poa_batch_run_2piece", "poa_batch_fetch_planes_2piece",
           "poa_graph_sweep_slots", "poa_batch_create_ex", "poa_batch_workspace_bytes", "poa_graph_checkpoint_plan", "poa_graph_checkpoint_plan2",
           "poa_multi_footprint", "poa_multi_create", "poa_multi_run", "poa_multi_fetch", "poa_multi_stats", "poa_multi_device_results",
           "poa_multi_workspace_bytes", "poa_multi_destroy", "poa_align_multi",
           "poa_multi_footprint_2piece", "poa_multi_create_2piece", "poa_multi_run_2piece", "poa_align_multi_2piece",
           "poa_scoreset_footprint", "poa_scoreset_create", "poa_scoreset_run", "poa_scoreset_run_2piece", "poa_scoreset_fetch",
           "poa_scoreset_stats", "poa_scoreset_device_results", "poa_scoreset_workspace_bytes", "poa_scoreset_destroy",
           "poa_score_pairs", "poa_score_pairs_2piece",
           "poa_graph_sweep_checks"]
# every symbol include/poasta_amd_scoreset_cap.h declares (checked by tests/test_sweep_checks.py)
EXPORTS_SCORESET_CAP = ["poa_scoreset_run_capped", "poa_scoreset_run_2piece_capped", "poa_scoreset_fetch_swept"]
# every symbol include/poasta_amd_scoreset_best.h declares (checked by tests/test_scoreset_best_plan.py)
EXPORTS_SCORESET_BEST = ["poa_scoreset_run_best", "poa_scoreset_run_2piece_best", "poa_scoreset_fetch_best", "poa_scoreset_device_best",
                         "poa_score_best", "poa_score_best_2piece"]
CFG_BEST_PAIR_ORDER = 2
# every symbol include/poasta_amd_tb.h declares (checked by tests/test_tb_lean.py)
EXPORTS_TB = ["poa_batch_tb_info"]
TB_LEAN_SHIFT = 4
# every symbol include/poasta_amd_multi_dense.h declares (checked by tests/test_multi_dense_plan.py)
EXPORTS_MULTI_DENSE = ["poa_multi_footprint_dense", "poa_multi_create_dense", "poa_multi_run_dense", "poa_align_multi_dense",
                       "poa_graph_compact_elems", "poa_multi_last_launch"]
# every symbol include/poasta_amd_multi_exact.h declares (checked by tests/test_multi_exact_plan.py)
EXPORTS_MULTI_EXACT = ["poa_multi_footprint_exact", "poa_multi_create_exact", "poa_multi_run_exact", "poa_multi_fetch_search_counters",
                       "poa_align_multi_exact", "poa_multi_replay_info"]
# every symbol include/poasta_amd_multi_dense2.h declares (checked by tests/test_multi_dense2_plan.py)
EXPORTS_MULTI_DENSE2 = ["poa_multi_footprint_dense_2piece", "poa_multi_create_dense_2piece", "poa_multi_run_dense_2piece",
                        "poa_align_multi_dense_2piece", "poa_multi_fetch_planes_2piece"]


class PoaBest(C.Structure):
    """poa_best_t: one record per query of a best-of score-set run."""
    _fields_ = [("pair", C.c_uint32), ("score", C.c_uint32), ("flags", C.c_uint32), ("second_score", C.c_uint32),
                ("n_within", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class PoaCosts2(C.Structure):
    _fields_ = [("mismatch", C.c_uint8), ("gap_open1", C.c_uint8), ("gap_extend1", C.c_uint8), ("gap_open2", C.c_uint8),
                ("gap_extend2", C.c_uint8), ("wide_planes", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class PoaCosts(C.Structure):
    _fields_ = [("mismatch", C.c_uint8), ("gap_open", C.c_uint8), ("gap_extend", C.c_uint8), ("reserved", C.c_uint8)]


class PoaBound(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("value", C.c_uint32)]


class PoaConfig(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("heuristic", C.c_uint32), ("pruning", C.c_uint32), ("queue_entries_per_cell", C.c_float),
                ("flags", C.c_uint32), ("span", C.c_uint32), ("qry_free_begin", PoaBound), ("qry_free_end", PoaBound),
                ("graph_free_begin", PoaBound), ("graph_free_end", PoaBound), ("tune", C.c_uint32 * 32)]


# poa_config_t.tune (include/poasta_amd.h: POA_TUNE_*): the library reads no environment variable; A/B scripts and the variant
# sweep set POA_<NAME> and this binding copies them into the config of every call (tune_from_env).
TUNE_KEYS = ("PLANES", "COMPACT", "PACKED", "RELATIVE", "PX", "MF", "MW", "PXMW", "FWD_QUADS", "FUSE_TB", "TB_GROUP", "TB_DEPTH",
             "EXACT_IMPL", "EXACT_LANES", "EXACT_LDS", "WS_LANES", "WS_GROUP", "WS_WAVES", "WS_RING_GLOBAL", "WS_STATIC",
             "WS_CHUNK_CAP", "WS_PROF", "PS_LANES", "PS_LEAN", "TIMING", "WS_ADAPT", "WS_REC", "CKPT_ROWS", "BAND", "BAND_DELTA", "BAND_PAIR", "CAP_STRIDE")
EXACT_IMPLS = {"lane": 1, "wave": 2, "flat": 3}


def tune_from_env(cfg=None, **overrides):
    """Fill cfg.tune from POA_<NAME> environment variables and keyword overrides (exact_impl="flat", ws_lanes=1, ...).
    Returns cfg (a dense-mode PoaConfig if none was given), or None if nothing is set and no cfg was given."""
    vals = {}
    for i, k in enumerate(TUNE_KEYS):
        v = overrides.get(k.lower(), os.environ.get("POA_" + k))
        if v is None or v == "":
            continue
        vals[i] = EXACT_IMPLS[v] if (k == "EXACT_IMPL" and v in EXACT_IMPLS) else int(v)
    # POA_BAND_NARROW (0: never the narrow tier of the paired banded pass, 1: for every pair whose class has a narrow band): the
    # table is full, so it rides in BAND_PAIR's entry (poasta_amd.h: POA_BAND_NARROW_SHIFT; pairing 2 = by the rule, as if unset)
    nv = overrides.get("band_narrow", os.environ.get("POA_BAND_NARROW"))
    if nv is not None and nv != "":
        i = TUNE_KEYS.index("BAND_PAIR")
        vals[i] = (min(vals[i], 1) if i in vals else 2) | ((2 if int(nv) else 1) << 2)
    # POA_TB_LEAN (0: never the lean traceback kernel, 1: wherever it is eligible) rides in the same entry, above the narrow tier's
    # bits (poasta_amd_tb.h: POA_TB_LEAN_SHIFT)
    lv = overrides.get("tb_lean", os.environ.get("POA_TB_LEAN"))
    if lv is not None and lv != "":
        i = TUNE_KEYS.index("BAND_PAIR")
        vals[i] = (vals[i] if i in vals else 2) | ((2 if int(lv) else 1) << TB_LEAN_SHIFT)
    if cfg is None:
        if not vals:
            return None
        cfg = PoaConfig()
    for i, v in vals.items():
        cfg.tune[i] = v + 1
    return cfg


BOUND_UNBOUNDED, BOUND_INCLUDED, BOUND_EXCLUDED = 0, 1, 2
SPAN_GLOBAL, SPAN_ENDS_FREE = 0, 1


MODE_DENSE, MODE_EXACT, MODE_HYBRID, MODE_SCORE, MODE_CHECKPOINT, MODE_CHECKPOINT2 = 0, 1, 2, 3, 4, 5
HEURISTIC_DIJKSTRA, HEURISTIC_MINGAP = 0, 1
FLAG_EXACT_OVERFLOW = 0x40
CFG_FULL_PLANES = 1
CFG_WIDE_QUERIES = 2    # POA_CFG_WIDE_QUERIES: dense and exact multi-graph batches with queries of more than 1023 symbols
LAUNCH_STRIPS = 4       # POA_LAUNCH_STRIPS in out[2] of poa_multi_last_launch


class PoaStats(C.Structure):
    _fields_ = [("cells", C.c_uint64), ("bases", C.c_uint64), ("plane_bytes", C.c_uint64), ("n_queries", C.c_uint32),
                ("n_chunks", C.c_uint32), ("n_forward_launches", C.c_uint32), ("n_flagged", C.c_uint32),
                ("ms_forward", C.c_float), ("ms_traceback", C.c_float), ("ms_h2d", C.c_float), ("ms_d2h", C.c_float),
                ("ms_exact", C.c_float), ("n_exact", C.c_uint32), ("ms_total", C.c_float), ("n_runs", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ }


class PoaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERRORS.get(code, "POA_ERR"), code, msg))
        self.code = code


def build(force=False):
    """Compile the HIP engine for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(_HERE, "..", "include", h) for h in ("poasta_amd.h", "poasta_amd_scoreset_cap.h", "poasta_amd_scoreset_best.h", "poasta_amd_tb.h", "poasta_amd_multi_dense.h", "poasta_amd_multi_exact.h", "poasta_amd_multi_dense2.h")]
    stale = not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC] + (["-B"] if force else []))
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("poasta_amd: %s is missing — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.poa_version.restype = C.c_char_p
    L.poa_last_error.restype = C.c_char_p
    L.poa_device_count.restype = C.c_int
    L.poa_graph_create.restype = C.c_int
    L.poa_graph_create.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, C.POINTER(vp)]
    L.poa_graph_destroy.argtypes = [vp]
    L.poa_graph_destroy.restype = None
    L.poa_graph_rows.restype = C.c_uint32
    L.poa_graph_rows.argtypes = [vp]
    L.poa_graph_node_rows.restype = C.c_int
    L.poa_graph_node_rows.argtypes = [vp, vp]
    L.poa_align_batch.restype = C.c_int
    L.poa_align_batch.argtypes = [vp, C.POINTER(PoaCosts), C.c_uint32, vp, vp, vp, vp, vp, C.c_uint64, vp,
                                  C.POINTER(PoaStats), C.c_int]
    L.poa_align_batch_ex.restype = C.c_int
    L.poa_align_batch_ex.argtypes = [vp, C.POINTER(PoaCosts), C.POINTER(PoaConfig), C.c_uint32, vp, vp, vp, vp, vp, C.c_uint64, vp,
                                     C.POINTER(PoaStats), C.c_int]
    L.poa_align_batch_2piece.restype = C.c_int
    L.poa_align_batch_2piece.argtypes = [vp, C.POINTER(PoaCosts2), C.c_uint32, vp, vp, vp, vp, vp, C.c_uint64, vp,
                                         C.POINTER(PoaStats), C.c_int]
    L.poa_align_batch_2piece_ex.restype = C.c_int
    L.poa_align_batch_2piece_ex.argtypes = [vp, C.POINTER(PoaCosts2), C.POINTER(PoaConfig), C.c_uint32, vp, vp, vp, vp, vp, C.c_uint64, vp,
                                            C.POINTER(PoaStats), vp, C.c_int]
    L.poa_planes_2piece.restype = C.c_int
    L.poa_planes_2piece.argtypes = [vp, C.POINTER(PoaCosts2), vp, C.c_uint32, vp, vp, vp, vp, vp, C.c_int]
    L.poa_batch_run_ex.restype = C.c_int
    L.poa_batch_run_ex.argtypes = [vp, C.POINTER(PoaCosts), C.POINTER(PoaConfig), vp]
    L.poa_batch_create.restype = C.c_int
    L.poa_batch_create.argtypes = [vp, C.c_int, C.c_uint32, vp, vp, C.c_uint64, C.POINTER(vp)]
    L.poa_graph_sweep_slots.restype = C.c_int
    L.poa_graph_sweep_slots.argtypes = [vp, vp, vp]
    if hasattr(L, "poa_graph_sweep_checks"):   # (POA_LIB_PATH may name the build of an older tree: A/B runs)
        L.poa_graph_sweep_checks.restype = C.c_int
        L.poa_graph_sweep_checks.argtypes = [vp, C.c_uint32, vp, vp]
        L.poa_scoreset_run_capped.restype = C.c_int
        L.poa_scoreset_run_capped.argtypes = [vp, C.POINTER(PoaCosts), C.POINTER(PoaConfig), vp, vp]
        L.poa_scoreset_run_2piece_capped.restype = C.c_int
        L.poa_scoreset_run_2piece_capped.argtypes = [vp, C.POINTER(PoaCosts2), C.POINTER(PoaConfig), vp, vp]
        L.poa_scoreset_fetch_swept.restype = C.c_int
        L.poa_scoreset_fetch_swept.argtypes = [vp, vp]
    if hasattr(L, "poa_scoreset_run_best"):   # (as above)
        L.poa_scoreset_run_best.restype = C.c_int
        L.poa_scoreset_run_best.argtypes = [vp, C.POINTER(PoaCosts), C.POINTER(PoaConfig), C.c_uint32, vp, vp]
        L.poa_scoreset_run_2piece_best.restype = C.c_int
        L.poa_scoreset_run_2piece_best.argtypes = [vp, C.POINTER(PoaCosts2), C.POINTER(PoaConfig), C.c_uint32, vp, vp]
        L.poa_scoreset_fetch_best.restype = C.c_int
        L.poa_scoreset_fetch_best.argtypes = [vp, vp]
        L.poa_scoreset_device_best.restype = C.c_int
        L.poa_scoreset_device_best.argtypes = [vp, C.POINTER(vp)]
        L.poa_score_best.restype = C.c_int
        L.poa_score_best.argtypes = [vp, C.c_uint32, C.POINTER(PoaCosts), C.POINTER(PoaConfig), C.c_uint32, vp, vp, C.c_uint64, vp, vp,
                                     C.c_uint32, vp, vp, vp, vp, C.POINTER(PoaStats), C.c_int]
        L.poa_score_best_2piece.restype = C.c_int
        L.poa_score_best_2piece.argtypes = [vp, C.c_uint32, C.POINTER(PoaCosts2), C.POINTER(PoaConfig), C.c_uint32, vp, vp, C.c_uint64, vp, vp,
                                            C.c_uint32, vp, vp, vp, vp, C.POINTER(PoaStats), C.c_int]
    L.poa_graph_checkpoint_plan.restype = C.c_int
    L.poa_graph_checkpoint_plan.argtypes = [vp, C.c_uint32, vp, vp, vp]
    L.poa_graph_checkpoint_plan2.restype = C.c_int
    L.poa_graph_checkpoint_plan2.argtypes = [vp, C.c_uint32, vp, vp, vp]
    L.poa_batch_create_ex.restype = C.c_int
    L.poa_batch_create_ex.argtypes = [vp, C.c_int, C.c_uint32, vp, vp, C.POINTER(PoaConfig), C.c_uint64, C.POINTER(vp)]
    L.poa_batch_workspace_bytes.restype = C.c_int
    L.poa_batch_workspace_bytes.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.poa_batch_run.restype = C.c_int
    L.poa_batch_run.argtypes = [vp, C.POINTER(PoaCosts), vp]
    L.poa_batch_fetch.restype = C.c_int
    L.poa_batch_fetch.argtypes = [vp, vp, vp, vp, C.c_uint64, vp, C.POINTER(PoaStats)]
    L.poa_batch_stats.restype = C.c_int
    L.poa_batch_stats.argtypes = [vp, C.POINTER(PoaStats)]
    L.poa_batch_fetch_search_counters.restype = C.c_int
    L.poa_batch_fetch_search_counters.argtypes = [vp, vp]
    L.poa_batch_last_layout.restype = C.c_int
    L.poa_batch_last_layout.argtypes = [vp, vp]
    if hasattr(L, "poa_batch_band_info"):   # (POA_LIB_PATH may name the build of an older tree: A/B runs)
        L.poa_batch_band_info.restype = C.c_int
        L.poa_batch_band_info.argtypes = [vp, vp]
    if hasattr(L, "poa_batch_band_pair_info"):
        L.poa_batch_band_pair_info.restype = C.c_int
        L.poa_batch_band_pair_info.argtypes = [vp, vp]
    if hasattr(L, "poa_batch_band_narrow_info"):
        L.poa_batch_band_narrow_info.restype = C.c_int
        L.poa_batch_band_narrow_info.argtypes = [vp, vp]
    if hasattr(L, "poa_batch_tb_info"):
        L.poa_batch_tb_info.restype = C.c_int
        L.poa_batch_tb_info.argtypes = [vp, vp]
    if hasattr(L, "poa_batch_last_launch"):
        L.poa_batch_last_launch.restype = C.c_int
        L.poa_batch_last_launch.argtypes = [vp, C.c_uint32, vp]
    if hasattr(L, "poa_batch_replay_info"):   # (POA_LIB_PATH may name the build of an older tree: A/B runs)
        L.poa_batch_replay_info.restype = C.c_int
        L.poa_batch_replay_info.argtypes = [vp, C.c_uint32, vp]
    L.poa_batch_device_results.restype = C.c_int
    L.poa_batch_device_results.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.poa_batch_fetch_planes.restype = C.c_int
    L.poa_batch_fetch_planes.argtypes = [vp, C.c_uint32, vp, vp, vp]
    if hasattr(L, "poa_batch_fetch_compact"):
        L.poa_batch_fetch_compact.restype = C.c_int
        L.poa_batch_fetch_compact.argtypes = [vp, C.c_uint32, vp, vp, vp]
    L.poa_batch_run_2piece.restype = C.c_int
    L.poa_batch_run_2piece.argtypes = [vp, C.POINTER(PoaCosts2), C.POINTER(PoaConfig), vp]
    L.poa_batch_fetch_planes_2piece.restype = C.c_int
    L.poa_batch_fetch_planes_2piece.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp]
    L.poa_batch_destroy.argtypes = [vp]
    L.poa_batch_destroy.restype = None
    # multi-graph batch: graphs is an array of n_graphs handles (c_void_p * n_graphs)
    L.poa_multi_footprint.restype = C.c_int
    L.poa_multi_footprint.argtypes = [vp, C.c_uint32, vp, vp, C.POINTER(PoaConfig), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.poa_multi_create.restype = C.c_int
    L.poa_multi_create.argtypes = [vp, C.c_uint32, vp, C.c_int, vp, vp, C.POINTER(PoaConfig), C.c_uint64, C.POINTER(vp)]
    L.poa_multi_run.restype = C.c_int
    L.poa_multi_run.argtypes = [vp, C.POINTER(PoaCosts), C.POINTER(PoaConfig), vp]
    L.poa_multi_fetch.restype = C.c_int
    L.poa_multi_fetch.argtypes = [vp, vp, vp, vp, C.c_uint64, vp, C.POINTER(PoaStats)]
    L.poa_multi_stats.restype = C.c_int
    L.poa_multi_stats.argtypes = [vp, C.POINTER(PoaStats)]
    L.poa_multi_device_results.restype = C.c_int
    L.poa_multi_device_results.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.poa_multi_workspace_bytes.restype = C.c_int
    L.poa_multi_workspace_bytes.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.poa_multi_destroy.argtypes = [vp]
    L.poa_multi_destroy.restype = None
    L.poa_align_multi.restype = C.c_int
    L.poa_align_multi.argtypes = [vp, C.c_uint32, vp, C.POINTER(PoaCosts), C.POINTER(PoaConfig), vp, vp, vp, vp, vp, C.c_uint64, vp,
                                  C.POINTER(PoaStats), C.c_int]
    # the two-piece model on the same object: the argument lists of the namesakes, poa_costs2_t for the costs
    L.poa_multi_footprint_2piece.restype = C.c_int
    L.poa_multi_footprint_2piece.argtypes = L.poa_multi_footprint.argtypes
    L.poa_multi_create_2piece.restype = C.c_int
    L.poa_multi_create_2piece.argtypes = L.poa_multi_create.argtypes
    L.poa_multi_run_2piece.restype = C.c_int
    L.poa_multi_run_2piece.argtypes = [vp, C.POINTER(PoaCosts2), C.POINTER(PoaConfig), vp]
    L.poa_align_multi_2piece.restype = C.c_int
    L.poa_align_multi_2piece.argtypes = [vp, C.c_uint32, vp, C.POINTER(PoaCosts2), C.POINTER(PoaConfig), vp, vp, vp, vp, vp, C.c_uint64, vp,
                                         C.POINTER(PoaStats), C.c_int]
    if hasattr(L, "poa_multi_create_dense"):   # (POA_LIB_PATH may name the build of an older tree: A/B runs)
        # the dense batch kind on the same object: the argument lists of the namesakes
        L.poa_multi_footprint_dense.restype = C.c_int
        L.poa_multi_footprint_dense.argtypes = L.poa_multi_footprint.argtypes
        L.poa_multi_create_dense.restype = C.c_int
        L.poa_multi_create_dense.argtypes = L.poa_multi_create.argtypes
        L.poa_multi_run_dense.restype = C.c_int
        L.poa_multi_run_dense.argtypes = L.poa_multi_run.argtypes
        L.poa_align_multi_dense.restype = C.c_int
        L.poa_align_multi_dense.argtypes = L.poa_align_multi.argtypes
        L.poa_graph_compact_elems.restype = C.c_int
        L.poa_graph_compact_elems.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint64)]
        L.poa_multi_last_launch.restype = C.c_int
        L.poa_multi_last_launch.argtypes = [vp, C.c_uint32, vp]
    if hasattr(L, "poa_multi_create_exact"):   # (as above)
        # the exact batch kind on the same object: the argument lists of the namesakes
        L.poa_multi_footprint_exact.restype = C.c_int
        L.poa_multi_footprint_exact.argtypes = L.poa_multi_footprint.argtypes
        L.poa_multi_create_exact.restype = C.c_int
        L.poa_multi_create_exact.argtypes = L.poa_multi_create.argtypes
        L.poa_multi_run_exact.restype = C.c_int
        L.poa_multi_run_exact.argtypes = L.poa_multi_run.argtypes
        L.poa_multi_fetch_search_counters.restype = C.c_int
        L.poa_multi_fetch_search_counters.argtypes = [vp, vp]
        if hasattr(L, "poa_multi_replay_info"):
            L.poa_multi_replay_info.restype = C.c_int
            L.poa_multi_replay_info.argtypes = [vp, C.c_uint32, vp]
        L.poa_align_multi_exact.restype = C.c_int
        L.poa_align_multi_exact.argtypes = L.poa_align_multi.argtypes
    if hasattr(L, "poa_multi_create_dense_2piece"):   # (as above)
        # the dense two-piece batch kind on the same object: the argument lists of the _2piece namesakes
        L.poa_multi_footprint_dense_2piece.restype = C.c_int
        L.poa_multi_footprint_dense_2piece.argtypes = L.poa_multi_footprint.argtypes
        L.poa_multi_create_dense_2piece.restype = C.c_int
        L.poa_multi_create_dense_2piece.argtypes = L.poa_multi_create.argtypes
        L.poa_multi_run_dense_2piece.restype = C.c_int
        L.poa_multi_run_dense_2piece.argtypes = L.poa_multi_run_2piece.argtypes
        L.poa_align_multi_dense_2piece.restype = C.c_int
        L.poa_align_multi_dense_2piece.argtypes = L.poa_align_multi_2piece.argtypes
        L.poa_multi_fetch_planes_2piece.restype = C.c_int
        L.poa_multi_fetch_planes_2piece.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp]
    # score set: graphs is an array of n_graphs handles; pair_query / pair_graph are u32 arrays, or both NULL (the full matrix)
    L.poa_scoreset_footprint.restype = C.c_int
    L.poa_scoreset_footprint.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, vp, C.POINTER(PoaConfig), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint64)]
    L.poa_scoreset_create.restype = C.c_int
    L.poa_scoreset_create.argtypes = [vp, C.c_uint32, C.c_int, C.c_uint32, vp, vp, C.c_uint64, vp, vp, C.POINTER(PoaConfig), C.c_uint64,
                                      C.POINTER(vp)]
    L.poa_scoreset_run.restype = C.c_int
    L.poa_scoreset_run.argtypes = [vp, C.POINTER(PoaCosts), C.POINTER(PoaConfig), vp]
    L.poa_scoreset_run_2piece.restype = C.c_int
    L.poa_scoreset_run_2piece.argtypes = [vp, C.POINTER(PoaCosts2), C.POINTER(PoaConfig), vp]
    L.poa_scoreset_fetch.restype = C.c_int
    L.poa_scoreset_fetch.argtypes = [vp, vp, vp, C.POINTER(PoaStats)]
    L.poa_scoreset_stats.restype = C.c_int
    L.poa_scoreset_stats.argtypes = [vp, C.POINTER(PoaStats)]
    L.poa_scoreset_device_results.restype = C.c_int
    L.poa_scoreset_device_results.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.poa_scoreset_workspace_bytes.restype = C.c_int
    L.poa_scoreset_workspace_bytes.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.poa_scoreset_destroy.argtypes = [vp]
    L.poa_scoreset_destroy.restype = None
    L.poa_score_pairs.restype = C.c_int
    L.poa_score_pairs.argtypes = [vp, C.c_uint32, C.POINTER(PoaCosts), C.POINTER(PoaConfig), C.c_uint32, vp, vp, C.c_uint64, vp, vp, vp, vp,
                                  C.POINTER(PoaStats), C.c_int]
    L.poa_score_pairs_2piece.restype = C.c_int
    L.poa_score_pairs_2piece.argtypes = [vp, C.c_uint32, C.POINTER(PoaCosts2), C.POINTER(PoaConfig), C.c_uint32, vp, vp, C.c_uint64, vp, vp,
                                         vp, vp, C.POINTER(PoaStats), C.c_int]
    _lib = L
    return L


def check(rc):
    if rc != POA_OK:
        raise PoaError(rc, lib().poa_last_error().decode(errors="replace"))
