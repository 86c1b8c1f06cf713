"""ctypes mirror of the plain-C structs of include/kueue_tas.h (ABI version 5).

For bindings that call the device layer directly (kueue_tas_snapshot_load,
kueue_tas_eval_batch) instead of going through the JSON host layer; the
field order and widths follow the header line by line, and
tests/test_raw_abi.py pins them against the library."""
import ctypes as c

MAX_LEVELS = 16
MAX_COLS = 32
MAX_SELECTORS = 8
MAX_LAYERS = 4

F_REQUIRED = 1
F_UNCONSTRAINED = 2
F_LFC = 4
F_SIMULATE_EMPTY = 8
F_LEADER = 16
F_MULTILAYER = 32
F_AFFINITY = 64
F_DOMAIN = 128
F_SELECTOR_EXT = 256

ST_OK = 0
ST_NO_DOMAINS = 1
ST_NOT_FIT = 2
ST_MULTILAYER = 3
ST_INTERNAL = 4


class SnapshotDesc(c.Structure):  # kueue_tas_snapshot_desc
    _fields_ = [
        ("num_levels", c.c_int32),
        ("level_sizes", c.POINTER(c.c_int32)),
        ("child_offsets", c.POINTER(c.c_int32)),
        ("num_cols", c.c_int32),
        ("free_capacity", c.POINTER(c.c_int64)),
        ("tas_usage", c.POINTER(c.c_int64)),
        ("free_present", c.POINTER(c.c_uint32)),
        ("usage_present", c.POINTER(c.c_uint32)),
        ("lowest_is_hostname", c.c_int32),
        ("taint_profile", c.POINTER(c.c_int32)),
        ("num_label_cols", c.c_int32),
        ("label_values", c.POINTER(c.c_int32)),
        ("domain_id_rank", c.POINTER(c.c_int32)),
    ]


class Delta(c.Structure):  # kueue_tas_delta
    _fields_ = [("leaf", c.c_int32), ("col", c.c_int32), ("delta", c.c_int64)]


class EvalReq(c.Structure):  # kueue_tas_eval_req
    _fields_ = [
        ("flags", c.c_uint32),
        ("count", c.c_int32),
        ("slice_size", c.c_int32),
        ("requested_level", c.c_int32),
        ("slice_level", c.c_int32),
        ("num_req", c.c_int32),
        ("num_leader_req", c.c_int32),
        ("num_selectors", c.c_int32),
        ("req_col", c.c_int32 * MAX_COLS),
        ("req_val", c.c_int64 * MAX_COLS),
        ("leader_col", c.c_int32 * MAX_COLS),
        ("leader_val", c.c_int64 * MAX_COLS),
        ("slice_size_at_level", c.c_int32 * MAX_LEVELS),
        ("sel_col", c.c_int32 * MAX_SELECTORS),
        ("sel_val", c.c_int32 * MAX_SELECTORS),
        ("num_layers", c.c_int32),
        ("layer_level", c.c_int32 * MAX_LAYERS),
        ("layer_size", c.c_int32 * MAX_LAYERS),
        ("taint_table", c.c_int32),
        ("assumed_begin", c.c_int32),
        ("assumed_end", c.c_int32),
        ("affinity_begin", c.c_int32),
        ("affinity_end", c.c_int32),
        ("domain_begin", c.c_int32),
        ("domain_end", c.c_int32),
        ("selector_begin", c.c_int32),
        ("selector_end", c.c_int32),
    ]


class AffinityReq(c.Structure):  # kueue_tas_affinity_req
    _fields_ = [("term", c.c_int32), ("col", c.c_int32), ("negate", c.c_int32), ("begin", c.c_int32),
                ("len", c.c_int32)]


class Assumed(c.Structure):  # kueue_tas_assumed
    _fields_ = [("leaf", c.c_int32), ("col", c.c_int32), ("value", c.c_int64)]


class EvalOut(c.Structure):  # kueue_tas_eval_out
    _fields_ = [
        ("status", c.c_int32),
        ("a", c.c_int32),
        ("b", c.c_int32),
        ("fit_level", c.c_int32),
        ("num_workers", c.c_int32),
        ("num_leaders", c.c_int32),
        ("assignment_nil", c.c_int32),
        ("total_nodes", c.c_int32),
        ("excl_selector", c.c_int32),
        ("excl_affinity", c.c_int32),
        ("excl_topology", c.c_int32),
        ("ml_fit", c.c_int32 * MAX_LAYERS),
        ("ml_need", c.c_int32 * MAX_LAYERS),
        ("reserved", c.c_int32 * 2),
    ]


class SpliceDesc(c.Structure):  # kueue_tas_splice_desc
    _fields_ = [
        ("topo", c.POINTER(SnapshotDesc)),
        ("leaf_src", c.POINTER(c.c_int32)),
        ("num_new", c.c_int32),
        ("new_free_capacity", c.POINTER(c.c_int64)),
        ("new_tas_usage", c.POINTER(c.c_int64)),
        ("new_free_present", c.POINTER(c.c_uint32)),
        ("new_usage_present", c.POINTER(c.c_uint32)),
        ("new_taint_profile", c.POINTER(c.c_int32)),
        ("new_label_values", c.POINTER(c.c_int32)),
        ("new_leaf_tags", c.POINTER(c.c_uint64)),
    ]


class FitsReq(c.Structure):  # kueue_tas_fits_req
    _fields_ = [("leaf", c.c_int32), ("count", c.c_int32), ("term_begin", c.c_int32), ("num_terms", c.c_int32)]


class FitsTerm(c.Structure):  # kueue_tas_fits_term
    _fields_ = [("value", c.c_int64), ("col", c.c_int32), ("pad", c.c_int32)]


class Config(c.Structure):  # kueue_tas_config
    _fields_ = [("list_cap", c.c_int32), ("max_batch", c.c_int32), ("device", c.c_int32), ("flags", c.c_int32)]


def bind_device_layer(lib):
    """argtypes of the device-layer entry points the raw bindings call."""
    P = c.POINTER
    lib.kueue_tas_ctx_create.argtypes = [P(Config)]
    lib.kueue_tas_ctx_create.restype = c.c_void_p
    lib.kueue_tas_ctx_destroy.argtypes = [c.c_void_p]
    lib.kueue_tas_ctx_destroy.restype = None
    lib.kueue_tas_last_error.argtypes = [c.c_void_p]
    lib.kueue_tas_last_error.restype = c.c_char_p
    lib.kueue_tas_snapshot_load.argtypes = [c.c_void_p, P(SnapshotDesc)]
    lib.kueue_tas_snapshot_load.restype = c.c_int
    lib.kueue_tas_snapshot_apply_deltas.argtypes = [c.c_void_p, P(Delta), c.c_size_t, c.c_void_p]
    lib.kueue_tas_snapshot_apply_deltas.restype = c.c_int
    lib.kueue_tas_eval_batch.argtypes = [c.c_void_p, P(EvalReq), c.c_size_t, c.c_void_p, c.c_size_t, c.c_int32,
                                         c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t,
                                         P(EvalOut), P(c.c_int64), c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p]
    lib.kueue_tas_eval_batch.restype = c.c_int
    lib.kueue_tas_fetch_entries.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t]
    lib.kueue_tas_fetch_entries.restype = c.c_int
    lib.kueue_tas_fits.argtypes = [c.c_void_p, P(FitsReq), c.c_size_t, P(FitsTerm), c.c_size_t, P(c.c_int32)]
    lib.kueue_tas_fits.restype = c.c_int
    lib.kueue_tas_admit.argtypes = [c.c_void_p, P(FitsReq), c.c_size_t, P(FitsTerm), c.c_size_t, P(c.c_int64),
                                    c.c_size_t, c.c_int32, P(c.c_int32)]
    lib.kueue_tas_admit.restype = c.c_int
    lib.kueue_tas_admit_targets.argtypes = [c.c_void_p, P(FitsReq), c.c_size_t, P(FitsTerm), c.c_size_t, P(c.c_int64),
                                            c.c_size_t, c.c_int32, P(Delta), P(c.c_int64), c.c_size_t, P(c.c_int32),
                                            P(c.c_int64), P(c.c_int32)]
    lib.kueue_tas_admit_targets.restype = c.c_int
    lib.kueue_tas_admit_table.argtypes = [c.c_void_p, P(c.c_int32), c.c_int32, P(c.c_int32), P(FitsTerm), c.c_size_t]
    lib.kueue_tas_admit_table.restype = c.c_int
    lib.kueue_tas_admit_block.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, P(c.c_int64), c.c_int32, c.c_int32,
                                          P(c.c_int32), P(c.c_int32), c.c_size_t, P(c.c_size_t), P(P(Delta)),
                                          P(c.c_size_t)]
    lib.kueue_tas_admit_block.restype = c.c_int
    lib.kueue_tas_admit_block_targets.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, P(c.c_int64), c.c_int32, c.c_int32,
                                                  P(Delta), P(c.c_int64), c.c_size_t, P(c.c_int32), P(c.c_int64),
                                                  P(c.c_int32), c.c_size_t, P(c.c_int32), P(c.c_int32), c.c_size_t,
                                                  P(c.c_size_t), P(P(Delta)), P(c.c_size_t)]
    lib.kueue_tas_admit_block_targets.restype = c.c_int
    lib.kueue_tas_snapshot_set_free.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p]
    lib.kueue_tas_snapshot_set_free.restype = c.c_int
    lib.kueue_tas_snapshot_set_leaf_attrs.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p]
    lib.kueue_tas_snapshot_set_leaf_attrs.restype = c.c_int
    lib.kueue_tas_snapshot_set_leaf_live.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    lib.kueue_tas_snapshot_set_leaf_live.restype = c.c_int
    lib.kueue_tas_snapshot_set_leaf_tags.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t]
    lib.kueue_tas_snapshot_set_leaf_tags.restype = c.c_int
    lib.kueue_tas_snapshot_splice.argtypes = [c.c_void_p, P(SpliceDesc)]
    lib.kueue_tas_snapshot_splice.restype = c.c_int
    lib.kueue_tas_snapshot_digest.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, P(c.c_size_t), c.c_void_p, c.c_size_t,
                                              P(c.c_size_t)]
    lib.kueue_tas_snapshot_digest.restype = c.c_int
    lib.kueue_tas_snapshot_read_leaves.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t] + [c.c_void_p] * 8
    lib.kueue_tas_snapshot_read_leaves.restype = c.c_int
    lib.kueue_tas_last_digest_ms.argtypes = [c.c_void_p, P(c.c_float)]
    lib.kueue_tas_last_digest_ms.restype = c.c_int
    lib.kueue_tas_removal_tables_build.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p,
                                                   c.c_void_p, c.c_size_t]
    lib.kueue_tas_removal_tables_build.restype = c.c_int
    lib.kueue_tas_removal_tables_build_flags.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p,
                                                         c.c_void_p, c.c_size_t, c.c_uint32]
    lib.kueue_tas_removal_tables_build_flags.restype = c.c_int
    lib.kueue_tas_removal_tables_clear.argtypes = [c.c_void_p]
    lib.kueue_tas_removal_tables_clear.restype = c.c_int
    # (reqs: an array of pointers to the requests, as kueue_tas_eval_batch_ptrs takes them)
    lib.kueue_tas_eval_batch_removals.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_int32,
                                                  c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p,
                                                  c.c_size_t, P(EvalOut), P(c.c_int64), c.c_void_p, c.c_size_t,
                                                  c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    lib.kueue_tas_eval_batch_removals.restype = c.c_int
    lib.kueue_tas_removal_stats.argtypes = [c.c_void_p, P(c.c_int64)]
    lib.kueue_tas_removal_stats.restype = c.c_int
    lib.kueue_tas_removal_large_stats.argtypes = [c.c_void_p, P(c.c_int64)]
    lib.kueue_tas_removal_large_stats.restype = c.c_int
    return lib


REMOVAL_MAX_CANDIDATES = 64  # KUEUE_TAS_REMOVAL_MAX_CANDIDATES
REMOVAL_SET_CAP = 4096       # KUEUE_TAS_REMOVAL_SET_CAP: records one removal_table_kernel workgroup sorts
REMOVAL_EXPAND_TILE = 256    # table records removal_expand_kernel compacts per step (tas_internal.h)
REMOVAL_LARGE_SET_CAP = 1 << 20  # KUEUE_TAS_REMOVAL_LARGE_SET_CAP: records of a set built with RT_LARGE_SETS
REMOVAL_EXPAND_SEGMENT = 4096    # table records per removal_expand_seg_kernel workgroup (tas_internal.h)
RT_LARGE_SETS = 1                # KUEUE_TAS_RT_LARGE_SETS


def removal_tables_build(lib, ctx, targets, sets, flags=0):
    """kueue_tas_removal_tables_build from Python lists: ``targets[t]`` the
    (leaf, col, delta) records of target t, ``sets[s]`` the target indices of
    set s.  With ``flags`` (RT_LARGE_SETS) through
    kueue_tas_removal_tables_build_flags.  Returns the call's code."""
    import numpy as np
    recs = np.array([r for t in targets for r in t], dtype=[("leaf", "<i4"), ("col", "<i4"), ("delta", "<i8")])
    toff = np.cumsum([0] + [len(t) for t in targets], dtype=np.int64)
    cand = np.array([x for s in sets for x in s], dtype=np.int32)
    coff = np.cumsum([0] + [len(s) for s in sets], dtype=np.int64)
    if flags:
        return lib.kueue_tas_removal_tables_build_flags(ctx, recs.ctypes.data if recs.size else None, toff.ctypes.data,
                                                        len(targets), cand.ctypes.data if cand.size else None,
                                                        coff.ctypes.data, len(sets), flags)
    return lib.kueue_tas_removal_tables_build(ctx, recs.ctypes.data if recs.size else None, toff.ctypes.data,
                                              len(targets), cand.ctypes.data if cand.size else None, coff.ctypes.data,
                                              len(sets))


DIGEST_CHUNK = 2048  # KUEUE_TAS_DIGEST_CHUNK
DIGEST_FIXED = ("topology", "live", "taints", "tags")  # then free[R], usage[R], label[K]


def snapshot_digest(lib, ctx):
    """kueue_tas_snapshot_digest of a raw context: (words, chunk words) as numpy uint64."""
    import numpy as np
    n, nc = c.c_size_t(), c.c_size_t()
    rc = lib.kueue_tas_snapshot_digest(ctx, None, 0, c.byref(n), None, 0, c.byref(nc))
    if rc not in (0, -5):
        raise RuntimeError(f"kueue_tas_snapshot_digest failed ({rc}): {lib.kueue_tas_last_error(ctx).decode()}")
    words = np.zeros(n.value, dtype=np.uint64)
    chunks = np.zeros(max(nc.value, 1), dtype=np.uint64)
    rc = lib.kueue_tas_snapshot_digest(ctx, words.ctypes.data, words.size, c.byref(n), chunks.ctypes.data, chunks.size,
                                       c.byref(nc))
    if rc:
        raise RuntimeError(f"kueue_tas_snapshot_digest failed ({rc}): {lib.kueue_tas_last_error(ctx).decode()}")
    return words, chunks[: nc.value]


def read_leaves(lib, ctx, leaves, n, R, K):
    """kueue_tas_snapshot_read_leaves of a raw context (``leaves`` None: leaves
    0 .. n-1): dict of numpy arrays free [n, R], free_present, usage [n, R],
    usage_present, profiles, labels [n, K], live, tags."""
    import numpy as np
    ids = None if leaves is None else np.ascontiguousarray(leaves, dtype=np.int32)
    out = dict(free=np.zeros((n, R), np.int64), free_present=np.zeros(n, np.uint32), usage=np.zeros((n, R), np.int64),
               usage_present=np.zeros(n, np.uint32), profiles=np.zeros(n, np.int32), labels=np.zeros((n, K), np.int32),
               live=np.zeros(n, np.int32), tags=np.zeros(n, np.uint64))
    rc = lib.kueue_tas_snapshot_read_leaves(ctx, None if ids is None else ids.ctypes.data, n,
                                            *[a.ctypes.data for a in out.values()])
    if rc:
        raise RuntimeError(f"kueue_tas_snapshot_read_leaves failed ({rc}): {lib.kueue_tas_last_error(ctx).decode()}")
    return out
