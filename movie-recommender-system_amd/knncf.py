"""ctypes binding of libknncf.so (include/knncf.h).

This is the only door into the engine: there is no Python/NumPy/torch compute path behind it.
If the shared library is missing or no gfx950 device is usable the calls raise — they never fall
back to a CPU implementation.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libknncf.so")

OK = 0
E_INVALID, E_NONFINITE, E_DUPLICATE, E_NOMEM, E_HIP, E_STATE, E_UNSUPPORTED, E_NODEVICE, E_RCCL = range(-1, -10, -1)
SIM_COSINE, SIM_ONE, SIM_JACCARD = 0, 1, 2
PRED_GLOBAL_AVG, PRED_USER_AVG, PRED_ITEM_AVG, PRED_BASELINE, PRED_BASELINE_RDD, PRED_KNN, PRED_PERSONALIZED = range(7)
FLAG_VERIFY_BOUND = 1
FLAG_OVERLAP = 2
FLAG_BF16_FILTER = 4  # default filter operand type is fp16 (narrower error band, same MFMA rate)
FLAG_F32_PANEL = 8    # default similarity panel storage is fp16
HEAD_ALL = 0xFFFFFFFF
EXPLAIN_SUM_ORDER, EXPLAIN_BY_WEIGHT = 0, 1  # KNNCF_EXPLAIN_*: the order of the terms of Engine.explain*
APPEND_MAX_CHANGERS = 128  # KNNCF_APPEND_MAX_CHANGERS: Appends.append with more distinct users carries no list (a plain refit)
AMEND_TILE = 2048  # KNNCF_AMEND_TILE: the train rows that one workgroup of knncf_amend's removal stage takes

_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_f64p = C.POINTER(C.c_double)


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("k", C.c_int32),
                ("similarity", C.c_int32), ("shard_rank", C.c_int32), ("shard_count", C.c_int32),
                ("workspace_bytes", C.c_int64), ("flags", C.c_uint32), ("head_items", C.c_uint32)]


class Ratings(C.Structure):
    """knncf_ratings of include/knncf.h"""
    _fields_ = [("n", C.c_int64), ("users", C.POINTER(C.c_int32)), ("items", C.POINTER(C.c_int32)),
                ("ratings", C.POINTER(C.c_double))]


def load_file(path, separator="\t", threads=0, cache=None, info=None):
    """`load` shared/predictions.scala:35-49 through the library's multithreaded parser: (users, items, ratings) in
    file order.  No GPU needed.  cache: path of the binary cache (knncf_load_file_cached): read when it matches the
    file as it is now, (re)written otherwise; info (a dict) then receives {"from_cache": bool}."""
    L = load_library()
    r = Ratings()
    err = C.create_string_buffer(512)
    if cache is None:
        st = L.knncf_load_file(os.fsencode(path), separator.encode(), threads, C.byref(r), err, len(err))
    else:
        hit = C.c_int(0)
        st = L.knncf_load_file_cached(os.fsencode(path), separator.encode(), threads, os.fsencode(cache), C.byref(r),
                                      C.byref(hit), err, len(err))
        if info is not None:
            info["from_cache"] = bool(hit.value)
    if st != 0:
        raise KnncfError(st, err.value.decode(errors="replace"))
    try:
        n = r.n
        u = np.ctypeslib.as_array(r.users, shape=(max(n, 1),))[:n].copy()
        i = np.ctypeslib.as_array(r.items, shape=(max(n, 1),))[:n].copy()
        x = np.ctypeslib.as_array(r.ratings, shape=(max(n, 1),))[:n].copy()
    finally:
        L.knncf_free_ratings(C.byref(r))
    return u, i, x


class Personal(C.Structure):
    """knncf_personal of include/knncf.h"""
    _fields_ = [("n_rows", C.c_int64), ("row_ids", C.POINTER(C.c_int32)), ("row_names", C.POINTER(C.c_char_p)),
                ("name_storage", C.c_void_p), ("ratings", Ratings)]


def load_personal(path, user=944):
    """recommend/Recommender.scala:40-54 through knncf_load_personal: (names, (users, items, ratings)) — `names` is the
    list of (id, title) of every row in file order, the header as (0, "header"); the ratings are the non-zero ones."""
    L = load_library()
    p = Personal()
    err = C.create_string_buffer(512)
    st = L.knncf_load_personal(os.fsencode(path), user, C.byref(p), err, len(err))
    if st != 0:
        raise KnncfError(st, err.value.decode(errors="replace"))
    try:
        names = [(int(p.row_ids[j]), p.row_names[j].decode("utf-8", errors="replace")) for j in range(p.n_rows)]
        n = p.ratings.n
        u = np.ctypeslib.as_array(p.ratings.users, shape=(max(n, 1),))[:n].copy()
        i = np.ctypeslib.as_array(p.ratings.items, shape=(max(n, 1),))[:n].copy()
        x = np.ctypeslib.as_array(p.ratings.ratings, shape=(max(n, 1),))[:n].copy()
    finally:
        L.knncf_free_personal(C.byref(p))
    return names, (u, i, x)


class Timings(C.Structure):
    _fields_ = [("prep_ms", C.c_double), ("densify_ms", C.c_double), ("gemm_ms", C.c_double),
                ("tail_ms", C.c_double), ("select_ms", C.c_double), ("rerank_ms", C.c_double), ("predict_ms", C.c_double),
                ("gemm_launches", C.c_int64), ("gemm_flops_executed", C.c_double),
                ("gemm_flops_algorithmic", C.c_double), ("shortlist_total", C.c_int64),
                ("fallback_rows", C.c_int64), ("max_bound_violation", C.c_double),
                ("head_items", C.c_int64), ("tail_pair_updates", C.c_double),
                ("rerank_row_bytes", C.c_double), ("select_row_bytes", C.c_double), ("select_launches", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ShardView(C.Structure):
    _fields_ = [("user_begin", C.c_int32), ("user_end", C.c_int32), ("nnz_begin", C.c_int64),
                ("nnz_end", C.c_int64), ("num_users", C.c_int32), ("num_ratings", C.c_int64),
                ("d_user_avg", C.c_void_p), ("d_user_norm", C.c_void_p), ("d_dev", C.c_void_p),
                ("d_pre", C.c_void_p)]


EXPORTS = [
    "knncf_version", "knncf_status_string", "knncf_create", "knncf_destroy", "knncf_last_error",
    "knncf_fit", "knncf_fit_device", "knncf_num_users", "knncf_num_items", "knncf_global_avg",
    "knncf_user_avg", "knncf_item_avg", "knncf_item_avg_dev", "knncf_item_avg_dev_rdd", "knncf_similarity",
    "knncf_knn_similarity", "knncf_similarity_batch", "knncf_similarity_batch_device", "knncf_knn_similarity_batch", "knncf_neighbors", "knncf_neighbors_batch", "knncf_predict", "knncf_recommend", "knncf_recommend_batch",
    "knncf_explain", "knncf_explain_batch", "knncf_explain_batch_device",
    "knncf_explain_personalized", "knncf_explain_personalized_batch",
    "knncf_query_neighbors", "knncf_query_predict", "knncf_query_recommend",
    "knncf_query_neighbors_batch", "knncf_query_predict_batch", "knncf_query_recommend_batch",
    "knncf_update_neighbors", "knncf_update_predict", "knncf_update_recommend",
    "knncf_update_neighbors_batch", "knncf_update_predict_batch", "knncf_update_recommend_batch",
    "knncf_revise_neighbors", "knncf_revise_predict", "knncf_revise_recommend",
    "knncf_revise_neighbors_batch", "knncf_revise_predict_batch", "knncf_revise_recommend_batch",
    "knncf_query_explain", "knncf_update_explain", "knncf_revise_explain",
    "knncf_query_explain_batch", "knncf_update_explain_batch", "knncf_revise_explain_batch",
    "knncf_query_explain_personalized", "knncf_update_explain_personalized", "knncf_revise_explain_personalized",
    "knncf_query_explain_personalized_batch", "knncf_update_explain_personalized_batch", "knncf_revise_explain_personalized_batch",
    "knncf_query_recommend_explain", "knncf_update_recommend_explain", "knncf_revise_recommend_explain",
    "knncf_query_recommend_explain_batch", "knncf_update_recommend_explain_batch", "knncf_revise_recommend_explain_batch",
    "knncf_query_bystander_neighbors", "knncf_query_bystander_predict",
    "knncf_query_bystander_neighbors_batch", "knncf_query_bystander_predict_batch",
    "knncf_update_bystander_neighbors", "knncf_update_bystander_predict",
    "knncf_update_bystander_neighbors_batch", "knncf_update_bystander_predict_batch",
    "knncf_revise_bystander_neighbors", "knncf_revise_bystander_predict",
    "knncf_revise_bystander_neighbors_batch", "knncf_revise_bystander_predict_batch",
    "knncf_query_entered", "knncf_query_entered_batch",
    "knncf_update_entered", "knncf_update_entered_batch", "knncf_revise_entered", "knncf_revise_entered_batch",
    "knncf_append", "knncf_amend", "knncf_remove_users",
    "knncf_predict_batch",
    "knncf_predict_batch_device", "knncf_mae", "knncf_mae_device", "knncf_mae_sweep", "knncf_mae_sweep_device", "knncf_shard_view_get",
    "knncf_shard_commit", "knncf_get_timings", "knncf_reset_timings", "knncf_reset_neighbors",
    "knncf_set_k", "knncf_load_file", "knncf_load_file_cached", "knncf_free_ratings", "knncf_load_personal", "knncf_free_personal", "knncf_neighbors_save", "knncf_neighbors_load",
    "knncf_group_create", "knncf_group_destroy", "knncf_group_last_error", "knncf_group_size", "knncf_group_handle",
    "knncf_group_fit", "knncf_group_mae", "knncf_group_predict_batch",
]


class KnncfError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"knncf status {status}: {message}")
        self.status = status


_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64; if libknncf.so
    pulled in /opt/rocm's copy first, torch could no longer see the GPU later in the same process.
    Pre-load torch's copy (without importing torch) so both bind to the same runtime."""
    import importlib.util

    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return
    lib_dir = os.path.join(os.path.dirname(spec.origin), "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(lib_dir, name)
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                pass


def _share_rccl_with_torch():
    """knncf_group_* resolves RCCL at run time and reuses a copy that is already in the process.  Under Python that must
    be the one PyTorch bundles (built against the HIP runtime _share_hip_runtime_with_torch bound the library to): load it
    — importing torch does — before the first group is created, so that /opt/rocm's copy is not pulled in beside it."""
    import importlib.util

    if importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401  (libtorch_hip links librccl)


def load_library():
    """Load libknncf.so (built in-tree by build.py).  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} not found: build the HIP extension first (python __graft_entry__.py or "
            f"movie-recommender-system_amd/build.py); there is no CPU fallback")
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH)
    L.knncf_version.restype = C.c_char_p
    L.knncf_status_string.restype = C.c_char_p
    L.knncf_status_string.argtypes = [C.c_int]
    L.knncf_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
    L.knncf_destroy.argtypes = [C.c_void_p]
    L.knncf_destroy.restype = None
    L.knncf_last_error.argtypes = [C.c_void_p]
    L.knncf_last_error.restype = C.c_char_p
    L.knncf_fit.argtypes = [C.c_void_p, _i32p, _i32p, _f64p, C.c_int64]
    L.knncf_fit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    L.knncf_num_users.argtypes = [C.c_void_p, _i32p]
    L.knncf_num_items.argtypes = [C.c_void_p, _i32p]
    L.knncf_global_avg.argtypes = [C.c_void_p, _f64p]
    for n in ("knncf_user_avg", "knncf_item_avg", "knncf_item_avg_dev", "knncf_item_avg_dev_rdd"):
        getattr(L, n).argtypes = [C.c_void_p, C.c_int32, _f64p]
    for n in ("knncf_similarity", "knncf_knn_similarity"):
        getattr(L, n).argtypes = [C.c_void_p, C.c_int32, C.c_int32, _f64p]
    for n in ("knncf_similarity_batch", "knncf_knn_similarity_batch"):
        getattr(L, n).argtypes = [C.c_void_p, _i32p, _i32p, C.c_int64, _f64p]
    L.knncf_similarity_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.knncf_neighbors.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _i32p, _f64p, _i32p]
    L.knncf_neighbors_batch.argtypes = [C.c_void_p, _i32p, C.c_int64, C.c_int32, _i32p, _f64p, _i32p]
    L.knncf_predict.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, _f64p]
    L.knncf_recommend.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, _i32p, _f64p, C.POINTER(C.c_int32)]
    L.knncf_recommend_batch.argtypes = [C.c_void_p, C.c_int, _i32p, C.c_int64, C.c_int32, _i32p, _f64p, _i32p]
    L.knncf_explain.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i32p, _f64p, _f64p, _i32p, _f64p, _f64p]
    L.knncf_explain_batch.argtypes = [C.c_void_p, _i32p, _i32p, C.c_int64, C.c_int32, C.c_int32, _i32p, _f64p, _f64p, _i32p, _f64p,
                                      _f64p]
    L.knncf_explain_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 6
    L.knncf_explain_personalized.argtypes = L.knncf_explain.argtypes
    L.knncf_explain_personalized_batch.argtypes = L.knncf_explain_batch.argtypes
    for fam in ("query", "update"):  # fold-in queries and update queries share their argument lists
        f = lambda name: getattr(L, f"knncf_{fam}_{name}")
        f("neighbors").argtypes = [C.c_void_p, C.c_int32, _i32p, _f64p, C.c_int64, C.c_int32, _i32p, _f64p, _i32p]
        f("predict").argtypes = [C.c_void_p, C.c_int, C.c_int32, _i32p, _f64p, C.c_int64, _i32p, C.c_int64, _f64p]
        f("recommend").argtypes = [C.c_void_p, C.c_int, C.c_int32, _i32p, _f64p, C.c_int64, C.c_int32, _i32p, _f64p, _i32p]
        f("neighbors_batch").argtypes = [C.c_void_p, _i32p, _i64p, _i32p, _f64p, C.c_int64, C.c_int32, _i32p, _f64p, _i32p, _i32p]
        f("predict_batch").argtypes = [C.c_void_p, C.c_int, _i32p, _i64p, _i32p, _f64p, C.c_int64, _i64p, _i32p, _f64p, _i32p]
        f("recommend_batch").argtypes = [C.c_void_p, C.c_int, _i32p, _i64p, _i32p, _f64p, C.c_int64, C.c_int32, _i32p, _f64p,
                                         _i32p, _i32p]
        # the predict argument lists up to the requested items, then order, cap and the explain_batch outputs
        terms = [C.c_int32, C.c_int32, _i32p, _f64p, _f64p, _i32p, _f64p, _f64p]
        f("explain").argtypes = f("predict").argtypes[:-1] + terms
        f("explain_batch").argtypes = f("predict_batch").argtypes[:-2] + terms + [_i32p]
        # the Personalized explanations: the explain lists without the predictor
        f("explain_personalized").argtypes = f("explain").argtypes[:1] + f("explain").argtypes[2:]
        f("explain_personalized_batch").argtypes = f("explain_batch").argtypes[:1] + f("explain_batch").argtypes[2:]
        # the fused calls: the recommend lists up to n, order and cap, the recommend outputs, the explain outputs without predictions
        f("recommend_explain").argtypes = (f("recommend").argtypes[:-3] + [C.c_int32, C.c_int32] + f("recommend").argtypes[-3:]
                                           + terms[2:-1])
        f("recommend_explain_batch").argtypes = (f("recommend_batch").argtypes[:-4] + [C.c_int32, C.c_int32]
                                                 + f("recommend_batch").argtypes[-4:-1] + terms[2:-1] + [_i32p])
    # bystander queries: the fold-in or update query, then its rows (a fitted user each; the predict forms: with an item)
    for fam in ("query", "update"):
        getattr(L, f"knncf_{fam}_bystander_neighbors").argtypes = [C.c_void_p, C.c_int32, _i32p, _f64p, C.c_int64, _i32p, C.c_int64,
                                                                  C.c_int32, _i32p, _f64p, _i32p]
        getattr(L, f"knncf_{fam}_bystander_predict").argtypes = [C.c_void_p, C.c_int, C.c_int32, _i32p, _f64p, C.c_int64, _i32p, _i32p,
                                                                C.c_int64, _f64p]
        getattr(L, f"knncf_{fam}_bystander_neighbors_batch").argtypes = [C.c_void_p, _i32p, _i64p, _i32p, _f64p, C.c_int64, _i64p, _i32p,
                                                                        C.c_int32, _i32p, _f64p, _i32p, _i32p]
        getattr(L, f"knncf_{fam}_bystander_predict_batch").argtypes = [C.c_void_p, C.c_int, _i32p, _i64p, _i32p, _f64p, C.c_int64, _i64p,
                                                                      _i32p, _i32p, _f64p, _i32p]
    # bystanders of revise queries: the removals in front of the additional rows, as knncf_revise_* take them
    rm_single, rm_batch = [_i32p, C.c_int64], [_i64p, _i32p]
    for name, head in (("neighbors", 2), ("predict", 3)):
        single, batch = getattr(L, f"knncf_update_bystander_{name}").argtypes, getattr(L, f"knncf_update_bystander_{name}_batch").argtypes
        getattr(L, f"knncf_revise_bystander_{name}").argtypes = single[:head] + rm_single + single[head:]
        getattr(L, f"knncf_revise_bystander_{name}_batch").argtypes = batch[:head] + rm_batch + batch[head:]
    # entered queries: the fold-in query, cap, then users / sims / positions / displaced and the count(s)
    L.knncf_query_entered.argtypes = [C.c_void_p, C.c_int32, _i32p, _f64p, C.c_int64, C.c_int32, _i32p, _f64p, _i32p, _i32p, _i32p]
    # the same for update queries: users / sims / positions / previous / other and the count(s)
    L.knncf_update_entered.argtypes = [C.c_void_p, C.c_int32, _i32p, _f64p, C.c_int64, C.c_int32, _i32p, _f64p, _i32p, _i32p, _i32p,
                                       _i32p]
    L.knncf_update_entered_batch.argtypes = [C.c_void_p, _i32p, _i64p, _i32p, _f64p, C.c_int64, C.c_int32, _i32p, _f64p, _i32p, _i32p,
                                             _i32p, _i32p, _i32p]
    L.knncf_query_entered_batch.argtypes = [C.c_void_p, _i32p, _i64p, _i32p, _f64p, C.c_int64, C.c_int32, _i32p, _f64p, _i32p, _i32p,
                                            _i32p, _i32p]
    # the same for revise queries: the removals in front of the additional rows
    L.knncf_revise_entered.argtypes = L.knncf_update_entered.argtypes[:2] + rm_single + L.knncf_update_entered.argtypes[2:]
    L.knncf_revise_entered_batch.argtypes = (L.knncf_update_entered_batch.argtypes[:2] + rm_batch +
                                             L.knncf_update_entered_batch.argtypes[2:])
    # append: the rows, then |K|, |B ∩ S| and the dropped raw ids with their cap
    L.knncf_append.argtypes = [C.c_void_p, _i32p, _i32p, _f64p, C.c_int64, _i64p, _i64p, _i32p, C.c_int64]
    # amend: the removals (users, items, their number) in front of knncf_append's arguments
    L.knncf_amend.argtypes = [C.c_void_p, _i32p, _i32p, C.c_int64] + L.knncf_append.argtypes[1:]
    # remove users: the ids and their number, then knncf_append's outputs
    L.knncf_remove_users.argtypes = [C.c_void_p, _i32p, C.c_int64] + L.knncf_append.argtypes[5:]
    # revise queries: the update argument lists with the removals in front of the additional rows
    for name, at, single in (("neighbors", 2, True), ("predict", 3, True), ("recommend", 3, True), ("explain", 3, True),
                             ("explain_personalized", 2, True), ("neighbors_batch", 2, False), ("predict_batch", 3, False),
                             ("recommend_batch", 3, False), ("explain_batch", 3, False), ("explain_personalized_batch", 2, False),
                             ("recommend_explain", 3, True), ("recommend_explain_batch", 3, False)):
        base = getattr(L, f"knncf_update_{name}").argtypes
        getattr(L, f"knncf_revise_{name}").argtypes = base[:at] + ([_i32p, C.c_int64] if single else [_i64p, _i32p]) + base[at:]
    L.knncf_predict_batch.argtypes = [C.c_void_p, C.c_int, _i32p, _i32p, C.c_int64, _f64p]
    L.knncf_predict_batch_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.knncf_mae.argtypes = [C.c_void_p, C.c_int, _i32p, _i32p, _f64p, C.c_int64, _f64p]
    L.knncf_mae_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                   _f64p, C.POINTER(C.c_int64), C.c_void_p]
    L.knncf_mae_sweep.argtypes = [C.c_void_p, _i32p, C.c_int32, _i32p, _i32p, _f64p, C.c_int64, _f64p, _f64p]
    L.knncf_mae_sweep_device.argtypes = [C.c_void_p, _i32p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, _f64p,
                                         C.POINTER(C.c_int64), C.c_void_p]
    L.knncf_shard_view_get.argtypes = [C.c_void_p, C.POINTER(ShardView)]
    L.knncf_shard_commit.argtypes = [C.c_void_p]
    L.knncf_get_timings.argtypes = [C.c_void_p, C.POINTER(Timings)]
    L.knncf_reset_timings.argtypes = [C.c_void_p]
    L.knncf_reset_neighbors.argtypes = [C.c_void_p]
    L.knncf_set_k.argtypes = [C.c_void_p, C.c_int32]
    L.knncf_load_file.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(Ratings), C.c_char_p, C.c_int]
    L.knncf_load_file_cached.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.POINTER(Ratings), C.POINTER(C.c_int),
                                         C.c_char_p, C.c_int]
    L.knncf_free_ratings.argtypes = [C.POINTER(Ratings)]
    L.knncf_free_ratings.restype = None
    L.knncf_load_personal.argtypes = [C.c_char_p, C.c_int32, C.POINTER(Personal), C.c_char_p, C.c_int]
    L.knncf_free_personal.argtypes = [C.POINTER(Personal)]
    L.knncf_free_personal.restype = None
    L.knncf_neighbors_save.argtypes = [C.c_void_p, C.c_char_p]
    L.knncf_neighbors_load.argtypes = [C.c_void_p, C.c_char_p]
    L.knncf_group_create.argtypes = [C.POINTER(Config), _i32p, C.c_int32, C.POINTER(C.c_void_p)]
    L.knncf_group_destroy.argtypes = [C.c_void_p]
    L.knncf_group_destroy.restype = None
    L.knncf_group_last_error.argtypes = [C.c_void_p]
    L.knncf_group_last_error.restype = C.c_char_p
    L.knncf_group_size.argtypes = [C.c_void_p, _i32p]
    L.knncf_group_handle.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.knncf_group_fit.argtypes = [C.c_void_p, _i32p, _i32p, _f64p, C.c_int64]
    L.knncf_group_mae.argtypes = [C.c_void_p, C.c_int, _i32p, _i32p, _f64p, C.c_int64, _f64p]
    L.knncf_group_predict_batch.argtypes = [C.c_void_p, C.c_int, _i32p, _i32p, C.c_int64, _f64p]
    _lib = L
    return L


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _dev_ptr(t, dtype_name):
    """Raw device pointer of a contiguous torch tensor (torch is only plumbing for device memory)."""
    import torch

    want = {"int32": torch.int32, "float64": torch.float64}[dtype_name]
    if not t.is_cuda or t.dtype != want or not t.is_contiguous():
        raise ValueError(f"expected a contiguous cuda tensor of dtype {dtype_name}")
    return C.c_void_p(t.data_ptr())


def _producer_done(t):
    """The engine runs on its own non-blocking HIP streams and does not know the stream that produced a caller's
    tensor: the "_device" entry points require their inputs to be COMPLETE at the call (include/knncf.h).  Work queued
    on torch's current stream of that device is drained here, so tensors produced asynchronously are never read stale."""
    import torch

    torch.cuda.current_stream(t.device).synchronize()


class Engine:
    """One knncf handle == one set of the reference's closures over a training set."""

    def __init__(self, k=300, similarity=SIM_COSINE, device=0, shard_rank=0, shard_count=1,
                 workspace_bytes=0, flags=0, head_items=0):
        self._lib = load_library()
        cfg = Config(C.sizeof(Config), device, k, similarity, shard_rank, shard_count, workspace_bytes, flags,
                     head_items)
        h = C.c_void_p()
        st = self._lib.knncf_create(C.byref(cfg), C.byref(h))
        if st != OK:
            raise KnncfError(st, self._lib.knncf_status_string(st).decode())
        self._h = h
        self.device = device
        self.k = k

    def close(self):
        if getattr(self, "_h", None):
            self._lib.knncf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != OK:
            raise KnncfError(st, self._lib.knncf_last_error(self._h).decode())

    # ---- fit ---------------------------------------------------------------------------
    def fit(self, users, items, ratings):
        u, i, r = _i32(users), _i32(items), _f64(ratings)
        if not (len(u) == len(i) == len(r)):
            raise ValueError("users/items/ratings differ in length")
        self._check(self._lib.knncf_fit(self._h, u.ctypes.data_as(_i32p), i.ctypes.data_as(_i32p),
                                        r.ctypes.data_as(_f64p), len(u)))
        return self

    def fit_device(self, users, items, ratings):
        """users/items int32, ratings float64: contiguous torch tensors on this engine's device."""
        n = users.numel()
        _producer_done(users)
        self._check(self._lib.knncf_fit_device(self._h, _dev_ptr(users, "int32"), _dev_ptr(items, "int32"),
                                               _dev_ptr(ratings, "float64"), n))
        return self

    @property
    def num_users(self):
        v = C.c_int32()
        self._check(self._lib.knncf_num_users(self._h, C.byref(v)))
        return v.value

    @property
    def num_items(self):
        v = C.c_int32()
        self._check(self._lib.knncf_num_items(self._h, C.byref(v)))
        return v.value

    # ---- scalar queries ----------------------------------------------------------------
    def _scalar(self, fn, *args):
        v = C.c_double()
        self._check(fn(self._h, *args, C.byref(v)))
        return v.value

    def global_avg(self):
        return self._scalar(self._lib.knncf_global_avg)

    def user_avg(self, u):
        return self._scalar(self._lib.knncf_user_avg, u)

    def item_avg(self, i):
        return self._scalar(self._lib.knncf_item_avg, i)

    def item_avg_dev(self, i):
        return self._scalar(self._lib.knncf_item_avg_dev, i)

    def item_avg_dev_rdd(self, i):
        return self._scalar(self._lib.knncf_item_avg_dev_rdd, i)

    def similarity(self, u, v):
        return self._scalar(self._lib.knncf_similarity, u, v)

    def knn_similarity(self, u, v):
        return self._scalar(self._lib.knncf_knn_similarity, u, v)

    @staticmethod
    def _pair_ids(us, vs):
        """validated raw ids of a batch of pairs: ValueError before any C call"""
        out = []
        for a in (us, vs):
            a = np.asarray(a)
            if a.ndim != 1:
                raise ValueError("us and vs must be 1-D arrays of ids")
            if len(a) and (a.dtype.kind not in "iu" or a.min() < -2**31 or a.max() >= 2**31):
                raise ValueError("us and vs must be 32-bit integer ids")
            out.append(_i32(a))
        if len(out[0]) != len(out[1]):
            raise ValueError("us and vs differ in length")
        return out

    def _pair_batch(self, entry, us, vs):
        u, v = self._pair_ids(us, vs)
        out = np.empty(len(u), dtype=np.float64)
        p = self._ptr
        self._check(getattr(self._lib, entry)(self._h, p(u, _i32p), p(v, _i32p), len(u), p(out, _f64p)))
        return out

    def similarity_batch(self, us, vs):
        """similarity(us[j], vs[j]) for every j in one device pass (knncf_similarity_batch): float64 [n].  Every pair is
        answered on a closure of its own, us[j] as the first argument; the handle is only read."""
        return self._pair_batch("knncf_similarity_batch", us, vs)

    def knn_similarity_batch(self, us, vs):
        """knn_similarity(us[j], vs[j]) for every j, as if called in this order (knncf_knn_similarity_batch): float64 [n].
        Missing neighbourhoods are built in one batch: the handle is left as neighbors_batch leaves it over us with an
        absent id wherever us[j] or vs[j] is absent from train."""
        return self._pair_batch("knncf_knn_similarity_batch", us, vs)

    def similarity_batch_device(self, us, vs, out):
        """similarity_batch on contiguous torch tensors of this engine's device: us, vs int32 [n], out float64 [n]"""
        import torch

        for t, dt in ((us, torch.int32), (vs, torch.int32), (out, torch.float64)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1:
                raise ValueError("us, vs must be 1-D int32 tensors and out a 1-D float64 tensor")
        if not (us.numel() == vs.numel() == out.numel()):
            raise ValueError("us, vs and out differ in length")
        if not (us.is_cuda and vs.is_cuda and out.is_cuda and us.is_contiguous() and vs.is_contiguous() and out.is_contiguous()):
            raise ValueError("us, vs and out must be contiguous tensors on the device")
        _producer_done(us)
        self._check(self._lib.knncf_similarity_batch_device(self._h, _dev_ptr(us, "int32"), _dev_ptr(vs, "int32"), us.numel(),
                                                            _dev_ptr(out, "float64")))
        return out

    def neighbors(self, u):
        cap = max(1, self.k)
        ids = np.empty(cap, dtype=np.int32)
        sims = np.empty(cap, dtype=np.float64)
        c = C.c_int32()
        self._check(self._lib.knncf_neighbors(self._h, u, cap, ids.ctypes.data_as(_i32p),
                                              sims.ctypes.data_as(_f64p), C.byref(c)))
        return ids[:c.value].copy(), sims[:c.value].copy()

    def neighbors_batch(self, users):
        """getNeighbors for many users at once (knncf_neighbors_batch): (ids [n, k], sims [n, k], counts [n]); cells past
        a row's count are -1 / nan"""
        u = _i32(users)
        cap = max(1, self.k)
        ids = np.full((len(u), cap), -1, dtype=np.int32)
        sims = np.full((len(u), cap), np.nan, dtype=np.float64)
        counts = np.zeros(len(u), dtype=np.int32)
        self._check(self._lib.knncf_neighbors_batch(self._h, u.ctypes.data_as(_i32p), len(u), cap, ids.ctypes.data_as(_i32p),
                                                    sims.ctypes.data_as(_f64p), counts.ctypes.data_as(_i32p)))
        return ids, sims, counts

    def predict(self, predictor, u, i):
        return self._scalar(self._lib.knncf_predict, predictor, u, i)

    def neighbors_save(self, path):
        """checkpoint of the U x k neighbour table (knncf_neighbors_save)"""
        self._check(self._lib.knncf_neighbors_save(self._h, os.fsencode(path)))

    def neighbors_load(self, path):
        """resume from a checkpoint written by a handle fitted on the same data with the same k (knncf_neighbors_load)"""
        self._check(self._lib.knncf_neighbors_load(self._h, os.fsencode(path)))

    def recommend(self, predictor, user, n):
        """recommendations(train, predictor)(user, n) shared/predictions.scala:651-674: (item ids, predictions).  The
        batched call over one user (knncf_recommend)"""
        ids = np.empty(max(1, n), dtype=np.int32)
        preds = np.empty(max(1, n), dtype=np.float64)
        c = C.c_int32()
        self._check(self._lib.knncf_recommend(self._h, predictor, user, n, ids.ctypes.data_as(_i32p),
                                              preds.ctypes.data_as(_f64p), C.byref(c)))
        return ids[:c.value].copy(), preds[:c.value].copy()

    def recommend_batch(self, predictor, users, n):
        """recommend(predictor, users[b], n) for every b, as if called in this order (knncf_recommend_batch): (items [B, n]
        int32, preds [B, n] float64, counts [B] int32); cells past a row's count are -1 / nan.  Missing neighbourhoods are
        built in one batch; PRED_KNN leaves the handle as neighbors_batch over the users whose mean is not negative leaves it."""
        u = np.asarray(users)
        if u.ndim != 1:
            raise ValueError("users must be a 1-D array of ids")
        if len(u) and (u.dtype.kind not in "iu" or u.min() < -2**31 or u.max() >= 2**31):
            raise ValueError("users must be 32-bit integer ids")
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0 or n >= 2**31:
            raise ValueError("n must be a non-negative 32-bit integer")
        u, n = _i32(u), int(n)
        B = len(u)
        items = np.full((B, n), -1, dtype=np.int32)
        preds = np.full((B, n), np.nan, dtype=np.float64)
        counts = np.zeros(B, dtype=np.int32)
        p = self._ptr
        self._check(self._lib.knncf_recommend_batch(self._h, predictor, p(u, _i32p), B, n, p(items.reshape(-1), _i32p),
                                                    p(preds.reshape(-1), _f64p), p(counts, _i32p)))
        return items, preds, counts

    # ---- explanations: the neighbour terms behind kNN predictions (knncf_explain*) ----------
    @staticmethod
    def _explain_args(cap, order):
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or cap < 0 or cap >= 2**31:
            raise ValueError("cap must be a non-negative 32-bit integer")
        if order not in (EXPLAIN_SUM_ORDER, EXPLAIN_BY_WEIGHT):
            raise ValueError("order must be EXPLAIN_SUM_ORDER or EXPLAIN_BY_WEIGHT")
        return int(cap), int(order)

    def _explain_row(self, entry, user, item, cap, order):
        cap, order = self._explain_args(cap, order)
        fn = getattr(self._lib, entry)
        raters = np.empty(max(1, cap), dtype=np.int32)
        sims = np.empty(max(1, cap), dtype=np.float64)
        devs = np.empty(max(1, cap), dtype=np.float64)
        c, sums, pred = C.c_int32(), np.zeros(2, dtype=np.float64), C.c_double()
        p = self._ptr
        self._check(fn(self._h, user, item, order, cap, p(raters, _i32p), p(sims, _f64p), p(devs, _f64p), C.byref(c), p(sums, _f64p),
                       C.byref(pred)))
        m = min(c.value, cap)
        return raters[:m].copy(), sims[:m].copy(), devs[:m].copy(), c.value, (float(sums[0]), float(sums[1])), pred.value

    def _explain_rows(self, entry, users, items, cap, order):
        cap, order = self._explain_args(cap, order)
        u, i = _i32(users), _i32(items)
        if u.ndim != 1 or u.shape != i.shape:
            raise ValueError("users and items must be 1-D arrays of one length")
        fn = getattr(self._lib, entry)
        n = len(u)
        raters = np.full((n, cap), -1, dtype=np.int32)
        sims = np.full((n, cap), np.nan, dtype=np.float64)
        devs = np.full((n, cap), np.nan, dtype=np.float64)
        counts = np.zeros(n, dtype=np.int32)
        sums = np.zeros((n, 2), dtype=np.float64)
        preds = np.empty(n, dtype=np.float64)
        p = self._ptr
        self._check(fn(self._h, p(u, _i32p), p(i, _i32p), n, order, cap, p(raters.reshape(-1), _i32p), p(sims.reshape(-1), _f64p),
                       p(devs.reshape(-1), _f64p), p(counts, _i32p), p(sums.reshape(-1), _f64p), p(preds, _f64p)))
        return raters, sims, devs, counts, sums, preds

    def explain(self, user, item, cap=None, order=EXPLAIN_SUM_ORDER):
        """The terms behind predict(PRED_KNN, user, item) (knncf_explain): (raters int32, sims, devs, count, (num, den),
        prediction) — the neighbours of `user` with a non-zero similarity that rated `item`, in `order`; the arrays hold
        min(count, cap) terms.  cap=None: the handle's min(k, U - 1), which every row fits."""
        if cap is None:
            cap = max(0, min(self.k, self.num_users - 1))
        return self._explain_row("knncf_explain", user, item, cap, order)

    def explain_batch(self, users, items, cap, order=EXPLAIN_SUM_ORDER):
        """explain for every row (users[j], items[j]) (knncf_explain_batch): (raters [n, cap] int32, sims [n, cap], devs
        [n, cap], counts [n] int32, sums [n, 2], predictions [n]); cells past a row's min(count, cap) terms are -1 / nan.
        Missing neighbourhoods are built as predict_batch(PRED_KNN, users, items) builds them."""
        return self._explain_rows("knncf_explain_batch", users, items, cap, order)

    def explain_personalized(self, user, item, cap=16, order=EXPLAIN_BY_WEIGHT):
        """The terms behind predict(PRED_PERSONALIZED, user, item) (knncf_explain_personalized), as explain returns them: every
        rater of `item` whose similarity with `user` is non-zero is a term, `user` itself included when it rated the item in
        train.  The defaults answer "which 16 users carried this prediction"; cap=None: num_users, which every row fits."""
        if cap is None:
            cap = self.num_users
        return self._explain_row("knncf_explain_personalized", user, item, cap, order)

    def explain_personalized_batch(self, users, items, cap, order=EXPLAIN_SUM_ORDER):
        """explain_personalized for every row (users[j], items[j]) (knncf_explain_personalized_batch), as explain_batch returns
        it.  Read-only on the neighbour table."""
        return self._explain_rows("knncf_explain_personalized_batch", users, items, cap, order)

    def explain_batch_device(self, users, items, cap, raters, sims, devs, counts, sums=None, predictions=None,
                             order=EXPLAIN_SUM_ORDER):
        """explain_batch in one pass on contiguous torch tensors of this engine's device (knncf_explain_batch_device): users /
        items int32 [n]; raters int32, sims / devs float64 [n, cap] (None with cap == 0); counts int32 [n]; sums float64
        [n, 2] and predictions float64 [n] optional.  Cells past a row's terms are left as they are."""
        cap, order = self._explain_args(cap, order)
        n = users.numel()
        if items.numel() != n or counts.numel() != n:
            raise ValueError("users, items and counts must have one length")
        for t, width in ((raters, cap), (sims, cap), (devs, cap), (sums, 2), (predictions, 1)):
            if t is not None and t.numel() != n * width:
                raise ValueError("an output tensor does not hold n rows")
        if cap > 0 and (raters is None or sims is None or devs is None):
            raise ValueError("cap > 0 needs raters, sims and devs")
        opt = lambda t, name: _dev_ptr(t, name) if t is not None else None
        _producer_done(users)
        self._check(self._lib.knncf_explain_batch_device(
            self._h, _dev_ptr(users, "int32"), _dev_ptr(items, "int32"), n, order, cap, opt(raters, "int32"),
            opt(sims, "float64"), opt(devs, "float64"), _dev_ptr(counts, "int32"), opt(sums, "float64"),
            opt(predictions, "float64")))

    # ---- fold-in queries: a user outside the fit (knncf_query_*), and update queries: any user, the rows being additional
    # to its train rows (knncf_update_*).  The two families share their argument lists; `fam` picks the entry points. ----
    # The predict / recommend forms take predictor=PRED_KNN (the default) or PRED_PERSONALIZED: the Personalized predictor on
    # aug, every rating of an item a term and the handle's k without a part (include/knncf.h "Personalized queries").
    @staticmethod
    def _query_rows(user, items, ratings, allow_empty=False):
        """validated (user, items, ratings) of a query: ValueError before any C call"""
        if isinstance(user, (bool, np.bool_)) or not isinstance(user, (int, np.integer)) or not -2**31 <= int(user) < 2**31:
            raise ValueError("user must be a 32-bit integer id")
        it = np.asarray(items)
        rt = np.asarray(ratings)
        if it.ndim != 1 or rt.ndim != 1 or len(it) != len(rt):
            raise ValueError("items and ratings must be 1-D and of the same length")
        if len(it) == 0:
            if not allow_empty:
                raise ValueError("a query needs at least one rating")
            return int(user), np.empty(0, dtype=np.int32), np.empty(0, dtype=np.float64)
        if it.dtype.kind not in "iu" or (len(it) and (it.min() < -2**31 or it.max() >= 2**31)):
            raise ValueError("items must be 32-bit integer ids")
        if rt.dtype.kind not in "iuf":
            raise ValueError("ratings must be numbers")
        return int(user), _i32(it), _f64(rt)

    @staticmethod
    def _ptr(a, t):
        return a.ctypes.data_as(t) if len(a) else C.cast(None, t)

    @staticmethod
    def _removed(removed):
        """validated removed item ids of a revise query: ValueError before any C call"""
        rm = np.asarray(removed)
        if rm.ndim != 1:
            raise ValueError("removed items must be 1-D")
        if len(rm) == 0:
            return np.empty(0, dtype=np.int32)
        if rm.dtype.kind not in "iu" or rm.min() < -2**31 or rm.max() >= 2**31:
            raise ValueError("removed items must be 32-bit integer ids")
        return _i32(rm)

    def _rm_args(self, fam, removed):
        """the removals of a single revise call as C arguments (nothing for the other families)"""
        if fam != "revise":
            return ()
        rm = self._removed(removed)
        return (self._ptr(rm, _i32p), len(rm))

    def _neighbors_q(self, fam, user, items, ratings, cap, removed=None):
        q, it, rt = self._query_rows(user, items, ratings, allow_empty=fam != "query")
        rm = self._rm_args(fam, removed)
        if cap is None:
            cap = max(1, self.k)
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or cap < 0:
            raise ValueError("cap must be a non-negative integer")
        cap = int(cap)
        ids = np.empty(max(1, cap), dtype=np.int32)
        sims = np.empty(max(1, cap), dtype=np.float64)
        c = C.c_int32()
        p = self._ptr
        self._check(getattr(self._lib, f"knncf_{fam}_neighbors")(self._h, q, *rm, p(it, _i32p), p(rt, _f64p), len(it), cap,
                                                                 ids.ctypes.data_as(_i32p), sims.ctypes.data_as(_f64p), C.byref(c)))
        m = min(c.value, cap)
        return ids[:m].copy(), sims[:m].copy()

    def _predict_q(self, fam, user, items, ratings, pred_items, removed=None, predictor=PRED_KNN):
        q, it, rt = self._query_rows(user, items, ratings, allow_empty=fam != "query")
        rm = self._rm_args(fam, removed)
        pi = np.asarray(pred_items)
        if pi.ndim != 1 or (len(pi) and pi.dtype.kind not in "iu"):
            raise ValueError("pred_items must be a 1-D array of integer ids")
        pi = _i32(pi)
        out = np.empty(max(1, len(pi)), dtype=np.float64)
        p = self._ptr
        self._check(getattr(self._lib, f"knncf_{fam}_predict")(self._h, predictor, q, *rm, p(it, _i32p), p(rt, _f64p), len(it),
                                                               pi.ctypes.data_as(_i32p), len(pi), out.ctypes.data_as(_f64p)))
        return out[:len(pi)].copy()

    def _recommend_q(self, fam, user, items, ratings, n, removed=None, predictor=PRED_KNN):
        q, it, rt = self._query_rows(user, items, ratings, allow_empty=fam != "query")
        rm = self._rm_args(fam, removed)
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0 or n >= 2**31:
            raise ValueError("n must be a non-negative 32-bit integer")
        n = int(n)
        ids = np.empty(max(1, n), dtype=np.int32)
        preds = np.empty(max(1, n), dtype=np.float64)
        c = C.c_int32()
        p = self._ptr
        self._check(getattr(self._lib, f"knncf_{fam}_recommend")(self._h, predictor, q, *rm, p(it, _i32p), p(rt, _f64p), len(it), n,
                                                                 ids.ctypes.data_as(_i32p), preds.ctypes.data_as(_f64p), C.byref(c)))
        return ids[:c.value].copy(), preds[:c.value].copy()

    def neighbors_for(self, user, items, ratings, cap=None):
        """getNeighbors(train ++ user's ratings, k, sim)(user) for a user outside the fit: (ids, sims)"""
        return self._neighbors_q("query", user, items, ratings, cap)

    def predict_for(self, user, items, ratings, pred_items, predictor=PRED_KNN):
        """kNN predictions (PRED_KNN) of a user outside the fit, given its ratings, for every id of pred_items"""
        return self._predict_q("query", user, items, ratings, pred_items, predictor=predictor)

    def recommend_for(self, user, items, ratings, n, predictor=PRED_KNN):
        """recommendations(train ++ user's ratings, kNN predictor)(user, n) for a user outside the fit: (item ids, predictions)"""
        return self._recommend_q("query", user, items, ratings, n, predictor=predictor)

    def neighbors_with(self, user, items, ratings, cap=None):
        """getNeighbors(train ++ the additional ratings, k, sim)(user) for any user, of the fit or not: (ids, sims).  A user
        of the fit is not its own neighbour; items / ratings may be empty for it."""
        return self._neighbors_q("update", user, items, ratings, cap)

    def predict_with(self, user, items, ratings, pred_items, predictor=PRED_KNN):
        """kNN predictions (PRED_KNN) of a user with additional ratings (beside its train rows, if any) for every id of pred_items"""
        return self._predict_q("update", user, items, ratings, pred_items, predictor=predictor)

    def recommend_with(self, user, items, ratings, n, predictor=PRED_KNN):
        """recommendations(train ++ the additional ratings, kNN predictor)(user, n) for any user: (item ids, predictions)"""
        return self._recommend_q("update", user, items, ratings, n, predictor=predictor)

    def neighbors_revised(self, user, removed, items, ratings, cap=None):
        """getNeighbors(aug, k, sim)(user) where aug is train without the user's rows on the `removed` items, plus the additional
        (items, ratings): (ids, sims).  An item both removed and given again is re-rated."""
        return self._neighbors_q("revise", user, items, ratings, cap, removed)

    def predict_revised(self, user, removed, items, ratings, pred_items, predictor=PRED_KNN):
        """kNN predictions (PRED_KNN) of a user that removed the `removed` train items and rated (items, ratings) in addition"""
        return self._predict_q("revise", user, items, ratings, pred_items, removed, predictor)

    def recommend_revised(self, user, removed, items, ratings, n, predictor=PRED_KNN):
        """recommendations(aug, kNN predictor)(user, n) on that aug: (item ids, predictions)"""
        return self._recommend_q("revise", user, items, ratings, n, removed, predictor)

    @staticmethod
    def _pred_items(pred_items):
        pi = np.asarray(pred_items)
        if pi.ndim != 1 or (len(pi) and pi.dtype.kind not in "iu"):
            raise ValueError("pred_items must be a 1-D array of integer ids")
        return _i32(pi)

    @staticmethod
    def _explain_out(m, cap):
        """the outputs of m explained rows, term cells padded with -1 / nan as explain_batch pads them"""
        return (np.full((m, cap), -1, dtype=np.int32), np.full((m, cap), np.nan, dtype=np.float64),
                np.full((m, cap), np.nan, dtype=np.float64), np.zeros(m, dtype=np.int32), np.full((m, 2), np.nan, dtype=np.float64),
                np.full(m, np.nan, dtype=np.float64))

    def _explain_ptrs(self, out):
        p = self._ptr
        raters, sims, devs, counts, sums, preds = out
        return (p(raters.reshape(-1), _i32p), p(sims.reshape(-1), _f64p), p(devs.reshape(-1), _f64p), p(counts, _i32p),
                p(sums.reshape(-1), _f64p), p(preds, _f64p))

    @staticmethod
    def _explain_entry(fam, tail, predictor):
        """the explain entry point of a family and its leading predictor argument: knncf_*_explain* takes PRED_KNN,
        knncf_*_explain_personalized* (PRED_PERSONALIZED) has no predictor argument.  ValueError for any other predictor"""
        if isinstance(predictor, (bool, np.bool_)) or not isinstance(predictor, (int, np.integer)) or predictor not in (PRED_KNN, PRED_PERSONALIZED):
            raise ValueError("predictor must be PRED_KNN or PRED_PERSONALIZED")
        if predictor == PRED_PERSONALIZED:
            return f"knncf_{fam}_explain_personalized{tail}", ()
        return f"knncf_{fam}_explain{tail}", (PRED_KNN,)

    def _explain_q(self, fam, user, items, ratings, pred_items, cap, order, removed=None, predictor=PRED_KNN):
        cap, order = self._explain_args(cap, order)
        entry, lead = self._explain_entry(fam, "", predictor)
        q, it, rt = self._query_rows(user, items, ratings, allow_empty=fam != "query")
        rm = self._rm_args(fam, removed)
        pi = self._pred_items(pred_items)
        out = self._explain_out(len(pi), cap)
        p = self._ptr
        self._check(getattr(self._lib, entry)(self._h, *lead, q, *rm, p(it, _i32p), p(rt, _f64p), len(it),
                                              p(pi, _i32p), len(pi), order, cap, *self._explain_ptrs(out)))
        return out

    def explain_for(self, user, items, ratings, pred_items, cap, order=EXPLAIN_SUM_ORDER, predictor=PRED_KNN):
        """The terms behind predict_for(user, items, ratings, pred_items) (knncf_query_explain), one row per requested item:
        (raters [m, cap] int32, sims [m, cap], devs [m, cap], counts [m] int32, sums [m, 2], predictions [m]); the cells past a
        row's min(count, cap) terms are -1 / nan.  predictions is predict_for's answer bit for bit.
        predictor=PRED_PERSONALIZED (knncf_query_explain_personalized): the terms behind predict_for(..., predictor=
        PRED_PERSONALIZED) — every rater of the item in aug with a non-zero similarity, the user itself among them."""
        return self._explain_q("query", user, items, ratings, pred_items, cap, order, predictor=predictor)

    def explain_with(self, user, items, ratings, pred_items, cap, order=EXPLAIN_SUM_ORDER, predictor=PRED_KNN):
        """The terms behind predict_with(...) (knncf_update_explain / knncf_update_explain_personalized): as explain_for, for any
        user, of the fit or not"""
        return self._explain_q("update", user, items, ratings, pred_items, cap, order, predictor=predictor)

    def explain_revised(self, user, removed, items, ratings, pred_items, cap, order=EXPLAIN_SUM_ORDER, predictor=PRED_KNN):
        """The terms behind predict_revised(...) (knncf_revise_explain / knncf_revise_explain_personalized): as explain_for, on aug
        without the removed rows"""
        return self._explain_q("revise", user, items, ratings, pred_items, cap, order, removed, predictor)

    # ---- batched forms (knncf_query_*_batch, knncf_update_*_batch, knncf_revise_*_batch) --------
    def _batch_args(self, fam, queries):
        """the validated queries of a batched call as C arguments: users, [the CSR of the removals,] the CSR of the rows, B"""
        p = self._ptr
        if fam != "revise":
            us, off, it, rt = self._query_batch(queries)
            return (p(us, _i32p), p(off, _i64p), p(it, _i32p), p(rt, _f64p), len(us)), (us, off, it, rt)
        rms, roff, triples = [], [0], []
        for q in queries:
            if not isinstance(q, (tuple, list)) or len(q) != 4:
                raise ValueError("a revise query is (user, removed_items, items, ratings)")
            rms.append(self._removed(q[1]))
            roff.append(roff[-1] + len(rms[-1]))
            triples.append((q[0], q[2], q[3]))
        if roff[-1] >= 2**31:
            raise ValueError("fewer than 2^31 removed items per call")
        us, off, it, rt = self._query_batch(triples)
        roff = np.asarray(roff, dtype=np.int64)
        rm = np.ascontiguousarray(np.concatenate(rms) if rms else np.empty(0), dtype=np.int32)
        return (p(us, _i32p), p(roff, _i64p), p(rm, _i32p), p(off, _i64p), p(it, _i32p), p(rt, _f64p), len(us)), (us, roff, rm, off, it, rt)

    @staticmethod
    def _query_batch(queries):
        """validated CSR (users, offsets, items, ratings) of a sequence of (user, items, ratings): ValueError before any C
        call.  An empty query is allowed here: it gets its own status (E_INVALID for a fold-in query or a user outside the
        fit), like every per-query failure."""
        users, its, rts, offsets = [], [], [], [0]
        for q in queries:
            if not isinstance(q, (tuple, list)) or len(q) != 3:
                raise ValueError("a query is (user, items, ratings)")
            user, items, ratings = q
            if isinstance(user, (bool, np.bool_)) or not isinstance(user, (int, np.integer)) or not -2**31 <= int(user) < 2**31:
                raise ValueError("user must be a 32-bit integer id")
            it, rt = np.asarray(items), np.asarray(ratings)
            if it.ndim != 1 or rt.ndim != 1 or len(it) != len(rt):
                raise ValueError("items and ratings must be 1-D and of the same length")
            if len(it):
                if it.dtype.kind not in "iu" or it.min() < -2**31 or it.max() >= 2**31:
                    raise ValueError("items must be 32-bit integer ids")
                if rt.dtype.kind not in "iuf":
                    raise ValueError("ratings must be numbers")
            users.append(int(user))
            its.append(it.astype(np.int32))
            rts.append(rt.astype(np.float64))
            offsets.append(offsets[-1] + len(it))
        if offsets[-1] >= 2**31:
            raise ValueError("fewer than 2^31 query ratings per call")
        cat = lambda parts, dt: np.ascontiguousarray(np.concatenate(parts) if parts else np.empty(0), dtype=dt)
        return (np.asarray(users, dtype=np.int32), np.asarray(offsets, dtype=np.int64), cat(its, np.int32), cat(rts, np.float64))

    def _neighbors_qb(self, fam, queries, cap):
        qargs, keep = self._batch_args(fam, queries)
        if cap is None:
            cap = max(1, self.k)
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or cap < 0:
            raise ValueError("cap must be a non-negative integer")
        cap, B = int(cap), qargs[-1]
        ids = np.empty((B, cap), dtype=np.int32)
        sims = np.empty((B, cap), dtype=np.float64)
        counts = np.zeros(B, dtype=np.int32)
        st = np.zeros(B, dtype=np.int32)
        p = self._ptr
        self._check(getattr(self._lib, f"knncf_{fam}_neighbors_batch")(
            self._h, *qargs, cap, p(ids.reshape(-1), _i32p),
            p(sims.reshape(-1), _f64p), p(counts, _i32p), p(st, _i32p)))
        return [(ids[b, :min(counts[b], cap)].copy(), sims[b, :min(counts[b], cap)].copy()) for b in range(B)], st

    def _predict_qb(self, fam, queries, pred_items, predictor=PRED_KNN):
        qargs, keep = self._batch_args(fam, queries)
        B = qargs[-1]
        pis = [np.asarray(x) for x in pred_items]
        if len(pis) != B:
            raise ValueError("one pred_items sequence per query")
        for x in pis:
            if x.ndim != 1 or (len(x) and x.dtype.kind not in "iu"):
                raise ValueError("pred_items must be 1-D arrays of integer ids")
        poff = np.zeros(B + 1, dtype=np.int64)
        poff[1:] = np.cumsum([len(x) for x in pis])
        pi = np.ascontiguousarray(np.concatenate(pis) if B and poff[-1] else np.empty(0), dtype=np.int32)
        out = np.full(int(poff[-1]), np.nan, dtype=np.float64)
        st = np.zeros(B, dtype=np.int32)
        p = self._ptr
        self._check(getattr(self._lib, f"knncf_{fam}_predict_batch")(
            self._h, predictor, *qargs, p(poff, _i64p), p(pi, _i32p),
            p(out, _f64p), p(st, _i32p)))
        return [out[poff[b]:poff[b + 1]].copy() for b in range(B)], st

    def _recommend_qb(self, fam, queries, n, predictor=PRED_KNN):
        qargs, keep = self._batch_args(fam, queries)
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0 or n >= 2**31:
            raise ValueError("n must be a non-negative 32-bit integer")
        n, B = int(n), qargs[-1]
        ids = np.empty((B, n), dtype=np.int32)
        preds = np.empty((B, n), dtype=np.float64)
        counts = np.zeros(B, dtype=np.int32)
        st = np.zeros(B, dtype=np.int32)
        p = self._ptr
        self._check(getattr(self._lib, f"knncf_{fam}_recommend_batch")(
            self._h, predictor, *qargs, n, p(ids.reshape(-1), _i32p),
            p(preds.reshape(-1), _f64p), p(counts, _i32p), p(st, _i32p)))
        return [(ids[b, :counts[b]].copy(), preds[b, :counts[b]].copy()) for b in range(B)], st

    def neighbors_for_batch(self, queries, cap=None):
        """neighbors_for of every (user, items, ratings) of `queries`, answered in chunks on the device:
        ([(ids, sims)] per query, statuses int32 [B]).  A failed query (status != OK) has empty arrays."""
        return self._neighbors_qb("query", queries, cap)

    def predict_for_batch(self, queries, pred_items, predictor=PRED_KNN):
        """predict_for of every query; pred_items is one sequence of item ids per query: ([float64 array] per query, statuses).
        A failed query's array holds NaN."""
        return self._predict_qb("query", queries, pred_items, predictor)

    def recommend_for_batch(self, queries, n, predictor=PRED_KNN):
        """recommend_for(n) of every query: ([(item ids, predictions)] per query, statuses).  A failed query has empty arrays."""
        return self._recommend_qb("query", queries, n, predictor)

    def neighbors_with_batch(self, queries, cap=None):
        """neighbors_with of every (user, additional items, additional ratings) of `queries`, users of the fit and others
        mixed: ([(ids, sims)] per query, statuses int32 [B]).  A failed query (status != OK) has empty arrays."""
        return self._neighbors_qb("update", queries, cap)

    def predict_with_batch(self, queries, pred_items, predictor=PRED_KNN):
        """predict_with of every query; pred_items is one sequence of item ids per query: ([float64 array] per query, statuses).
        A failed query's array holds NaN."""
        return self._predict_qb("update", queries, pred_items, predictor)

    def recommend_with_batch(self, queries, n, predictor=PRED_KNN):
        """recommend_with(n) of every query: ([(item ids, predictions)] per query, statuses).  A failed query has empty arrays."""
        return self._recommend_qb("update", queries, n, predictor)

    def neighbors_revised_batch(self, queries, cap=None):
        """neighbors_revised of every (user, removed_items, additional items, additional ratings) of `queries`:
        ([(ids, sims)] per query, statuses int32 [B]).  A failed query (status != OK) has empty arrays."""
        return self._neighbors_qb("revise", queries, cap)

    def predict_revised_batch(self, queries, pred_items, predictor=PRED_KNN):
        """predict_revised of every query; pred_items is one sequence of item ids per query: ([float64 array] per query, statuses).
        A failed query's array holds NaN."""
        return self._predict_qb("revise", queries, pred_items, predictor)

    def recommend_revised_batch(self, queries, n, predictor=PRED_KNN):
        """recommend_revised(n) of every query: ([(item ids, predictions)] per query, statuses).  A failed query has empty arrays."""
        return self._recommend_qb("revise", queries, n, predictor)

    def _explain_qb(self, fam, queries, pred_items, cap, order, predictor=PRED_KNN):
        cap, order = self._explain_args(cap, order)
        entry, lead = self._explain_entry(fam, "_batch", predictor)
        qargs, keep = self._batch_args(fam, queries)
        B = qargs[-1]
        pred_items = list(pred_items)
        if len(pred_items) != B:
            raise ValueError("one pred_items sequence per query")
        pis = [self._pred_items(x) for x in pred_items]
        poff = np.zeros(B + 1, dtype=np.int64)
        poff[1:] = np.cumsum([len(x) for x in pis])
        pi = np.ascontiguousarray(np.concatenate(pis) if B and poff[-1] else np.empty(0), dtype=np.int32)
        out = self._explain_out(int(poff[-1]), cap)
        st = np.zeros(B, dtype=np.int32)
        p = self._ptr
        self._check(getattr(self._lib, entry)(
            self._h, *lead, *qargs, p(poff, _i64p), p(pi, _i32p), order, cap, *self._explain_ptrs(out), p(st, _i32p)))
        return [tuple(a[poff[b]:poff[b + 1]].copy() for a in out) for b in range(B)], st

    def explain_for_batch(self, queries, pred_items, cap, order=EXPLAIN_SUM_ORDER, predictor=PRED_KNN):
        """explain_for of every query; pred_items is one sequence of item ids per query: ([the explain_for tuple] per query,
        statuses).  A failed query's arrays hold only padding (-1 / nan, counts 0).  predictor as in explain_for."""
        return self._explain_qb("query", queries, pred_items, cap, order, predictor)

    def explain_with_batch(self, queries, pred_items, cap, order=EXPLAIN_SUM_ORDER, predictor=PRED_KNN):
        """explain_with of every query: ([the explain_with tuple] per query, statuses)"""
        return self._explain_qb("update", queries, pred_items, cap, order, predictor)

    def explain_revised_batch(self, queries, pred_items, cap, order=EXPLAIN_SUM_ORDER, predictor=PRED_KNN):
        """explain_revised of every (user, removed_items, items, ratings): ([the explain_revised tuple] per query, statuses)"""
        return self._explain_qb("revise", queries, pred_items, cap, order, predictor)

    # ---- recommendations with their explanations in one pass (knncf_*_recommend_explain*) --------
    @staticmethod
    def _reco_explain_args(n, cap, order, predictor):
        """validated (n, cap, order, predictor) of a fused call: the checks of the recommend and of the explain wrappers"""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0 or n >= 2**31:
            raise ValueError("n must be a non-negative 32-bit integer")
        cap, order = Engine._explain_args(cap, order)
        Engine._explain_entry("query", "", predictor)
        return int(n), cap, order, int(predictor)

    def _recommend_explain_q(self, fam, user, items, ratings, n, cap, order, removed=None, predictor=PRED_KNN):
        n, cap, order, predictor = self._reco_explain_args(n, cap, order, predictor)
        q, it, rt = self._query_rows(user, items, ratings, allow_empty=fam != "query")
        rm = self._rm_args(fam, removed)
        ids = np.empty(max(1, n), dtype=np.int32)
        preds = np.empty(max(1, n), dtype=np.float64)
        c = C.c_int32()
        out = self._explain_out(n, cap)
        p = self._ptr
        self._check(getattr(self._lib, f"knncf_{fam}_recommend_explain")(
            self._h, predictor, q, *rm, p(it, _i32p), p(rt, _f64p), len(it), n, order, cap, ids.ctypes.data_as(_i32p),
            preds.ctypes.data_as(_f64p), C.byref(c), *self._explain_ptrs(out)[:-1]))
        return (ids[:c.value].copy(), preds[:c.value].copy()) + tuple(a[:c.value].copy() for a in out[:-1])

    def _recommend_explain_qb(self, fam, queries, n, cap, order, predictor=PRED_KNN):
        n, cap, order, predictor = self._reco_explain_args(n, cap, order, predictor)
        qargs, keep = self._batch_args(fam, queries)
        B = qargs[-1]
        ids = np.empty((B, n), dtype=np.int32)
        preds = np.empty((B, n), dtype=np.float64)
        counts = np.zeros(B, dtype=np.int32)
        st = np.zeros(B, dtype=np.int32)
        out = self._explain_out(B * n, cap)
        p = self._ptr
        self._check(getattr(self._lib, f"knncf_{fam}_recommend_explain_batch")(
            self._h, predictor, *qargs, n, order, cap, p(ids.reshape(-1), _i32p), p(preds.reshape(-1), _f64p), p(counts, _i32p),
            *self._explain_ptrs(out)[:-1], p(st, _i32p)))
        return [(ids[b, :counts[b]].copy(), preds[b, :counts[b]].copy()) + tuple(a[b * n:b * n + counts[b]].copy() for a in out[:-1])
                for b in range(B)], st

    def recommend_explain_for(self, user, items, ratings, n, cap, order=EXPLAIN_SUM_ORDER, predictor=PRED_KNN):
        """recommend_for(user, items, ratings, n) and the terms behind each recommended item from one pass over the fit
        (knncf_query_recommend_explain): (item ids [c], predictions [c], raters [c, cap] int32, sims [c, cap], devs [c, cap],
        term_counts [c] int32, sums [c, 2]) with c recommended items.  The first two are recommend_for's answer, the rest
        explain_for's for pred_items = those items, both bit for bit; the cells past a row's min(count, cap) terms are -1 /
        nan.  There is no predictions array of the explanation: the recommended predictions are the explained ones."""
        return self._recommend_explain_q("query", user, items, ratings, n, cap, order, predictor=predictor)

    def recommend_explain_with(self, user, items, ratings, n, cap, order=EXPLAIN_SUM_ORDER, predictor=PRED_KNN):
        """recommend_with and explain_with of its items in one pass (knncf_update_recommend_explain): as recommend_explain_for,
        for any user, of the fit or not"""
        return self._recommend_explain_q("update", user, items, ratings, n, cap, order, predictor=predictor)

    def recommend_explain_revised(self, user, removed, items, ratings, n, cap, order=EXPLAIN_SUM_ORDER, predictor=PRED_KNN):
        """recommend_revised and explain_revised of its items in one pass (knncf_revise_recommend_explain): as
        recommend_explain_for, on aug without the removed rows"""
        return self._recommend_explain_q("revise", user, items, ratings, n, cap, order, removed, predictor)

    def recommend_explain_for_batch(self, queries, n, cap, order=EXPLAIN_SUM_ORDER, predictor=PRED_KNN):
        """recommend_explain_for of every query: ([the recommend_explain_for tuple] per query, statuses).  A failed query has
        empty arrays, as in recommend_for_batch."""
        return self._recommend_explain_qb("query", queries, n, cap, order, predictor)

    def recommend_explain_with_batch(self, queries, n, cap, order=EXPLAIN_SUM_ORDER, predictor=PRED_KNN):
        """recommend_explain_with of every query: ([the recommend_explain_with tuple] per query, statuses)"""
        return self._recommend_explain_qb("update", queries, n, cap, order, predictor)

    def recommend_explain_revised_batch(self, queries, n, cap, order=EXPLAIN_SUM_ORDER, predictor=PRED_KNN):
        """recommend_explain_revised of every (user, removed_items, items, ratings): ([the tuple] per query, statuses)"""
        return self._recommend_explain_qb("revise", queries, n, cap, order, predictor)

    # ---- batch -------------------------------------------------------------------------
    def predict_batch(self, predictor, users, items):
        u, i = _i32(users), _i32(items)
        out = np.empty(len(u), dtype=np.float64)
        self._check(self._lib.knncf_predict_batch(self._h, predictor, u.ctypes.data_as(_i32p),
                                                  i.ctypes.data_as(_i32p), len(u), out.ctypes.data_as(_f64p)))
        return out

    def mae(self, predictor, users, items, ratings):
        u, i, r = _i32(users), _i32(items), _f64(ratings)
        v = C.c_double()
        self._check(self._lib.knncf_mae(self._h, predictor, u.ctypes.data_as(_i32p), i.ctypes.data_as(_i32p),
                                        r.ctypes.data_as(_f64p), len(u), C.byref(v)))
        return v.value

    def mae_device(self, predictor, users, items, ratings, pred_out=None):
        """Partial (sum |r - p|, count) over the rows this shard owns; tensors on the device."""
        s, c = C.c_double(), C.c_int64()
        p = _dev_ptr(pred_out, "float64") if pred_out is not None else None
        _producer_done(users)
        self._check(self._lib.knncf_mae_device(self._h, predictor, _dev_ptr(users, "int32"), _dev_ptr(items, "int32"),
                                               _dev_ptr(ratings, "float64"), users.numel(), C.byref(s), C.byref(c), p))
        return s.value, c.value

    def mae_sweep(self, ks, users, items, ratings, predictions=False):
        """MAE of PRED_KNN at every k of ks (strictly ascending) from one neighbour build (predict/kNN.scala:73):
        float64 [n_k]; with predictions=True also the per-row predictions [n_k, n].  The handle's k is unchanged and its
        neighbour memo dropped afterwards."""
        kk, u, i, r = _i32(ks), _i32(users), _i32(items), _f64(ratings)
        out = np.empty(len(kk), dtype=np.float64)
        per = np.empty((len(kk), len(u)), dtype=np.float64) if predictions else None
        self._check(self._lib.knncf_mae_sweep(self._h, kk.ctypes.data_as(_i32p), len(kk), u.ctypes.data_as(_i32p),
                                              i.ctypes.data_as(_i32p), r.ctypes.data_as(_f64p), len(u),
                                              out.ctypes.data_as(_f64p),
                                              per.ctypes.data_as(_f64p) if per is not None else None))
        return (out, per) if predictions else out

    def mae_sweep_device(self, ks, users, items, ratings, pred_out=None):
        """Per-k partial sums (sums[n_k], count) over the rows this shard owns; tensors on the device, pred_out [n_k, n]."""
        kk = _i32(ks)
        sums = np.zeros(len(kk), dtype=np.float64)
        c = C.c_int64()
        p = _dev_ptr(pred_out, "float64") if pred_out is not None else None
        _producer_done(users)
        self._check(self._lib.knncf_mae_sweep_device(self._h, kk.ctypes.data_as(_i32p), len(kk), _dev_ptr(users, "int32"),
                                                     _dev_ptr(items, "int32"), _dev_ptr(ratings, "float64"), users.numel(),
                                                     sums.ctypes.data_as(_f64p), C.byref(c), p))
        return sums, c.value

    # ---- sharding ----------------------------------------------------------------------
    def shard_view(self):
        v = ShardView()
        self._check(self._lib.knncf_shard_view_get(self._h, C.byref(v)))
        return v

    def shard_commit(self):
        self._check(self._lib.knncf_shard_commit(self._h))

    # ---- introspection -----------------------------------------------------------------
    def timings(self):
        t = Timings()
        self._check(self._lib.knncf_get_timings(self._h, C.byref(t)))
        return t.as_dict()

    def reset_timings(self):
        self._check(self._lib.knncf_reset_timings(self._h))

    def reset_neighbors(self):
        self._check(self._lib.knncf_reset_neighbors(self._h))

    def set_k(self, k):
        self._check(self._lib.knncf_set_k(self._h, k))
        self.k = k


class BystanderQueries:
    """Bystander queries (knncf_query_bystander_*, knncf_update_bystander_*, knncf_revise_bystander_*) on a fitted Engine: a FITTED
    user's kNN answers once the user of a fold-in query has joined the data (*_for), or a user that may be in the fit has added
    ratings (*_with) or has removed or re-rated items as well (*_with(..., removed=...)), without a refit.  A query is (user, items, ratings) as Engine.neighbors_for takes it; a row names the
    fitted user (`others`), the predict forms an item beside it (`pred_items`).  Read-only on the engine's handle: the
    neighbour lists and their build history stay as they were.

        by = BystanderQueries(engine)
        by.predict_for(944, items, ratings, [1], [1])"""

    def __init__(self, engine):
        self._e = engine

    @staticmethod
    def _row_ids(a, what):
        """validated 32-bit ids of the rows of a bystander query: ValueError before any C call"""
        x = np.asarray(a)
        if x.ndim != 1:
            raise ValueError(f"{what} must be 1-D")
        if len(x) == 0:
            return np.empty(0, dtype=np.int32)
        if x.dtype.kind not in "iu" or x.min() < -2**31 or x.max() >= 2**31:
            raise ValueError(f"{what} must be 32-bit integer ids")
        return _i32(x)

    @staticmethod
    def _row_cap(cap, k):
        if cap is None:
            cap = max(1, k)
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or cap < 0 or cap >= 2**31:
            raise ValueError("cap must be a non-negative integer")
        return int(cap)

    def _rows(self, B, others, pred_items):
        """the rows of a batched bystander call: (row_offsets, others, pred_items or None), one sequence per query"""
        oth = [self._row_ids(x, "others") for x in others]
        if len(oth) != B:
            raise ValueError("one others sequence per query")
        roff = np.zeros(B + 1, dtype=np.int64)
        roff[1:] = np.cumsum([len(x) for x in oth])
        if roff[-1] >= 2**31:
            raise ValueError("fewer than 2^31 rows per call")
        cat = lambda parts: np.ascontiguousarray(np.concatenate(parts) if parts else np.empty(0), dtype=np.int32)
        if pred_items is None:
            return roff, cat(oth), None
        pis = [self._row_ids(x, "pred_items") for x in pred_items]
        if len(pis) != B:
            raise ValueError("one pred_items sequence per query")
        if any(len(a) != len(b) for a, b in zip(oth, pis)):
            raise ValueError("others and pred_items must be of the same length")
        return roff, cat(oth), cat(pis)

    def _fn(self, fam, name):
        return getattr(self._e._lib, f"knncf_{fam}_bystander_{name}")

    def _neighbors(self, fam, user, items, ratings, others, cap, removed=None):
        q, it, rt = self._e._query_rows(user, items, ratings, allow_empty=fam != "query")
        rm = self._e._rm_args(fam, removed)
        oth = self._row_ids(others, "others")
        cap, m = self._row_cap(cap, self._e.k), len(oth)
        ids = np.empty((m, cap), dtype=np.int32)
        sims = np.empty((m, cap), dtype=np.float64)
        counts = np.zeros(m, dtype=np.int32)
        p = self._e._ptr
        self._e._check(self._fn(fam, "neighbors")(self._e._h, q, *rm, p(it, _i32p), p(rt, _f64p), len(it), p(oth, _i32p), m, cap,
                                                  p(ids.reshape(-1), _i32p), p(sims.reshape(-1), _f64p), p(counts, _i32p)))
        return [(ids[r, :min(counts[r], cap)].copy(), sims[r, :min(counts[r], cap)].copy()) for r in range(m)]

    def _predict(self, fam, user, items, ratings, others, pred_items, removed=None):
        q, it, rt = self._e._query_rows(user, items, ratings, allow_empty=fam != "query")
        rm = self._e._rm_args(fam, removed)
        oth, pi = self._row_ids(others, "others"), self._row_ids(pred_items, "pred_items")
        if len(oth) != len(pi):
            raise ValueError("others and pred_items must be of the same length")
        out = np.full(len(oth), np.nan, dtype=np.float64)
        p = self._e._ptr
        self._e._check(self._fn(fam, "predict")(self._e._h, PRED_KNN, q, *rm, p(it, _i32p), p(rt, _f64p), len(it), p(oth, _i32p),
                                                p(pi, _i32p), len(oth), p(out, _f64p)))
        return out

    def _neighbors_batch(self, fam, queries, others, cap):
        qargs, keep = self._e._batch_args(fam, queries)
        B = qargs[-1]
        roff, oth, _ = self._rows(B, others, None)
        cap, m = self._row_cap(cap, self._e.k), int(roff[-1])
        ids = np.empty((m, cap), dtype=np.int32)
        sims = np.empty((m, cap), dtype=np.float64)
        counts = np.zeros(m, dtype=np.int32)
        st = np.zeros(B, dtype=np.int32)
        p = self._e._ptr
        self._e._check(self._fn(fam, "neighbors_batch")(
            self._e._h, *qargs, p(roff, _i64p), p(oth, _i32p), cap, p(ids.reshape(-1), _i32p), p(sims.reshape(-1), _f64p),
            p(counts, _i32p), p(st, _i32p)))
        row = lambda r: (ids[r, :min(counts[r], cap)].copy(), sims[r, :min(counts[r], cap)].copy())
        return [[row(r) for r in range(roff[b], roff[b + 1])] for b in range(B)], st

    def _predict_batch(self, fam, queries, others, pred_items):
        qargs, keep = self._e._batch_args(fam, queries)
        B = qargs[-1]
        roff, oth, pi = self._rows(B, others, pred_items)
        out = np.full(int(roff[-1]), np.nan, dtype=np.float64)
        st = np.zeros(B, dtype=np.int32)
        p = self._e._ptr
        self._e._check(self._fn(fam, "predict_batch")(
            self._e._h, PRED_KNN, *qargs, p(roff, _i64p), p(oth, _i32p), p(pi, _i32p), p(out, _f64p), p(st, _i32p)))
        return [out[roff[b]:roff[b + 1]].copy() for b in range(B)], st

    def neighbors_for(self, user, items, ratings, others, cap=None):
        """getNeighbors(train ++ user's ratings, k, sim)(v) for every v of `others`, fitted users (or unknown ids) other than the
        newcomer `user`: [(ids, sims)] per row; the newcomer's own id where it is a neighbour"""
        return self._neighbors("query", user, items, ratings, others, cap)

    def predict_for(self, user, items, ratings, others, pred_items):
        """kNN predictions of (others[r], pred_items[r]) on train ++ user's ratings: a float64 array, one cell per row"""
        return self._predict("query", user, items, ratings, others, pred_items)

    def neighbors_for_batch(self, queries, others, cap=None):
        """neighbors_for of every (user, items, ratings) of `queries` with others[b] its rows:
        ([[(ids, sims)] per row] per query, statuses int32 [B]).  A failed query's rows have empty arrays."""
        return self._neighbors_batch("query", queries, others, cap)

    def predict_for_batch(self, queries, others, pred_items):
        """predict_for of every query; others / pred_items hold one sequence per query:
        ([float64 array] per query, statuses).  A failed query's array holds NaN."""
        return self._predict_batch("query", queries, others, pred_items)

    # the same four for a `user` that may be in the fit (knncf_update_bystander_*): the given rows are ADDITIONAL to its train
    # rows, as Engine.neighbors_with takes them, and may be empty for a fitted user.  With `removed` (knncf_revise_bystander_*) the
    # user also takes train items OUT, as Engine.neighbors_revised takes them: aug = train without the user's rows on the removed
    # items ++ the additional rows, and an item both removed and given again is re-rated.  removed=None is the update call itself;
    # a batch takes one sequence of removed items per query.  (The family is an argument and not four more methods: the public
    # methods of this class are the call kinds of the stateful model in tests/call_sequences.py.)
    def _revise_queries(self, queries, removed):
        """the (user, removed_items, items, ratings) of a batch whose queries are (user, items, ratings)"""
        queries, removed = list(queries), list(removed)
        if len(removed) != len(queries):
            raise ValueError("one removed sequence per query")
        for q in queries:
            if not isinstance(q, (tuple, list)) or len(q) != 3:
                raise ValueError("a query is (user, items, ratings)")
        return [(q[0], rm, q[1], q[2]) for q, rm in zip(queries, removed)]

    def neighbors_with(self, user, items, ratings, others, cap=None, removed=None):
        """getNeighbors(train ++ user's additional ratings, k, sim)(v) for every v of `others`: [(ids, sims)] per row; with
        `removed`, on train without the user's rows on those items ++ the additional ratings"""
        if removed is None:
            return self._neighbors("update", user, items, ratings, others, cap)
        return self._neighbors("revise", user, items, ratings, others, cap, removed)

    def predict_with(self, user, items, ratings, others, pred_items, removed=None):
        """kNN predictions of (others[r], pred_items[r]) on train ++ user's additional ratings: a float64 array; with `removed`,
        on train without the user's rows on those items ++ the additional ratings"""
        if removed is None:
            return self._predict("update", user, items, ratings, others, pred_items)
        return self._predict("revise", user, items, ratings, others, pred_items, removed)

    def neighbors_with_batch(self, queries, others, cap=None, removed=None):
        """neighbors_with of every query (removed: one sequence of removed items per query): ([[(ids, sims)] per row] per query,
        statuses)"""
        if removed is None:
            return self._neighbors_batch("update", queries, others, cap)
        return self._neighbors_batch("revise", self._revise_queries(queries, removed), others, cap)

    def predict_with_batch(self, queries, others, pred_items, removed=None):
        """predict_with of every query (removed: one sequence of removed items per query): ([float64 array] per query, statuses)"""
        if removed is None:
            return self._predict_batch("update", queries, others, pred_items)
        return self._predict_batch("revise", self._revise_queries(queries, removed), others, pred_items)


class Appends:
    """knncf_append and knncf_amend on a fitted Engine: new ratings go INTO the fit, and train rows come OUT of it.  NOT read-only
    on the engine's handle: the fit becomes train (without the removed rows) ++ the rows, the neighbour lists the call cannot
    change are kept and the other ones dropped.

        carried, dropped = Appends(engine).append(users, items, ratings)
        carried, dropped = Appends(engine).amend(removed_users, removed_items, users, items, ratings)"""

    def __init__(self, engine):
        self._e = engine

    @staticmethod
    def _ids(pair, what):
        """validated 32-bit ids of two 1-D arrays of one length: ValueError before any C call"""
        for a in pair:
            if a.ndim != 1 or len(a) != len(pair[0]):
                raise ValueError(f"{what} must be 1-D arrays of one length")
            if len(a) and (a.dtype.kind not in "iu" or a.min() < -2**31 or a.max() >= 2**31):
                raise ValueError(f"{what} must be 32-bit integer ids")
        return tuple(_i32(a) if len(a) else np.empty(0, dtype=np.int32) for a in pair)

    def _rows(self, users, items, ratings):
        u, i, r = np.asarray(users), np.asarray(items), np.asarray(ratings)
        if not (u.ndim == i.ndim == r.ndim == 1 and len(u) == len(i) == len(r)):
            raise ValueError("users, items and ratings must be 1-D arrays of one length")
        u, i = self._ids((u, i), "users and items")
        if len(r) and r.dtype.kind not in "iuf":
            raise ValueError("ratings must be numbers")
        return u, i, _f64(r) if len(r) else np.empty(0, dtype=np.float64)

    def _call(self, fn, front, rows, return_dropped):
        e = self._e
        u, i, r = rows
        carried, gone = C.c_int64(), C.c_int64()
        cap = e.num_users if return_dropped else 0  # (B ∩ S are users of the fit as it stands)
        ids = np.empty(max(1, cap), dtype=np.int32)
        p = e._ptr
        e._check(fn(e._h, *front, p(u, _i32p), p(i, _i32p), p(r, _f64p), len(u), C.byref(carried), C.byref(gone),
                    p(ids, _i32p) if cap else None, cap))
        if return_dropped:
            return carried.value, gone.value, ids[:gone.value].copy()
        return carried.value, gone.value

    def append(self, users, items, ratings, return_dropped=False):
        """knncf_append: the rows become part of the fit, and the neighbour lists they cannot change are kept.  Every later
        answer is that of fit(train ++ rows).  Returns (carried, dropped_count): the built lists that were kept, and those of the
        changers and of the users whose list holds a changer before or after, which the next call rebuilds; with return_dropped
        also their raw ids in the new fit's set order (int32 [dropped_count])."""
        rows = self._rows(users, items, ratings)
        return self._call(self._e._lib.knncf_append, (), rows, return_dropped)

    def amend(self, removed_users, removed_items, users, items, ratings, return_dropped=False):
        """knncf_amend: the train rows (removed_users[j], removed_items[j]) leave the fit and the rows join it, in one call; an
        item both removed and given again is re-rated.  Every later answer is that of fit(train without the removed rows ++ rows).
        Both parts may be empty.  Returns what append returns: (carried, dropped_count[, the dropped raw ids]), a user that left
        the fit standing among the dropped ids where its id would stand."""
        ru, ri = self._ids((np.asarray(removed_users), np.asarray(removed_items)), "removed_users and removed_items")
        rows = self._rows(users, items, ratings)
        p = self._e._ptr
        return self._call(self._e._lib.knncf_amend, (p(ru, _i32p), p(ri, _i32p), len(ru)), rows, return_dropped)


def remove_users(engine, users, return_dropped=False):
    """knncf_remove_users: the fitted users `users` leave the fit with every row they have; the neighbour lists that hold none of
    them are kept.  Every later answer is that of fit(train without those users' rows).  Returns what Appends.append returns:
    (carried, dropped_count[, the dropped raw ids]), a leaver that had a list standing among the dropped ids where its id would
    stand.  The ids are validated as Appends.amend validates its removals: ValueError before any C call.

    A module-level function on purpose, not a method of Engine or Appends: every public method of those classes has a kind in
    the tests' call-sequence model, which does not know this call yet."""
    (u,) = Appends._ids((np.asarray(users),), "users")
    e = engine
    carried, gone = C.c_int64(), C.c_int64()
    cap = e.num_users if return_dropped else 0  # (B ∩ S are users of the fit as it stands)
    ids = np.empty(max(1, cap), dtype=np.int32)
    e._check(e._lib.knncf_remove_users(e._h, e._ptr(u, _i32p), len(u), C.byref(carried), C.byref(gone),
                                       e._ptr(ids, _i32p) if cap else None, cap))
    if return_dropped:
        return carried.value, gone.value, ids[:gone.value].copy()
    return carried.value, gone.value


class EnteredQueries:
    """Entered queries (knncf_query_entered*, knncf_update_entered*, knncf_revise_entered*) on a fitted Engine: the FITTED users whose neighbour list the user of a fold-in
    query joins, without a refit.  A query is (user, items, ratings) as Engine.neighbors_for takes it.  NOT read-only on the
    engine's handle: a call first BUILDS THE NEIGHBOUR LISTS THAT ARE MISSING, all in one batch in ascending raw id, as
    Engine.neighbors_batch over those users would.

        users, sims, positions, displaced = EnteredQueries(engine).entered(944, items, ratings)"""

    def __init__(self, engine):
        self._e = engine

    @staticmethod
    def _cap(cap):
        if cap is None:
            return None
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or cap < 0 or cap >= 2**31:
            raise ValueError("cap must be a non-negative integer")
        return int(cap)

    def _call(self, qargs, B, cap):
        """one knncf_query_entered_batch call: (users, sims, positions, displaced) [B, cap], counts, statuses"""
        us = np.empty((B, cap), dtype=np.int32)
        sims = np.empty((B, cap), dtype=np.float64)
        pos = np.empty((B, cap), dtype=np.int32)
        disp = np.empty((B, cap), dtype=np.int32)
        counts = np.zeros(B, dtype=np.int32)
        st = np.zeros(B, dtype=np.int32)
        p = self._e._ptr
        self._e._check(self._e._lib.knncf_query_entered_batch(
            self._e._h, *qargs, cap, p(us.reshape(-1), _i32p), p(sims.reshape(-1), _f64p), p(pos.reshape(-1), _i32p),
            p(disp.reshape(-1), _i32p), p(counts, _i32p), p(st, _i32p)))
        return (us, sims, pos, disp), counts, st

    def entered_batch(self, queries, cap=None):
        """entered() of every (user, items, ratings) of `queries`: ([(users, sims, positions, displaced)] per query, statuses
        int32 [B]); a failed query has empty arrays.  cap=None asks for the counts first, then for all entries.  Builds the
        neighbour lists the handle has not built yet."""
        qargs, keep = self._e._batch_args("query", queries)
        B, cap = qargs[-1], self._cap(cap)
        if cap is None:
            _, counts, _ = self._call(qargs, B, 0)
            cap = int(counts.max()) if B else 0
        out, counts, st = self._call(qargs, B, cap)
        return [tuple(a[b, :min(counts[b], cap)].copy() for a in out) for b in range(B)], st

    def entered(self, user, items, ratings, cap=None):
        """the fitted users v with `user` in getNeighbors(train ++ user's ratings, k, sim)(v), in the fit's set order:
        (users, sims = S(v, user), positions of `user` in v's list, displaced = the raw id that leaves v's list or -1).
        cap=None asks for the count first, then for all entries.  Builds the neighbour lists the handle has not built yet."""
        q, it, rt = self._e._query_rows(user, items, ratings)
        cap = self._cap(cap)
        p = self._e._ptr

        def call(cap):
            us = np.empty(cap, dtype=np.int32)
            sims = np.empty(cap, dtype=np.float64)
            pos = np.empty(cap, dtype=np.int32)
            disp = np.empty(cap, dtype=np.int32)
            c = C.c_int32()
            self._e._check(self._e._lib.knncf_query_entered(self._e._h, q, p(it, _i32p), p(rt, _f64p), len(it), cap, p(us, _i32p),
                                                            p(sims, _f64p), p(pos, _i32p), p(disp, _i32p), C.byref(c)))
            m = min(c.value, cap)
            return (us[:m].copy(), sims[:m].copy(), pos[:m].copy(), disp[:m].copy()), c.value

        if cap is None:
            cap = call(0)[1]
        return call(cap)[0]

    # entered_with* take `removed` as BystanderQueries.*_with do: removed=None is the update call itself (knncf_update_entered*);
    # otherwise the user also takes train items OUT (knncf_revise_entered*), one sequence of removed items per query in the batch
    # form.  (A keyword and not two more methods: the public methods of this class are call kinds of tests/call_sequences.py.)
    def _call_with(self, qargs, B, cap, fam="update"):
        """one knncf_update_entered_batch / knncf_revise_entered_batch call: (users, sims, positions, previous, other) [B, cap],
        counts, statuses"""
        out = (np.empty((B, cap), dtype=np.int32), np.empty((B, cap), dtype=np.float64), np.empty((B, cap), dtype=np.int32),
               np.empty((B, cap), dtype=np.int32), np.empty((B, cap), dtype=np.int32))
        counts = np.zeros(B, dtype=np.int32)
        st = np.zeros(B, dtype=np.int32)
        p = self._e._ptr
        self._e._check(getattr(self._e._lib, f"knncf_{fam}_entered_batch")(
            self._e._h, *qargs, cap, *(p(a.reshape(-1), _f64p if a.dtype == np.float64 else _i32p) for a in out), p(counts, _i32p),
            p(st, _i32p)))
        return out, counts, st

    def entered_with_batch(self, queries, cap=None, removed=None):
        """entered_with() of every (user, items, ratings) of `queries` (removed: one sequence of removed items per query):
        ([(users, sims, positions, previous, other)] per query, statuses int32 [B]); a failed query has empty arrays.  cap=None
        asks for the counts first, then for all entries."""
        fam = "update" if removed is None else "revise"
        if removed is not None:
            queries = BystanderQueries._revise_queries(None, queries, removed)
        qargs, keep = self._e._batch_args(fam, queries)
        B, cap = qargs[-1], self._cap(cap)
        if cap is None:
            _, counts, _ = self._call_with(qargs, B, 0, fam)
            cap = int(counts.max()) if B else 0
        out, counts, st = self._call_with(qargs, B, cap, fam)
        return [tuple(a[b, :min(counts[b], cap)].copy() for a in out) for b in range(B)], st

    def entered_with(self, user, items, ratings, cap=None, removed=None):
        """knncf_update_entered: `user` may be IN the fit and (items, ratings) are its ADDITIONAL ratings.  The fitted users v
        whose kNN list holds `user` on train or on train ++ those ratings, in the fit's set order: (users, sims = S(v, user) on
        aug, positions of `user` in v's list on aug or -1 if it left, previous = its position on train or -1 if it entered,
        other = the raw id that left the list (entered) or came into it (left), else -1).  cap=None asks for the count first.
        With `removed` (knncf_revise_entered) aug is train without the user's rows on those items ++ the additional ratings."""
        q, it, rt = self._e._query_rows(user, items, ratings, allow_empty=True)
        fam = "update" if removed is None else "revise"
        rm = self._e._rm_args(fam, removed)
        cap = self._cap(cap)
        p = self._e._ptr

        def call(cap):
            us, pos, prev, other = (np.empty(cap, dtype=np.int32) for _ in range(4))
            sims = np.empty(cap, dtype=np.float64)
            c = C.c_int32()
            fn = getattr(self._e._lib, f"knncf_{fam}_entered")
            self._e._check(fn(self._e._h, q, *rm, p(it, _i32p), p(rt, _f64p), len(it), cap, p(us, _i32p), p(sims, _f64p), p(pos, _i32p),
                              p(prev, _i32p), p(other, _i32p), C.byref(c)))
            m = min(c.value, cap)
            return (us[:m].copy(), sims[:m].copy(), pos[:m].copy(), prev[:m].copy(), other[:m].copy()), c.value

        if cap is None:
            cap = call(0)[1]
        return call(cap)[0]


class Group:
    """knncf_group_*: one process, several GPUs — n shard handles + RCCL communicators (ncclCommInitAll) inside the library;
    fit = every shard's fit + ncclAllGather of the (mean, norm) segments + commit, mae = every shard's partial sums +
    ncclAllReduce.  What a JVM binds; here the ctypes mirror for the tests."""

    def __init__(self, devices, k=300, similarity=SIM_COSINE, flags=0, head_items=0, workspace_bytes=0):
        self._lib = load_library()
        _share_rccl_with_torch()
        devs = _i32(devices)
        cfg = Config(C.sizeof(Config), 0, k, similarity, 0, 1, workspace_bytes, flags, head_items)
        g = C.c_void_p()
        st = self._lib.knncf_group_create(C.byref(cfg), devs.ctypes.data_as(_i32p), len(devs), C.byref(g))
        if st != OK:
            raise KnncfError(st, self._lib.knncf_status_string(st).decode())
        self._g = g
        self.k = k
        self.size = len(devs)

    def close(self):
        if getattr(self, "_g", None):
            self._lib.knncf_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != OK:
            raise KnncfError(st, self._lib.knncf_group_last_error(self._g).decode())

    def fit(self, users, items, ratings):
        u, i, r = _i32(users), _i32(items), _f64(ratings)
        self._check(self._lib.knncf_group_fit(self._g, u.ctypes.data_as(_i32p), i.ctypes.data_as(_i32p), r.ctypes.data_as(_f64p), len(u)))
        return self

    def mae(self, predictor, users, items, ratings):
        u, i, r = _i32(users), _i32(items), _f64(ratings)
        v = C.c_double()
        self._check(self._lib.knncf_group_mae(self._g, predictor, u.ctypes.data_as(_i32p), i.ctypes.data_as(_i32p),
                                              r.ctypes.data_as(_f64p), len(u), C.byref(v)))
        return v.value

    def predict_batch(self, predictor, users, items):
        u, i = _i32(users), _i32(items)
        out = np.empty(len(u), dtype=np.float64)
        self._check(self._lib.knncf_group_predict_batch(self._g, predictor, u.ctypes.data_as(_i32p), i.ctypes.data_as(_i32p),
                                                        len(u), out.ctypes.data_as(_f64p)))
        return out

    def shard(self, rank):
        """the shard handle of `rank` as a borrowed Engine (queries, timings); owned by the group"""
        h = C.c_void_p()
        self._check(self._lib.knncf_group_handle(self._g, rank, C.byref(h)))
        e = Engine.__new__(Engine)
        e._lib, e._h, e.device, e.k = self._lib, h, None, self.k
        e.close = lambda: None  # borrowed
        return e
