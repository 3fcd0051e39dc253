"""The entry points of knncf_revise_bystander_* (a fitted user's answers once another user has removed or re-rated items) at the
C boundary and in the binding, without a GPU: the four symbols are declared, exported and listed in EXPORTS with the documented
argument types, a null handle gets KNNCF_E_INVALID, and the Python wrappers
(BystanderQueries.*_with(..., removed=...)) reject ragged input before any C call."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("knncf_revise_bystander_neighbors", "knncf_revise_bystander_predict",
         "knncf_revise_bystander_neighbors_batch", "knncf_revise_bystander_predict_batch")
i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def kn(pkg):
    importlib.import_module(pkg.__name__ + ".build").build()
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def test_declared_exported_and_listed(kn):
    raw = open(os.path.join(ROOT, "include", "knncf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = kn.load_library()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name), name
        assert name in kn.EXPORTS, name
    assert "Bystanders of revise queries" in raw and "bystander-revise slots=" in raw
    assert "revise queries: not\n * served" not in raw  # the sentences this lifts


def test_argtypes(kn):
    lib = kn.load_library()
    h, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    query = [i32, i32p, i64, i32p, f64p, i64]           # user, removed_items, n_removed, items, ratings, n_ratings
    batch = [i32p, i64p, i32p, i64p, i32p, f64p, i64]   # users, removed_offsets, removed_items, offsets, items, ratings, n_queries
    assert lib.knncf_revise_bystander_neighbors.argtypes == [h] + query + [i32p, i64, i32, i32p, f64p, i32p]
    assert lib.knncf_revise_bystander_predict.argtypes == [h, C.c_int] + query + [i32p, i32p, i64, f64p]
    assert lib.knncf_revise_bystander_neighbors_batch.argtypes == [h] + batch + [i64p, i32p, i32, i32p, f64p, i32p, i32p]
    assert lib.knncf_revise_bystander_predict_batch.argtypes == [h, C.c_int] + batch + [i64p, i32p, i32p, f64p, i32p]
    # the query part is the revise calls', the row part the update-bystander calls'
    assert lib.knncf_revise_bystander_predict.argtypes[:8] == lib.knncf_revise_predict.argtypes[:8]
    assert lib.knncf_revise_bystander_predict_batch.argtypes[:10] == lib.knncf_revise_predict_batch.argtypes[:10]
    assert lib.knncf_revise_bystander_neighbors.argtypes[7:] == lib.knncf_update_bystander_neighbors.argtypes[5:]
    assert lib.knncf_revise_bystander_predict_batch.argtypes[9:] == lib.knncf_update_bystander_predict_batch.argtypes[7:]


def test_null_handle(kn):
    lib = kn.load_library()
    us = np.array([5], dtype=np.int32)
    off = np.array([0, 2], dtype=np.int64)
    roff = np.array([0, 1], dtype=np.int64)
    its = np.array([1, 2], dtype=np.int32)
    rm = np.array([3], dtype=np.int32)
    rts = np.array([3.0, 4.0])
    oth = np.array([7, 8], dtype=np.int32)
    ids = np.empty(4, dtype=np.int32)
    out = np.empty(4, dtype=np.float64)
    cnt = np.zeros(2, dtype=np.int32)
    st = np.zeros(1, dtype=np.int32)
    p = lambda a, t: a.ctypes.data_as(t)
    assert lib.knncf_revise_bystander_neighbors(None, 5, p(rm, i32p), 1, p(its, i32p), p(rts, f64p), 2, p(oth, i32p), 2, 2, p(ids, i32p),
                                                p(out, f64p), p(cnt, i32p)) == kn.E_INVALID
    assert lib.knncf_revise_bystander_predict(None, kn.PRED_KNN, 5, p(rm, i32p), 1, p(its, i32p), p(rts, f64p), 2, p(oth, i32p),
                                              p(its, i32p), 2, p(out, f64p)) == kn.E_INVALID
    q = (p(us, i32p), p(roff, i64p), p(rm, i32p), p(off, i64p), p(its, i32p), p(rts, f64p), 1)
    assert lib.knncf_revise_bystander_neighbors_batch(None, *q, p(off, i64p), p(oth, i32p), 2, p(ids, i32p), p(out, f64p), p(cnt, i32p),
                                                      p(st, i32p)) == kn.E_INVALID
    assert lib.knncf_revise_bystander_predict_batch(None, kn.PRED_KNN, *q, p(off, i64p), p(oth, i32p), p(its, i32p), p(out, f64p),
                                                    p(st, i32p)) == kn.E_INVALID


class _NoCalls:
    def __getattr__(self, name):
        raise AssertionError(f"C entry point {name} called with bad arguments")


@pytest.fixture
def engine(kn):
    e = kn.Engine.__new__(kn.Engine)  # no device: every C call would fail loudly
    e._lib, e._h, e.k, e.device = _NoCalls(), None, 10, 0
    return kn.BystanderQueries(e)


GOOD = (5, [1, 2], [3.0, 4.0])


@pytest.mark.parametrize("call", [
    lambda e: e.neighbors_with(5, [1, 2], [3.0], [7], removed=[9]),                     # lengths of the query differ
    lambda e: e.neighbors_with(5, [1], [3.0], [7], removed=[[9]]),                      # 2-D removed items
    lambda e: e.neighbors_with(5, [1], [3.0], [7], removed=[9.5]),                      # non-integer removed item
    lambda e: e.neighbors_with(5, [1], [3.0], [7], removed=[2**31]),                    # removed item beyond int32
    lambda e: e.neighbors_with(5, [1], [3.0], [[7]], removed=[9]),                      # 2-D others
    lambda e: e.neighbors_with(5, [1], [3.0], [7.5], removed=[9]),                      # non-integer bystander
    lambda e: e.neighbors_with(5, [1], [3.0], [7], cap=-1, removed=[9]),
    lambda e: e.neighbors_with(5.5, [1], [3.0], [7], removed=[9]),                      # non-integer user
    lambda e: e.predict_with(5, [1], [3.0], [7, 8], [1], removed=[9]),                  # others and pred_items differ in length
    lambda e: e.predict_with(5, [1], [3.0], [7], [1.5], removed=[9]),                   # non-integer item
    lambda e: e.predict_with(5, [1], [3.0], [7], [1], removed=[9.5]),
    lambda e: e.neighbors_with_batch([GOOD, GOOD], [[7]], removed=[[9], [9]]),          # one others sequence per query
    lambda e: e.neighbors_with_batch([GOOD, GOOD], [[7], [8]], removed=[[9]]),          # one removed sequence per query
    lambda e: e.neighbors_with_batch([(5, [9], [1, 2], [3.0, 4.0])], [[7]], removed=[[9]]),  # the removals inside the query
    lambda e: e.neighbors_with_batch([GOOD], [[7]], removed=[[[9]]]),                   # 2-D removed items
    lambda e: e.neighbors_with_batch([GOOD], [[7]], cap=-1, removed=[[9]]),
    lambda e: e.neighbors_with_batch([GOOD, (6, [1, 2], [3.0])], [[7], [8]], removed=[[9], []]),  # a ragged query
    lambda e: e.predict_with_batch([GOOD, GOOD], [[7], [8]], [[1]], removed=[[9], [9]]),  # one pred_items sequence per query
    lambda e: e.predict_with_batch([GOOD], [[7, 8]], [[1]], removed=[[9]]),             # lengths differ inside a query
    lambda e: e.predict_with_batch([GOOD], [[7]], [[1.5]], removed=[[9]]),
    lambda e: e.predict_with_batch([GOOD], [[7]], [[1]], removed=[[9.5]]),
])
def test_wrappers_reject_ragged_input(engine, call):
    with pytest.raises(ValueError):
        call(engine)

