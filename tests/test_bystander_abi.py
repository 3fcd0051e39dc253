"""Bystander query entry points (knncf_query_bystander_*: a fitted user's answers once a newcomer has joined) at the C boundary
and in the binding, without a GPU: the four symbols are declared, exported and listed in EXPORTS with the documented argument
types, a null handle gets KNNCF_E_INVALID, and the Python wrappers (BystanderQueries) reject ragged input before any C call."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("knncf_query_bystander_neighbors", "knncf_query_bystander_predict",
         "knncf_query_bystander_neighbors_batch", "knncf_query_bystander_predict_batch")
i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def kn(pkg):
    importlib.import_module(pkg.__name__ + ".build").build()
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def test_declared_exported_and_listed(kn):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "knncf.h")).read(), flags=re.S)
    lib = kn.load_library()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name), name
        assert name in kn.EXPORTS, name


def test_argtypes(kn):
    lib = kn.load_library()
    h, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    query = [i32, i32p, f64p, i64]           # user, items, ratings, n_ratings
    batch = [i32p, i64p, i32p, f64p, i64]    # users, offsets, items, ratings, n_queries
    assert lib.knncf_query_bystander_neighbors.argtypes == [h] + query + [i32p, i64, i32, i32p, f64p, i32p]
    assert lib.knncf_query_bystander_predict.argtypes == [h, C.c_int] + query + [i32p, i32p, i64, f64p]
    assert lib.knncf_query_bystander_neighbors_batch.argtypes == [h] + batch + [i64p, i32p, i32, i32p, f64p, i32p, i32p]
    assert lib.knncf_query_bystander_predict_batch.argtypes == [h, C.c_int] + batch + [i64p, i32p, i32p, f64p, i32p]
    # the query part is the fold-in calls'
    assert lib.knncf_query_bystander_predict.argtypes[:6] == lib.knncf_query_predict.argtypes[:6]
    assert lib.knncf_query_bystander_predict_batch.argtypes[:8] == lib.knncf_query_predict_batch.argtypes[:8]


def test_null_handle(kn):
    lib = kn.load_library()
    us = np.array([5], dtype=np.int32)
    off = np.array([0, 2], dtype=np.int64)
    its = np.array([1, 2], dtype=np.int32)
    rts = np.array([3.0, 4.0])
    oth = np.array([7, 8], dtype=np.int32)
    ids = np.empty(4, dtype=np.int32)
    out = np.empty(4, dtype=np.float64)
    cnt = np.zeros(2, dtype=np.int32)
    st = np.zeros(1, dtype=np.int32)
    p = lambda a, t: a.ctypes.data_as(t)
    assert lib.knncf_query_bystander_neighbors(None, 5, p(its, i32p), p(rts, f64p), 2, p(oth, i32p), 2, 2, p(ids, i32p), p(out, f64p),
                                               p(cnt, i32p)) == kn.E_INVALID
    assert lib.knncf_query_bystander_predict(None, kn.PRED_KNN, 5, p(its, i32p), p(rts, f64p), 2, p(oth, i32p), p(its, i32p), 2,
                                             p(out, f64p)) == kn.E_INVALID
    q = (p(us, i32p), p(off, i64p), p(its, i32p), p(rts, f64p), 1)
    assert lib.knncf_query_bystander_neighbors_batch(None, *q, p(off, i64p), p(oth, i32p), 2, p(ids, i32p), p(out, f64p), p(cnt, i32p),
                                                     p(st, i32p)) == kn.E_INVALID
    assert lib.knncf_query_bystander_predict_batch(None, kn.PRED_KNN, *q, p(off, i64p), p(oth, i32p), p(its, i32p), p(out, f64p),
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
    lambda e: e.neighbors_for(5, [1, 2], [3.0], [7]),                         # lengths of the query differ
    lambda e: e.neighbors_for(5, [], [], [7]),                                # an empty query
    lambda e: e.neighbors_for(5, [1], [3.0], [[7]]),                          # 2-D others
    lambda e: e.neighbors_for(5, [1], [3.0], [7.5]),                          # non-integer bystander
    lambda e: e.neighbors_for(5, [1], [3.0], [2**31]),                        # bystander beyond int32
    lambda e: e.neighbors_for(5, [1], [3.0], [7], cap=-1),
    lambda e: e.neighbors_for(5.5, [1], [3.0], [7]),                          # non-integer user
    lambda e: e.predict_for(5, [1], [3.0], [7, 8], [1]),                      # others and pred_items differ in length
    lambda e: e.predict_for(5, [1], [3.0], [7], [[1]]),                       # 2-D pred_items
    lambda e: e.predict_for(5, [1], [3.0], [7], [1.5]),                       # non-integer item
    lambda e: e.predict_for(5, [1.5], [3.0], [7], [1]),
    lambda e: e.neighbors_for_batch([GOOD, GOOD], [[7]]),                     # one others sequence per query
    lambda e: e.neighbors_for_batch([GOOD], [[[7]]]),                         # 2-D others
    lambda e: e.neighbors_for_batch([GOOD], [[7.5]]),
    lambda e: e.neighbors_for_batch([GOOD], [[7]], cap=-1),
    lambda e: e.neighbors_for_batch([GOOD, (6, [1, 2], [3.0])], [[7], [8]]),  # a ragged query
    lambda e: e.predict_for_batch([GOOD, GOOD], [[7]], [[1], [1]]),           # one others sequence per query
    lambda e: e.predict_for_batch([GOOD, GOOD], [[7], [8]], [[1]]),           # one pred_items sequence per query
    lambda e: e.predict_for_batch([GOOD], [[7, 8]], [[1]]),                   # lengths differ inside a query
    lambda e: e.predict_for_batch([GOOD], [[7]], [[1.5]]),
    lambda e: e.predict_for_batch([GOOD], [[7]], [[[1]]]),
])
def test_wrappers_reject_ragged_input(engine, call):
    with pytest.raises(ValueError):
        call(engine)
