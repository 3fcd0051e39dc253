"""Update query entry points (knncf_update_*: a user of the fit with additional ratings) at the C boundary and in the binding,
without a GPU: the six symbols are declared, exported and listed in EXPORTS, a null handle gets KNNCF_E_INVALID, and the
Python wrappers reject ragged input before any C call."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("knncf_update_neighbors", "knncf_update_predict", "knncf_update_recommend",
         "knncf_update_neighbors_batch", "knncf_update_predict_batch", "knncf_update_recommend_batch")


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
        # the argument list is the fold-in call's
        assert getattr(lib, name).argtypes == getattr(lib, name.replace("_update_", "_query_")).argtypes, name


def test_null_handle(kn):
    lib = kn.load_library()
    us = np.array([5], dtype=np.int32)
    off = np.array([0, 2], dtype=np.int64)
    its = np.array([1, 2], dtype=np.int32)
    rts = np.array([3.0, 4.0])
    ids = np.empty(2, dtype=np.int32)
    out = np.empty(2, dtype=np.float64)
    cnt = np.zeros(1, dtype=np.int32)
    st = np.zeros(1, dtype=np.int32)
    c = C.c_int32()
    i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    p = lambda a, t: a.ctypes.data_as(t)
    assert lib.knncf_update_neighbors(None, 5, p(its, i32p), p(rts, f64p), 2, 2, p(ids, i32p), p(out, f64p), C.byref(c)) == kn.E_INVALID
    assert lib.knncf_update_predict(None, kn.PRED_KNN, 5, p(its, i32p), p(rts, f64p), 2, p(its, i32p), 2, p(out, f64p)) == kn.E_INVALID
    assert lib.knncf_update_recommend(None, kn.PRED_KNN, 5, p(its, i32p), p(rts, f64p), 2, 2, p(ids, i32p), p(out, f64p),
                                      C.byref(c)) == kn.E_INVALID
    q = (p(us, i32p), p(off, i64p), p(its, i32p), p(rts, f64p), 1)
    assert lib.knncf_update_neighbors_batch(None, *q, 2, p(ids, i32p), p(out, f64p), p(cnt, i32p), p(st, i32p)) == kn.E_INVALID
    assert lib.knncf_update_predict_batch(None, kn.PRED_KNN, *q, p(off, i64p), p(its, i32p), p(out, f64p), p(st, i32p)) == kn.E_INVALID
    assert lib.knncf_update_recommend_batch(None, kn.PRED_KNN, *q, 2, p(ids, i32p), p(out, f64p), p(cnt, i32p),
                                            p(st, i32p)) == kn.E_INVALID


class _NoCalls:
    def __getattr__(self, name):
        raise AssertionError(f"C entry point {name} called with bad arguments")


@pytest.fixture
def engine(kn):
    e = kn.Engine.__new__(kn.Engine)  # no device: every C call would fail loudly
    e._lib, e._h, e.k, e.device = _NoCalls(), None, 10, 0
    return e


GOOD = (5, [1, 2], [3.0, 4.0])


@pytest.mark.parametrize("call", [
    lambda e: e.neighbors_with(5, [1, 2], [3.0]),                           # lengths differ
    lambda e: e.neighbors_with(5, [[1]], [[3.0]]),                          # 2-D arrays
    lambda e: e.neighbors_with(5, [1], [3.0], cap=-1),
    lambda e: e.neighbors_with(5.5, [1], [3.0]),                            # non-integer user
    lambda e: e.predict_with(5, [1.5], [3.0], [1]),                         # non-integer item
    lambda e: e.predict_with(5, [1], [3.0], [[1]]),
    lambda e: e.recommend_with(5, [1], ["x"], 3),
    lambda e: e.recommend_with(5, [1], [3.0], -1),
    lambda e: e.recommend_with(5, [], [3.0], 3),                            # empty items beside one rating
    lambda e: e.neighbors_with_batch([GOOD, (6, [1, 2], [3.0])]),           # lengths differ
    lambda e: e.neighbors_with_batch([GOOD, (6, [[1]], [[3.0]])]),          # 2-D arrays
    lambda e: e.neighbors_with_batch([GOOD], cap=-1),
    lambda e: e.neighbors_with_batch([GOOD, (6.5, [1], [3.0])]),            # non-integer user
    lambda e: e.neighbors_with_batch([GOOD, (2**31, [1], [3.0])]),          # user beyond int32
    lambda e: e.neighbors_with_batch([GOOD, (6, [1.5], [3.0])]),            # non-integer item
    lambda e: e.neighbors_with_batch([GOOD, (6, [1])]),                     # not a (user, items, ratings) triple
    lambda e: e.predict_with_batch([GOOD, GOOD], [[1]]),                    # one pred_items sequence per query
    lambda e: e.predict_with_batch([GOOD], [[[1]]]),
    lambda e: e.predict_with_batch([GOOD], [[1.5]]),
    lambda e: e.recommend_with_batch([GOOD], -1),
    lambda e: e.recommend_with_batch([GOOD, (6, [1], ["x"])], 3),
    lambda e: e.recommend_with_batch([GOOD, (6, [2**31], [3.0])], 3),
    lambda e: e.recommend_with_batch([GOOD, (6, [1, 2], [[3.0, 4.0]])], 3),  # ratings 2-D
])
def test_wrappers_reject_ragged_input(engine, call):
    with pytest.raises(ValueError):
        call(engine)
