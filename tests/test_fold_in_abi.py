"""Fold-in query entry points at the C boundary and in the binding, without a GPU: the three symbols are declared and
exported, a null handle gets KNNCF_E_INVALID like every other entry point, and the Python wrappers reject bad arguments
before any C call."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("knncf_query_neighbors", "knncf_query_predict", "knncf_query_recommend")


@pytest.fixture(scope="module")
def kn(pkg):
    importlib.import_module(pkg.__name__ + ".build").build()
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def test_declared_and_exported(kn):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "knncf.h")).read(), flags=re.S)
    lib = kn.load_library()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name), name


def test_null_handle(kn):
    lib = kn.load_library()
    its = np.array([1, 2], dtype=np.int32)
    rts = np.array([3.0, 4.0])
    ids = np.empty(2, dtype=np.int32)
    out = np.empty(2, dtype=np.float64)
    c = C.c_int32()
    i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    p = lambda a, t: a.ctypes.data_as(t)
    assert lib.knncf_query_neighbors(None, 5, p(its, i32p), p(rts, f64p), 2, 2, p(ids, i32p), p(out, f64p), C.byref(c)) == kn.E_INVALID
    assert lib.knncf_query_predict(None, kn.PRED_KNN, 5, p(its, i32p), p(rts, f64p), 2, p(its, i32p), 2, p(out, f64p)) == kn.E_INVALID
    assert lib.knncf_query_recommend(None, kn.PRED_KNN, 5, p(its, i32p), p(rts, f64p), 2, 2, p(ids, i32p), p(out, f64p),
                                     C.byref(c)) == kn.E_INVALID


class _NoCalls:
    def __getattr__(self, name):
        raise AssertionError(f"C entry point {name} called with bad arguments")


@pytest.fixture
def engine(kn):
    e = kn.Engine.__new__(kn.Engine)  # no device: every C call would fail loudly
    e._lib, e._h, e.k, e.device = _NoCalls(), None, 10, 0
    return e


@pytest.mark.parametrize("call", [
    lambda e: e.neighbors_for(5, [1, 2], [3.0]),             # lengths differ
    lambda e: e.neighbors_for(5, [], []),                    # empty query
    lambda e: e.neighbors_for(5.5, [1], [3.0]),              # non-integer user
    lambda e: e.neighbors_for(2**31, [1], [3.0]),            # user beyond int32
    lambda e: e.neighbors_for(5, [1.5], [3.0]),              # non-integer item
    lambda e: e.neighbors_for(5, [[1]], [[3.0]]),            # not 1-D
    lambda e: e.neighbors_for(5, [1], [3.0], cap=-1),
    lambda e: e.predict_for(5, [1], [3.0], [[1]]),
    lambda e: e.predict_for(5, [1], [3.0], [1.5]),
    lambda e: e.recommend_for(5, [1], [3.0], -1),
    lambda e: e.recommend_for(5, [1], ["x"], 3),
    lambda e: e.recommend_for(5, [2**31], [3.0], 3),
])
def test_wrappers_reject_bad_arguments(engine, call):
    with pytest.raises(ValueError):
        call(engine)
