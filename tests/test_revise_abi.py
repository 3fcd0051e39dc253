"""Revise query entry points (knncf_revise_*: a user of the fit who removed or re-rated items) at the C boundary and in the
binding, without a GPU: the six symbols are declared, exported and listed in EXPORTS, a null handle gets KNNCF_E_INVALID, and
the Python wrappers reject ragged input before any C call."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("knncf_revise_neighbors", "knncf_revise_predict", "knncf_revise_recommend",
         "knncf_revise_neighbors_batch", "knncf_revise_predict_batch", "knncf_revise_recommend_batch")


@pytest.fixture(scope="module")
def kn(pkg):
    importlib.import_module(pkg.__name__ + ".build").build()
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def test_declared_exported_and_listed(kn):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "knncf.h")).read(), flags=re.S)
    lib = kn.load_library()
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name), name
        assert name in kn.EXPORTS, name
        # the argument list is the update call's with the removals in front of the additional rows
        base = getattr(lib, name.replace("_revise_", "_update_")).argtypes
        at = 2 if "neighbors" in name else 3  # behind (handle, [predictor,] user / users)
        extra = [i64p, i32p] if name.endswith("_batch") else [i32p, C.c_int64]
        assert getattr(lib, name).argtypes == base[:at] + extra + base[at:], name
    # ... and so says the header: the removals stand right before the additional rows
    for name in NAMES:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text).group(1)
        args = [a.strip() for a in decl.replace("\n", " ").split(",")]
        first = "const int64_t* removed_offsets" if name.endswith("_batch") else "const int32_t* removed_items"
        second = "const int32_t* removed_items" if name.endswith("_batch") else "int64_t n_removed"
        at = args.index(first)
        assert args[at + 1] == second, name
        assert args[at + 2] == ("const int64_t* offsets" if name.endswith("_batch") else "const int32_t* items"), name


def test_null_handle(kn):
    lib = kn.load_library()
    us = np.array([5], dtype=np.int32)
    off = np.array([0, 2], dtype=np.int64)
    roff = np.array([0, 1], dtype=np.int64)
    its = np.array([1, 2], dtype=np.int32)
    rm = np.array([7], dtype=np.int32)
    rts = np.array([3.0, 4.0])
    ids = np.empty(2, dtype=np.int32)
    out = np.empty(2, dtype=np.float64)
    cnt = np.zeros(1, dtype=np.int32)
    st = np.zeros(1, dtype=np.int32)
    c = C.c_int32()
    i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    p = lambda a, t: a.ctypes.data_as(t)
    one = (p(rm, i32p), 1, p(its, i32p), p(rts, f64p), 2)
    assert lib.knncf_revise_neighbors(None, 5, *one, 2, p(ids, i32p), p(out, f64p), C.byref(c)) == kn.E_INVALID
    assert lib.knncf_revise_predict(None, kn.PRED_KNN, 5, *one, p(its, i32p), 2, p(out, f64p)) == kn.E_INVALID
    assert lib.knncf_revise_recommend(None, kn.PRED_KNN, 5, *one, 2, p(ids, i32p), p(out, f64p), C.byref(c)) == kn.E_INVALID
    q = (p(us, i32p), p(roff, i64p), p(rm, i32p), p(off, i64p), p(its, i32p), p(rts, f64p), 1)
    assert lib.knncf_revise_neighbors_batch(None, *q, 2, p(ids, i32p), p(out, f64p), p(cnt, i32p), p(st, i32p)) == kn.E_INVALID
    assert lib.knncf_revise_predict_batch(None, kn.PRED_KNN, *q, p(off, i64p), p(its, i32p), p(out, f64p), p(st, i32p)) == kn.E_INVALID
    assert lib.knncf_revise_recommend_batch(None, kn.PRED_KNN, *q, 2, p(ids, i32p), p(out, f64p), p(cnt, i32p),
                                            p(st, i32p)) == kn.E_INVALID


class _NoCalls:
    def __getattr__(self, name):
        raise AssertionError(f"C entry point {name} called with bad arguments")


@pytest.fixture
def engine(kn):
    e = kn.Engine.__new__(kn.Engine)  # no device: every C call would fail loudly
    e._lib, e._h, e.k, e.device = _NoCalls(), None, 10, 0
    return e


GOOD = (5, [7], [1, 2], [3.0, 4.0])


@pytest.mark.parametrize("call", [
    lambda e: e.neighbors_revised(5, [[7]], [1], [3.0]),                       # removed 2-D
    lambda e: e.neighbors_revised(5, [7.5], [1], [3.0]),                       # non-integer removed item
    lambda e: e.neighbors_revised(5, [2**31], [1], [3.0]),                     # removed item beyond int32
    lambda e: e.neighbors_revised(5, [7], [1, 2], [3.0]),                      # lengths differ
    lambda e: e.neighbors_revised(5, [7], [1], [3.0], cap=-1),
    lambda e: e.neighbors_revised(5.5, [7], [1], [3.0]),                       # non-integer user
    lambda e: e.predict_revised(5, [[7]], [1], [3.0], [1]),
    lambda e: e.predict_revised(5, ["x"], [1], [3.0], [1]),
    lambda e: e.predict_revised(5, [7], [1.5], [3.0], [1]),                    # non-integer item
    lambda e: e.predict_revised(5, [7], [1], [3.0], [[1]]),
    lambda e: e.recommend_revised(5, [-2**31 - 1], [1], [3.0], 3),
    lambda e: e.recommend_revised(5, [7], [1], ["x"], 3),
    lambda e: e.recommend_revised(5, [7], [1], [3.0], -1),
    lambda e: e.recommend_revised(5, [7], [], [3.0], 3),                       # empty items beside one rating
    lambda e: e.neighbors_revised_batch([GOOD, (6, [1, 2], [3.0, 4.0])]),      # a 3-tuple where a 4-tuple is due
    lambda e: e.neighbors_revised_batch([GOOD, (6, [[7]], [1], [3.0])]),       # removed 2-D
    lambda e: e.neighbors_revised_batch([GOOD, (6, [7.5], [1], [3.0])]),       # non-integer removed item
    lambda e: e.neighbors_revised_batch([GOOD, (6, [2**31], [1], [3.0])]),     # removed item beyond int32
    lambda e: e.neighbors_revised_batch([GOOD, (6, [7], [1, 2], [3.0])]),      # lengths differ
    lambda e: e.neighbors_revised_batch([GOOD], cap=-1),
    lambda e: e.neighbors_revised_batch([GOOD, (6.5, [7], [1], [3.0])]),       # non-integer user
    lambda e: e.predict_revised_batch([GOOD, GOOD], [[1]]),                    # one pred_items sequence per query
    lambda e: e.predict_revised_batch([GOOD, (6, [1], [3.0])], [[1], [1]]),    # a 3-tuple
    lambda e: e.predict_revised_batch([GOOD], [[1.5]]),
    lambda e: e.recommend_revised_batch([GOOD], -1),
    lambda e: e.recommend_revised_batch([GOOD, (6, [[7]], [1], [3.0])], 3),
    lambda e: e.recommend_revised_batch([GOOD, (6, [7], [2**31], [3.0])], 3),
    lambda e: e.recommend_revised_batch([GOOD, (6, [7], [1], [3.0], 4)], 3),   # a 5-tuple
])
def test_wrappers_reject_ragged_input(engine, call):
    with pytest.raises(ValueError):
        call(engine)
