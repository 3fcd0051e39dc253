"""Entry points of the entered queries of update queries (knncf_update_entered*: whose kNN lists a user's additional ratings
change) at the C boundary and in the binding, without a GPU: both symbols are declared, exported and listed in EXPORTS with the
documented argument types, the header has their section and no longer calls the question unserved, a null handle gets
KNNCF_E_INVALID, and the Python wrappers (EnteredQueries.entered_with*) reject ragged input before any C call."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("knncf_update_entered", "knncf_update_entered_batch")
i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def kn(pkg):
    importlib.import_module(pkg.__name__ + ".build").build()
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _header():
    return open(os.path.join(ROOT, "include", "knncf.h")).read()


def test_declared_exported_and_listed(kn):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = kn.load_library()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name), name
        assert name in kn.EXPORTS, name


def test_header_text():
    text = " ".join(_header().replace(" * ", " ").split())
    assert "---- Entered queries of update queries:" in text
    section = text[text.index("---- Entered queries of update queries:"):]
    section = section[:section.index("int knncf_update_entered(")]
    for word in ("out_prev", "out_other", "REPORTED", "Tail rows", "NOT read-only", "n_ratings == 0", "identical bits",
                 "more than 65536 train ratings", "OUT OF SCOPE: revise queries"):
        assert word in section, word
    # the two notes that called the question unserved now point at the section
    assert "a changer that leaves a list needs that user's full row" not in text
    assert "the entered question itself is not served for them" not in text
    assert text.count('"Entered queries of update queries" below') == 2


def test_argtypes(kn):
    lib = kn.load_library()
    h, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    query = [i32, i32p, f64p, i64]           # user, items, ratings, n_ratings
    batch = [i32p, i64p, i32p, f64p, i64]    # users, offsets, items, ratings, n_queries
    outs = [i32p, f64p, i32p, i32p, i32p]    # out_users, out_sims, out_pos, out_prev, out_other
    assert lib.knncf_update_entered.argtypes == [h] + query + [i32] + outs + [i32p]
    assert lib.knncf_update_entered_batch.argtypes == [h] + batch + [i32] + outs + [i32p, i32p]
    # the query part is the update calls'
    assert lib.knncf_update_entered.argtypes[:6] == lib.knncf_update_neighbors.argtypes[:6]
    assert lib.knncf_update_entered_batch.argtypes[:7] == lib.knncf_update_neighbors_batch.argtypes[:7]


def test_null_handle(kn):
    lib = kn.load_library()
    us = np.array([5], dtype=np.int32)
    off = np.array([0, 2], dtype=np.int64)
    its = np.array([1, 2], dtype=np.int32)
    rts = np.array([3.0, 4.0])
    ids, pos, prev, other = (np.empty(4, dtype=np.int32) for _ in range(4))
    sims = np.empty(4, dtype=np.float64)
    cnt = np.zeros(1, dtype=np.int32)
    st = np.zeros(1, dtype=np.int32)
    p = lambda a, t: a.ctypes.data_as(t)
    outs = (p(ids, i32p), p(sims, f64p), p(pos, i32p), p(prev, i32p), p(other, i32p))
    assert lib.knncf_update_entered(None, 5, p(its, i32p), p(rts, f64p), 2, 4, *outs, p(cnt, i32p)) == kn.E_INVALID
    assert lib.knncf_update_entered_batch(None, p(us, i32p), p(off, i64p), p(its, i32p), p(rts, f64p), 1, 4, *outs, p(cnt, i32p),
                                          p(st, i32p)) == kn.E_INVALID


class _NoCalls:
    def __getattr__(self, name):
        raise AssertionError(f"C entry point {name} called with bad arguments")


@pytest.fixture
def entered(kn):
    e = kn.Engine.__new__(kn.Engine)  # no device: every C call would fail loudly
    e._lib, e._h, e.k, e.device = _NoCalls(), None, 10, 0
    return kn.EnteredQueries(e)


GOOD = (5, [1, 2], [3.0, 4.0])


@pytest.mark.parametrize("call", [
    lambda e: e.entered_with(5, [1, 2], [3.0]),                         # lengths of the query differ
    lambda e: e.entered_with(5, [[1]], [[3.0]]),                        # 2-D rows
    lambda e: e.entered_with(5.5, [1], [3.0]),                          # non-integer user
    lambda e: e.entered_with(2**31, [1], [3.0]),                        # user beyond int32
    lambda e: e.entered_with(5, [1.5], [3.0]),                          # non-integer item
    lambda e: e.entered_with(5, [1], ["x"]),                            # a rating that is no number
    lambda e: e.entered_with(5, [1], [3.0], cap=-1),
    lambda e: e.entered_with(5, [1], [3.0], cap=1.5),
    lambda e: e.entered_with(5, [1], [3.0], cap=True),
    lambda e: e.entered_with_batch([GOOD, (6, [1, 2], [3.0])]),         # a ragged query
    lambda e: e.entered_with_batch([GOOD, (6, [1, 2])]),                # not a triple
    lambda e: e.entered_with_batch([(6.5, [1], [3.0])]),
    lambda e: e.entered_with_batch([(6, [1.5], [3.0])]),
    lambda e: e.entered_with_batch([GOOD], cap=-1),
    lambda e: e.entered_with_batch([GOOD], cap=2**31),
])
def test_wrappers_reject_ragged_input(entered, call):
    with pytest.raises(ValueError):
        call(entered)


def test_an_empty_query_reaches_the_library(entered):
    """an update query may come without rows (a fitted user: a valid query that reports nothing): the wrapper passes it on"""
    with pytest.raises(AssertionError, match="knncf_update_entered"):
        entered.entered_with(5, [], [])
