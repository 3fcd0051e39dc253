"""Entry points of the entered queries of revise queries (knncf_revise_entered*: whose kNN lists a user's removals change) at the C
boundary and in the binding, without a GPU: both symbols are declared, exported and listed in EXPORTS with the documented argument
types, the header has their section and the neighbouring sections point at it, a null handle gets KNNCF_E_INVALID, and the Python
wrappers (EnteredQueries.entered_with*(..., removed=...)) reject ragged input before any C call."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("knncf_revise_entered", "knncf_revise_entered_batch")
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
    head = "---- Entered queries of revise queries:"
    assert head in text and text.index("---- Entered queries of update queries:") < text.index(head) < text.index("---- Append:")
    section = text[text.index(head):]
    section = section[:section.index("int knncf_revise_entered(")]
    for word in ("REPORTED", "n_removed == 0 AND n_ratings == 0", "only removes is an ordinary query", "SAME value", "identical bits",
                 "FALLS TO 4 OR FEWER ROWS", "An item that leaves aug", "changes no list", "removed item listed twice",
                 "left without a row", "more than 65536 train ratings", "NOT read-only", "TRAIN set has a user of 4 or fewer ratings",
                 "removed_offsets that are null", "bit for bit through the same code", "knncf-dispatch entered_revise slots=",
                 "OUT OF SCOPE: removals in knncf_append"):
        assert word in section, word
    # the notes that called the question unserved point at the section
    assert "it is not served for revise queries" not in text
    assert "OUT OF SCOPE: the entered question for revise queries" not in text
    assert text.count('"Entered queries of revise queries" below') == 3


def test_argtypes(kn):
    lib = kn.load_library()
    h, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    query = [i32, i32p, i64, i32p, f64p, i64]            # user, removed_items, n_removed, items, ratings, n_ratings
    batch = [i32p, i64p, i32p, i64p, i32p, f64p, i64]    # users, removed_offsets, removed_items, offsets, items, ratings, n_queries
    outs = [i32p, f64p, i32p, i32p, i32p]                # out_users, out_sims, out_pos, out_prev, out_other
    assert lib.knncf_revise_entered.argtypes == [h] + query + [i32] + outs + [i32p]
    assert lib.knncf_revise_entered_batch.argtypes == [h] + batch + [i32] + outs + [i32p, i32p]
    # the query part is the revise calls', the rest the update form's
    assert lib.knncf_revise_entered.argtypes[:8] == lib.knncf_revise_neighbors.argtypes[:8]
    assert lib.knncf_revise_entered_batch.argtypes[:9] == lib.knncf_revise_neighbors_batch.argtypes[:9]
    assert lib.knncf_revise_entered.argtypes[7:] == lib.knncf_update_entered.argtypes[5:]
    assert lib.knncf_revise_entered_batch.argtypes[8:] == lib.knncf_update_entered_batch.argtypes[6:]


def test_null_handle(kn):
    lib = kn.load_library()
    us = np.array([5], dtype=np.int32)
    roff = np.array([0, 1], dtype=np.int64)
    rm = np.array([7], dtype=np.int32)
    off = np.array([0, 2], dtype=np.int64)
    its = np.array([1, 2], dtype=np.int32)
    rts = np.array([3.0, 4.0])
    ids, pos, prev, other = (np.empty(4, dtype=np.int32) for _ in range(4))
    sims = np.empty(4, dtype=np.float64)
    cnt = np.zeros(1, dtype=np.int32)
    st = np.zeros(1, dtype=np.int32)
    p = lambda a, t: a.ctypes.data_as(t)
    outs = (p(ids, i32p), p(sims, f64p), p(pos, i32p), p(prev, i32p), p(other, i32p))
    assert lib.knncf_revise_entered(None, 5, p(rm, i32p), 1, p(its, i32p), p(rts, f64p), 2, 4, *outs, p(cnt, i32p)) == kn.E_INVALID
    assert lib.knncf_revise_entered_batch(None, p(us, i32p), p(roff, i64p), p(rm, i32p), p(off, i64p), p(its, i32p), p(rts, f64p), 1, 4,
                                          *outs, p(cnt, i32p), p(st, i32p)) == kn.E_INVALID


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
    lambda e: e.entered_with_batch([GOOD, GOOD], removed=[[7]]),             # fewer removed sequences than queries
    lambda e: e.entered_with_batch([GOOD], removed=[[7], [8]]),              # more
    lambda e: e.entered_with_batch([GOOD], removed=[]),
    lambda e: e.entered_with_batch([GOOD], removed=[[[7]]]),                 # 2-D removed items
    lambda e: e.entered_with_batch([GOOD], removed=[[7.5]]),                 # a non-integer removed item
    lambda e: e.entered_with_batch([GOOD], removed=[[2**31]]),
    lambda e: e.entered_with_batch([GOOD, (6, [1, 2])], removed=[[7], []]),  # not a triple
    lambda e: e.entered_with_batch([GOOD], cap=-1, removed=[[7]]),
    lambda e: e.entered_with(5, [1, 2], [3.0], removed=[7]),                 # lengths of the query differ
    lambda e: e.entered_with(5, [1], [3.0], removed=[[7]]),
    lambda e: e.entered_with(5, [1], [3.0], removed=[7.5]),
    lambda e: e.entered_with(5, [1], [3.0], cap=-1, removed=[7]),
    lambda e: e.entered_with(5, [1], [3.0], cap=True, removed=[7]),
])
def test_wrappers_reject_ragged_input(entered, call):
    with pytest.raises(ValueError):
        call(entered)


def test_the_keyword_picks_the_entry_point(entered):
    """removed=None is the update call; a removal-only query of a fitted user (no rows) and an empty removed list reach the revise
    entry points"""
    with pytest.raises(AssertionError, match="knncf_update_entered "):
        entered.entered_with(5, [], [])
    with pytest.raises(AssertionError, match="knncf_revise_entered "):
        entered.entered_with(5, [], [], removed=[7])
    with pytest.raises(AssertionError, match="knncf_revise_entered "):
        entered.entered_with(5, [1], [3.0], removed=[])
    with pytest.raises(AssertionError, match="knncf_update_entered_batch "):
        entered.entered_with_batch([GOOD])
    with pytest.raises(AssertionError, match="knncf_revise_entered_batch "):
        entered.entered_with_batch([GOOD, GOOD], removed=[[7], []])
