"""knncf_query_explain* / knncf_update_explain* / knncf_revise_explain* at the C boundary and in the binding, without a GPU:
the six symbols are declared, exported and listed in EXPORTS, the ctypes signatures are the header's, a null handle gets
KNNCF_E_INVALID, the sub-range rule and the scope notes are written in the header, and the wrappers reject bad input before
any C call."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("query", "update", "revise")
NAMES = tuple(f"knncf_{fam}_explain{tail}" for fam in FAMILIES for tail in ("", "_batch"))
i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def kn(pkg):
    importlib.import_module(pkg.__name__ + ".build").build()
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _header(comments=False):
    text = open(os.path.join(ROOT, "include", "knncf.h")).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _params(name):
    return [" ".join(p.split()) for p in re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", _header(), flags=re.S).group(1).split(",")]


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_listed(kn, name):
    assert re.search(r"\bint\s+" + name + r"\s*\(", _header())
    assert hasattr(kn.load_library(), name)
    assert name in kn.EXPORTS


def _ctype_of(param):
    if "knncf_handle*" in param:
        return C.c_void_p
    if "*" in param:
        return C.POINTER({"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}[param.replace("const ", "").split("*")[0].strip()])
    return {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64}[param.split()[0]]


@pytest.mark.parametrize("name", NAMES)
def test_ctypes_signature_is_the_headers(kn, name):
    want = [_ctype_of(p) for p in _params(name)]
    assert len(want) == {"knncf_query_explain": 16, "knncf_update_explain": 16, "knncf_revise_explain": 18,
                         "knncf_query_explain_batch": 18, "knncf_update_explain_batch": 18, "knncf_revise_explain_batch": 20}[name]
    assert list(getattr(kn.load_library(), name).argtypes) == want


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("tail,drop", [("", 1), ("_batch", 2)])
def test_query_arguments_are_the_predict_calls(fam, tail, drop):
    """the argument list is that of knncf_*_predict* up to the requested items, then order, cap and knncf_explain_batch's outputs"""
    predict, explain = _params(f"knncf_{fam}_predict{tail}"), _params(f"knncf_{fam}_explain{tail}")
    assert explain[:len(predict) - drop] == predict[:-drop]
    outputs = ["int32_t order", "int32_t cap", "int32_t* raters", "double* sims", "double* devs", "int32_t* counts", "double* sums",
               "double* predictions"]
    assert explain[len(predict) - drop:] == outputs + (["int32_t* statuses"] if tail else [])


def test_sub_range_rule_and_scope_are_documented():
    text = _header(comments=True)
    assert "R = max(1, budget / (20 * cap + 28))" in text and "workspace_bytes / 2" in text
    # what tests/test_explain_abi.py reads in the knncf_explain block is still there
    assert "C = max(1, budget / (20 * cap + 28))" in text
    assert re.search(r"STATE\s+THAT\s+knncf_predict_batch\s+OVER\s+THE\s+SAME\s+ROWS\s+LEAVES", text)
    assert re.search(r"SHARDED\s+EXPLANATIONS\s+ARE\s+OUT\s+OF\s+SCOPE", text)
    # the knncf_explain block no longer calls the query explanations out of scope; the new block names what stays out
    assert not re.search(r"as\s+are\s+explanations\s+of\s+fold-in", text)
    block = text[text.index("Explanations of query predictions: the terms behind"):]
    block = re.sub(r"\n \*", " ", block[:block.index("*/")])  # (the comment's line starts are no part of its sentences)
    for phrase in (r"KNNCF_PRED_PERSONALIZED\s+explanations", r"sharded\s+explanations", r"recommend\s+and\s+explain\s+in\s+one\s+pass"):
        assert re.search(phrase, block), phrase
    assert re.search(r"OUT\s+OF\s+SCOPE", block)


def test_null_handle(kn):
    lib = kn.load_library()
    p = lambda a, t: a.ctypes.data_as(t)
    us, off = np.array([5, 6], dtype=np.int32), np.array([0, 1, 2], dtype=np.int64)
    its, rts = np.array([1, 2], dtype=np.int32), np.array([3.0, 4.0])
    raters, sims, devs = np.empty(6, dtype=np.int32), np.empty(6), np.empty(6)
    cnt, sums, preds, st = np.zeros(2, dtype=np.int32), np.zeros(4), np.zeros(2), np.zeros(2, dtype=np.int32)
    out = (p(raters, i32p), p(sims, f64p), p(devs, f64p), p(cnt, i32p), p(sums, f64p), p(preds, f64p))
    rows = (p(its, i32p), p(rts, f64p), 2, p(its, i32p), 2)
    csr = (p(off, i64p), p(its, i32p), p(rts, f64p), 2, p(off, i64p), p(its, i32p))
    assert lib.knncf_query_explain(None, kn.PRED_KNN, 5, *rows, 0, 3, *out) == kn.E_INVALID
    assert lib.knncf_update_explain(None, kn.PRED_KNN, 5, *rows, 0, 3, *out) == kn.E_INVALID
    assert lib.knncf_revise_explain(None, kn.PRED_KNN, 5, p(its, i32p), 1, *rows, 0, 3, *out) == kn.E_INVALID
    assert lib.knncf_query_explain_batch(None, kn.PRED_KNN, p(us, i32p), *csr, 0, 3, *out, p(st, i32p)) == kn.E_INVALID
    assert lib.knncf_update_explain_batch(None, kn.PRED_KNN, p(us, i32p), *csr, 0, 3, *out, p(st, i32p)) == kn.E_INVALID
    assert lib.knncf_revise_explain_batch(None, kn.PRED_KNN, p(us, i32p), p(off, i64p), p(its, i32p), *csr, 0, 3, *out,
                                          p(st, i32p)) == kn.E_INVALID


class _NoCalls:
    def __getattr__(self, name):
        raise AssertionError(f"C entry point {name} called with bad arguments")


@pytest.fixture
def engine(kn):
    e = kn.Engine.__new__(kn.Engine)  # no device: every C call would fail loudly
    e._lib, e._h, e.k, e.device = _NoCalls(), None, 10, 0
    return e


def _calls(e, pred_items, pred_items_batch, cap, order):
    """the six wrappers on one valid query"""
    its, rts = [1, 2], [3.0, 4.0]
    return [lambda: e.explain_for(5, its, rts, pred_items, cap, order=order),
            lambda: e.explain_with(5, its, rts, pred_items, cap, order=order),
            lambda: e.explain_revised(5, [7], its, rts, pred_items, cap, order=order),
            lambda: e.explain_for_batch([(5, its, rts)], pred_items_batch, cap, order=order),
            lambda: e.explain_with_batch([(5, its, rts)], pred_items_batch, cap, order=order),
            lambda: e.explain_revised_batch([(5, [7], its, rts)], pred_items_batch, cap, order=order)]


@pytest.mark.parametrize("cap,order", [(-1, 0), (2.0, 0), (True, 0), (2**31, 0), (4, 2), (4, -1), (4, None)])
def test_wrappers_reject_bad_cap_and_order(engine, cap, order):
    for call in _calls(engine, [3, 4], [[3, 4]], cap, order):
        with pytest.raises(ValueError):
            call()


def test_wrappers_reject_ragged_pred_items(engine):
    for call in _calls(engine, [[3, 4]], [[[3, 4]]], 4, 0):  # 2-D where 1-D ids belong
        with pytest.raises(ValueError):
            call()
    for call in _calls(engine, [3.5], [[3.5]], 4, 0):  # not integer ids
        with pytest.raises(ValueError):
            call()
    for call in _calls(engine, [3], [[3], [4]], 4, 0)[3:]:  # two pred_items sequences for one query
        with pytest.raises(ValueError):
            call()
    for call in _calls(engine, [3], [], 4, 0)[3:]:  # none
        with pytest.raises(ValueError):
            call()
