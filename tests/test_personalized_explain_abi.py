"""knncf_explain_personalized* at the C boundary and in the binding, without a GPU: the two symbols are declared, exported and
listed in EXPORTS, their arguments are knncf_explain's / knncf_explain_batch's, the ctypes signatures are the header's, a null
handle gets KNNCF_E_INVALID, the header states the sub-range rule and the scope notes, and the wrappers reject bad input before
any C call."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("knncf_explain_personalized", "knncf_explain_personalized_batch")
i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)


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


def _comment(title):
    text = _header(comments=True)
    block = text[text.index(title):]
    return re.sub(r"\n \*", " ", block[:block.index("*/")])  # (the comment's line starts are no part of its sentences)


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_listed(kn, name):
    assert re.search(r"\bint\s+" + name + r"\s*\(", _header())
    assert hasattr(kn.load_library(), name)
    assert name in kn.EXPORTS


def test_arguments_are_the_knn_calls():
    assert _params("knncf_explain_personalized") == _params("knncf_explain")
    assert _params("knncf_explain_personalized_batch") == _params("knncf_explain_batch")
    assert _params("knncf_explain_personalized_batch")[4:] == [
        "int32_t order", "int32_t cap", "int32_t* raters", "double* sims", "double* devs", "int32_t* counts", "double* sums",
        "double* predictions"]


@pytest.mark.parametrize("name", NAMES)
def test_ctypes_signature_is_the_headers(kn, name):
    def ctype(param):
        if "knncf_handle*" in param:
            return C.c_void_p
        if "*" in param:
            return C.POINTER({"int32_t": C.c_int32, "double": C.c_double}[param.replace("const ", "").split("*")[0].strip()])
        return {"int32_t": C.c_int32, "int64_t": C.c_int64}[param.split()[0]]

    want = [ctype(p) for p in _params(name)]
    assert len(want) == {"knncf_explain_personalized": 11, "knncf_explain_personalized_batch": 12}[name]
    assert list(getattr(kn.load_library(), name).argtypes) == want


def test_sub_range_rule_and_scope_are_documented():
    block = _comment("---- Explanations of Personalized predictions")
    assert "R = max(1, budget / (40 * cap + 28))" in block and "workspace_bytes / 2" in block
    for phrase in ("THE USER IS ITS OWN TERM", "S(u, u)", "no fused multiply-add", "+-0.0", "predict/Personalized.scala:61-72",
                   ":513-517", ":520-524", "earliest in summation order", "prep_ms", "rerank_ms", "predict_ms",
                   "Read-only on the kNN state", "allocates no device memory", "nothing to explain", "4 or fewer ratings",
                   "SHARDED EXPLANATIONS ARE OUT OF SCOPE", "OUT OF SCOPE: a device-pointer form"):
        assert phrase in block, phrase
    # the kNN block points here and keeps its own scope; the query block keeps its refusal and points here too
    knn = _comment("---- Explanations: the neighbour terms behind KNNCF_PRED_KNN predictions")
    assert "knncf_explain_personalized*" in knn and "explains KNNCF_PRED_KNN only" in knn
    assert "SHARDED EXPLANATIONS ARE OUT OF SCOPE" in knn
    query = _comment("Explanations of query predictions: the terms behind")
    assert "KNNCF_PRED_PERSONALIZED explanations" in query and "knncf_explain_personalized*" in query


def test_null_handle(kn):
    lib = kn.load_library()
    us, its = np.array([5, 6], dtype=np.int32), np.array([1, 2], dtype=np.int32)
    raters, sims, devs = np.empty(6, dtype=np.int32), np.empty(6), np.empty(6)
    cnt, sums, preds = np.zeros(2, dtype=np.int32), np.zeros(4), np.zeros(2)
    p = lambda a, t: a.ctypes.data_as(t)
    out = (p(raters, i32p), p(sims, f64p), p(devs, f64p), p(cnt, i32p), p(sums, f64p), p(preds, f64p))
    assert lib.knncf_explain_personalized_batch(None, p(us, i32p), p(its, i32p), 2, 0, 3, *out) == kn.E_INVALID
    assert lib.knncf_explain_personalized(None, 5, 1, 0, 3, *out) == kn.E_INVALID


class _NoCalls:
    def __getattr__(self, name):
        raise AssertionError(f"C entry point {name} called with bad arguments")


@pytest.fixture
def engine(kn):
    e = kn.Engine.__new__(kn.Engine)  # no device: every C call would fail loudly
    e._lib, e._h, e.k, e.device = _NoCalls(), None, 10, 0
    return e


@pytest.mark.parametrize("cap,order", [(-1, 0), (2.0, 0), (True, 0), (2**31, 0), (4, 2), (4, -1), (4, None)])
def test_wrappers_reject_bad_input(engine, cap, order):
    with pytest.raises(ValueError):
        engine.explain_personalized_batch([1, 2], [3, 4], cap, order=order)
    with pytest.raises(ValueError):
        engine.explain_personalized(1, 3, cap=cap, order=order)


def test_batch_wrapper_rejects_ragged_rows(engine):
    with pytest.raises(ValueError):
        engine.explain_personalized_batch([1, 2], [3], 4)
    with pytest.raises(ValueError):
        engine.explain_personalized_batch([[1, 2]], [[3, 4]], 4)
