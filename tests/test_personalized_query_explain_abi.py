"""knncf_query_explain_personalized* / knncf_update_explain_personalized* / knncf_revise_explain_personalized* at the C boundary
and in the binding, without a GPU: the six symbols are declared, exported and listed in EXPORTS, each argument list is the
matching knncf_*_explain* list without `int predictor`, the ctypes signatures are the header's, a null handle gets
KNNCF_E_INVALID, the header block states its sub-range rule and its scope, and the wrappers take predictor= and reject bad
input before any C call."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("query", "update", "revise")
NAMES = tuple(f"knncf_{fam}_explain_personalized{tail}" for fam in FAMILIES for tail in ("", "_batch"))
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


def _comment(title):
    text = _header(comments=True)
    block = text[text.index(title):]
    block = re.sub(r"\n \*", " ", block[:block.index("*/")])  # (the comment's line starts are no part of its sentences,
    return " ".join(block.split())                               # nor is where a line happens to break)


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_listed(kn, name):
    assert re.search(r"\bint\s+" + name + r"\s*\(", _header())
    assert hasattr(kn.load_library(), name)
    assert name in kn.EXPORTS


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("tail", ["", "_batch"])
def test_arguments_are_the_explain_calls_without_the_predictor(fam, tail):
    explain = _params(f"knncf_{fam}_explain{tail}")
    assert explain[1] == "int predictor"
    assert _params(f"knncf_{fam}_explain_personalized{tail}") == explain[:1] + explain[2:]


def _ctype_of(param):
    if "knncf_handle*" in param:
        return C.c_void_p
    if "*" in param:
        return C.POINTER({"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}[param.replace("const ", "").split("*")[0].strip()])
    return {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64}[param.split()[0]]


@pytest.mark.parametrize("name", NAMES)
def test_ctypes_signature_is_the_headers(kn, name):
    want = [_ctype_of(p) for p in _params(name)]
    assert len(want) == {"knncf_query_explain_personalized": 15, "knncf_update_explain_personalized": 15,
                         "knncf_revise_explain_personalized": 17, "knncf_query_explain_personalized_batch": 17,
                         "knncf_update_explain_personalized_batch": 17, "knncf_revise_explain_personalized_batch": 19}[name]
    assert list(getattr(kn.load_library(), name).argtypes) == want


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
    assert lib.knncf_query_explain_personalized(None, 5, *rows, 0, 3, *out) == kn.E_INVALID
    assert lib.knncf_update_explain_personalized(None, 5, *rows, 0, 3, *out) == kn.E_INVALID
    assert lib.knncf_revise_explain_personalized(None, 5, p(its, i32p), 1, *rows, 0, 3, *out) == kn.E_INVALID
    assert lib.knncf_query_explain_personalized_batch(None, p(us, i32p), *csr, 0, 3, *out, p(st, i32p)) == kn.E_INVALID
    assert lib.knncf_update_explain_personalized_batch(None, p(us, i32p), *csr, 0, 3, *out, p(st, i32p)) == kn.E_INVALID
    assert lib.knncf_revise_explain_personalized_batch(None, p(us, i32p), p(off, i64p), p(its, i32p), *csr, 0, 3, *out,
                                                       p(st, i32p)) == kn.E_INVALID


def test_sub_range_rule_and_scope_are_documented():
    block = _comment("---- Explanations of Personalized query predictions")
    assert "R = max(1, budget / (40 * cap + 28))" in block and "workspace_bytes / 2" in block
    for phrase in ("NEW CALLS, NOT A LIFTED REFUSAL", "without `int predictor`", "THE USER IS ITS OWN TERM", "S(u, u)", ":513-517",
                   ":520-524", "no fused multiply-add", "+-0.0", "earliest in summation order", "stands last", "a removed row is no term",
                   "exactly one term", "prep_ms", "predict_ms", "allocates no device memory", "do not depend on R",
                   "OUT OF SCOPE: a device-pointer form", "recommend and explain in one pass"):
        assert phrase in block, phrase
    # the three places that called this out of scope keep their refusal and point here
    for title in ("---- Explanations of Personalized predictions", "---- Personalized queries: KNNCF_PRED_PERSONALIZED on the query families",
                  "Explanations of query predictions: the terms behind"):
        assert "knncf_*_explain_personalized*" in _comment(title), title
    assert "OUT OF SCOPE" in _comment("Explanations of query predictions: the terms behind")


class _NoCalls:
    def __getattr__(self, name):
        raise AssertionError(f"C entry point {name} called with bad arguments")


class _Recorder:
    """stands in for the library: records the entry point a wrapper picked and answers KNNCF_OK"""

    def __init__(self):
        self.called = []

    def __getattr__(self, name):
        def call(*args):
            self.called.append((name, args))
            return 0
        return call


@pytest.fixture
def engine(kn):
    e = kn.Engine.__new__(kn.Engine)  # no device: every C call would fail loudly
    e._lib, e._h, e.k, e.device = _NoCalls(), None, 10, 0
    return e


def _calls(e, kn, cap, order, predictor):
    """the six wrappers on one valid query"""
    its, rts = [1, 2], [3.0, 4.0]
    kw = dict(order=order, predictor=predictor)
    return [lambda: e.explain_for(5, its, rts, [3, 4], cap, **kw),
            lambda: e.explain_with(5, its, rts, [3, 4], cap, **kw),
            lambda: e.explain_revised(5, [7], its, rts, [3, 4], cap, **kw),
            lambda: e.explain_for_batch([(5, its, rts)], [[3, 4]], cap, **kw),
            lambda: e.explain_with_batch([(5, its, rts)], [[3, 4]], cap, **kw),
            lambda: e.explain_revised_batch([(5, [7], its, rts)], [[3, 4]], cap, **kw)]


@pytest.mark.parametrize("cap,order,predictor", [(-1, 0, 6), (2.0, 0, 6), (True, 0, 6), (2**31, 0, 6), (4, 2, 6), (4, -1, 6), (4, None, 6),
                                                 (4, 0, 0), (4, 0, 4), (4, 0, 7), (4, 0, -1), (4, 0, None), (4, 0, True), (4, 0, 6.0)])
def test_wrappers_reject_bad_cap_order_and_predictor(engine, kn, cap, order, predictor):
    assert kn.PRED_PERSONALIZED == 6 and kn.PRED_KNN == 5
    for call in _calls(engine, kn, cap, order, predictor):
        with pytest.raises(ValueError):
            call()


def test_predictor_routes_to_the_new_calls(engine, kn):
    for predictor, tail, lead in ((kn.PRED_PERSONALIZED, "_personalized", 0), (kn.PRED_KNN, "", 1)):
        rec = _Recorder()
        engine._lib = rec
        for call in _calls(engine, kn, 4, kn.EXPLAIN_BY_WEIGHT, predictor):
            out = call()
        assert [name for name, _ in rec.called] == [f"knncf_{fam}_explain{tail}{b}" for b in ("", "_batch") for fam in FAMILIES]
        want = {"knncf_query_explain": 16, "knncf_update_explain": 16, "knncf_revise_explain": 18, "knncf_query_explain_batch": 18,
                "knncf_update_explain_batch": 18, "knncf_revise_explain_batch": 20}
        for name, args in rec.called:
            assert len(args) == want[name.replace("_personalized", "")] - (1 - lead), name
            assert (args[1] == kn.PRED_KNN) if lead else True
        # return shapes and padding are those of the kNN forms: ([per query (raters [m, cap], ...)], statuses)
        per_query, st = out
        raters, sims, devs, counts, sums, preds = per_query[0]
        assert raters.shape == (2, 4) and (raters == -1).all() and np.isnan(sims).all() and np.isnan(devs).all()
        assert counts.tolist() == [0, 0] and sums.shape == (2, 2) and preds.shape == (2,) and st.tolist() == [0]
