"""knncf_query_recommend_explain* / knncf_update_recommend_explain* / knncf_revise_recommend_explain* at the C boundary and in
the binding, without a GPU: the six symbols are declared, exported and listed in EXPORTS, each argument list is the matching
knncf_*_recommend* list with order, cap and the explain outputs (no predictions array), the ctypes signatures are the header's,
a null handle gets KNNCF_E_INVALID, the header block states its contract, the blocks that called the fused call out of scope keep
their sentences and point to it, and the wrappers reject bad input before any C call."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("query", "update", "revise")
NAMES = tuple(f"knncf_{fam}_recommend_explain{tail}" for fam in FAMILIES for tail in ("", "_batch"))
TITLE = "---- Recommendations with their explanations"
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
    block = re.sub(r"\n \*", " ", block[:block.index("*/")])
    return " ".join(block.split())


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_listed(kn, name):
    assert re.search(r"\bint\s+" + name + r"\s*\(", _header())
    assert hasattr(kn.load_library(), name)
    assert name in kn.EXPORTS


@pytest.mark.parametrize("fam", FAMILIES)
def test_arguments_are_the_recommend_calls_with_the_explain_outputs(fam):
    terms = ["int32_t* raters", "double* sims", "double* devs", "int32_t* term_counts", "double* sums"]
    reco = _params(f"knncf_{fam}_recommend")
    assert reco[-3:] == ["int32_t* out_items", "double* out_preds", "int32_t* count"] and reco[-4] == "int32_t n"
    assert _params(f"knncf_{fam}_recommend_explain") == reco[:-3] + ["int32_t order", "int32_t cap"] + reco[-3:] + terms
    reco = _params(f"knncf_{fam}_recommend_batch")
    assert reco[-4:] == ["int32_t* out_items", "double* out_preds", "int32_t* counts", "int32_t* statuses"]
    assert _params(f"knncf_{fam}_recommend_explain_batch") == reco[:-4] + ["int32_t order", "int32_t cap"] + reco[-4:-1] + terms + reco[-1:]
    assert not any("predictions" in p for tail in ("", "_batch") for p in _params(f"knncf_{fam}_recommend_explain{tail}"))


def _ctype_of(param):
    if "knncf_handle*" in param:
        return C.c_void_p
    if "*" in param:
        return C.POINTER({"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}[param.replace("const ", "").split("*")[0].strip()])
    return {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64}[param.split()[0]]


@pytest.mark.parametrize("name", NAMES)
def test_ctypes_signature_is_the_headers(kn, name):
    want = [_ctype_of(p) for p in _params(name)]
    assert len(want) == {"knncf_query_recommend_explain": 17, "knncf_update_recommend_explain": 17, "knncf_revise_recommend_explain": 19,
                         "knncf_query_recommend_explain_batch": 19, "knncf_update_recommend_explain_batch": 19,
                         "knncf_revise_recommend_explain_batch": 21}[name]
    assert list(getattr(kn.load_library(), name).argtypes) == want


def test_null_handle(kn):
    lib = kn.load_library()
    p = lambda a, t: a.ctypes.data_as(t)
    us, off = np.array([5, 6], dtype=np.int32), np.array([0, 1, 2], dtype=np.int64)
    its, rts = np.array([1, 2], dtype=np.int32), np.array([3.0, 4.0])
    ids, preds, cnt = np.empty(6, dtype=np.int32), np.empty(6), np.zeros(2, dtype=np.int32)
    raters, sims, devs = np.empty(24, dtype=np.int32), np.empty(24), np.empty(24)
    tc, sums, st = np.zeros(6, dtype=np.int32), np.zeros(12), np.zeros(2, dtype=np.int32)
    out = (p(ids, i32p), p(preds, f64p), p(cnt, i32p), p(raters, i32p), p(sims, f64p), p(devs, f64p), p(tc, i32p), p(sums, f64p))
    rows = (p(its, i32p), p(rts, f64p), 2)
    csr = (p(off, i64p), p(its, i32p), p(rts, f64p), 2)
    assert lib.knncf_query_recommend_explain(None, kn.PRED_KNN, 5, *rows, 3, 0, 4, *out) == kn.E_INVALID
    assert lib.knncf_update_recommend_explain(None, kn.PRED_KNN, 5, *rows, 3, 0, 4, *out) == kn.E_INVALID
    assert lib.knncf_revise_recommend_explain(None, kn.PRED_KNN, 5, p(its, i32p), 1, *rows, 3, 0, 4, *out) == kn.E_INVALID
    assert lib.knncf_query_recommend_explain_batch(None, kn.PRED_KNN, p(us, i32p), *csr, 3, 0, 4, *out, p(st, i32p)) == kn.E_INVALID
    assert lib.knncf_update_recommend_explain_batch(None, kn.PRED_KNN, p(us, i32p), *csr, 3, 0, 4, *out, p(st, i32p)) == kn.E_INVALID
    assert lib.knncf_revise_recommend_explain_batch(None, kn.PRED_KNN, p(us, i32p), p(off, i64p), p(its, i32p), *csr, 3, 0, 4, *out,
                                                    p(st, i32p)) == kn.E_INVALID


def test_the_contract_is_documented():
    block = _comment(TITLE)
    for phrase in ("NEW CALLS: no refusal of the explain calls above is lifted", "KNNCF_PRED_KNN or KNNCF_PRED_PERSONALIZED",
                   "exactly what knncf_*_recommend_batch writes for the same arguments, bit for bit", "the cells past counts[b] are untouched",
                   "a refused query gets counts[b] = 0 and its row is untouched", "explain row r = b * n + j",
                   "knncf_*_explain_batch for KNNCF_PRED_KNN", "knncf_*_explain_personalized_batch for KNNCF_PRED_PERSONALIZED",
                   "pred_items = its recommended items", "Every explain cell of a row j >= counts[b] is untouched",
                   "NO PREDICTIONS ARRAY", "out_preds[r] already is the explained prediction", "are not restated here",
                   "KNNCF_E_INVALID for cap < 0 and for an unknown order", "a null term_counts with n > 0",
                   "a null raters / sims / devs with n > 0 and cap > 0", "sums may be null", "n == 0 is KNNCF_OK with counts[b] = 0",
                   "a single form has set *count = 0", "A single form returns the query's status",
                   "R = max(1, budget / (20 * cap + 28))", "R = max(1, budget / (40 * cap + 28))", "workspace_bytes / 2",
                   "no host round trip between the selection and the first explain launch", "depend on neither C nor R",
                   "allocates no device memory", "knncf_neighbors_save bytes stay as they were", "prep_ms", "predict_ms",
                   "OUT OF SCOPE: a fused call for users as the fit holds them"):
        assert phrase in block, phrase


def test_the_old_blocks_keep_their_sentences_and_point_here():
    knn = _comment("Explanations of query predictions: the terms behind")
    assert 'a fused "recommend and explain in one pass" call: explain the items knncf_*_recommend returned with a second call' in knn
    assert "OUT OF SCOPE here as above" in knn
    personalized = _comment("---- Explanations of Personalized query predictions")
    assert 'OUT OF SCOPE: a device-pointer form, shard handles, KNNCF_SIM_ONE, a fused "recommend and explain in one pass" call' in personalized
    fitted = _comment("---- Explanations of Personalized predictions")
    assert "OUT OF SCOPE: a device-pointer form" in fitted and "Those have calls of their own:" in fitted
    for block in (knn, personalized, fitted):
        assert 'knncf_*_recommend_explain* ("Recommendations with their explanations" below)' in block


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


def _calls(e, n, cap, order, predictor, its=(1, 2), rts=(3.0, 4.0), user=5):
    """the six wrappers on one query"""
    its, rts = list(its), list(rts)
    kw = dict(order=order, predictor=predictor)
    return [lambda: e.recommend_explain_for(user, its, rts, n, cap, **kw),
            lambda: e.recommend_explain_with(user, its, rts, n, cap, **kw),
            lambda: e.recommend_explain_revised(user, [7], its, rts, n, cap, **kw),
            lambda: e.recommend_explain_for_batch([(user, its, rts)], n, cap, **kw),
            lambda: e.recommend_explain_with_batch([(user, its, rts)], n, cap, **kw),
            lambda: e.recommend_explain_revised_batch([(user, [7], its, rts)], n, cap, **kw)]


@pytest.mark.parametrize("n,cap,order,predictor", [(-1, 4, 0, 5), (2.0, 4, 0, 5), (True, 4, 0, 5), (2**31, 4, 0, 5),   # the recommend wrappers' n
                                                   (3, -1, 0, 6), (3, 2.0, 0, 6), (3, True, 0, 6), (3, 2**31, 0, 6),   # the explain wrappers' cap,
                                                   (3, 4, 2, 6), (3, 4, -1, 6), (3, 4, None, 6),                          # order
                                                   (3, 4, 0, 0), (3, 4, 0, 4), (3, 4, 0, 7), (3, 4, 0, None), (3, 4, 0, True), (3, 4, 0, 6.0)])
def test_wrappers_reject_bad_n_cap_order_and_predictor(engine, kn, n, cap, order, predictor):
    assert kn.PRED_PERSONALIZED == 6 and kn.PRED_KNN == 5
    for call in _calls(engine, n, cap, order, predictor):
        with pytest.raises(ValueError):
            call()


def test_wrappers_reject_bad_queries(engine, kn):
    for kw in (dict(its=(1, 2), rts=(3.0,)), dict(its=(1.5, 2.0)), dict(user=2**31), dict(user=True)):
        for call in _calls(engine, 3, 4, kn.EXPLAIN_SUM_ORDER, kn.PRED_KNN, **kw):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        engine.recommend_explain_for(5, [], [], 3, 4)  # a fold-in query needs a rating
    with pytest.raises(ValueError):
        engine.recommend_explain_revised_batch([(5, [1, 2], [3.0, 4.0])], 3, 4)  # a revise query has four parts


@pytest.mark.parametrize("predictor", [5, 6])
def test_wrappers_route_and_shape_their_answers(engine, kn, predictor):
    rec = _Recorder()
    engine._lib = rec
    outs = [call() for call in _calls(engine, 3, 4, kn.EXPLAIN_BY_WEIGHT, predictor)]
    assert [name for name, _ in rec.called] == [f"knncf_{fam}_recommend_explain{b}" for b in ("", "_batch") for fam in FAMILIES]
    want = {"knncf_query_recommend_explain": 17, "knncf_update_recommend_explain": 17, "knncf_revise_recommend_explain": 19,
            "knncf_query_recommend_explain_batch": 19, "knncf_update_recommend_explain_batch": 19, "knncf_revise_recommend_explain_batch": 21}
    for name, args in rec.called:
        assert len(args) == want[name] and args[1] == predictor, name
    for single in outs[:3]:  # the recorder leaves *count = 0: nothing recommended, nothing explained
        items, preds, raters, sims, devs, term_counts, sums = single
        assert items.shape == preds.shape == (0,) and raters.shape == sims.shape == devs.shape == (0, 4)
        assert term_counts.shape == (0,) and sums.shape == (0, 2)
    for per_query, st in outs[3:]:
        assert st.tolist() == [0] and len(per_query) == 1 and len(per_query[0]) == 7
        assert per_query[0][2].shape == (0, 4) and per_query[0][6].shape == (0, 2)
