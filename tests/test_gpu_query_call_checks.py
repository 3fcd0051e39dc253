"""The call-level checks of the 24 query entry points (knncf_{query,update,revise}_{neighbors,predict,recommend,explain}
and their _batch forms), asked at the C boundary with sentinel-filled outputs on every call.

This is a characterisation test: the status of every case, and which outputs a call wrote, are the ones recorded in
tests/golden/query_call_checks.json from a run of observe() below on the commit in front of the one that gave the query
host path its request type.  Nothing in that file was worked out from the code.  Beyond the recorded values the test asserts
that a call that fails leaves every output array as the caller filled it.

The train set is 6 users x 8 items, made by hand: five users is the least the query path accepts and none of the checks
depends on size."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "query_call_checks.json")

PRED_BASELINE, PRED_KNN = 3, 5
FAMILIES = ("query", "update", "revise")
FORMS = ("neighbors", "predict", "recommend", "explain")
ENTRIES = [f"knncf_{fam}_{form}{tail}" for fam in FAMILIES for form in FORMS for tail in ("", "_batch")]

TRAIN = {  # user: {item: rating}
    1: {1: 5.0, 2: 3.0, 3: 4.0, 4: 1.0},
    2: {2: 4.0, 3: 2.0, 5: 5.0, 6: 3.0},
    3: {1: 2.0, 4: 5.0, 6: 3.0, 7: 4.0},
    4: {3: 1.0, 5: 4.0, 7: 2.0, 8: 5.0},
    5: {1: 3.0, 2: 5.0, 6: 1.0, 8: 4.0},
    6: {2: 5.0, 4: 4.0, 5: 2.0, 7: 3.0, 8: 1.0},
}
# the queries of a good call: (user, removed train items, additional items, their ratings)
QUERIES = {
    "query": [(50, [], [1, 3, 6], [4.0, 2.0, 5.0]), (51, [], [2, 4], [3.0, 5.0])],
    "update": [(1, [], [5, 7], [2.0, 4.0]), (2, [], [1, 4], [4.0, 1.0])],
    "revise": [(1, [2], [5, 7], [2.0, 4.0]), (2, [], [1, 4], [4.0, 1.0])],
}
PRED_ITEMS = [1, 5, 8]
WIDTH = 2  # cap of the neighbour and explain forms, n of the recommend forms

_I32, _I64, _F64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)


def _i32(a):
    return np.asarray(a, dtype=np.int32)


def _i64(a):
    return np.asarray(a, dtype=np.int64)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _sentinel(dtype, n):
    return np.full(n, -77 if dtype == np.int32 else -77.5, dtype=dtype)


def good_call(entry, queries=None):
    """(argument names in the order of include/knncf.h, {name: value}, names of the outputs) of a call that succeeds;
    arrays are numpy arrays, outputs are sentinel-filled"""
    _, fam, form = entry.split("_")[:3]
    batch = entry.endswith("_batch")
    revise = fam == "revise"
    qs = (queries or QUERIES[fam])[: 2 if batch else 1]
    B, m = len(qs), len(PRED_ITEMS)
    a = {}
    names = [] if form == "neighbors" else ["predictor"]
    a["predictor"] = PRED_KNN
    if batch:
        names += ["users"] + (["removed_offsets", "removed_items"] if revise else []) + ["offsets", "items", "ratings", "n_queries"]
        a["users"] = _i32([q[0] for q in qs])
        a["removed_offsets"] = _i64(np.concatenate([[0], np.cumsum([len(q[1]) for q in qs])]))
        a["offsets"] = _i64(np.concatenate([[0], np.cumsum([len(q[2]) for q in qs])]))
        a["n_queries"] = B
    else:
        names += ["user"] + (["removed_items", "n_removed"] if revise else []) + ["items", "ratings", "n_ratings"]
        a["user"] = qs[0][0]
        a["n_removed"] = len(qs[0][1])
        a["n_ratings"] = len(qs[0][2])
    a["removed_items"] = _i32(np.concatenate([q[1] for q in qs]))
    a["items"] = _i32(np.concatenate([q[2] for q in qs]))
    a["ratings"] = _f64(np.concatenate([q[3] for q in qs]))
    rows = B * m
    if form in ("predict", "explain"):
        if batch:
            names += ["pred_offsets", "pred_items"]
            a["pred_offsets"] = _i64(np.arange(B + 1) * m)
        else:
            names += ["pred_items", "m"]
            a["m"] = m
        a["pred_items"] = _i32(PRED_ITEMS * B)
    count = "counts" if batch else "count"
    if form == "neighbors":
        names += ["cap", "ids", "sims", count]
        outs = {"ids": (np.int32, B * WIDTH), "sims": (np.float64, B * WIDTH), count: (np.int32, B)}
        a["cap"] = WIDTH
    elif form == "predict":
        names += ["out"]
        outs = {"out": (np.float64, rows)}
    elif form == "recommend":
        names += ["n", "out_items", "out_preds", count]
        outs = {"out_items": (np.int32, B * WIDTH), "out_preds": (np.float64, B * WIDTH), count: (np.int32, B)}
        a["n"] = WIDTH
    else:
        names += ["order", "cap", "raters", "sims", "devs", "counts", "sums", "predictions"]
        outs = {"raters": (np.int32, rows * WIDTH), "sims": (np.float64, rows * WIDTH), "devs": (np.float64, rows * WIDTH),
                "counts": (np.int32, rows), "sums": (np.float64, 2 * rows), "predictions": (np.float64, rows)}
        a["order"], a["cap"] = 0, WIDTH
    if batch:
        names += ["statuses"]
        outs["statuses"] = (np.int32, B)
    for name, (dtype, n) in outs.items():
        a[name] = _sentinel(dtype, n)
    return names, a, list(outs)


def cases_of(entry):
    """{case: {argument: replacement}} for one entry point; "handle": "unfitted" picks the handle without a fit"""
    names, a, outs = good_call(entry)
    batch = entry.endswith("_batch")
    form = entry.split("_")[2]
    cases = {"unfitted": {"handle": "unfitted"}, "good": {}}
    if batch:
        for name in ("users", "offsets", "statuses"):
            cases[f"null_{name}"] = {name: None}
        cases["n_queries_negative"] = {"n_queries": -1}
        cases["n_queries_zero"] = {"n_queries": 0}
        for name in ("offsets", "removed_offsets", "pred_offsets"):
            if name in names:
                cases[f"{name}_first_nonzero"] = {name: a[name] + 1}
                down = a[name].copy()
                down[1], down[2] = down[2] + 1, down[1]
                cases[f"{name}_decrease"] = {name: down}
    width = {"neighbors": "cap", "recommend": "n"}.get(form)
    if width:
        cases[f"{width}_negative"] = {width: -1}
    if form == "explain":
        cases["explain_order_unknown"] = {"order": 7}
        cases["explain_cap_negative"] = {"cap": -1}
    for name in outs:
        if name != "statuses":
            cases[f"null_{name}"] = {name: None}
    if "predictor" in names:
        cases["predictor_other"] = {"predictor": PRED_BASELINE}
    return cases


def call(lib, handles, entry, changes, queries=None):
    """one call with fresh sentinel outputs: (status, names of the outputs that no longer hold their sentinel, outputs)"""
    names, a, outs = good_call(entry, queries)
    a.update({k: v for k, v in changes.items() if k != "handle"})
    kept = {name: a[name] for name in outs if a[name] is not None}

    def as_arg(v):
        if v is None or not isinstance(v, np.ndarray):
            return v
        return v.ctypes.data_as({np.dtype(np.int32): _I32, np.dtype(np.int64): _I64, np.dtype(np.float64): _F64}[v.dtype])

    status = getattr(lib, entry)(handles[changes.get("handle", "fitted")], *[as_arg(a[n]) for n in names])
    touched = sorted(n for n, v in kept.items() if v.tolist() != _sentinel(v.dtype.type, len(v)).tolist())
    return status, touched, kept


def observe(lib, handles, entry):
    """what the golden file records for one entry point: {case: {"status": s, "touched": [output names]}}"""
    seen = {}
    for case, changes in cases_of(entry).items():
        status, touched, _ = call(lib, handles, entry, changes)
        seen[case] = {"status": status, "touched": touched}
    return seen


def precedence_cases():
    """{case: (entry, changes, queries or None)}: two refusals in one call"""
    cases = {}
    for fam in FAMILIES:
        for form, out in (("neighbors", "count"), ("predict", "out"), ("recommend", "count")):
            cases[f"knncf_{fam}_{form}:null_{out}_unfitted"] = (f"knncf_{fam}_{form}", {out: None, "handle": "unfitted"}, None)
        cases[f"knncf_{fam}_explain:order_unknown_unfitted"] = (f"knncf_{fam}_explain", {"order": 7, "handle": "unfitted"}, None)
        # (the neighbour forms have no predictor argument, the predict forms no width)
        cases[f"knncf_{fam}_recommend_batch:n_negative_predictor_other"] = (
            f"knncf_{fam}_recommend_batch", {"n": -1, "predictor": PRED_BASELINE}, None)
        cases[f"knncf_{fam}_explain_batch:cap_negative_predictor_other"] = (
            f"knncf_{fam}_explain_batch", {"cap": -1, "predictor": PRED_BASELINE}, None)
    # user 1 rated items 1 2 3 4 in train: item 2 removed twice, and an additional row for item 5 twice / for train item 3
    twice = [(1, [2, 2], [5, 5], [2.0, 4.0]), (2, [], [1, 4], [4.0, 1.0])]
    again = [(1, [2, 2], [5, 3], [2.0, 4.0]), (2, [], [1, 4], [4.0, 1.0])]
    for form in FORMS:
        for tail in ("", "_batch"):
            cases[f"knncf_revise_{form}{tail}:removed_twice_item_twice"] = (f"knncf_revise_{form}{tail}", {}, twice)
            cases[f"knncf_revise_{form}{tail}:removed_twice_train_item_again"] = (f"knncf_revise_{form}{tail}", {}, again)
    return cases


def observe_precedence(lib, handles):
    seen = {}
    for case, (entry, changes, queries) in precedence_cases().items():
        status, touched, kept = call(lib, handles, entry, changes, queries)
        seen[case] = {"status": status, "touched": touched}
        if "statuses" in kept:
            seen[case]["statuses"] = kept["statuses"].tolist()
    return seen


def make_handles(kn):
    """{"fitted": a handle over TRAIN, "unfitted": one that never saw a fit}, and the engines that own them"""
    u = [user for user, row in TRAIN.items() for _ in row]
    i = [item for row in TRAIN.values() for item in row]
    r = [rating for row in TRAIN.values() for rating in row.values()]
    fitted = kn.Engine(k=3)
    fitted.fit(_i32(u), _i32(i), _f64(r))
    unfitted = kn.Engine(k=3)
    return {"fitted": fitted._h, "unfitted": unfitted._h}, (fitted, unfitted)


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def handles(kn):
    hs, engines = make_handles(kn)
    yield hs
    for e in engines:
        e.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _arrays_untouched(entry, status, touched):
    """a call refused as a whole leaves every output array alone (the *count of a single form is a scalar: the record decides)"""
    if status != 0:
        assert [n for n in touched if n != "count"] == [], (entry, touched)


@pytest.mark.parametrize("entry", ENTRIES)
def test_call_level_checks(kn, handles, golden, entry):
    lib = kn.load_library()
    want = golden["entries"][entry]
    cases = cases_of(entry)
    assert sorted(cases) == sorted(want)
    for case, changes in cases.items():
        status, touched, kept = call(lib, handles, entry, changes)
        print(entry, case, status, touched)
        assert status == want[case]["status"], (case, lib.knncf_last_error(handles[changes.get("handle", "fitted")]).decode())
        assert touched == want[case]["touched"], case
        _arrays_untouched(entry, status, touched)
        if case == "n_queries_zero":
            assert status == 0 and touched == []
        if case == "good":
            assert status == 0
            if "statuses" in kept:
                assert kept["statuses"].tolist() == [0] * len(kept["statuses"])


def test_precedence_of_two_refusals(kn, handles, golden):
    lib = kn.load_library()
    want = golden["precedence"]
    cases = precedence_cases()
    assert sorted(cases) == sorted(want)
    for case, (entry, changes, queries) in cases.items():
        status, touched, kept = call(lib, handles, entry, changes, queries)
        print(case, status, touched)
        assert status == want[case]["status"], case
        assert touched == want[case]["touched"], case
        if queries is None:  # (a refused query of a single explain form has its rows' counts zeroed: the record decides)
            _arrays_untouched(entry, status, touched)
        if "statuses" in kept:
            assert kept["statuses"].tolist() == want[case]["statuses"], case
