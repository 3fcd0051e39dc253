"""The call-level checks of the 46 query entry points, asked at the C boundary with sentinel-filled outputs on every call:
knncf_{query,update,revise}_{neighbors,predict,recommend,explain} and their _batch forms (ENTRIES, 24), and the
*_explain_personalized*, *_recommend_explain*, *_bystander_* and knncf_query_entered* calls (ROWS_ENTRIES, 22).

This is a characterisation test: the status of every case, and which outputs a call wrote, are the ones recorded in
tests/golden/query_call_checks.json from a run of observe() below on the commit in front of the one that gave the query
host path its request type.  The ROWS_ENTRIES are recorded the same way in tests/golden/query_call_checks_rows.json, from the
commit in front of the one that gave the query host path one chunk view and one slot packer; that file also holds the text of
knncf_last_error of every refused case, and the statuses array where there is one.  Nothing in either file was worked out from
the code.  Beyond the recorded values the test asserts that a call that fails leaves every output array as the caller filled it.

The train set is 6 users x 8 items, made by hand: five users is the least the query path accepts and none of the checks
depends on size."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "query_call_checks.json")
GOLDEN_ROWS = os.path.join(ROOT, "tests", "golden", "query_call_checks_rows.json")
HEADER = os.path.join(ROOT, "include", "knncf.h")

PRED_BASELINE, PRED_KNN, PRED_PERSONALIZED = 3, 5, 6
FAMILIES = ("query", "update", "revise")
FORMS = ("neighbors", "predict", "recommend", "explain")
ENTRIES = [f"knncf_{fam}_{form}{tail}" for fam in FAMILIES for form in FORMS for tail in ("", "_batch")]
ROWS_ENTRIES = ([f"knncf_{fam}_{form}{tail}" for form in ("explain_personalized", "recommend_explain") for fam in FAMILIES
                 for tail in ("", "_batch")]
                + [f"knncf_{fam}_bystander_{form}{tail}" for fam in ("query", "update") for form in ("neighbors", "predict")
                   for tail in ("", "_batch")]
                + ["knncf_query_entered", "knncf_query_entered_batch"])

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
# the rows of a bystander query: two users of the fit that are not the query's, and one unknown to it
OTHERS = {"query": [1, 3, 99], "update": [3, 4, 99]}
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


def parts(entry):
    """(family, form, batch) of an entry point's name"""
    batch = entry.endswith("_batch")
    fam, form = entry[len("knncf_"): len(entry) - (len("_batch") if batch else 0)].split("_", 1)
    return fam, form, batch


def good_call(entry, queries=None):
    """(argument names in the order of include/knncf.h, {name: value}, names of the outputs) of a call that succeeds;
    arrays are numpy arrays, outputs are sentinel-filled"""
    fam, form, batch = parts(entry)
    revise = fam == "revise"
    qs = (queries or QUERIES[fam])[: 2 if batch else 1]
    B, m = len(qs), len(PRED_ITEMS)
    a = {}
    names = [] if form in ("neighbors", "explain_personalized", "bystander_neighbors", "entered") else ["predictor"]
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
    if form.startswith("bystander"):  # m rows per query: (others[r]) or (others[r], pred_items[r])
        names += (["row_offsets"] if batch else []) + ["others"] + (["pred_items"] if form == "bystander_predict" else [])
        names += [] if batch else ["m"]
        a["row_offsets"], a["m"] = _i64(np.arange(B + 1) * m), m
        a["others"], a["pred_items"] = _i32(OTHERS[fam] * B), _i32(PRED_ITEMS * B)
    if form in ("predict", "explain", "explain_personalized"):
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
    elif form == "bystander_neighbors":
        names += ["cap", "ids", "sims", "counts"]
        outs = {"ids": (np.int32, rows * WIDTH), "sims": (np.float64, rows * WIDTH), "counts": (np.int32, rows)}
        a["cap"] = WIDTH
    elif form == "entered":
        names += ["cap", "out_users", "out_sims", "out_pos", "out_displaced", count]
        outs = {"out_users": (np.int32, B * WIDTH), "out_sims": (np.float64, B * WIDTH), "out_pos": (np.int32, B * WIDTH),
                "out_displaced": (np.int32, B * WIDTH), count: (np.int32, B)}
        a["cap"] = WIDTH
    elif form in ("predict", "bystander_predict"):
        names += ["out"]
        outs = {"out": (np.float64, rows)}
    elif form == "recommend_explain":  # the explain rows are the B * n cells of the selection
        names += ["n", "order", "cap", "out_items", "out_preds", count, "raters", "sims", "devs", "term_counts", "sums"]
        cells = B * WIDTH
        outs = {"out_items": (np.int32, cells), "out_preds": (np.float64, cells), count: (np.int32, B),
                "raters": (np.int32, cells * WIDTH), "sims": (np.float64, cells * WIDTH), "devs": (np.float64, cells * WIDTH),
                "term_counts": (np.int32, cells), "sums": (np.float64, 2 * cells)}
        a["n"], a["order"], a["cap"] = WIDTH, 0, WIDTH
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
    fam, form, batch = parts(entry)
    cases = {"unfitted": {"handle": "unfitted"}, "good": {}}
    if entry in ROWS_ENTRIES:  # (the record of ENTRIES has no case for these inputs)
        for name in ("items", "ratings", "removed_offsets", "removed_items", "pred_offsets", "pred_items", "others"):
            if name in names:
                cases[f"null_{name}"] = {name: None}
    if batch:
        for name in ("users", "offsets", "statuses"):
            cases[f"null_{name}"] = {name: None}
        if "row_offsets" in names:
            cases["null_row_offsets"] = {"row_offsets": None}
        cases["n_queries_negative"] = {"n_queries": -1}
        cases["n_queries_zero"] = {"n_queries": 0}
        for name in ("offsets", "removed_offsets", "pred_offsets", "row_offsets"):
            if name in names:
                cases[f"{name}_first_nonzero"] = {name: a[name] + 1}
                down = a[name].copy()
                down[1], down[2] = down[2] + 1, down[1]
                cases[f"{name}_decrease"] = {name: down}
    width = {"neighbors": "cap", "recommend": "n", "recommend_explain": "n", "bystander_neighbors": "cap", "entered": "cap"}.get(form)
    if width:
        cases[f"{width}_negative"] = {width: -1}
    if form in ("explain", "explain_personalized", "recommend_explain"):
        cases["explain_order_unknown"] = {"order": 7}
        cases["explain_cap_negative"] = {"cap": -1}
    if form.startswith("bystander"):
        if not batch:
            cases["m_negative"] = {"m": -1}
        # a per-query refusal: a row that names the query's own user
        own = a["others"].copy()
        own[1] = QUERIES[fam][0][0]
        cases["query_own_user_row"] = {"others": own}
        if fam == "update" and not batch:  # (user 1 is in the fit, user 77 is not)
            cases["n_ratings_zero_fitted"] = {"n_ratings": 0}
            cases["query_n_ratings_zero_absent"] = {"n_ratings": 0, "user": 77}
        if fam == "update" and batch:
            cases["n_ratings_zero_fitted"] = {"offsets": _i64([0, 0, 2]), "items": a["items"][2:], "ratings": a["ratings"][2:]}
            cases["query_n_ratings_zero_absent"] = {"offsets": _i64([0, 0, 2]), "items": a["items"][2:], "ratings": a["ratings"][2:],
                                                    "users": _i32([77, 2])}
    if form == "entered":
        cases["cap_zero"] = {"cap": 0}
        cases["cap_zero_null_outputs"] = {"cap": 0, "out_users": None, "out_sims": None, "out_pos": None, "out_displaced": None}
        cases["cosine_short_rows"] = {"handle": "fitted"}
    for name in outs:
        if name != "statuses":
            cases[f"null_{name}"] = {name: None}
    if "predictor" in names:
        cases["predictor_other"] = {"predictor": PRED_BASELINE}
        if form == "bystander_predict":
            cases["predictor_personalized"] = {"predictor": PRED_PERSONALIZED}
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

    status = getattr(lib, entry)(handle_of(handles, entry, changes), *[as_arg(a[n]) for n in names])
    touched = sorted(n for n, v in kept.items() if v.tolist() != _sentinel(v.dtype.type, len(v)).tolist())
    return status, touched, kept


def handle_of(handles, entry, changes):
    """the handle of a case: the entered calls refuse a cosine fit with users of four ratings, so theirs is the Jaccard one"""
    return handles[changes.get("handle", "fitted_jaccard" if parts(entry)[1] == "entered" else "fitted")]


def record(lib, handles, entry, changes, queries, rows):
    """one call as the golden files record it; rows: with the statuses array and, for a call that refused anything, the text of
    knncf_last_error (a call that refused nothing leaves the text of an earlier call in place)"""
    status, touched, kept = call(lib, handles, entry, changes, queries)
    seen = {"status": status, "touched": touched}
    if "statuses" in kept:
        seen["statuses"] = kept["statuses"].tolist()
    if rows:
        refused = status != 0 or ("statuses" in touched and any(seen["statuses"]))
        seen["error"] = lib.knncf_last_error(handle_of(handles, entry, changes)).decode() if refused else ""
    return seen, kept


def observe(lib, handles, entry):
    """what the golden files record for one entry point: {case: {"status": s, "touched": [output names]}}, and for the
    ROWS_ENTRIES "statuses" and "error" beside them"""
    rows = entry in ROWS_ENTRIES
    seen = {}
    for case, changes in cases_of(entry).items():
        seen[case], kept = record(lib, handles, entry, changes, None, rows)
        if not rows:
            seen[case].pop("statuses", None)
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


def precedence_cases_rows():
    """{case: (entry, changes, queries or None)} for the ROWS_ENTRIES: two refusals in one call, and the per-query refusal of an
    item given twice on its own"""
    cases = {}
    null_out = {"explain_personalized": "counts", "recommend_explain": "count", "bystander_neighbors": "counts",
                "bystander_predict": "out", "entered": "count"}
    # the first query rates an item twice: item 1 for the absent user 50, item 5 for user 1 of the fit (train items 1 2 3 4)
    twice = {"query": [(50, [], [1, 1, 6], [4.0, 2.0, 5.0]), QUERIES["query"][1]],
             "update": [(1, [], [5, 5], [2.0, 4.0]), QUERIES["update"][1]],
             "revise": [(1, [2], [5, 5], [2.0, 4.0]), QUERIES["revise"][1]]}
    for entry in ROWS_ENTRIES:
        fam, form, batch = parts(entry)
        out = null_out[form] + ("s" if batch and null_out[form] == "count" else "")
        cases[f"{entry}:null_{out}_unfitted"] = (entry, {out: None, "handle": "unfitted"}, None)
        cases[f"{entry}:item_twice"] = (entry, {}, twice[fam])
        if form == "recommend_explain":
            cases[f"{entry}:n_negative_predictor_other"] = (entry, {"n": -1, "predictor": PRED_BASELINE}, None)
            cases[f"{entry}:cap_negative_predictor_other"] = (entry, {"cap": -1, "predictor": PRED_BASELINE}, None)
            cases[f"{entry}:order_unknown_unfitted"] = (entry, {"order": 7, "handle": "unfitted"}, None)
        if form == "explain_personalized":
            cases[f"{entry}:cap_negative_order_unknown"] = (entry, {"cap": -1, "order": 7}, None)
            cases[f"{entry}:order_unknown_null_raters"] = (entry, {"order": 7, "raters": None}, None)
        if form.startswith("bystander"):
            own = _i32(OTHERS[fam] * 2)
            own[1] = twice[fam][0][0]
            cases[f"{entry}:item_twice_own_user_row"] = (entry, {"others": own}, twice[fam])
            cases[f"{entry}:null_others_unfitted"] = (entry, {"others": None, "handle": "unfitted"}, None)
        if form == "bystander_neighbors":
            cases[f"{entry}:cap_negative_null_others"] = (entry, {"cap": -1, "others": None}, None)
        if form == "bystander_predict":
            cases[f"{entry}:predictor_other_null_out"] = (entry, {"predictor": PRED_BASELINE, "out": None}, None)
        if form == "entered":
            cases[f"{entry}:cap_negative_cosine_short_rows"] = (entry, {"cap": -1, "handle": "fitted"}, None)
            cases[f"{entry}:null_out_pos_cosine_short_rows"] = (entry, {"out_pos": None, "handle": "fitted"}, None)
    return cases


def observe_precedence(lib, handles, rows=False):
    seen = {}
    for case, (entry, changes, queries) in (precedence_cases_rows() if rows else precedence_cases()).items():
        seen[case], _ = record(lib, handles, entry, changes, queries, rows)
    return seen


def observe_rows(lib, handles):
    """the whole of tests/golden/query_call_checks_rows.json"""
    return {"entries": {entry: observe(lib, handles, entry) for entry in ROWS_ENTRIES}, "precedence": observe_precedence(lib, handles, True)}


def make_handles(kn):
    """{"fitted": a handle over TRAIN, "fitted_jaccard": the same under the Jaccard similarity, "unfitted": one that never saw a
    fit}, and the engines that own them"""
    u = [user for user, row in TRAIN.items() for _ in row]
    i = [item for row in TRAIN.values() for item in row]
    r = [rating for row in TRAIN.values() for rating in row.values()]
    fitted = kn.Engine(k=3)
    fitted.fit(_i32(u), _i32(i), _f64(r))
    jaccard = kn.Engine(k=3, similarity=kn.SIM_JACCARD)
    jaccard.fit(_i32(u), _i32(i), _f64(r))
    unfitted = kn.Engine(k=3)
    return {"fitted": fitted._h, "fitted_jaccard": jaccard._h, "unfitted": unfitted._h}, (fitted, jaccard, unfitted)


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


# ---- the ROWS_ENTRIES: tests/golden/query_call_checks_rows.json ---------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_rows():
    with open(GOLDEN_ROWS) as f:
        return json.load(f)


def header_arguments(entry):
    """the argument names of an entry point's prototype in include/knncf.h, without the handle"""
    with open(HEADER) as f:
        text = f.read()
    args = re.search(r"\bint " + entry + r"\(([^)]*)\);", text).group(1)
    return [re.split(r"[\s*]+", arg.strip())[-1] for arg in args.split(",")][1:]


@pytest.mark.parametrize("entry", ROWS_ENTRIES)
def test_cases_follow_the_header(entry):
    """good_call passes the arguments of include/knncf.h in its order, so cases_of covers what the header declares: every
    pointer argument has its null case, and the explain_personalized forms have no predictor to refuse"""
    names, a, outs = good_call(entry)
    assert names == header_arguments(entry)
    cases = cases_of(entry)
    for name in names:
        if isinstance(a[name], np.ndarray):
            assert f"null_{name}" in cases, name
    form = parts(entry)[1]
    assert ("predictor" in names) == (form in ("recommend_explain", "bystander_predict"))
    assert ("predictor_other" in cases) == ("predictor" in names)


def _rows_untouched(entry, per_query, status, touched):
    """a call refused as a whole leaves every output array alone.  The *count of a single form is a scalar, and a single form
    whose one query is refused has zeroed that query's rows of counts (explain_personalized, bystander_neighbors): the record
    decides those"""
    allowed = {"count"}
    if per_query and parts(entry)[1] in ("explain_personalized", "bystander_neighbors"):
        allowed.add("counts")
    if status != 0:
        assert [n for n in touched if n not in allowed] == [], (entry, touched)


def _check_recorded(lib, handles, want, case, entry, changes, queries):
    seen, kept = record(lib, handles, entry, changes, queries, True)
    print(case, seen)
    assert seen["status"] == want["status"], (case, lib.knncf_last_error(handle_of(handles, entry, changes)).decode())
    assert seen["touched"] == want["touched"], case
    assert seen.get("statuses") == want.get("statuses"), case
    assert seen["error"] == want["error"], case
    return seen, kept


@pytest.mark.parametrize("entry", ROWS_ENTRIES)
def test_call_level_checks_rows(kn, handles, golden_rows, entry):
    lib = kn.load_library()
    want = golden_rows["entries"][entry]
    cases = cases_of(entry)
    assert sorted(cases) == sorted(want)
    for case, changes in cases.items():
        seen, kept = _check_recorded(lib, handles, want[case], f"{entry}:{case}", entry, changes, None)
        _rows_untouched(entry, case.startswith("query_"), seen["status"], seen["touched"])
        if case == "n_queries_zero":
            assert seen["status"] == 0 and seen["touched"] == []
        if case in ("good", "n_ratings_zero_fitted", "cap_zero", "cap_zero_null_outputs"):
            assert seen["status"] == 0
            if "statuses" in kept:
                assert kept["statuses"].tolist() == [0] * len(kept["statuses"])


def test_precedence_of_two_refusals_rows(kn, handles, golden_rows):
    lib = kn.load_library()
    want = golden_rows["precedence"]
    cases = precedence_cases_rows()
    assert sorted(cases) == sorted(want)
    for case, (entry, changes, queries) in cases.items():
        seen, _ = _check_recorded(lib, handles, want[case], case, entry, changes, queries)
        _rows_untouched(entry, queries is not None, seen["status"], seen["touched"])
