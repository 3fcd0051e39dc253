"""knncf_explain_personalized*: the terms behind the Personalized predictions of fitted users, bit for bit.

The expected terms come from tests/personalized_explain_model.py, which derives them from the CPU oracle's raw similarities,
deviations and the training file (test_personalized_explain_premises.py shows on the CPU that their fold IS the oracle's wsd
and prediction, and that every input has the feature its test here relies on).  Every comparison is == on int32 ids and on
fp64 bit patterns.  Raw calls through the C ABI with sentinel-filled outputs prove which cells a call writes;
KNNCF_DEBUG_TRACE_DISPATCH lines on the library's stderr show the launches."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest

from tests import personalized_explain_model as pm
from tests.personalized_explain_model import ABSENT_ITEM, ABSENT_USER, BY_WEIGHT, SUM_ORDER
from tests.test_gpu_recommend_batch import _table

pytestmark = pytest.mark.gpu
TRACE = "KNNCF_DEBUG_TRACE_DISPATCH"
STREAM = "KNNCF_DEBUG_PERSONALIZED_STREAM"
SENT_I, SENT_F = -7, 7.5
i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _sims(kn, oracle, name):
    return {"cosine": (kn.SIM_COSINE, oracle.SIM_COSINE), "jaccard": (kn.SIM_JACCARD, oracle.SIM_JACCARD)}[name]


def _raw(e, users, items, cap, order=SUM_ORDER, null_terms=False, null_sums=False):
    """knncf_explain_personalized_batch through the C ABI on sentinel-filled outputs: (status, raters, sims, devs, counts, sums,
    preds)"""
    u, i = np.ascontiguousarray(users, dtype=np.int32), np.ascontiguousarray(items, dtype=np.int32)
    n = len(u)
    w = max(cap, 0)
    raters = np.full((n, w), SENT_I, dtype=np.int32)
    sims, devs = np.full((n, w), SENT_F), np.full((n, w), SENT_F)
    counts = np.full(n, SENT_I, dtype=np.int32)
    sums, preds = np.full((n, 2), SENT_F), np.full(n, SENT_F)
    p = lambda a, t: None if a.size == 0 else a.ctypes.data_as(t)
    terms = (None, None, None) if null_terms else (p(raters, i32p), p(sims, f64p), p(devs, f64p))
    st = e._lib.knncf_explain_personalized_batch(e._h, p(u, i32p), p(i, i32p), n, order, cap, *terms, p(counts, i32p),
                                                 None if null_sums else p(sums, f64p), None if null_sums else p(preds, f64p))
    return st, raters, sims, devs, counts, sums, preds


def _assert_rows(got, want_rows, order, what, pad=(-1, np.nan)):
    """a result against the model's rows: counts, sums, predictions, the first min(count, cap) terms in `order`, and the
    cells beyond them as the caller left them"""
    raters, sims, devs, counts, sums, preds = got
    cap = raters.shape[1]
    assert counts.tolist() == [r.count for r in want_rows], what
    assert np.array_equal(_bits(sums), _bits([[r.num, r.den] for r in want_rows])), what
    assert np.array_equal(_bits(preds), _bits([r.prediction for r in want_rows])), what
    for j, row in enumerate(want_rows):
        r, s, d = row.terms(order)
        m = min(row.count, cap)
        assert raters[j, :m].tolist() == r[:m].tolist(), (what, j)
        assert np.array_equal(_bits(sims[j, :m]), _bits(s[:m])) and np.array_equal(_bits(devs[j, :m]), _bits(d[:m])), (what, j)
        assert (raters[j, m:] == pad[0]).all(), (what, j)
        for x in (sims[j, m:], devs[j, m:]):
            assert np.isnan(x).all() if np.isnan(pad[1]) else (x == pad[1]).all(), (what, j)


def _same(a, b):
    return all(np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y)
               for x, y in zip(a, b))


def _free_device_bytes():
    """hipMemGetInfo's free bytes of device 0, from the HIP runtime the library is bound to"""
    import importlib.util
    import os

    spec = importlib.util.find_spec("torch")
    names = [os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")] if spec and spec.origin else []
    for name in names + ["libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"]:
        try:
            hip = C.CDLL(name)
        except OSError:
            continue
        free, total = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value
    raise AssertionError("no HIP runtime found")


def _launches(capfd):
    """(order, cap, rows) of every explain_all dispatch line since the last look"""
    found = re.findall(r"^knncf-dispatch explain_all order=(\d+) cap=(\d+) rows=(\d+)$", capfd.readouterr().err, flags=re.M)
    return [tuple(int(x) for x in f) for f in found]


# ---- shared, unchanged state --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return pm.small_case()


@pytest.fixture(scope="module")
def want_small(oracle, small):
    """similarity name -> the model's rows of the small case, computed once"""
    cache = {}

    def get(sim_name):
        if sim_name not in cache:
            osim = {"cosine": oracle.SIM_COSINE, "jaccard": oracle.SIM_JACCARD}[sim_name]
            cache[sim_name] = pm.PersonalTermModel(oracle, oracle.Model(*small[0]), osim).rows(small[1], small[2])
        return cache[sim_name]

    return get


# ---- 1. both orders and a range of caps, against the model and against both fitted regimes of the predictor -----------------
@pytest.mark.parametrize("regime", ["table", "stream"])
@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_orders_and_caps_against_the_model(kn, oracle, small, want_small, monkeypatch, sim_name, regime):
    train, u, i = small
    want = want_small(sim_name)
    count = max(r.count for r in want)
    e = kn.Engine(k=10, similarity=_sims(kn, oracle, sim_name)[0]).fit(*train)
    if regime == "stream":
        monkeypatch.setenv(STREAM, "1")
    yardstick = e.predict_batch(kn.PRED_PERSONALIZED, u, i)
    monkeypatch.delenv(STREAM, raising=False)
    ua = {int(x): e.user_avg(int(x)) for x in np.unique(u) if x != ABSENT_USER}
    for order in (SUM_ORDER, BY_WEIGHT):
        for cap in pm.caps_of(count):
            st, *got = _raw(e, u, i, cap, order, null_terms=cap == 0)
            assert st == kn.OK, (order, cap)
            _assert_rows(got, want, order, (sim_name, order, cap), pad=(SENT_I, SENT_F))
            raters, sims, devs, counts, sums, preds = got
            assert np.array_equal(_bits(preds), _bits(yardstick)), (order, cap)
            for j in np.flatnonzero(counts <= cap):  # the caller's left fold and combine
                m = counts[j]
                if order == SUM_ORDER:
                    assert np.array_equal(_bits(pm.fold(sims[j, :m], devs[j, :m])), _bits(sums[j])), (cap, j)
                if int(u[j]) in ua and ua[int(u[j])] >= 0:
                    assert _bits(pm.combine(oracle, ua[int(u[j])], *sums[j].tolist())) == _bits(preds[j]), (cap, j)
    st, *_, counts, sums, preds = _raw(e, u, i, 3, BY_WEIGHT, null_sums=True)  # sums and predictions may be null
    assert st == kn.OK and counts.tolist() == [r.count for r in want] and (sums == SENT_F).all() and (preds == SENT_F).all()
    # the single call is the batch of one row (cap=None: num_users)
    for j in (0, len(want) // 2, len(want) - 1):
        r, s, d, c, (num, den), pred = e.explain_personalized(int(u[j]), int(i[j]), cap=None, order=BY_WEIGHT)
        wr, ws, wd = want[j].terms(BY_WEIGHT)
        assert c == want[j].count and r.tolist() == wr.tolist() and np.array_equal(_bits(s), _bits(ws)) and np.array_equal(_bits(d), _bits(wd))
        assert np.array_equal(_bits([num, den, pred]), _bits([want[j].num, want[j].den, want[j].prediction]))
    e.close()


# ---- 2. segment-length edges: 64 raters per load of the walk, 256 per load group of the select and emit passes, 64 staged keys
# per sweep step and 256 staged terms per sweep of the rank ---------------------------------------------------------------------
@pytest.mark.parametrize("n_users", [63, 64, 65, 255, 256, 257, 600])
def test_segment_length_edges(kn, oracle, n_users):
    train, u, i = pm.dense_case(n_users)
    want = pm.PersonalTermModel(oracle, oracle.Model(*train), oracle.SIM_COSINE).rows(u, i)
    assert [r.count for r in want[:3]] == [n_users] * 3
    e = kn.Engine(k=10).fit(*train)
    for order, cap in ((BY_WEIGHT, 16), (BY_WEIGHT, n_users), (SUM_ORDER, n_users), (BY_WEIGHT, n_users - 1)):
        _assert_rows(e.explain_personalized_batch(u, i, cap, order=order), want, order, (n_users, order, cap))
    e.close()


# ---- 3. ties: a cap that ends inside a group of equal magnitudes keeps the earliest in summation order ----------------------
@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_caps_inside_tie_groups_keep_the_earliest(kn, oracle, sim_name):
    train, u, i = pm.clone_case()
    ksim, osim = _sims(kn, oracle, sim_name)
    want = pm.PersonalTermModel(oracle, oracle.Model(*train), osim).rows(u, i)
    cuts = {}  # cap -> rows it cuts inside a tie group
    for j, r in enumerate(want):
        s = np.abs(r.sims[r.by_weight])
        for cap in range(1, r.count):
            if s[cap - 1] == s[cap]:
                cuts.setdefault(cap, []).append(j)
    caps = sorted(cuts, key=lambda c: -len(cuts[c]))[:4]
    assert caps
    e = kn.Engine(k=10, similarity=ksim).fit(*train)
    full = e.explain_personalized_batch(u, i, max(r.count for r in want), order=SUM_ORDER)
    for cap in caps:
        got = e.explain_personalized_batch(u, i, cap, order=BY_WEIGHT)
        _assert_rows(got, want, BY_WEIGHT, (sim_name, cap))
        for j in cuts[cap]:
            t = abs(got[1][j, cap - 1])  # the magnitude the cap cuts through
            place = {r: q for q, r in enumerate(full[0][j, :full[3][j]].tolist())}  # (a rater occurs once per item)
            tied = [q for q in range(full[3][j]) if abs(full[1][j, q]) == t]
            kept = [place[int(r)] for r, s in zip(got[0][j], got[1][j]) if abs(s) == t]
            assert kept == tied[:len(kept)] and len(kept) < len(tied), (cap, j)
    e.close()


# ---- 4. zero similarities: raters that are no terms ---------------------------------------------------------------------------
@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_zero_similarity_raters_are_no_terms(kn, oracle, sim_name):
    train, u, i, cold = pm.disjoint_case()
    ksim, osim = _sims(kn, oracle, sim_name)
    want = pm.PersonalTermModel(oracle, oracle.Model(*train), osim).rows(u, i)
    e = kn.Engine(k=10, similarity=ksim).fit(*train)
    cap = max(r.count for r in want)
    for order in (SUM_ORDER, BY_WEIGHT):
        got = e.explain_personalized_batch(u, i, cap, order=order)
        _assert_rows(got, want, order, (sim_name, order))
    raters, _, _, counts, sums, preds = got
    cold = set(cold.tolist())
    lonely = [j for j in range(len(u)) if int(u[j]) in cold and counts[j] == 0]
    assert lonely
    for j in lonely:  # every rater at similarity 0.0: count 0, sums (+0.0, +0.0), the mean
        assert _bits(sums[j]).tolist() == [0, 0] and _bits(preds[j]) == _bits(e.user_avg(int(u[j])))
    for j in range(len(u)):
        if int(u[j]) not in cold:
            assert not cold & set(raters[j, :min(counts[j], cap)].tolist()), j
    e.close()


# ---- 5. row kinds by hand -----------------------------------------------------------------------------------------------------
def test_row_kinds(kn, oracle, small, want_small):
    train, su, si = small
    e = kn.Engine(k=10).fit(*train)
    known = int(train[0][4321])
    own_item = int(train[1][4321])
    u = np.array([ABSENT_USER, known, known, known], dtype=np.int32)
    i = np.array([own_item, ABSENT_ITEM, own_item, own_item], dtype=np.int32)
    cap = e.num_users
    raters, sims, devs, counts, sums, preds = e.explain_personalized_batch(u, i, cap)
    assert counts[0] == 0 and _bits(sums[0]).tolist() == [0, 0] and _bits(preds[0]) == _bits(e.global_avg())
    assert counts[1] == 0 and _bits(sums[1]).tolist() == [0, 0] and _bits(preds[1]) == _bits(e.user_avg(known))
    # the same user twice: the same row twice
    assert counts[2] == counts[3] and all(np.array_equal(_bits(a[2, :counts[2]]), _bits(a[3, :counts[2]])) for a in (sims, devs))
    # a training pair: the own term, at its file place among the item's raters, with weight S(u, u)
    file_raters = train[0][train[1] == own_item].tolist()
    got = raters[2, :counts[2]].tolist()
    assert known in got and got == [x for x in file_raters if x in set(got)]
    model = pm.PersonalTermModel(oracle, oracle.Model(*train), oracle.SIM_COSINE)
    assert _bits(sims[2, got.index(known)]) == _bits(model.similarity(known, known))
    assert got == model.row(known, own_item).raters.tolist()
    e.close()
    # a user whose mean is negative: the global average, no terms; as a rater it is a term of other users' rows
    train, u, i, low = pm.negative_case()
    want = pm.PersonalTermModel(oracle, oracle.Model(*train), oracle.SIM_COSINE).rows(u, i)
    e = kn.Engine(k=10).fit(*train)
    assert all(e.user_avg(int(x)) < 0 for x in low)
    got = e.explain_personalized_batch(u, i, 48, order=BY_WEIGHT)
    _assert_rows(got, want, BY_WEIGHT, "negative")
    assert got[3].tolist()[:2] == [0, 0] and _bits(got[5][0]) == _bits(e.global_avg()) and set(low.tolist()) <= set(got[0][2].tolist())
    e.close()


# ---- 6. blocks and sub-ranges, allocations, dispatch --------------------------------------------------------------------------
def test_blocks_and_sub_ranges_do_not_show(kn, oracle, small, want_small, monkeypatch, capfd):
    train, u, i = small
    want = want_small("cosine")
    cap, workspace = 64, 16 << 10
    n, U = len(u), len(np.unique(train[0]))
    per_block = (workspace // 2) // (8 * U)  # users per block: the rule of include/knncf.h
    sub = (workspace // 2) // (40 * cap + 28)  # rows per launch
    distinct = len({int(x) for x, y in zip(u, i) if x != ABSENT_USER and y != ABSENT_ITEM})
    assert 1 <= per_block and -(-distinct // per_block) >= 3 and 1 <= sub and -(-n // sub) >= 3
    monkeypatch.setenv(TRACE, "1")
    tight = kn.Engine(k=10, workspace_bytes=workspace).fit(*train)
    roomy = kn.Engine(k=10).fit(*train)
    for order in (SUM_ORDER, BY_WEIGHT):
        capfd.readouterr()
        a = tight.explain_personalized_batch(u, i, cap, order=order)
        lines = _launches(capfd)
        assert len(lines) >= max(-(-distinct // per_block), -(-n // sub)) and sum(ln[2] for ln in lines) == n
        assert all(ln[:2] == (order, cap) and 1 <= ln[2] <= sub for ln in lines)
        b = roomy.explain_personalized_batch(u, i, cap, order=order)
        assert _launches(capfd) == [(order, cap, n)]  # one launch, one line
        assert _same(a, b), order
        _assert_rows(a, want, order, order)
        for e in (tight, roomy):  # a repeated call of the same shape allocates no device memory (a call returns drained)
            free = _free_device_bytes()
            again = e.explain_personalized_batch(u, i, cap, order=order)
            assert _free_device_bytes() >= free and _same(a, again), order
    tight.close()
    roomy.close()


# ---- 7. read-only on the kNN state; timings -----------------------------------------------------------------------------------
def test_read_only_and_timings(kn, small, tmp_path):
    train, u, i = small
    e = kn.Engine(k=10).fit(*train)
    some = np.unique(u[u != ABSENT_USER])[:5]
    lists = e.neighbors_batch(some)
    before = _table(e, tmp_path / "before.nb")
    assert sum(s >= 0 for s in before["seq"]) >= 5
    e.reset_timings()
    first = e.explain_personalized_batch(u, i, 16, order=BY_WEIGHT)
    t = e.timings()
    assert t["prep_ms"] > 0 and t["rerank_ms"] > 0 and t["predict_ms"] > 0  # rater copies, similarity rows, everything else
    assert all(t[name] == 0 for name in ("densify_ms", "gemm_ms", "tail_ms", "select_ms", "gemm_launches", "select_launches"))
    e.reset_timings()
    again = e.explain_personalized_batch(u, i, 16, order=BY_WEIGHT)
    t = e.timings()
    assert t["prep_ms"] == 0 and t["rerank_ms"] > 0 and t["predict_ms"] > 0 and _same(first, again)
    assert _table(e, tmp_path / "after.nb") == before
    assert open(tmp_path / "after.nb", "rb").read() == open(tmp_path / "before.nb", "rb").read()
    assert _same(lists, e.neighbors_batch(some))
    e.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(kn, small, tmp_path):
    train, su, si = small
    u, i = su[:5], si[:5]

    def untouched(res):
        return all((x == (SENT_I if x.dtype == np.int32 else SENT_F)).all() for x in res[1:])

    fresh = kn.Engine(k=10)
    res = _raw(fresh, u, i, 4)
    assert res[0] == kn.E_STATE and untouched(res)
    fresh.close()
    one = kn.Engine(k=10, similarity=kn.SIM_ONE).fit(*train)
    res = _raw(one, u, i, 4)
    assert res[0] == kn.E_UNSUPPORTED and untouched(res)
    with pytest.raises(kn.KnncfError, match="nothing to explain") as err:
        one.explain_personalized_batch(u, i, 4)
    assert err.value.status == kn.E_UNSUPPORTED
    one.close()
    shard = kn.Engine(k=10, shard_rank=0, shard_count=2).fit(*train)
    res = _raw(shard, u, i, 4)
    assert res[0] == kn.E_UNSUPPORTED and untouched(res)
    shard.close()
    # the adjusted cosine with a train user of 4 or fewer ratings: refused as the fitted predictor refuses it; Jaccard answers
    tu, ti, tr = train
    short = np.concatenate([tu, np.full(3, 555_555, dtype=tu.dtype)]), np.concatenate([ti, ti[:3]]), np.concatenate([tr, tr[:3]])
    few = kn.Engine(k=10).fit(*short)
    with pytest.raises(kn.KnncfError) as err:
        few.predict_batch(kn.PRED_PERSONALIZED, u, i)
    assert err.value.status == kn.E_UNSUPPORTED
    for _ in range(2):  # (the refusal does not wear off)
        res = _raw(few, u, i, 4)
        assert res[0] == kn.E_UNSUPPORTED and untouched(res)
    few.close()
    few = kn.Engine(k=10, similarity=kn.SIM_JACCARD).fit(*short)
    assert _raw(few, u, i, 4)[0] == kn.OK
    few.close()
    e = kn.Engine(k=10).fit(*train)
    before = _table(e, tmp_path / "before.nb")
    for order, cap in ((2, 4), (-1, 4), (SUM_ORDER, -1)):
        res = _raw(e, u, i, cap, order)
        assert res[0] == kn.E_INVALID and untouched(res), (order, cap)
    res = _raw(e, u, i, 4, null_terms=True)  # cap > 0 needs the term arrays
    assert res[0] == kn.E_INVALID and untouched(res)
    p = lambda a, t: a.ctypes.data_as(t)
    counts = np.full(5, SENT_I, dtype=np.int32)
    f = e._lib.knncf_explain_personalized_batch
    assert f(e._h, p(u, i32p), p(i, i32p), -1, 0, 0, None, None, None, p(counts, i32p), None, None) == kn.E_INVALID
    assert f(e._h, p(u, i32p), p(i, i32p), 2**32 - 1, 0, 0, None, None, None, p(counts, i32p), None, None) == kn.E_INVALID
    assert f(e._h, p(u, i32p), None, 5, 0, 0, None, None, None, p(counts, i32p), None, None) == kn.E_INVALID
    assert f(e._h, p(u, i32p), p(i, i32p), 5, 0, 0, None, None, None, None, None, None) == kn.E_INVALID
    assert f(e._h, None, None, 0, 0, 4, None, None, None, None, None, None) == kn.OK  # n == 0
    assert (counts == SENT_I).all() and _table(e, tmp_path / "after.nb") == before  # nothing built, nothing written
    e.close()
