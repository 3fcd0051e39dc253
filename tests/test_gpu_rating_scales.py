"""Ratings off the MovieLens star scale, the HIP engine against the CPU oracle: non-dyadic ratings (the sequential average,
the file-order fold of usersAvg), the two limits of the dyadic rule, fitted users with a negative mean (answered with the
global average :572-573 by every predictor), predictions of both signs (the sign branch of the recommendation keys) and
deviations beyond [-1, 1].  The cases are tests/rating_scales.py; tests/test_rating_scale_premises.py shows on the CPU that
each sits where it claims and that the oracle equals the literal Scala model on these domains.  Every comparison is on bit
patterns except the MAE, which is held to MAE_TOL * max(1, the oracle's MAE): the errors here are not O(1)."""
import importlib

import numpy as np
import pytest

from tests import explain_model, rating_scales as rs
from tests.explain_model import BY_WEIGHT, SUM_ORDER
from tests.query_helpers import _same_pair
from tests.test_gpu_explain import _assert_rows
from tests.test_gpu_fold_in import _check as _check_fold_in
from tests.test_gpu_k_classes import MAE_TOL, PATH_ENV, _handle, _knn_lines, _predict_line, _trace, handles  # noqa: F401
from tests.test_gpu_revise import _check as _check_revise
from tests.test_gpu_update import _check as _check_update
from tests.test_oracle_semantics import _no_zero_scale

pytestmark = pytest.mark.gpu
SEEDS = range(4)
WIDE_KS = (10, 300)
SWEEP_KS = (10, 300, 942)
RECO_NS = (3, 32, 33, None)  # the arg-min selection, its limit RB_FAST_N, the segmented full order, every item


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(got, want, what=""):
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), np.asarray(got)[bad[:8]].tolist(), np.asarray(want)[bad[:8]].tolist())


def _mae_close(got, want, what=""):
    assert abs(got - want) <= MAE_TOL * max(1.0, want), (what, got, want)


def _means_equal_the_oracle(e, m, tr):
    assert _bits(e.global_avg()) == _bits(m.average())
    users, items = np.unique(tr[0]).tolist(), np.unique(tr[1]).tolist()
    _same_bits([e.user_avg(u) for u in users], [m.users_avg(u) for u in users], "user_avg")
    _same_bits([e.item_avg(i) for i in items], [m.items_avg(i) for i in items], "item_avg")


# ---- small cases of every domain ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("domain", rs.DOMAINS)
def test_small_cases_bitwise(kn, oracle, domain, seed):
    """test_gpu_parity.test_random_small_cases_bitwise on every rating domain (the same cases as the premise file's)"""
    rng = np.random.default_rng([1234, rs.DOMAINS.index(domain), seed])
    train, test = rs.split_small(rs.small_case(rng, domain, tiny_rows=seed % 3))
    if not _no_zero_scale(train):
        pytest.skip("scale() == 0 corner")
    tr, te = rs.cols(train), rs.cols(test)
    m = oracle.Model(*tr)
    users, items = np.unique(tr[0]).tolist(), np.unique(tr[1]).tolist()
    for k in (1, 4, len(users) + 3):
        e = kn.Engine(k=k, flags=kn.FLAG_VERIFY_BOUND).fit(*tr)
        _means_equal_the_oracle(e, m, tr)
        _same_bits([e.item_avg_dev(i) for i in items], [m.items_avg_dev(i) for i in items], "item_avg_dev")
        _same_bits([e.item_avg_dev_rdd(i) for i in items], [m.items_avg_dev_spark(i) for i in items], "item_avg_dev_rdd")
        for kind, okind in ((kn.PRED_GLOBAL_AVG, oracle.KIND_GLOBAL), (kn.PRED_USER_AVG, oracle.KIND_USER),
                            (kn.PRED_ITEM_AVG, oracle.KIND_ITEM), (kn.PRED_BASELINE, oracle.KIND_BASELINE),
                            (kn.PRED_BASELINE_RDD, oracle.KIND_BASELINE_SPARK)):
            want, preds = m.mae(okind, *te, True)
            _same_bits(e.predict_batch(kind, te[0], te[1]), preds, (kind, k))
            _mae_close(e.mae(kind, *te), want, (kind, k))
        p = m.pipeline(oracle.SIM_COSINE, k)  # the timed expression of predict/kNN.scala:42-45: the same closure history
        want, preds = p.mae(*te, True)
        got = e.mae(kn.PRED_KNN, *te)
        _same_bits(e.predict_batch(kn.PRED_KNN, te[0], te[1]), preds, ("knn", k))
        _mae_close(got, want, ("knn", k))
        for u in users:
            ids, sims = e.neighbors(u)
            oids, osims = p.neighbors(u)
            assert ids.tolist() == oids.tolist(), (u, k)
            _same_bits(sims, osims, (u, k))
        assert e.timings()["max_bound_violation"] <= 0.0
        e.close()
    pu = np.concatenate([te[0], tr[0][:12]])
    pi = np.concatenate([te[1], tr[1][:12]])
    jac = kn.Engine(similarity=kn.SIM_JACCARD).fit(*tr)
    pj = m.pipeline(oracle.SIM_JACCARD, -1)
    _same_bits(jac.predict_batch(kn.PRED_PERSONALIZED, pu, pi), [pj.predict(int(a), int(b)) for a, b in zip(pu, pi)], "jaccard")
    jac.close()
    cosp = kn.Engine(similarity=kn.SIM_COSINE).fit(*tr)
    if np.bincount(np.unique(tr[0], return_inverse=True)[1]).min() > 4:
        pc = m.pipeline(oracle.SIM_COSINE, -1)
        _same_bits(cosp.predict_batch(kn.PRED_PERSONALIZED, pu, pi), [pc.predict(int(a), int(b)) for a, b in zip(pu, pi)], "cosine")
    else:  # the summation order of a <= 4-rating pair depends on the memo history: refused, not approximated
        with pytest.raises(kn.KnncfError):
            cosp.predict_batch(kn.PRED_PERSONALIZED, pu, pi)
    cosp.close()


def test_negative_mean_test_rows_build_no_neighbourhood(kn, oracle):
    """rating_scales.history_case: the predictor answers a negative-mean user at :573 before weightedSumDeviation runs, so
    its test rows leave the memo history alone; the lists queried afterwards show which history the handle followed"""
    train, test = rs.history_case()
    tr, te = rs.cols(train), rs.cols(test)
    m = oracle.Model(*tr)
    users = np.unique(tr[0]).tolist()
    for k in (1, 4, len(users) + 3):
        e = kn.Engine(k=k, flags=kn.FLAG_VERIFY_BOUND).fit(*tr)
        p = m.pipeline(oracle.SIM_COSINE, k)
        want, preds = p.mae(*te, True)
        _same_bits(e.predict_batch(kn.PRED_KNN, te[0], te[1]), preds, k)
        _mae_close(e.mae(kn.PRED_KNN, *te), want, k)
        for u in users:
            ids, sims = e.neighbors(u)
            oids, osims = p.neighbors(u)
            assert ids.tolist() == oids.tolist(), (u, k)
            _same_bits(sims, osims, (u, k))
        e.close()


# ---- the average and the means at the FOLD_CHUNK edges -----------------------------------------------------------------------
@pytest.mark.parametrize("n,where", rs.avg_edge_cases())
def test_avg_edge_means_equal_the_oracle(kn, oracle, n, where):
    tr = rs.avg_edge(n, where)
    e = kn.Engine(k=3).fit(*tr)
    _means_equal_the_oracle(e, oracle.Model(*tr), tr)
    e.close()


# ---- the two limits of the dyadic rule -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", rs.DYADIC_LIMIT_CASES)
def test_dyadic_limits(kn, oracle, kind):
    tr, te = rs.dyadic_limits()[kind]
    m = oracle.Model(*tr)
    e = kn.Engine(k=10, flags=kn.FLAG_VERIFY_BOUND).fit(*tr)
    _means_equal_the_oracle(e, m, tr)
    want, preds = m.pipeline(oracle.SIM_COSINE, 10).mae(*te, True)
    _same_bits(e.predict_batch(kn.PRED_KNN, te[0], te[1]), preds, kind)
    _mae_close(e.mae(kn.PRED_KNN, *te), want, kind)
    assert e.timings()["max_bound_violation"] <= 0.0
    e.close()


# ---- wide100k: shared, unchanged state ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(oracle):
    tr, te = rs.wide100k()
    m = oracle.Model(*tr)
    sets = rs.wide_user_sets(oracle)
    return {"tr": tr, "te": te, "model": m, "sets": sets, "avg": m.average(),
            "neg_rows": np.flatnonzero(np.isin(te[0], sets["negative"]))}


@pytest.fixture(scope="module")
def answers(oracle, wide):
    """(similarity, k) -> (MAE, predictions of every test row, the pipeline that made them); every train user has more than
    4 ratings, so no answer depends on the order of the calls"""
    cache = {}

    def get(sim, k):
        if (sim, k) not in cache:
            p = wide["model"].pipeline(sim, k)
            want, preds = p.mae(*wide["te"], True)
            preds.setflags(write=False)
            cache[sim, k] = (want, preds, p)
        return cache[sim, k]

    return get


def _check_wide_knn(kn, e, capfd, answer, wide, k, path):
    want, opreds, p = answer
    te, tr = wide["te"], wide["tr"]
    kcap = min(k, e.num_users - 1)
    e.set_k(k)
    e.reset_neighbors()  # (another test may have left this k's neighbourhoods on the shared handle)
    e.reset_timings()
    capfd.readouterr()
    preds = e.predict_batch(kn.PRED_KNN, te[0], te[1])
    mae = e.mae(kn.PRED_KNN, *te)
    list_users = sorted(set(np.unique(tr[0])[::23].tolist()) | set(wide["sets"]["negative"]))
    lists = [e.neighbors(int(u)) for u in list_users]
    lines = _trace(capfd)
    assert set(lines) == _knn_lines(path, kcap, False), (k, path, lines)
    assert lines.count(_predict_line(path, kcap)) == 2, (k, path)
    _same_bits(preds, opreds, (k, path))
    _mae_close(mae, want, (k, path))
    # every test row of a fitted user with a negative mean is the global average
    assert len(wide["neg_rows"]) >= 100
    assert (_bits(preds[wide["neg_rows"]]) == _bits(wide["avg"])).all(), (k, path)
    for u, (ids, sims) in zip(list_users, lists):
        oids, osims = p.neighbors(int(u))
        assert len(ids) == kcap and ids.tolist() == oids.tolist(), (k, path, int(u))
        _same_bits(sims, osims, (k, path, int(u)))
    assert e.timings()["max_bound_violation"] <= 0.0, (k, path)


@pytest.mark.parametrize("path", list(PATH_ENV))
def test_wide100k_knn_on_every_prediction_path(kn, oracle, wide, answers, handles, monkeypatch, capfd, path):
    e = _handle(kn, handles, monkeypatch, "wide100k", wide["tr"], kn.SIM_COSINE, path)
    expect = {"default": "predict items", "no_lds_bitmaps": "predict rows", "no_item_bitmaps": "predict general"}[path]
    for k in WIDE_KS:
        assert _predict_line(path, k).startswith(expect)
        _check_wide_knn(kn, e, capfd, answers(oracle.SIM_COSINE, k), wide, k, path)
    # the sweep from one neighbour build against a fresh oracle pipeline per k
    te = wide["te"]
    maes, preds = e.mae_sweep(SWEEP_KS, *te, predictions=True)
    for q, k in enumerate(SWEEP_KS):
        want, opreds, _ = answers(oracle.SIM_COSINE, k)
        _same_bits(preds[q], opreds, ("sweep", path, k))
        _mae_close(maes[q], want, ("sweep", path, k))
        assert (_bits(preds[q][wide["neg_rows"]]) == _bits(wide["avg"])).all()


def test_wide100k_general_kernel_by_kcap(kn, oracle, wide, answers, monkeypatch, capfd):
    """a handle of k = 600: kcap > 512 sends the default path to the general kernel as well"""
    monkeypatch.setenv("KNNCF_DEBUG_TRACE_DISPATCH", "1")
    for env in PATH_ENV.values():
        if env:
            monkeypatch.delenv(env, raising=False)
    assert _predict_line("default", 600) == "predict general CAP=1024"
    e = kn.Engine(k=600, flags=kn.FLAG_VERIFY_BOUND).fit(*wide["tr"])
    _check_wide_knn(kn, e, capfd, answers(oracle.SIM_COSINE, 600), wide, 600, "default")
    e.close()


def test_wide100k_closed_forms_and_personalized(kn, oracle, wide):
    tr, te, m = wide["tr"], wide["te"], wide["model"]
    e = kn.Engine(k=10).fit(*tr)
    _means_equal_the_oracle(e, m, tr)
    for kind, okind in ((kn.PRED_GLOBAL_AVG, oracle.KIND_GLOBAL), (kn.PRED_USER_AVG, oracle.KIND_USER),
                        (kn.PRED_ITEM_AVG, oracle.KIND_ITEM), (kn.PRED_BASELINE, oracle.KIND_BASELINE),
                        (kn.PRED_BASELINE_RDD, oracle.KIND_BASELINE_SPARK)):
        want, preds = m.mae(okind, *te, True)
        _same_bits(e.predict_batch(kind, te[0], te[1]), preds, kind)
        _mae_close(e.mae(kind, *te), want, kind)
        if kind in (kn.PRED_BASELINE, kn.PRED_BASELINE_RDD):  # :226 the baseline's own `ua < 0` branch
            assert (_bits(preds[wide["neg_rows"]]) == _bits(wide["avg"])).all()
    e.close()
    jac = kn.Engine(similarity=kn.SIM_JACCARD).fit(*tr)
    want, preds = m.pipeline(oracle.SIM_JACCARD, -1).mae(*te, True)
    _same_bits(jac.predict_batch(kn.PRED_PERSONALIZED, te[0], te[1]), preds, "personalized")
    _mae_close(jac.mae(kn.PRED_PERSONALIZED, *te), want, "personalized")
    assert (_bits(preds[wide["neg_rows"]]) == _bits(wide["avg"])).all()
    jac.close()


# ---- recommendations: predictions of both signs, ties, flat lists -----------------------------------------------------------
def test_wide100k_recommendations(kn, oracle, wide, answers, handles, monkeypatch):
    tr, m, sets = wide["tr"], wide["model"], wide["sets"]
    e = _handle(kn, handles, monkeypatch, "wide100k", tr, kn.SIM_COSINE, "default")
    e.set_k(rs.WIDE_RECO_K)
    p = answers(oracle.SIM_COSINE, rs.WIDE_RECO_K)[2]
    n_items = e.num_items
    users = sets["negative"][:3] + sets["mixed_sign"] + sets["tied"] + [rs.UNKNOWN_USER]
    users = list(dict.fromkeys(users))
    signs = set()
    for pred, reco in ((kn.PRED_KNN, p.recommend), (kn.PRED_BASELINE, lambda u, n: m.recommend(oracle.KIND_BASELINE, u, n))):
        for n in RECO_NS:
            n = n_items if n is None else n
            items, preds, counts = e.recommend_batch(pred, users, n)
            for row, u in enumerate(users):
                wi, wp = reco(u, n)
                what = (pred, n, u)
                assert counts[row] == len(wi), what
                assert items[row, :counts[row]].tolist() == wi.tolist(), what
                _same_bits(preds[row, :counts[row]], wp, what)
                gi, gp = e.recommend(pred, u, n)
                assert gi.tolist() == wi.tolist(), what
                _same_bits(gp, wp, what)
                if u in sets["negative"] or u == rs.UNKNOWN_USER:  # all ties: pure ascending raw-id order
                    assert (_bits(gp) == _bits(wide["avg"])).all() and gi.tolist() == sorted(gi.tolist()), what
                if pred == kn.PRED_KNN and n == n_items:
                    if u in sets["mixed_sign"]:
                        assert (gp < 0.0).any() and (gp > 0.0).any(), what
                        signs.add(u)
                    if u in sets["tied"]:
                        assert len(np.unique(gp)) < len(gp), what
    assert signs == set(sets["mixed_sign"])


# ---- explain ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [SUM_ORDER, BY_WEIGHT])
def test_wide100k_explain(kn, oracle, wide, handles, monkeypatch, order):
    tr, te, sets = wide["tr"], wide["te"], wide["sets"]
    e = _handle(kn, handles, monkeypatch, "wide100k", tr, kn.SIM_COSINE, "default")
    k = rs.WIDE_RECO_K
    e.set_k(k)
    neg = wide["neg_rows"][:40]
    raters, sims, devs, counts, sums, preds = e.explain_batch(te[0][neg], te[1][neg], 8, order=order)
    assert (counts == 0).all() and (_bits(sums) == 0).all() and (_bits(preds) == _bits(wide["avg"])).all()
    assert (raters == -1).all() and np.isnan(sims).all() and np.isnan(devs).all()
    # per mixed-sign user: the items of its six lowest (negative) and six highest predictions, and its first test rows
    model = explain_model.TermModel(oracle, wide["model"], oracle.SIM_COSINE, k)
    us, its = [], []
    for u in sets["mixed_sign"]:
        ids, _ = model.pipeline.recommend(u, e.num_items)
        mine = np.concatenate([ids[:6], ids[-6:], te[1][te[0] == u][:6]])
        us.append(np.full(len(mine), u))
        its.append(mine)
    us, its = np.concatenate(us).astype(np.int32), np.concatenate(its).astype(np.int32)
    want = model.rows(us, its)
    assert sum(r.prediction < 0.0 for r in want) >= len(sets["mixed_sign"]) and sum(r.count >= 2 for r in want) >= 3
    assert any(abs(d) > 1.0 for r in want for d in r.devs.tolist())  # deviations beyond [-1, 1] among the terms
    cap = max(r.count for r in want)
    _assert_rows(e.explain_batch(us, its, cap, order=order), want, order, ("wide100k", order))


# ---- queries against the wide100k fit ---------------------------------------------------------------------------------------------
def test_wide100k_queries(kn, oracle, wide):
    tr = wide["tr"]
    k = rs.WIDE_RECO_K
    q = rs.wide_query_cases(oracle)
    e = kn.Engine(k=k).fit(*tr)
    all_items = np.unique(tr[1])
    # fold-in users with a positive mean whose recommendations hold predictions below zero
    for name in ("fold_clone", "fold_heavy"):
        user, items, ratings = q[name]
        pred_items = np.concatenate([all_items[::7], items[:5], [rs.UNKNOWN_ITEM]]).astype(np.int32)
        _check_fold_in(kn, oracle, e, tr, user, items, ratings, oracle.SIM_COSINE, k, pred_items, ns=(33, None))
    _, best = e.recommend_for(*q["fold_heavy"], 33)
    _, full = e.recommend_for(*q["fold_clone"], len(all_items))
    assert (best < 0.0).any() and (full < 0.0).any() and (full > 0.0).any()
    # an update that lifts a negative mean above zero is answered; one that leaves it below is refused
    _check_update(kn, oracle, e, tr, *q["lift"], oracle.SIM_COSINE, k, ns=(33, None))
    with pytest.raises(kn.KnncfError) as ex:
        e.recommend_with(*q["stay_negative"], 33)
    assert ex.value.status == kn.E_UNSUPPORTED
    with pytest.raises(kn.KnncfError) as ex:
        e.neighbors_with(q["stay_negative"][0], [], [])  # the fitted rows alone
    assert ex.value.status == kn.E_UNSUPPORTED
    # a revise that keeps the mean positive is answered; one that removes every positive rating is refused
    _check_revise(kn, oracle, e, tr, *q["revise_keep"], oracle.SIM_COSINE, k, ns=(33, None))
    for call in (lambda: e.neighbors_revised(*q["revise_negative"]),
                 lambda: e.predict_revised(*q["revise_negative"], all_items[:5]),
                 lambda: e.recommend_revised(*q["revise_negative"], 33)):
        with pytest.raises(kn.KnncfError) as ex:
            call()
        assert ex.value.status == kn.E_UNSUPPORTED
    # the same calls in one batch: per-query statuses, the answered queries as if alone
    pred_items = all_items[::11].astype(np.int32)
    batch = [q["lift"], q["stay_negative"], q["fold_clone"], q["stay_negative"], q["lift"]]
    want = [kn.OK, kn.E_UNSUPPORTED, kn.OK, kn.E_UNSUPPORTED, kn.OK]
    nb, st = e.neighbors_with_batch(batch)
    assert st.tolist() == want
    pr, st = e.predict_with_batch(batch, [pred_items] * len(batch))
    assert st.tolist() == want
    rcm, st = e.recommend_with_batch(batch, 33)
    assert st.tolist() == want
    for j, (status, query) in enumerate(zip(want, batch)):
        if status == kn.OK:
            _same_pair(nb[j], e.neighbors_with(*query), j)
            _same_bits(pr[j], e.predict_with(*query, pred_items), j)
            _same_pair(rcm[j], e.recommend_with(*query, 33), j)
        else:
            assert len(nb[j][0]) == 0 and len(rcm[j][0]) == 0 and np.isnan(pr[j]).all(), j
    batch = [q["revise_keep"], q["revise_negative"], q["revise_keep"]]
    want = [kn.OK, kn.E_UNSUPPORTED, kn.OK]
    nb, st = e.neighbors_revised_batch(batch)
    assert st.tolist() == want
    pr, st = e.predict_revised_batch(batch, [pred_items] * len(batch))
    assert st.tolist() == want
    rcm, st = e.recommend_revised_batch(batch, 33)
    assert st.tolist() == want
    for j in (0, 2):
        _same_pair(nb[j], e.neighbors_revised(*batch[j]), j)
        _same_bits(pr[j], e.predict_revised(*batch[j], pred_items), j)
        _same_pair(rcm[j], e.recommend_revised(*batch[j], 33), j)
    assert len(nb[1][0]) == 0 and len(rcm[1][0]) == 0 and np.isnan(pr[1]).all()
    # the fold-in family refuses a query whose own mean is negative
    with pytest.raises(kn.KnncfError) as ex:
        e.neighbors_for(rs.FOLD_CLONE, all_items[:6], np.full(6, -0.3))
    assert ex.value.status == kn.E_UNSUPPORTED
    e.close()


# ---- two shards on one GPU -------------------------------------------------------------------------------------------------------
def test_wide100k_two_shards_on_one_gpu(kn, pkg, oracle, wide, answers):
    """the shard protocol of test_gpu_parity.test_two_shards_on_one_gpu_equal_single_engine (file-order means on every shard)"""
    import torch

    sharded = importlib.import_module(pkg.__name__ + ".sharded")
    dev = torch.device("cuda", 0)
    tr = tuple(torch.from_numpy(np.array(a)).to(dev) for a in wide["tr"])
    te = tuple(torch.from_numpy(np.array(a)).to(dev) for a in wide["te"])
    k = 300
    single = kn.Engine(k=k)
    single.fit_device(*tr)
    single_preds = torch.zeros(len(wide["te"][0]), dtype=torch.float64, device=dev)
    s1, c1 = single.mae_device(kn.PRED_KNN, *te, pred_out=single_preds)
    engines = [kn.Engine(k=k, shard_rank=r, shard_count=2) for r in range(2)]
    views = []
    for e in engines:
        e.fit_device(*tr)
        views.append(sharded.DeviceEngineAdapter(e, dev).shard_tensors())
    assert views[0]["user_range"][1] == views[1]["user_range"][0]
    for me, other in ((0, 1), (1, 0)):
        ulo, uhi = views[other]["user_range"]
        for key in ("user_avg", "user_norm"):
            views[me][key][ulo:uhi] = views[other][key][ulo:uhi]
    torch.cuda.synchronize()
    total, count = 0.0, 0
    preds = torch.zeros(len(wide["te"][0]), dtype=torch.float64, device=dev)
    for e in engines:
        e.shard_commit()
        s, c = e.mae_device(kn.PRED_KNN, *te, pred_out=preds)
        total += s
        count += c
    assert count == c1 == len(wide["te"][0])
    want, opreds, _ = answers(oracle.SIM_COSINE, k)
    _same_bits(preds.cpu().numpy(), opreds, "shards")
    _same_bits(single_preds.cpu().numpy(), opreds, "single")
    _mae_close(total / count, want, "shards")
    _mae_close(s1 / c1, want, "single")
    for e in engines + [single]:
        e.close()


# ---- non-finite input ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_rating_fails_the_fit_and_the_handle_recovers(kn, oracle, bad):
    tr, te = rs.dyadic_limits()["sixteenths"]
    ratings = tr[2].copy()
    ratings[700] = bad
    e = kn.Engine(k=10)
    with pytest.raises(kn.KnncfError) as ex:
        e.fit(tr[0], tr[1], ratings)
    assert ex.value.status == kn.E_NONFINITE
    e.fit(*tr)
    m = oracle.Model(*tr)
    _means_equal_the_oracle(e, m, tr)
    want, preds = m.pipeline(oracle.SIM_COSINE, 10).mae(*te, True)
    _same_bits(e.predict_batch(kn.PRED_KNN, te[0], te[1]), preds, bad)
    _mae_close(e.mae(kn.PRED_KNN, *te), want, bad)
    e.close()
