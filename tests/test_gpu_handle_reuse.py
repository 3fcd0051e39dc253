"""A handle's later lives: re-fits on other data, k changed on a fitted handle, a refused fit in between, the call order
that decides a <= 4-rating pair's summation order, neighbour checkpoints carried across handles, and shard
handles queried before the replicated mae.  The handle keeps device buffers (grown, never shrunk), the neighbour table
(counts, build sequence numbers, epoch) and the lazily made id-sorted lists between calls: every answer after such a
history must still equal the oracle's on the CURRENT fit, and a fresh handle's, bit for bit."""
import importlib

import numpy as np
import pytest

from tests.test_gpu_fold_in import _check as _check_fold_in
from tests.test_oracle_semantics import _cols, _no_zero_scale, _random_case

pytestmark = pytest.mark.gpu
MAE_TOL = 1e-9
NEVER_USER, NEVER_ITEM = 2_000_000_011, 2_000_000_017  # ids no fit below contains
QUERY_USER = 1_999_999_999


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64).tolist()


def _split(d, n_test=3000, big=False):
    tr = (d.train.users, d.train.items, d.train.ratings)
    te = (d.test.users[:n_test], d.test.items[:n_test], d.test.ratings[:n_test])
    if big:  # raw ids outside the direct id tables: the hashed lookup path
        u = lambda a: (a.astype(np.int64) * 7919 - 40_000).astype(np.int32)
        i = lambda a: (a.astype(np.int64) * 7919 + (1 << 25)).astype(np.int32)
        tr, te = (u(tr[0]), i(tr[1]), tr[2]), (u(te[0]), i(te[1]), te[2])
    return tr, te


def _lists_equal(e, p, users, what):
    ids, sims, counts = e.neighbors_batch(users)
    for row, u in enumerate(users):
        oids, osims = p.neighbors(int(u))
        assert counts[row] == len(oids), (what, int(u))
        assert ids[row, : counts[row]].tolist() == oids.tolist(), (what, int(u))
        assert _bits(sims[row, : counts[row]]) == _bits(osims), (what, int(u))
    return ids, sims, counts


def _check_fit(kn, oracle, e, tr, te, sim_o, sim_k, k, gone=(None, None), what=""):
    """everything the issue lists against the oracle on (tr, te), then a fresh handle on the same rows"""
    m = oracle.Model(*tr)
    users, items = np.unique(tr[0]), np.unique(tr[1])
    assert e.num_users == len(users) and e.num_items == len(items), what
    assert e.global_avg() == m.average(), what
    for u in users[:: max(1, len(users) // 20)]:
        assert e.user_avg(int(u)) == m.users_avg(int(u)), (what, int(u))
    for i in items[:: max(1, len(items) // 20)]:
        assert e.item_avg_dev(int(i)) == m.items_avg_dev(int(i)), (what, int(i))
    want_b, preds_b = m.mae(oracle.KIND_BASELINE, *te, True)
    assert _bits(e.predict_batch(kn.PRED_BASELINE, te[0], te[1])) == _bits(preds_b), what
    p = m.pipeline(sim_o, k)
    want, preds = p.mae(*te, True)
    got = e.predict_batch(kn.PRED_KNN, te[0], te[1])
    assert _bits(got) == _bits(preds), what
    assert abs(e.mae(kn.PRED_KNN, *te) - want) <= MAE_TOL, what
    sample = users[:: max(1, len(users) // 40)]
    ids, sims, counts = _lists_equal(e, p, sample, what)
    for u in (int(users[1]), int(users[-2])):
        gi, gp = e.recommend(kn.PRED_KNN, u, 5)
        wi, wp = p.recommend(u, 5)
        assert gi.tolist() == wi.tolist() and _bits(gp) == _bits(wp), (what, u)
    # ids of the previous fit that this one lacks answer like ids nobody has seen
    gone_u, gone_i = gone
    for u in [NEVER_USER] + ([gone_u] if gone_u is not None else []):
        assert e.user_avg(u) == m.average(), (what, u)
        ids_u, sims_u = e.neighbors(u)
        oids, osims = p.neighbors(u)
        assert ids_u.tolist() == oids.tolist() and _bits(sims_u) == _bits(osims), (what, u)
        gi, gp = e.recommend(kn.PRED_KNN, u, 4)
        wi, wp = p.recommend(u, 4)
        assert gi.tolist() == wi.tolist() and _bits(gp) == _bits(wp), (what, u)
    for i in [NEVER_ITEM] + ([gone_i] if gone_i is not None else []):
        assert e.item_avg_dev(i) == e.item_avg_dev(NEVER_ITEM) == 0.0, (what, i)
    if gone_u is not None or gone_i is not None:
        pu = np.array([gone_u if gone_u is not None else NEVER_USER, int(users[0]), int(users[3])], dtype=np.int32)
        pi = np.array([int(items[0]), gone_i if gone_i is not None else NEVER_ITEM, int(items[2])], dtype=np.int32)
        assert _bits(e.predict_batch(kn.PRED_KNN, pu, pi)) == _bits([p.predict(int(a), int(b)) for a, b in zip(pu, pi)]), what
    # fold-in: a user outside the fit, with the test ratings of a train user as its ratings (the fit itself stays as it is)
    src = int(te[0][0])
    rows = te[0] == src
    q_items, q_ratings = te[1][rows], te[2][rows]
    _check_fold_in(kn, oracle, e, tr, QUERY_USER, q_items, q_ratings, sim_o, k,
                   np.concatenate([items[:40], q_items, [NEVER_ITEM]]), ns=(3,))
    # a fresh handle on the same rows: the same bits
    f = kn.Engine(k=k, similarity=sim_k).fit(*tr)
    assert _bits(f.predict_batch(kn.PRED_KNN, te[0], te[1])) == _bits(got), what
    fids, fsims, fcounts = f.neighbors_batch(sample)
    assert fcounts.tolist() == counts.tolist() and fids.tolist() == ids.tolist(), what
    assert _bits(fsims) == _bits(sims), what
    f.close()


@pytest.mark.parametrize("sim", ["cosine", "jaccard"])
def test_refit_sequence_on_one_handle(kn, oracle, synth, sim):
    """one handle, fitted six times: grow, shrink a lot, the same shape with other content (every buffer is kept),
    large raw ids (hashed lookups), small ids again"""
    sim_o, sim_k = (oracle.SIM_JACCARD, kn.SIM_JACCARD) if sim == "jaccard" else (oracle.SIM_COSINE, kn.SIM_COSINE)
    k = 50
    fits = [
        ("small", _split(synth.syn_scaled(900, 300, 40_000, seed=61))),
        ("grown", _split(synth.syn_scaled(2400, 500, 160_000, seed=62, shuffle=True))),
        ("shrunk", _split(synth.syn_scaled(900, 300, 40_000, seed=63))),
        ("same shape, other content", _split(synth.syn_scaled(900, 300, 40_000, seed=64))),
        ("large raw ids", _split(synth.syn_scaled(1500, 400, 80_000, seed=65), big=True)),
        ("small ids again", _split(synth.syn_scaled(1500, 400, 80_000, seed=66))),
    ]
    assert len(fits[2][1][0][0]) == len(fits[3][1][0][0])
    e = kn.Engine(k=k, similarity=sim_k)
    prev = None
    for what, (tr, te) in fits:
        e.fit(*tr)
        gone_u = gone_i = None
        if prev is not None:
            lost_u = np.setdiff1d(np.unique(prev[0]), tr[0])
            lost_i = np.setdiff1d(np.unique(prev[1]), tr[1])
            gone_u = int(lost_u[-1]) if len(lost_u) else None
            gone_i = int(lost_i[-1]) if len(lost_i) else None
        _check_fit(kn, oracle, e, tr, te, sim_o, sim_k, k, (gone_u, gone_i), what)
        prev = tr
    e.close()


@pytest.mark.parametrize("bitmaps", [True, False])
def test_set_k_across_prediction_paths(kn, oracle, syn100k, monkeypatch, bitmaps):
    """k = 300 -> 10 -> 1000 -> 5 on one fitted handle: 1000 (kcap 942 > 512) takes the id-sorted lists, the others the
    item-grouped kernel; without item bitmaps every k takes the id-sorted lists"""
    if not bitmaps:
        monkeypatch.setenv("KNNCF_DEBUG_NO_ITEM_BITMAPS", "1")
    d = syn100k
    tr = (d.train.users, d.train.items, d.train.ratings)
    te = (d.test.users, d.test.items, d.test.ratings)
    m = oracle.Model(*tr)
    users = np.unique(tr[0])
    e = kn.Engine(k=300).fit(*tr)
    for k in (300, 10, 1000, 5):
        e.set_k(k)
        p = m.pipeline(oracle.SIM_COSINE, k)
        want, preds = p.mae(*te, True)
        assert _bits(e.predict_batch(kn.PRED_KNN, te[0], te[1])) == _bits(preds), k
        assert abs(e.mae(kn.PRED_KNN, *te) - want) <= MAE_TOL, k
        _lists_equal(e, p, users[::23], f"k {k}")
    f = kn.Engine(k=5).fit(*tr)
    assert _bits(f.predict_batch(kn.PRED_KNN, te[0], te[1])) == _bits(e.predict_batch(kn.PRED_KNN, te[0], te[1]))
    f.close()
    e.close()


@pytest.mark.parametrize("k, bitmaps", [(500, False), (1000, True)])
def test_shrink_then_lower_k(kn, oracle, synth, monkeypatch, k, bitmaps):
    """a re-fit with fewer users leaves the neighbour table's buffers (and the previous fit's counts past the new U) in
    place; the lazy id-sort must walk the current users only, also after set_k lowers the row width"""
    if not bitmaps:
        monkeypatch.setenv("KNNCF_DEBUG_NO_ITEM_BITMAPS", "1")
    big = synth.syn_scaled(2400, 500, 160_000, seed=71, shuffle=True)
    small = synth.syn_scaled(900, 300, 40_000, seed=72)
    tr1, te1 = _split(big, 4000)
    tr2, te2 = _split(small)
    e = kn.Engine(k=k).fit(*tr1)
    want1 = oracle.Model(*tr1).pipeline(oracle.SIM_COSINE, k).mae(*te1)
    assert abs(e.mae(kn.PRED_KNN, *te1) - want1) <= MAE_TOL
    e.fit(*tr2)
    m2 = oracle.Model(*tr2)
    users = np.unique(tr2[0])
    for kk in (k, 10):
        if kk != k:
            e.set_k(kk)
        p = m2.pipeline(oracle.SIM_COSINE, kk)
        want, preds = p.mae(*te2, True)
        assert _bits(e.predict_batch(kn.PRED_KNN, te2[0], te2[1])) == _bits(preds), kk
        assert abs(e.mae(kn.PRED_KNN, *te2) - want) <= MAE_TOL, kk
        _lists_equal(e, p, users[::11], f"k {kk}")
    e.close()


def _refused_state(kn, e, tr, te):
    """after a refused fit every query is a state error, not the previous fit's answer"""
    u, i = int(tr[0][0]), int(tr[1][0])
    calls = [
        lambda: e.num_users,
        lambda: e.global_avg(),
        lambda: e.user_avg(u),
        lambda: e.item_avg_dev(i),
        lambda: e.similarity(u, int(tr[0][1])),
        lambda: e.neighbors(u),
        lambda: e.neighbors_batch([u]),
        lambda: e.predict(kn.PRED_KNN, u, i),
        lambda: e.predict_batch(kn.PRED_KNN, te[0], te[1]),
        lambda: e.predict_batch(kn.PRED_BASELINE, te[0], te[1]),
        lambda: e.mae(kn.PRED_KNN, *te),
        lambda: e.recommend(kn.PRED_KNN, u, 3),
        lambda: e.recommend_for(QUERY_USER, [i], [4.0], 3),
        lambda: e.reset_neighbors(),
    ]
    for j, call in enumerate(calls):
        with pytest.raises(kn.KnncfError) as ex:
            call()
        assert ex.value.status == kn.E_STATE, j


def test_failed_fit_in_the_middle(kn, oracle, synth):
    """fit A, a refused fit (duplicate pair / non-finite deviation), fit B: nothing of A answers in between, B is exact"""
    tra, tea = _split(synth.syn_scaled(900, 300, 40_000, seed=81))
    trb, teb = _split(synth.syn_scaled(1500, 400, 80_000, seed=82))
    k = 40
    e = kn.Engine(k=k)
    e.fit(*tra)
    _check_fit(kn, oracle, e, tra, tea, oracle.SIM_COSINE, kn.SIM_COSINE, k, what="A")
    dup = (np.append(tra[0], tra[0][5]), np.append(tra[1], tra[1][5]), np.append(tra[2], 3.0))
    with pytest.raises(kn.KnncfError) as ex:
        e.fit(*dup)
    assert ex.value.status == kn.E_DUPLICATE
    _refused_state(kn, e, tra, tea)
    with pytest.raises(kn.KnncfError) as ex:
        e.fit([1, 1, 1], [1, 2, 3], [0.5, 1.0, 1.5])
    assert ex.value.status == kn.E_NONFINITE
    _refused_state(kn, e, tra, tea)
    e.fit(*trb)
    lost_u = np.setdiff1d(np.unique(tra[0]), trb[0])
    _check_fit(kn, oracle, e, trb, teb, oracle.SIM_COSINE, kn.SIM_COSINE, k,
               (int(lost_u[0]) if len(lost_u) else None, None), "B")
    e.close()


def _tiny_case(seed):
    rng = np.random.default_rng(5200 + seed)
    rows = _random_case(rng, n_users=24 + 4 * seed, n_items=19, n_ratings=160 + 20 * seed, half=(seed % 2 == 1),
                        tiny_rows=3 + seed)
    cut = len(rows) * 4 // 5
    train, test = rows[:cut], rows[cut:]
    assert _no_zero_scale(train)
    tr, te = _cols(train), _cols(test)
    assert min(np.bincount(np.unique(tr[0], return_inverse=True)[1])) <= 4
    return (tuple(np.asarray(a, dt) for a, dt in zip(tr, (np.int32, np.int32, np.float64))),
            tuple(np.asarray(a, dt) for a, dt in zip(te, (np.int32, np.int32, np.float64))))


def _same_list(e, p, u):
    ids, sims = e.neighbors(int(u))
    oids, osims = p.neighbors(int(u))
    assert ids.tolist() == oids.tolist() and _bits(sims) == _bits(osims), int(u)


def _same_mae(kn, e, p, te):
    want, preds = p.mae(*te, True)
    assert abs(e.mae(kn.PRED_KNN, *te) - want) <= MAE_TOL
    assert _bits(e.predict_batch(kn.PRED_KNN, te[0], te[1])) == _bits(preds)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_call_order_with_tiny_rows(kn, oracle, seed, tmp_path):
    """<= 4-rating users: a pair's summation order is the first evaluating closure's, so the handle must play
    the memo history of ONE stateful oracle pipeline through any call order — and carry it through a checkpoint"""
    tr, te = _tiny_case(seed)
    m = oracle.Model(*tr)
    users = np.unique(tr[0])
    tiny = [int(u) for u in users if (tr[0] == u).sum() <= 4]
    first = tiny[:2] + [int(users[len(users) // 2])]
    rest = tiny[2:] + [int(users[0]), int(users[-1])]
    for k in (2, 6):
        # 1) neighbours of a few users, then mae; half way a checkpoint goes to a second handle that plays the rest
        p = m.pipeline(oracle.SIM_COSINE, k)
        e = kn.Engine(k=k).fit(*tr)
        for u in first:
            _same_list(e, p, u)
        path = str(tmp_path / f"nbr_{seed}_{k}.bin")
        e.neighbors_save(path)
        e2 = kn.Engine(k=k).fit(*tr)
        e2.neighbors_load(path)
        p_copy = m.pipeline(oracle.SIM_COSINE, k)
        for u in first:
            p_copy.neighbors(u)
        for u in rest:
            _same_list(e, p, u)
            _same_list(e2, p_copy, u)
        _same_mae(kn, e, p, te)
        _same_mae(kn, e2, p_copy, te)
        e.close()
        e2.close()
        # 2) a batch in a permuted order, then the predictions
        p = m.pipeline(oracle.SIM_COSINE, k)
        e = kn.Engine(k=k).fit(*tr)
        order = np.random.default_rng(seed).permutation(users)
        ids, sims, counts = e.neighbors_batch(order)
        for row, u in enumerate(order):
            oids, osims = p.neighbors(int(u))
            assert ids[row, : counts[row]].tolist() == oids.tolist() and _bits(sims[row, : counts[row]]) == _bits(osims)
        want, preds = p.mae(*te, True)
        assert _bits(e.predict_batch(kn.PRED_KNN, te[0], te[1])) == _bits(preds)
        # 3) mae, reset, neighbours, mae: the reset handle is a fresh pipeline
        e.reset_neighbors()
        p = m.pipeline(oracle.SIM_COSINE, k)
        _same_mae(kn, e, p, te)
        e.reset_neighbors()
        p = m.pipeline(oracle.SIM_COSINE, k)
        for u in rest:
            _same_list(e, p, u)
        _same_mae(kn, e, p, te)
        e.close()


@pytest.mark.parametrize("seed", [0, 1])
def test_sharded_query_before_mae(kn, pkg, oracle, seed):
    """shard handles with <= 4-rating users in train: a neighbour query before the replicated mae is either refused
    (KNNCF_E_UNSUPPORTED) or leaves every shard bit-equal to a single handle that ran the same calls"""
    import torch

    sharded = importlib.import_module(pkg.__name__ + ".sharded")
    trc, tec = _tiny_case(seed)
    users = np.unique(trc[0])
    tiny = [int(u) for u in users if (trc[0] == u).sum() <= 4]
    queries = [tiny[0], int(users[len(users) // 3])]
    dev = torch.device("cuda", 0)
    tr = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in trc)
    te = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in tec)
    world, k = 2, 3
    engines = [kn.Engine(k=k, shard_rank=r, shard_count=world) for r in range(world)]
    views = []
    for e in engines:
        e.fit_device(*tr)
        views.append(sharded.DeviceEngineAdapter(e, dev).shard_tensors())
    for me in range(world):
        other = 1 - me
        lo, hi = views[other]["user_range"]
        for key in ("user_avg", "user_norm"):
            views[me][key][lo:hi] = views[other][key][lo:hi]
    torch.cuda.synchronize()
    for e in engines:
        e.shard_commit()
    p = oracle.Model(*trc).pipeline(oracle.SIM_COSINE, k)
    for j, u in enumerate(queries):
        owner = None
        for r, e in enumerate(engines):
            try:
                if j == 0:
                    got = e.neighbors(u)
                else:
                    ids, sims, counts = e.neighbors_batch([u])
                    got = (ids[0, : counts[0]], sims[0, : counts[0]])
            except kn.KnncfError as ex:
                if ex.status == kn.E_INVALID:  # another shard's user
                    continue
                assert ex.status == kn.E_UNSUPPORTED, ex
                owner = r
                break
            owner = r
            oids, osims = p.neighbors(u)
            assert got[0].tolist() == oids.tolist() and _bits(got[1]) == _bits(osims), u
            break
        assert owner is not None, u
    want, opreds = p.mae(*tec, True)
    preds = torch.full((len(tec[0]),), float("nan"), dtype=torch.float64, device=dev)
    total, count = 0.0, 0
    for e in engines:
        s, c = e.mae_device(kn.PRED_KNN, *te, pred_out=preds)
        total += s
        count += c
    assert count == len(tec[0])
    assert _bits(preds.cpu().numpy()) == _bits(opreds)
    assert abs(total / count - want) <= 1e-13
    # after the mae every test user has its build number on every shard: the lists are the single handle's
    for u in np.unique(tec[0])[:6]:
        if int(u) not in set(users.tolist()):
            continue
        for e in engines:
            try:
                ids, sims = e.neighbors(int(u))
            except kn.KnncfError as ex:
                assert ex.status == kn.E_INVALID
                continue
            oids, osims = p.neighbors(int(u))
            assert ids.tolist() == oids.tolist() and _bits(sims) == _bits(osims), int(u)
    for e in engines:
        e.close()
