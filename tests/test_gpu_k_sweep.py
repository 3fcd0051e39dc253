"""knncf_mae_sweep: the MAE of predict/kNN.scala:73 at many k from one neighbour build, against the CPU oracle (fresh
closures per k) and against knncf_set_k + knncf_mae on a second handle, bit for bit."""
import importlib

import numpy as np
import pytest

from tests.test_oracle_semantics import _cols, _no_zero_scale, _random_case

pytestmark = pytest.mark.gpu
MAE_TOL = 1e-9
KNN_SCALA_KS = (10, 30, 50, 100, 200, 300, 400, 800, 943)


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _loop_maes(kn, tr, te, ks, sim):
    e = kn.Engine(k=300, similarity=sim)
    e.fit(*tr)
    out = []
    for k in ks:
        e.set_k(k)
        out.append(e.mae(kn.PRED_KNN, *te))
    e.close()
    return np.array(out)


def _check_against_oracle(kn, oracle, tr, te, ks, sim, osim):
    e = kn.Engine(k=7, similarity=sim)
    e.fit(*tr)
    maes, preds = e.mae_sweep(ks, *te, predictions=True)
    assert preds.shape == (len(ks), len(te[0]))
    m = oracle.Model(*tr)
    for q, k in enumerate(ks):
        want, opreds = m.pipeline(osim, k).mae(*te, True)
        assert np.array_equal(_bits(preds[q]), _bits(opreds)), k
        assert abs(maes[q] - want) <= MAE_TOL, k
    assert np.array_equal(_bits(maes), _bits(_loop_maes(kn, tr, te, ks, sim)))
    e.close()


def _with_unknowns(d):
    tr = (d.train.users, d.train.items, d.train.ratings)
    u = np.concatenate([d.test.users, [999_999, d.train.users[0]]]).astype(np.int32)
    i = np.concatenate([d.test.items, [d.train.items[0], 888_888]]).astype(np.int32)
    r = np.concatenate([d.test.ratings, [3.0, 4.0]])
    return tr, (u, i, r)


def test_syn100k_cosine_knn_scala_list(kn, oracle, syn100k):
    tr, te = _with_unknowns(syn100k)
    _check_against_oracle(kn, oracle, tr, te, KNN_SCALA_KS, kn.SIM_COSINE, oracle.SIM_COSINE)
    e = kn.Engine(k=10)
    e.fit(*tr)
    e.reset_timings()
    e.mae_sweep(KNN_SCALA_KS, *te)
    t = e.timings()
    assert t["gemm_launches"] == 1 and t["predict_ms"] > 0  # one build for the nine answers
    e.close()


def test_syn100k_without_item_bitmaps(kn, oracle, syn100k, monkeypatch):
    monkeypatch.setenv("KNNCF_DEBUG_NO_ITEM_BITMAPS", "1")  # read by the fit: the global-probe path of the kernel
    tr, te = _with_unknowns(syn100k)
    _check_against_oracle(kn, oracle, tr, te, KNN_SCALA_KS, kn.SIM_COSINE, oracle.SIM_COSINE)


def test_syn100k_jaccard(kn, oracle, syn100k):
    tr, te = _with_unknowns(syn100k)
    _check_against_oracle(kn, oracle, tr, te, (10, 300, 943), kn.SIM_JACCARD, oracle.SIM_JACCARD)


@pytest.mark.parametrize("seed", range(6))
def test_random_small_cases_with_tiny_rows(kn, oracle, seed):
    """users with <= 4 ratings: the pair summation order follows the build history, which the sweep's one build
    must reproduce for every k"""
    rng = np.random.default_rng(7300 + seed)
    rows = _random_case(rng, n_users=12 + 4 * seed, n_items=19, n_ratings=100 + 20 * seed, half=(seed % 2 == 1), tiny_rows=1 + seed % 4)
    cut = len(rows) * 4 // 5
    train, test = rows[:cut], rows[cut:]
    if not _no_zero_scale(train):
        pytest.skip("scale() == 0 corner")
    test += [(999_999, train[0][1], 3.0), (train[0][0], 888_888, 4.0)]
    tr, te = _cols(train), _cols(test)
    n_users = len(set(tr[0]))
    ks = (1, 2, 4, n_users - 1, n_users + 3)
    _check_against_oracle(kn, oracle, tr, te, ks, kn.SIM_COSINE, oracle.SIM_COSINE)


def test_single_k_equals_mae(kn, syn100k):
    tr, te = _with_unknowns(syn100k)
    e = kn.Engine(k=50)
    e.fit(*tr)
    want = e.mae(kn.PRED_KNN, *te)
    want_p = e.predict_batch(kn.PRED_KNN, te[0], te[1])
    maes, preds = e.mae_sweep([50], *te, predictions=True)
    assert _bits(maes).tolist() == _bits([want]).tolist()
    assert np.array_equal(_bits(preds[0]), _bits(want_p))
    e.close()


def test_handle_state_before_and_after(kn, syn100k, tmp_path):
    tr, te = _with_unknowns(syn100k)
    ks = (10, 100, 943)
    want = _loop_maes(kn, tr, te, ks, kn.SIM_COSINE)
    # a handle whose memo holds lists built by other calls: a mae over a partial test set (another build order), then lists
    # loaded from a checkpoint
    e = kn.Engine(k=300)
    e.fit(*tr)
    half = tuple(a[::-2] for a in te)
    e.mae(kn.PRED_KNN, *half)
    path = str(tmp_path / "nb.bin")
    e.neighbors_save(path)
    e.neighbors_load(path)
    assert np.array_equal(_bits(e.mae_sweep(ks, *te)), _bits(want))
    # afterwards: k unchanged, memo dropped — the same answers as a fresh handle at k = 300
    f = kn.Engine(k=300)
    f.fit(*tr)
    for u in (1, 2, 500, 943):
        gi, gs = e.neighbors(u)
        fi, fs = f.neighbors(u)
        assert len(gi) == 300 and gi.tolist() == fi.tolist() and _bits(gs).tolist() == _bits(fs).tolist(), u
    e.reset_neighbors()
    f.reset_neighbors()
    assert e.mae(kn.PRED_KNN, *te) == f.mae(kn.PRED_KNN, *te)
    # a second sweep on the same handle: the same answers
    assert np.array_equal(_bits(e.mae_sweep(ks, *te)), _bits(want))
    e.close()
    f.close()


def test_refusals(kn, syn100k):
    tr, te = _with_unknowns(syn100k)
    lib = kn.load_library()
    fresh = kn.Engine(k=10)
    with pytest.raises(kn.KnncfError) as ex:
        fresh.mae_sweep([10], *te)
    assert ex.value.status == kn.E_STATE
    fresh.close()
    e = kn.Engine(k=10)
    e.fit(*tr)
    for ks in ([], [10, 10], [30, 10], [0, 10], [10, 2049], list(range(1, 66))):
        with pytest.raises(kn.KnncfError) as ex:
            e.mae_sweep(ks, *te)
        assert ex.value.status == kn.E_INVALID, ks
    assert np.isnan(e.mae_sweep([10, 20], [], [], [])).all()
    assert e.mae_sweep(list(range(1, 65)), te[0][:50], te[1][:50], te[2][:50]).shape == (64,)
    assert lib.knncf_mae_sweep(None, None, 0, None, None, None, 0, None, None) == kn.E_INVALID
    e.close()
    one = kn.Engine(k=10, similarity=kn.SIM_ONE)
    one.fit(*tr)
    with pytest.raises(kn.KnncfError) as ex:
        one.mae_sweep([10], *te)
    assert ex.value.status == kn.E_UNSUPPORTED
    one.close()
    shard = kn.Engine(k=10, shard_rank=0, shard_count=2)
    shard.fit(*tr)
    with pytest.raises(kn.KnncfError) as ex:
        shard.mae_sweep([10], *te)
    assert ex.value.status == kn.E_STATE
    shard.close()


def test_shards_on_one_device(kn, pkg, syn100k):
    import torch

    sharded = importlib.import_module(pkg.__name__ + ".sharded")
    trh, teh = _with_unknowns(syn100k)
    ks = (10, 300, 943)
    single = kn.Engine(k=10)
    single.fit(*trh)
    want, want_p = single.mae_sweep(ks, *teh, predictions=True)
    single.close()
    dev = torch.device("cuda", 0)
    tr = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in trh)
    te = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in teh)
    n = len(teh[0])
    for world in (2, 3):
        engines = [kn.Engine(k=10, shard_rank=r, shard_count=world) for r in range(world)]
        views = []
        for e in engines:
            e.fit_device(*tr)
            views.append(sharded.DeviceEngineAdapter(e, dev).shard_tensors())
        for me in range(world):
            for other in range(world):
                if other != me:
                    lo, hi = views[other]["user_range"]
                    for key in ("user_avg", "user_norm"):
                        views[me][key][lo:hi] = views[other][key][lo:hi]
        torch.cuda.synchronize()
        preds = torch.full((len(ks), n), float("nan"), dtype=torch.float64, device=dev)
        sums, count = np.zeros(len(ks)), 0
        for e in engines:
            e.shard_commit()
            s, c = e.mae_sweep_device(ks, *te, pred_out=preds)
            sums += s
            count += c
            e.close()
        assert count == n
        assert np.array_equal(_bits(preds.cpu().numpy()), _bits(want_p)), world
        assert np.all(np.abs(sums / n - want) <= MAE_TOL), world


def test_syn25m_each_k_equals_set_k_mae(kn, synth):
    d = synth.syn_25m()
    tr = (d.train.users, d.train.items, d.train.ratings)
    te = (d.test.users, d.test.items, d.test.ratings)
    ks = (10, 300, 1000)
    e = kn.Engine(k=300)
    e.fit(*tr)
    maes, preds = e.mae_sweep(ks, *te, predictions=True)
    for q, k in enumerate(ks):
        e.set_k(k)
        assert _bits([e.mae(kn.PRED_KNN, *te)]).tolist() == _bits([maes[q]]).tolist(), k
        assert np.array_equal(_bits(e.predict_batch(kn.PRED_KNN, te[0], te[1])), _bits(preds[q])), k
    e.close()
