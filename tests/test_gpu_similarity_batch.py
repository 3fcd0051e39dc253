"""knncf_similarity_batch, knncf_similarity_batch_device and knncf_knn_similarity_batch on the GPU: every pair of
tests/similarity_pairs.case() (tests/test_similarity_batch_premises.py shows what that list can tell apart) against the
oracle and against a loop of the scalar calls on a twin handle, bit for bit; the device form, chunked calls and repeated calls;
what the calls leave in the handle (knncf_neighbors_save bytes); shard handles; the statuses.  Every comparison of values is ==
on int64 bit views."""
import importlib

import numpy as np
import pytest

from tests import similarity_pairs
from tests.similarity_pairs import ABSENT, bits
from tests.test_gpu_personalized_explain import _free_device_bytes

pytestmark = pytest.mark.gpu
TRACE = "KNNCF_DEBUG_TRACE_DISPATCH"
SIMS = ("cosine", "jaccard")


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def case():
    return similarity_pairs.case()


@pytest.fixture(scope="module")
def model(oracle, case):
    return oracle.Model(*case.train)


@pytest.fixture(scope="module")
def truth(oracle, case, model):
    """sim -> the oracle's fresh-closure similarity of every pair (computed once, read-only)"""
    out = {}
    for name, kind in (("cosine", oracle.SIM_COSINE), ("jaccard", oracle.SIM_JACCARD)):
        a = np.array([model.fresh_similarity(kind, u, v) for u, v in case.pairs])
        a.setflags(write=False)
        out[name] = a
    return out


def _sim(kn, oracle, name):
    return (kn.SIM_COSINE, oracle.SIM_COSINE) if name == "cosine" else (kn.SIM_JACCARD, oracle.SIM_JACCARD)


def _trace(capfd):
    return [ln[len("knncf-dispatch "):] for ln in capfd.readouterr().err.splitlines() if ln.startswith("knncf-dispatch ")]


def _same(got, want, what):
    bad = np.nonzero(bits(got) != bits(want))[0]
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), np.asarray(got)[bad[:4]].tolist(), np.asarray(want)[bad[:4]].tolist())


def _saved(e, tmp_path, name):
    path = str(tmp_path / name)
    e.neighbors_save(path)
    return open(path, "rb").read()


def _table(e, tmp_path, name):
    """knncf_neighbors_save parsed, every byte that the handle's state defines: header (with the call epoch), list lengths, build
    numbers and every built list.  (The cells of a list that was never built, and those past a list's length, are whatever the
    allocation held: two handles differ there, so they are masked — the rule of tests/test_gpu_recommend_batch.py.)"""
    raw = _saved(e, tmp_path, name)
    U, kcap = np.frombuffer(raw, dtype=np.int32, count=2, offset=8)
    kc = max(int(kcap), 1)
    at = 48
    cnt = np.frombuffer(raw, dtype=np.int32, count=U, offset=at); at += 4 * U
    seq = np.frombuffer(raw, dtype=np.int64, count=U, offset=at); at += 8 * U
    idx = np.frombuffer(raw, dtype=np.int32, count=U * kc, offset=at).reshape(U, kc); at += 4 * U * kc
    sim = np.frombuffer(raw, dtype=np.int64, count=U * kc, offset=at).reshape(U, kc)
    assert at + 8 * U * kc == len(raw)
    live = np.arange(kc)[None, :] < cnt[:, None]
    return {"header": raw[:48], "cnt": cnt.tolist(), "seq": seq.tolist(), "idx": np.where(live, idx, -1).tolist(),
            "sim": np.where(live, sim, 0).tolist()}


def _workspace_for(chunk):
    """workspace_bytes that makes the chunk rule of include/knncf.h (C = budget / 16, budget = workspace_bytes / 2) give `chunk`"""
    return 2 * 16 * chunk + 1


# ---- similarity_batch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", SIMS)
def test_pairs_equal_the_oracle_and_the_scalar_loop(kn, oracle, case, truth, monkeypatch, capfd, sim):
    import torch

    monkeypatch.setenv(TRACE, "1")
    n = len(case.us)
    e = kn.Engine(k=10, similarity=_sim(kn, oracle, sim)[0]).fit(*case.train)
    capfd.readouterr()
    got = e.similarity_batch(case.us, case.vs)
    assert _trace(capfd) == [f"pairs {sim} n={n}"]
    _same(got, truth[sim], "oracle")
    twin = kn.Engine(k=10, similarity=_sim(kn, oracle, sim)[0]).fit(*case.train)
    _same(got, [twin.similarity(u, v) for u, v in case.pairs], "scalar loop")
    twin.close()
    # a second call of the same shape: the same bits, and no device memory allocated
    free = _free_device_bytes()
    _same(e.similarity_batch(case.us, case.vs), got, "second call")
    assert _free_device_bytes() == free
    # the device form
    dev = torch.device("cuda", 0)
    d_us, d_vs = (torch.from_numpy(np.array(a)).to(dev) for a in (case.us, case.vs))
    d_out = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
    capfd.readouterr()
    e.similarity_batch_device(d_us, d_vs, d_out)
    assert _trace(capfd) == [f"pairs {sim} n={n}"]
    _same(d_out.cpu().numpy(), got, "device form")
    e.close()
    # chunks smaller than the pair count: 13 full chunks and a remainder
    chunk = 100
    small = kn.Engine(k=10, similarity=_sim(kn, oracle, sim)[0], workspace_bytes=_workspace_for(chunk)).fit(*case.train)
    capfd.readouterr()
    _same(small.similarity_batch(case.us, case.vs), got, "chunks")
    assert _trace(capfd) == [f"pairs {sim} n={chunk}"] * (n // chunk) + [f"pairs {sim} n={n % chunk}"]
    small.close()


def test_similarity_one(kn, case, monkeypatch, capfd):
    import torch

    monkeypatch.setenv(TRACE, "1")
    e = kn.Engine(k=10, similarity=kn.SIM_ONE).fit(*case.train)
    capfd.readouterr()
    _same(e.similarity_batch(case.us, case.vs), np.ones(len(case.us)), "host")
    d = lambda a: torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))
    out = d(np.zeros(len(case.us)))
    e.similarity_batch_device(d(case.us), d(case.vs), out)
    _same(out.cpu().numpy(), np.ones(len(case.us)), "device")
    assert _trace(capfd) == []
    with pytest.raises(kn.KnncfError) as ex:
        e.knn_similarity_batch(case.us[:4], case.vs[:4])
    assert ex.value.status == kn.E_UNSUPPORTED
    e.close()


@pytest.mark.parametrize("sim", SIMS)
def test_similarity_batch_only_reads_the_handle(kn, oracle, case, tmp_path, sim):
    e = kn.Engine(k=5, similarity=_sim(kn, oracle, sim)[0]).fit(*case.train)
    e.neighbors_batch(np.asarray(case.crafted[3:20:3] + [ABSENT[0]], dtype=np.int32))  # some lists exist, most do not
    before = _saved(e, tmp_path, "before.bin")
    e.similarity_batch(case.us, case.vs)
    assert _saved(e, tmp_path, "after.bin") == before
    # and the next build is numbered as if the call had not happened
    twin = kn.Engine(k=5, similarity=_sim(kn, oracle, sim)[0]).fit(*case.train)
    twin.neighbors_batch(np.asarray(case.crafted[3:20:3] + [ABSENT[0]], dtype=np.int32))
    rest = np.asarray(case.crafted[::-1], dtype=np.int32)
    e.neighbors_batch(rest)
    twin.neighbors_batch(rest)
    assert _table(e, tmp_path, "e.bin") == _table(twin, tmp_path, "twin.bin")
    e.close()
    twin.close()


@pytest.mark.parametrize("sim", SIMS)
def test_shards_answer_like_one_handle(kn, pkg, oracle, case, truth, sim):
    """two shard handles on the one GPU, committed as tests/test_gpu_handle_reuse.py commits them: after the commit every shard
    holds every user's preprocessed ratings and answers every pair"""
    import torch

    sharded = importlib.import_module(pkg.__name__ + ".sharded")
    dev = torch.device("cuda", 0)
    tr = tuple(torch.from_numpy(np.array(a)).to(dev) for a in case.train)
    world = 2
    engines = [kn.Engine(k=3, similarity=_sim(kn, oracle, sim)[0], shard_rank=r, shard_count=world) for r in range(world)]
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
    for r, e in enumerate(engines):
        _same(e.similarity_batch(case.us, case.vs), truth[sim], ("shard", r))
        e.close()


# ---- knn_similarity_batch -------------------------------------------------------------------------------------------------
def _n_users(case):
    return len(np.unique(case.train[0]))


def _oracle_knn(p, us, vs):
    """the stateful pipeline asked in this order"""
    return np.array([p.knn_similarity(int(u), int(v)) for u, v in zip(us, vs)])


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("k_of", [lambda U: 3, lambda U: 30, lambda U: U - 1, lambda U: U + 7], ids=["k3", "k30", "kU-1", "kU+7"])
def test_knn_pairs_equal_the_oracle_and_the_scalar_loop(kn, oracle, case, model, monkeypatch, capfd, k_of, sim):
    """k = 3; k = 30, beyond the number of users that share an item with most users (the lists end in 0.0 similarities); k = U - 1
    and beyond: every other user is in every list"""
    monkeypatch.setenv(TRACE, "1")
    U = _n_users(case)
    k = k_of(U)
    ksim, osim = _sim(kn, oracle, sim)
    e = kn.Engine(k=k, similarity=ksim).fit(*case.train)
    capfd.readouterr()
    got = e.knn_similarity_batch(case.us, case.vs)
    lines = _trace(capfd)
    assert lines.count(f"pairs lookup n={len(case.us)}") == 1 and not [ln for ln in lines if ln.startswith("pairs") and "lookup" not in ln]
    _same(got, _oracle_knn(model.pipeline(osim, k), case.us, case.vs), ("oracle", k))
    twin = kn.Engine(k=k, similarity=ksim).fit(*case.train)
    _same(got, [twin.knn_similarity(u, v) for u, v in case.pairs], ("scalar loop", k))
    known = set(case.train[0].tolist())
    zero = np.array([u == v or u not in known or v not in known for u, v in case.pairs])
    assert zero.sum() > len(case.crafted) and (bits(got[zero]) == 0).all()  # +0.0
    if k >= U - 1:
        # a list similarity of exactly 0.0 (users without a common item) comes back as +0.0, and it IS in the list
        a, b = case.crafted[21], case.crafted[22]
        ids, sims = twin.neighbors(a)
        j = case.pairs.index((a, b))
        assert b in ids.tolist() and sims[ids.tolist().index(b)] == 0.0 and bits(got[j:j + 1])[0] == 0
        assert (bits(got) != np.int64(-2**63)).all()  # never -0.0
    twin.close()
    free = _free_device_bytes()
    _same(e.knn_similarity_batch(case.us, case.vs), got, ("second call", k))
    assert _free_device_bytes() == free
    e.close()
    small = kn.Engine(k=k, similarity=ksim, workspace_bytes=_workspace_for(100)).fit(*case.train)
    _same(small.knn_similarity_batch(case.us, case.vs), got, ("chunks", k))
    small.close()


def _us_prime(case, us, vs):
    known = set(case.train[0].tolist())
    return np.asarray([u if (u in known and v in known) else ABSENT[0] for u, v in zip(us.tolist(), vs.tolist())], dtype=np.int32)


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("prebuilt", [False, True])
def test_knn_batch_leaves_the_state_of_neighbors_batch(kn, oracle, case, tmp_path, sim, prebuilt):
    """the knncf_neighbors_save file equals that of a twin that ran knncf_neighbors_batch over us' (_table).  The batch holds users that occur
    only beside an absent v: they must NOT be built."""
    c = case.crafted
    lonely = [c[2], c[12], c[25]]           # first arguments that only ever meet an absent second one
    body = [(u, v) for u, v in case.pairs[5::7] if u not in lonely]
    pairs = [(lonely[0], ABSENT[1])] + body[:60] + [(lonely[1], ABSENT[0]), (ABSENT[0], lonely[2])] + body[60:] + [(lonely[2], ABSENT[1])]
    us, vs = (np.asarray(x, dtype=np.int32) for x in zip(*pairs))
    prime = _us_prime(case, us, vs)
    assert not set(lonely) & set(prime.tolist()) and len(set(prime.tolist())) > 10
    ksim = _sim(kn, oracle, sim)[0]
    e, twin = (kn.Engine(k=4, similarity=ksim).fit(*case.train) for _ in range(2))
    first = np.asarray([c[30], c[1], c[18], c[7]] if prebuilt else [], dtype=np.int32)
    if prebuilt:
        e.neighbors_batch(first)
        twin.neighbors_batch(first)
    e.knn_similarity_batch(us, vs)
    twin.neighbors_batch(prime)
    mine, other = _table(e, tmp_path, "e.bin"), _table(twin, tmp_path, "twin.bin")
    assert mine == other and sum(q >= 0 for q in mine["seq"]) == len((set(prime.tolist()) | set(first.tolist())) - {ABSENT[0]})
    # nobody beside an absent id was built: asking for them now changes the file
    before = _saved(e, tmp_path, "before.bin")
    e.neighbors_batch(np.asarray(lonely, dtype=np.int32))
    assert _saved(e, tmp_path, "after.bin") != before
    e.close()
    twin.close()


def test_knn_batch_follows_its_own_order(kn, oracle, case, model):
    """<= 4-rating users in train: a pair's summation order is the first evaluating closure's, so the answers depend on
    the order of the batch — each order equals the oracle's pipeline asked in that order"""
    k = 6
    perm = np.random.default_rng(7).permutation(len(case.us))
    orders = [(case.us, case.vs), (case.us[::-1].copy(), case.vs[::-1].copy()), (case.us[perm], case.vs[perm])]
    for n, (us, vs) in enumerate(orders):
        e = kn.Engine(k=k).fit(*case.train)
        got = e.knn_similarity_batch(us, vs)
        _same(got, _oracle_knn(model.pipeline(oracle.SIM_COSINE, k), us, vs), ("order", n))
        e.close()


# ---- statuses -------------------------------------------------------------------------------------------------------------
def test_statuses(kn, case, tmp_path):
    import ctypes as C

    lib = kn.load_library()
    i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    us, vs = np.ascontiguousarray(case.us[:8]), np.ascontiguousarray(case.vs[:8])
    out = np.full(8, 7.0)
    pu, pv, po = us.ctypes.data_as(i32p), vs.ctypes.data_as(i32p), out.ctypes.data_as(f64p)
    null_i, null_f = C.cast(None, i32p), C.cast(None, f64p)
    host = (lib.knncf_similarity_batch, lib.knncf_knn_similarity_batch)
    e = kn.Engine(k=3)
    for f in host:  # before a fit
        assert f(e._h, pu, pv, 8, po) == kn.E_STATE
    assert lib.knncf_similarity_batch_device(e._h, None, None, 0, None) == kn.E_STATE
    e.fit(*case.train)
    before = _saved(e, tmp_path, "before.bin")
    for f in host:
        assert f(e._h, null_i, null_i, 0, null_f) == kn.OK          # n == 0 touches nothing
        assert f(e._h, pu, pv, -1, po) == kn.E_INVALID
        for args in ((null_i, pv, po), (pu, null_i, po), (pu, pv, null_f)):
            assert f(e._h, *args[:2], 8, args[2]) == kn.E_INVALID
    assert lib.knncf_similarity_batch_device(e._h, None, None, 0, None) == kn.OK
    assert lib.knncf_similarity_batch_device(e._h, None, None, -1, None) == kn.E_INVALID
    assert lib.knncf_similarity_batch_device(e._h, None, None, 8, None) == kn.E_INVALID
    assert out.tolist() == [7.0] * 8 and _saved(e, tmp_path, "after.bin") == before  # nothing written, nothing built
    assert len(e.similarity_batch([], [])) == 0 and len(e.knn_similarity_batch([], [])) == 0
    e.close()


def test_foreign_shard_user_is_refused_before_anything_is_built(kn, pkg, case):
    import ctypes as C

    import torch

    sharded = importlib.import_module(pkg.__name__ + ".sharded")
    dev = torch.device("cuda", 0)
    # (train without its <= 4-rating users: a shard may then build a list by a query)
    keep = ~np.isin(case.train[0], case.tiny)
    trc = tuple(np.ascontiguousarray(a[keep]) for a in case.train)
    tr = tuple(torch.from_numpy(a).to(dev) for a in trc)
    engines = [kn.Engine(k=3, shard_rank=r, shard_count=2) for r in range(2)]
    views = []
    for e in engines:
        e.fit_device(*tr)
        views.append(sharded.DeviceEngineAdapter(e, dev).shard_tensors())
    for me in range(2):
        lo, hi = views[1 - me]["user_range"]
        for key in ("user_avg", "user_norm"):
            views[me][key][lo:hi] = views[1 - me][key][lo:hi]
    torch.cuda.synchronize()
    for e in engines:
        e.shard_commit()
    users = [u for u in case.crafted if u not in case.tiny]
    owner = {}
    for u in users:
        for r, e in enumerate(engines):
            try:
                e.neighbors_batch([u])
                owner[u] = r
            except kn.KnncfError as ex:
                assert ex.status == kn.E_INVALID
    assert set(owner.values()) == {0, 1}
    for e in engines:
        e.reset_neighbors()
    mine = [u for u in users if owner[u] == 0]
    theirs = [u for u in users if owner[u] == 1]
    e = engines[0]
    us = np.asarray(mine[:5] + [theirs[0]] + mine[5:8], dtype=np.int32)
    vs = np.asarray(mine[1:6] + [mine[0]] + mine[:3], dtype=np.int32)
    out = np.full(len(us), 7.0)
    i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    e.reset_timings()
    before = e.timings()
    st = kn.load_library().knncf_knn_similarity_batch(e._h, us.ctypes.data_as(i32p), vs.ctypes.data_as(i32p), len(us), out.ctypes.data_as(f64p))
    assert st == kn.E_INVALID
    # nothing written, and no stage of a neighbour build ran (a shard handle writes no checkpoint to compare)
    assert out.tolist() == [7.0] * len(us) and e.timings() == before and before["select_launches"] == 0
    # the foreign user beside an absent v is not evaluated, hence not refused; a foreign v is only looked up
    us[5], vs[5] = theirs[0], ABSENT[0]
    vs[0] = theirs[1]
    got = e.knn_similarity_batch(us, vs)
    assert e.timings()["select_launches"] > 0
    single = kn.Engine(k=3).fit(*trc)
    _same(got, single.knn_similarity_batch(us, vs), "shard 0 against one handle")
    single.close()
    for e in engines:
        e.close()


# ---- raw ids outside the direct id tables: the hashed lookup on the device and on the host ---------------------------------
@pytest.mark.parametrize("sim", SIMS)
def test_ids_beyond_the_id_tables(kn, oracle, case, sim):
    """negative and large raw ids: the fit keeps no raw id -> dense index table, the pair kernels and the host look ids up in the
    sorted trie keys (and the dense order, hence every summation order, is another one)"""
    far = lambda a: (a.astype(np.int64) * 7919 - 60_000_000).astype(np.int32)
    train = (far(case.train[0]), (case.train[1].astype(np.int64) * 7919 + (1 << 25)).astype(np.int32), case.train[2])
    us, vs = far(case.us), far(case.vs)
    assert train[0].min() < 0 and len(np.unique(train[0])) == _n_users(case)
    ksim, osim = _sim(kn, oracle, sim)
    m = oracle.Model(*train)
    e = kn.Engine(k=3, similarity=ksim).fit(*train)
    _same(e.similarity_batch(us, vs), [m.fresh_similarity(osim, int(u), int(v)) for u, v in zip(us, vs)], "oracle")
    _same(e.knn_similarity_batch(us, vs), _oracle_knn(m.pipeline(osim, 3), us, vs), "kNN oracle")
    e.close()
