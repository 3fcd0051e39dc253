"""The premises of tests/test_gpu_predict_edges.py, from the data and the oracle alone (no GPU): every case of
tests/predict_edges.py has the match counts, the bitmap corners and the run structure it claims.  The kernels' fixed sizes
appear here as LITERALS: a product change that moves one of them must fail here, visibly, instead of silently turning the GPU
tests into ordinary-shape tests.

The conditions on similarity signs, exact zeros and summation order are conditions on the INPUTS (which is why the seeds of
predict_edges.SEEDS were picked): without them a kernel that folded its matches in list or id order would pass."""
import numpy as np
import pytest

from tests import boundary_shapes as bs
from tests import explain_model as em
from tests import predict_edges as pe

MCAP = 64          # predict.hip k_predict_knn_items: matches ranked by readlane up to here, in windows of 64 above
PRED_CHUNK = 64    # predict.hip: rows per workgroup of the item-grouped kernel (ksweep.hip SWEEP_CHUNK: the same)
ROWS_CHUNK = 32    # predict.hip k_predict_knn_rows: rows per wave
WAVES = 4          # both grouped kernels are launched with 4 waves
K = 2048
# kcap -> (TR, G) of the grouped kernels (predict.hip launch_predict), bitmap words ceil(U / 64)
GROUPED = {65: (1, 4), 66: (2, 4), 129: (2, 4), 257: (4, 2), 258: (5, 2), 321: (5, 2), 322: (8, 1), 513: (8, 1)}
IB_WORDS = {65: 2, 66: 2, 129: 3, 257: 5, 258: 5, 321: 6, 322: 6, 513: 9, 514: 9, 1025: 17, 2049: 33}
ALL_USERS = pe.GROUPED_USERS + pe.GENERAL_USERS
ISSUE_MATCHES = (0, 1, 3, 4, 5, 63, 64, 65, 67, 68, 69, 127, 128, 129, 131, 132, 191, 192, 193)  # + kcap - 1 and kcap


@pytest.fixture(scope="module")
def models(oracle):
    made = {}

    def get(U):
        if U not in made:
            m = oracle.Model(*pe.case(U).train)
            made[U] = (m, em.TermModel(oracle, m, oracle.SIM_COSINE, K))
        return made[U]

    return get


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- the training sets ----------------------------------------------------------------------------------------------------------
def test_case_lists_are_the_planned_ones():
    assert pe.GROUPED_USERS == tuple(GROUPED) and pe.GENERAL_USERS == (514, 1025, 2049) and pe.K == K
    assert [U - 1 for U in pe.GROUPED_USERS] == [64, 65, 128, 256, 257, 320, 321, 512]  # the ends of TR = 1, 2, 4, 5, 8
    for U, form in GROUPED.items():  # the form by 64-neighbour trips: 1, 2, 3-4, 5, 6-8
        trips = (U - 1 + 63) // 64
        assert form == ((1, 4) if trips <= 1 else (2, 4) if trips <= 2 else (4, 2) if trips <= 4 else (5, 2) if trips <= 5 else (8, 1))
    assert pe.counts_of(513) == (1, 4, 5, 64, 65, 68, 69, 128, 129, 132, 192, 193, 512, 513)
    assert pe.counts_of(65) == (1, 4, 5, 64, 65) and pe.counts_of(129) == (1, 4, 5, 64, 65, 68, 69, 128, 129)
    assert set(ALL_USERS) == set(pe.SEEDS) and (pe.WAVES, pe.ITEM_CHUNK, pe.ROW_CHUNK) == (WAVES, PRED_CHUNK, ROWS_CHUNK)


@pytest.mark.parametrize("U", ALL_USERS)
def test_conventions(U):
    c = pe.case(U)
    tr, te = c.train, c.test
    assert tr[0].dtype == np.int32 and tr[1].dtype == np.int32 and tr[2].dtype == np.float64
    assert np.array_equal(np.unique(tr[0]), np.arange(1, U + 1))
    assert np.array_equal(2 * tr[2], np.round(2 * tr[2])) and tr[2].min() >= 1.0 and tr[2].max() <= 5.0
    pairs = tr[0].astype(np.int64) * (1 << 32) + tr[1]
    assert len(np.unique(pairs)) == len(pairs)
    bg = tr[1] <= 40
    assert tr[1][bg].min() >= 2 and (np.bincount(tr[0][bg], minlength=U + 1)[1:] == 6).all()  # more than 4 ratings each
    lo, hi = np.full(U + 1, 9.0), np.zeros(U + 1)
    np.minimum.at(lo, tr[0][bg], tr[2][bg])
    np.maximum.at(hi, tr[0][bg], tr[2][bg])
    assert (lo[1:] < hi[1:]).all()
    assert not np.array_equal(tr[0], np.sort(tr[0])) and len(tr[0]) <= 20_000
    assert len(te[0]) == len(c.matches) == 2 * len(c.items) - 1  # a non-rater and a rater per item; c = U has no non-rater
    again = pe.planted(U, pe.counts_of(U), pe.SEEDS[U])
    assert all(np.array_equal(x, y) for x, y in zip(again.train + again.test, tr + te))


@pytest.mark.parametrize("U", ALL_USERS)
def test_bitmap_width_and_corner_raters(models, U):
    c = pe.case(U)
    words = (U + 63) // 64
    assert words == IB_WORDS[U] and words % 2 == {65: 0, 66: 0, 129: 1, 257: 1, 258: 1, 321: 0, 322: 0, 513: 1, 514: 1, 1025: 1, 2049: 1}[U]
    assert np.array_equal(models(U)[0].user_iteration_order(), bs.users_by_dense(U))
    dense = bs.dense_of(U)
    for cnt, item in c.items.items():
        got = np.sort(c.train[0][c.train[1] == item])
        assert len(got) == cnt and np.array_equal(got, c.raters[cnt])
        if cnt >= 4:  # the first bit, the last bit of word 0, the first bit of word 1, the last valid bit of the last word
            assert {0, 63, 64, U - 1} <= set(dense[got].tolist()), (U, cnt)
    assert (U - 1) // 64 == words - 1 and ((U - 1) % 64 == 0) == (U in (65, 129, 257, 321, 513, 1025, 2049))


@pytest.mark.parametrize("U", ALL_USERS)
def test_match_counts_are_the_planned_ones(models, U):
    c = pe.case(U)
    kcap = U - 1
    p = models(U)[1].pipeline
    got = []
    for u, i, want in zip(c.test[0].tolist(), c.test[1].tolist(), c.matches):
        ids, _ = p.neighbors(u)
        assert len(ids) == kcap and u not in ids  # every other user is in the list
        raters = c.train[0][c.train[1] == i]
        n = int(np.isin(ids, raters).sum())
        assert n == want == len(raters) - int(u in raters), (U, u, i)
        got.append(n)
    assert set(got) == pe.planned_matches(U) == {m for m in ISSUE_MATCHES if m <= kcap} | {kcap - 1, kcap}
    # both sides of MCAP, every window edge that the list length allows, both sides of the pad to 4, total == CAP
    assert {MCAP - 1, MCAP} <= set(got) and (kcap == MCAP or MCAP + 1 in set(got))
    for edge in (128, 192):
        if kcap > edge:
            assert {edge - 1, edge, edge + 1} <= set(got)
    assert {3, 4, 5} <= set(got) and any(m % 4 == 0 for m in got) and any(m % 4 == 3 for m in got) and kcap in got


@pytest.mark.parametrize("U", ALL_USERS)
def test_similarity_signs_zeros_and_summation_order(models, U):
    """file order is not id order and not list order, and it shows in the bits: of the rows with at least 3 non-zero terms at
    least half fold to other (num, den) bits in ascending dense id order, and at least half in the order of the user's list"""
    c = pe.case(U)
    _, tm = models(U)
    dense = bs.dense_of(U)
    zero_rows, mixed_rows, rows3, by_id, by_list = 0, 0, 0, 0, 0
    for u, i in zip(c.test[0].tolist(), c.test[1].tolist()):
        ids, sims = tm.pipeline.neighbors(u)
        hit = np.isin(ids, c.train[0][c.train[1] == i])
        zero_rows += bool((sims[hit] == 0.0).any())
        mixed_rows += bool((sims[hit] > 0.0).any() and (sims[hit] < 0.0).any())
        row = tm.row(u, i)
        if row.count < 3:
            continue
        rows3 += 1
        want = _bits(em.fold(row.sims, row.devs))
        assert np.array_equal(want, _bits([row.num, row.den]))
        place = np.full(U + 1, -1)
        place[ids] = np.arange(len(ids))
        for order, key in (("id", dense[row.raters]), ("list", place[row.raters])):
            perm = np.argsort(key, kind="stable")
            differs = not np.array_equal(_bits(em.fold(row.sims[perm], row.devs[perm])), want)
            by_id += differs and order == "id"
            by_list += differs and order == "list"
    assert zero_rows >= 1 and mixed_rows >= 1, (U, zero_rows, mixed_rows)
    assert rows3 >= 4 and 2 * by_id >= rows3 and 2 * by_list >= rows3, (U, rows3, by_id, by_list)


# ---- the batches: read back out of the order the engine sorts into ---------------------------------------------------------------
def _segments(keys, chunk):
    """(start, length, key) of every run of equal keys inside every chunk of `chunk` rows: what a workgroup (wave) walks"""
    out = []
    for c0 in range(0, len(keys), chunk):
        a = c0
        end = min(c0 + chunk, len(keys))
        while a < end:
            b = a + 1
            while b < end and keys[b] == keys[a]:
                b += 1
            out.append((a, b - a, int(keys[a])))
            a = b
    return out


def _whole_runs(keys):
    return [n for _, n, _ in _segments(keys, len(keys))]


@pytest.mark.parametrize("U", pe.RUN_USERS + (129,))  # (129: the batch of the two-shard test)
def test_item_grouped_batch_has_the_planted_runs(U):
    c = pe.case(U)
    TR, G = GROUPED[U]
    assert (TR, G) == {65: (1, 4), 129: (2, 4), 257: (4, 2), 513: (8, 1)}[U]
    W = WAVES * G
    b = pe.run_batch(c, f"items TR={TR} G={G}")
    assert 200 <= len(b[0]) <= 700 and not np.array_equal(b[1], np.sort(b[1]))  # shuffled
    order = pe.engine_order(c.train, b, by_item=True)
    users, items = b[0][order], b[1][order]
    known_item, known_user = np.isin(items, c.train[1]), users <= U
    active = known_item & known_user
    n_known = int(known_item.sum())
    assert known_item[:n_known].all() and n_known == len(items) - 4  # the unknown-item rows all land at the end
    dense_item = {int(v): d for d, v in enumerate(pe.items_by_dense(c.train))}
    assert [dense_item[int(v)] for v in items[:n_known]] == sorted(dense_item[int(v)] for v in items[:n_known])
    assert (~known_user[n_known:]).any() and known_user[n_known:].any()
    whole = _whole_runs(items[:n_known])
    for length in (1, W - 1, W, W + 1, 63, 64, 65, 129):
        assert length in whole, (U, "run length", length)
    if U in (257, 513):  # the long runs sit on items with more than 65 raters: every row has more than MCAP matches, all four waves window
        n_raters = np.bincount(c.train[1])
        long_runs = [(n, k) for _, n, k in _segments(items[:n_known], n_known) if n in (63, 64, 65, 129)]
        assert len(long_runs) == 4 and all(n_raters[k] - 1 > MCAP for _, k in long_runs), (U, long_runs)
    seg = _segments(items, PRED_CHUNK)
    starts = {a: n for a, n, _ in seg}
    assert len(items) % PRED_CHUNK == 1 and seg[-1][1] == 1  # a last chunk of 1 row
    for length in (1, W - 1, W, W + 1, 63, 64):  # inside ONE workgroup's chunk
        assert any(n == length and active[a:a + n].all() for a, n, _ in seg), (U, "segment length", length)
    # a run that starts on the last row of a chunk, and one that ends on the first row of a chunk
    assert any(a % PRED_CHUNK == PRED_CHUNK - 1 and items[a + 1] == k and active[a] for a, n, k in seg if a + 1 < len(items))
    assert any(a % PRED_CHUNK == 0 and n == 1 and a > 0 and items[a - 1] == k and active[a] for a, n, k in seg)
    # inactive rows in the first, a middle and the last slot of a group of G: wave w's trip t takes rows a + (t WAVES + w) G ..
    slots = set()
    for a, n, _ in seg:
        if 0 < (~active[a:a + n]).sum() < n and known_item[a]:
            slots |= {int(j - a) % G for j in np.flatnonzero(~active[a:a + n]) + a}
    assert {0, G // 2, G - 1} <= slots, (U, slots)
    # a run all of whose rows are inactive, an active run of another item right behind it in the same chunk: once with a
    # bitmap loaded before them in that chunk, once at the very start of a chunk
    after_loaded, at_chunk_start = False, False
    for (a, n, k), (a2, n2, k2) in zip(seg, seg[1:]):
        if known_item[a] and not active[a:a + n].any() and a2 // PRED_CHUNK == a // PRED_CHUNK and known_item[a2] and active[a2:a2 + n2].all():
            assert k2 != k
            at_chunk_start |= a % PRED_CHUNK == 0
            after_loaded |= a % PRED_CHUNK > 0 and active[a - 1]
    assert after_loaded and at_chunk_start
    assert starts[0] == 64


@pytest.mark.parametrize("U", pe.RUN_USERS)
def test_row_grouped_batch_has_the_planted_runs(U):
    c = pe.case(U)
    TR, G = GROUPED[U]
    b = pe.run_batch(c, f"rows TR={TR} G={G}")
    assert 100 <= len(b[0]) <= 500 and not np.array_equal(b[0], np.sort(b[0]))
    order = pe.engine_order(c.train, b, by_item=False)
    users, items = b[0][order], b[1][order]
    known_user, known_item = users <= U, np.isin(items, c.train[1])
    active = known_user & known_item
    n_known = int(known_user.sum())
    assert known_user[:n_known].all() and n_known == len(users) - 3  # the unknown-user rows all land at the end
    dense = bs.dense_of(U)
    assert np.array_equal(dense[users[:n_known]], np.sort(dense[users[:n_known]]))
    whole = _whole_runs(users[:n_known])
    for length in {1, G - 1, G, G + 1, 31, 32, 33, 65} - {0}:
        assert length in whole, (U, "run length", length)
    assert len(users) % ROWS_CHUNK == 1  # a last wave of 1 row
    assert len(users) > ROWS_CHUNK * WAVES  # more than one workgroup
    seg = _segments(users, ROWS_CHUNK)
    # a user change in the middle of a group: a run of all-active rows whose length is no multiple of G, another user's
    # active row behind it in the same wave
    if G > 1:
        assert any(n % G and active[a:a + n + 1].all() and (a + n) // ROWS_CHUNK == a // ROWS_CHUNK for a, n, _ in seg if a + n < n_known)
    # unknown-item rows inside a user's run: its first row, an inner row, its last row
    where = set()
    for a, n, _ in seg:
        off = np.flatnonzero(~active[a:a + n])
        if known_user[a] and 0 < len(off) < n:
            where |= {"first" if j == 0 else "last" if j == n - 1 else "inner" for j in off.tolist()}
    assert where == {"first", "inner", "last"}
    assert any(known_user[a] and not active[a:a + n].any() for a, n, _ in seg)  # and a user none of whose rows is active
    assert any(a % ROWS_CHUNK == ROWS_CHUNK - 1 and n == 1 and users[a + 1] == k for a, n, k in seg if a + 1 < n_known)  # straddles


@pytest.mark.parametrize("kcap", [U - 1 for U in (65, 129, 513, 1025, 2049)])
def test_sweep_lists(kcap):
    lists = pe.sweep_ks(kcap)
    assert [len(ks) for ks in lists] == [1, 63, 64]  # 64: the ABI's limit, one lane per k
    for ks in lists:
        assert all(a < b for a, b in zip(ks, ks[1:])) and 1 <= ks[0] and ks[-1] <= 2048
    for ks in lists[1:]:
        assert {1, 63, 64, 65, kcap - 1, kcap} <= set(ks)
        assert (max(ks) > kcap) == (kcap < 2048)
    assert lists[0] == [kcap - 1]  # (the table is built for max(ks): the case's CAP form with one live lane)
