"""The premises of tests/test_gpu_personalized_queries.py, from the oracle alone (no GPU): the inputs those tests use exercise
what is particular to the Personalized predictor on a query user — the value of the own term's weight S(u, u), the PLACE of the
own term in the item's file order, and the difference to the kNN predictor with k = U."""
import numpy as np

from tests import personalized_query_cases as pc


def _users(train):
    return pc.pick_users(train)[:4]


def test_own_term_value_place_and_knn_difference_syn100k(oracle, syn100k):
    full = pc.syn100k(syn100k)
    users = _users(full)
    train, rows = pc.hold_out(full, users, 3)
    n_users = len(np.unique(train[0]))
    moved = not_one = 0
    for q in users:
        aug = pc.aug_of(train, q, pc.NONE_I, *rows[q])
        model = oracle.Model(*aug)
        personalized, knn = model.pipeline(oracle.SIM_COSINE, -1), model.pipeline(oracle.SIM_COSINE, n_users)
        not_one += personalized.raw_similarity(q, q) != 1.0
        mine = set(aug[1][aug[0] == q].tolist())
        others = [int(i) for i in np.unique(aug[1]) if int(i) not in mine][::9]
        # an item the user has not rated: no own term, every other user a neighbour at k = U -> the same fold
        assert pc.bits([personalized.predict(q, i) for i in others]) == pc.bits([knn.predict(q, i) for i in others]), q
        # an item the user rates: the own term weighs S(u, u) here and 0 there
        own = sorted(mine)[:12]
        assert sum(a != b for a, b in zip(pc.bits([personalized.predict(q, i) for i in own]), pc.bits([knn.predict(q, i) for i in own]))) > 0, q
        # a surviving train item: the own term's place shows
        for i in train[1][train[0] == q][:12]:
            at, last = pc.fold_parts(oracle, aug, q, oracle.SIM_COSINE, int(i)), pc.fold_parts(oracle, aug, q, oracle.SIM_COSINE, int(i), own_last=True)
            moved += pc.bits(at) != pc.bits(last)
            w = at[0] / at[1] if at[1] > 0 else 0.0
            avg = model.users_avg(q)
            assert pc.bits([avg + w * pc_scale(avg + w, avg)]) == pc.bits([personalized.predict(q, int(i))]), (q, i)  # fold_parts is the oracle's fold
    assert moved >= 1
    assert not_one >= 1


def pc_scale(x, y):
    return 5 - y if x > y else (y - 1 if x < y else 1)


def test_edge_set_shape(oracle):
    train = pc.edge_set()
    u, i, r = train
    assert len(np.unique(u)) == 140
    counts = {int(a): int(b) for a, b in zip(*np.unique(i, return_counts=True))}
    assert counts == pc.EDGE_ITEMS  # 1, 63, 64, 65, 129: the boundaries of the 64-entry loads
    assert pc.NEW_ITEM not in counts and pc.UNKNOWN_ITEM not in counts
    per_user = np.unique(u, return_counts=True)[1]
    assert (per_user <= 4).sum() >= 20 and per_user.max() >= 5
    assert np.any(r != np.round(r * 2) / 2)  # non-dyadic
    long_rows = u[i == pc.EDGE_LONG]
    assert long_rows[0] == pc.EDGE_FIRST and long_rows[-1] == pc.EDGE_LAST
    assert 0 < int(np.flatnonzero(long_rows == pc.EDGE_MIDDLE)[0]) < len(long_rows) - 1
    assert u[i == pc.EDGE_LONE_ITEM].tolist() == [pc.EDGE_LONE_USER]
    qs = pc.edge_queries(train)
    rows_aug = lambda name: int((pc.aug_of(train, *qs[name])[0] == qs[name][0]).sum())
    assert [rows_aug(n) for n in ("new_1", "new_1_unknown", "new_4", "new_5", "new_6")] == [1, 1, 4, 5, 6]
    for name, (q, removed, items, ratings) in qs.items():
        assert pc.EDGE_NEVER not in items.tolist() and pc.EDGE_NEVER not in i[u == q].tolist(), name
        assert rows_aug(name) >= 1, name
        assert set(removed.tolist()) <= set(i[u == q].tolist()), name
    for place in ("first", "middle", "last"):
        assert f"revise_{place}_rerate_long" in qs and f"update_{place}" in qs
    assert sum(name.endswith("keep_long") for name in qs) >= 1 and sum(name.endswith("drop_long") for name in qs) >= 1
    # the own term's place shows on the hand set too, and the lone item has one term when re-rated, none when removed
    moved = 0
    for name in ("update_first", "update_middle", "update_last"):
        aug = pc.aug_of(train, *qs[name])
        q = qs[name][0]
        a, b = pc.fold_parts(oracle, aug, q, oracle.SIM_COSINE, pc.EDGE_LONG), pc.fold_parts(oracle, aug, q, oracle.SIM_COSINE, pc.EDGE_LONG, own_last=True)
        moved += pc.bits(a) != pc.bits(b)
    assert moved >= 1
    assert pc.EDGE_LONE_ITEM not in pc.aug_of(train, *qs["lone_removed"])[1].tolist()
    aug = pc.aug_of(train, *qs["lone_rerated"])
    assert aug[0][aug[1] == pc.EDGE_LONE_ITEM].tolist() == [pc.EDGE_LONE_USER]
    # an item that only the query user rates does not answer the mean
    aug = pc.aug_of(train, *qs["new_6"])
    m = oracle.Model(*aug)
    assert m.pipeline(oracle.SIM_COSINE, -1).predict(905, pc.NEW_ITEM) != m.users_avg(905)
    assert m.pipeline(oracle.SIM_COSINE, -1).predict(905, pc.UNKNOWN_ITEM) == m.users_avg(905)
