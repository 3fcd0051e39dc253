"""What the inputs of tests/revise_entered_cases.py reach, from the oracle alone (no GPU): the kinds of reported rows that the
removal cases hold — entered, left, moved, same position, tail rows — with the counts asserted, the guarantee for every unreported
user (lists and predictions, the removed items among them), the pair-order premise of a changer that falls to <= 4 rows on aug,
the Jaccard re-rating whose rows keep identical non-zero bits, the item that leaves aug, the zero-weight exception, and the list
positions and dense indices that the fixed-size cases put the changer at."""
from collections import Counter

import numpy as np
import pytest

from tests import revise_entered_cases as rc
from tests import update_entered_cases as uc
from tests.bystander_cases import _rows, _users
from tests.query_helpers import _bits

COS, JAC = rc.COS, rc.JAC
MAKERS = {"removes-3": rc.removes_3, "keeps-4": rc.keeps_4, "re-rates": rc.re_rates}
# (case, k, similarity) -> entered, left, moved, same position, tail rows
COUNTS = {("removes-3", 5, COS): (3, 4, 4, 4, 5), ("removes-3", 20, COS): (2, 7, 24, 6, 8), ("removes-3", 5, JAC): (0, 5, 3, 1, 6),
          ("keeps-4", 5, COS): (4, 9, 1, 2, 9), ("keeps-4", 20, COS): (1, 25, 10, 2, 25), ("keeps-4", 5, JAC): (0, 9, 0, 0, 9),
          ("re-rates", 5, COS): (3, 4, 5, 3, 5), ("re-rates", 20, COS): (5, 2, 31, 4, 3), ("re-rates", 5, JAC): (0, 0, 0, 9, 2)}


@pytest.mark.parametrize("name,k,sim", sorted(COUNTS))
def test_kinds(synth, oracle, name, k, sim):
    case = MAKERS[name](synth, k)
    out, kinds, quiet = rc.expected(oracle, case, sim, with_kinds=True)
    n = Counter(kinds)
    tails = rc.tail_rows(oracle, case, sim)
    assert (n["entered"], n["left"], n["moved"], n["same"], len(tails)) == COUNTS[name, k, sim]
    assert sum(p < 0 for p in tails) == n["left"]  # (a c that leaves sorts behind every other stored entry: always a tail row)
    assert len(out[0]) + len(quiet) == 59 and len(out[0]) > 0  # a removal-only query reports: aug is not train


@pytest.mark.parametrize("name", sorted(MAKERS))
@pytest.mark.parametrize("k", [59, 300])
@pytest.mark.parametrize("sim", [COS, JAC])
def test_short_lists(synth, oracle, name, k, sim):
    """k = U - 1 and beyond: nobody is outside a list, everybody is reported, nobody enters or leaves"""
    out, kinds, quiet = rc.expected(oracle, MAKERS[name](synth, k), sim, with_kinds=True)
    assert len(out[0]) == 59 and not quiet and set(kinds) <= {"moved", "same"} and (out[4] == -1).all()


@pytest.mark.parametrize("name", sorted(MAKERS))
@pytest.mark.parametrize("sim", [COS, JAC])
@pytest.mark.parametrize("k", [5, 20, 59])
def test_guarantee_for_unreported_users(synth, oracle, name, sim, k):
    """L1 == L0 in ids and similarity bytes, and the kNN predictions on every train item of the changer — the removed and the
    re-rated ones among them — are those on train"""
    case = MAKERS[name](synth, k)
    kind = uc.sim_kind(oracle, sim)
    out, kinds, quiet = rc.expected(oracle, case, sim, with_kinds=True)
    assert len(quiet) >= 17 or k == 59  # (k = 59 = U - 1: everybody is reported, no row is left)
    m0, m1 = oracle.Model(*case.train), oracle.Model(*case.aug)
    items = np.concatenate([_rows(case.train, case.q)[0], case.items]).tolist()
    assert set(case.removed.tolist()) <= set(items)
    for v, L0, L1 in quiet:
        assert L0[0] == L1[0] and _bits(L0[1]) == _bits(L1[1]), v
        p0, p1 = m0.pipeline(kind, k), m1.pipeline(kind, k)
        assert _bits([p0.predict(v, int(i)) for i in items]) == _bits([p1.predict(v, int(i)) for i in items]), v


def test_the_cases_cover_every_kind(synth, oracle):
    """across the removal cases: every kind, a same-position row whose bits changed, tail rows that stay and that leave"""
    new_bits = stay = leave = 0
    seen = set()
    for (name, k, sim) in COUNTS:
        case = MAKERS[name](synth, k)
        out, kinds, quiet = rc.expected(oracle, case, sim, with_kinds=True)
        rows, _ = rc.lists_of(oracle, case.train, case.q, case.removed, case.items, case.ratings, k, sim)
        lists = {v: (a, b) for v, a, b in rows}
        seen |= set(kinds)
        for v, s, pr, kind in zip(out[0], out[1], out[3], kinds):
            new_bits += kind == "same" and _bits([lists[int(v)][0][1][pr]]) != _bits([s])
        tails = rc.tail_rows(oracle, case, sim)
        stay += sum(p >= 0 for p in tails)
        leave += sum(p < 0 for p in tails)
    assert seen == {"entered", "left", "moved", "same"} and new_bits > 0 and stay > 0 and leave > 0


# ---- keeps-4: the pair stage ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,changer,rows", [(5, rc.KEEPS_4_K5_CHANGER, [55]), (20, rc.CHANGER, [53]), (59, rc.CHANGER, [21, 53]),
                                            (300, rc.CHANGER, [21, 53])])
def test_keeps_4_reports_rows_whose_bits_depend_on_the_owner(synth, oracle, k, changer, rows):
    """c has 4 rows on aug: S(c, v) folds in c's given order, S(v, c) in v's dense-item order.  At least one REPORTED row's
    out_sims differs in bits from fresh_similarity(c, v) on aug — without such a row the pair stage is not under test"""
    case = rc.keeps_4(synth, k, changer)
    assert len(_rows(case.aug, changer)[0]) == rc.KEPT
    got = rc.pair_order_rows(oracle, case)
    assert [v for v, _ in got] == rows and len(got) >= 1
    m1 = oracle.Model(*case.aug)
    for v, s in got:
        assert _bits([m1.fresh_similarity(oracle.SIM_COSINE, v, changer)]) == _bits([s])
        assert abs(m1.fresh_similarity(oracle.SIM_COSINE, changer, v) - s) < 1e-15  # (the same products in another order)


def test_keeps_4_of_user_5_reports_no_such_row_at_k5(synth, oracle):
    """why k = 5 has a changer of its own: the two pairs of user 5 whose bits depend on the owner (bystanders 21 and 53) are not
    reported there, and user 24 is the first changer, in ascending raw id, keeping 4 and then 3 rows, that has one"""
    assert rc.pair_order_rows(oracle, rc.keeps_4(synth, 5)) == []
    train = rc.keeps_4(synth, 5).train
    first = next(c for c in _users(train) for kept in (4, 3)
                 if rc.pair_order_rows(oracle, rc.keeps_4(synth, 5, c, kept)))
    assert first == rc.KEEPS_4_K5_CHANGER


# ---- re-ratings ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", rc.KS)
def test_jaccard_re_rating_keeps_identical_non_zero_bits(synth, oracle, k):
    """a re-rating changes no item set: every Jaccard similarity and every position stays — and every such row IS reported,
    because equal bits are silent only when they are +-0.0"""
    case = rc.re_rates(synth, k)
    out, kinds, quiet = rc.expected(oracle, case, JAC, with_kinds=True)
    rows, _ = rc.lists_of(oracle, case.train, case.q, case.removed, case.items, case.ratings, k, JAC)
    lists = {v: (a, b) for v, a, b in rows}
    assert set(kinds) == {"same"} and len(out[0]) == {5: 9, 20: 28}.get(k, 59)
    for v, s, p, pr in zip(out[0], out[1], out[2], out[3]):
        assert p == pr and s != 0.0 and _bits([lists[int(v)][0][1][pr]]) == _bits([s]), v
    assert all(case.q not in L0[0] for v, L0, L1 in quiet)


@pytest.mark.parametrize("sim", [COS, JAC])
def test_same_value_re_rating_is_an_ordinary_query(synth, oracle, sim):
    """the rows move behind every train row: the query is answered like any other, the users that hold c are reported"""
    case = rc.same_value(synth, 5)
    out, kinds, quiet = rc.expected(oracle, case, sim, with_kinds=True)
    assert len(out[0]) == {COS: 12, JAC: 9}[sim] and all(case.q not in L0[0] and case.q not in L1[0] for v, L0, L1 in quiet)


# ---- an item that leaves aug, the zero weight ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [COS, JAC])
def test_lone_item(synth, oracle, sim):
    """c's removed item has no other rater: it was a term of no pair, so it changes a list only through c's own similarity (its
    mean, deviations and norm moved) — as the removal of an item that others rate does.  Without c, every list on aug is the
    list on train up to the cell that c's move frees or takes"""
    gone, rerated, kept = rc.lone_item(synth, 5)
    for case in (gone, rerated, kept):
        rows, _ = rc.lists_of(oracle, case.train, case.q, case.removed, case.items, case.ratings, case.k, sim)
        for v, L0, L1 in rows:
            a = [(x, _bits([s])) for x, s in zip(L0[0], L0[1]) if x != case.q]
            b = [(x, _bits([s])) for x, s in zip(L1[0], L1[1]) if x != case.q]
            n = min(len(a), len(b))
            assert a[:n] == b[:n] and abs(len(a) - len(b)) <= 1, (case.name, v)
        assert len(rc.expected(oracle, case, sim)[0]) > 0
    m = oracle.Model(*gone.aug)
    assert rc.rb.LONE_ITEM not in np.asarray(gone.aug[1]).tolist() and m.num_items == oracle.Model(*gone.train).num_items - 1


@pytest.mark.parametrize("sim", [COS, JAC])
def test_zero_weight(synth, oracle, sim):
    case = rc.zero_weight(synth)
    z = case.note["planted"]
    rows, _ = rc.lists_of(oracle, case.train, case.q, case.removed, case.items, case.ratings, case.k, sim)
    L0, L1 = next((a, b) for v, a, b in rows if v == z)
    p = L0[0].index(case.q)
    assert L1[0].index(case.q) == p and _bits([L0[1][p], L1[1][p]]) == _bits([0.0, 0.0])
    out = rc.expected(oracle, case, sim)
    assert z not in out[0].tolist() and len(out[0]) == 59
    assert len(rc.expected_for(oracle, case.train, case.q, [], [], [], case.k, sim)[0]) == 0  # exception (a)


# ---- fixed-size edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", uc.EDGE_KS)
def test_list_edge_positions(synth, oracle, k):
    """on the fit of 140 users the changer of update_entered_cases.edge_changer stands at positions 0, 63, 64 and last of full
    lists; removing half of its rows, or three, moves it up in some lists and out of others"""
    train = uc.scaled(synth, uc.EDGE_USERS)
    c = uc.edge_changer(oracle, train, k)
    for n in rc.edge_removals(train, c):
        out, kinds, _ = rc.expected_for(oracle, train, c, rc.removed_rows(train, c, n), [], [], k, COS, with_kinds=True)
        assert uc.edge_positions(k) <= set(out[3].tolist())
        up = ((out[2] >= 0) & (out[3] >= 0) & (out[2] < out[3])).sum()
        assert up > 0 and kinds.count("left") > 0 and kinds.count("entered") > 0, (k, n)


@pytest.mark.parametrize("n_users", uc.EDGE_FITS)
def test_dense_index_edges(synth, oracle, n_users):
    """the changers of the U-edge cases stand at dense index 63, 64 (where the fit has it) and U - 1, keep more than 4 rows, and
    at k = U - 1 the users at those indices are reported"""
    train = uc.scaled(synth, n_users)
    order = uc.dense_order(oracle, train)
    for at in uc.edge_indices(n_users):
        c = order[at]
        out = rc.expected_for(oracle, train, c, rc.removed_rows(train, c, 3), [], [], n_users - 1, COS)
        assert len(out[0]) >= n_users - 4
        assert {order[x] for x in uc.edge_indices(n_users) if x != at} <= set(out[0].tolist())
