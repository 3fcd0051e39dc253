"""What the inputs of tests/update_entered_cases.py reach, from the oracle alone (no GPU): the kinds of reported rows that the
adds-3 cases hold — entered, left, moved, same position with new bits, tail rows of both outcomes — with the counts asserted, the
guarantee for every unreported user, the zero-weight exception, the tie at the cut on both sides of the set order, and the list
positions and dense indices that the fixed-size cases put the changer at."""
from collections import Counter

import numpy as np
import pytest

from tests import update_entered_cases as uc
from tests.query_helpers import _bits

# (k, similarity) -> entered, left, moved, same position, tail rows that stay
ADDS_COUNTS = {(5, uc.COS): (2, 7, 2, 3, 0), (5, uc.JAC): (2, 2, 5, 2, 2), (20, uc.COS): (4, 10, 24, 3, 1), (20, uc.JAC): (4, 5, 21, 2, 1)}


def _with_lists(oracle, case, sim):
    out, kinds, quiet = uc.expected(oracle, case, sim, with_kinds=True)
    rows, m1 = uc.lists_of(oracle, case.train, case.q, case.items, case.ratings, case.k, sim)
    return out, kinds, quiet, {v: (a, b) for v, a, b in rows}


@pytest.mark.parametrize("k,sim", sorted(ADDS_COUNTS))
def test_adds_3_kinds(synth, oracle, k, sim):
    case = uc.adds_3(synth, k)
    out, kinds, quiet, lists = _with_lists(oracle, case, sim)
    n = Counter(kinds)
    tails = [int(p) for v, p, pr in zip(out[0], out[2], out[3]) if uc.is_tail(k, int(pr), int(p), *lists[int(v)], case.q)]
    stay = sum(p >= 0 for p in tails)
    assert (n["entered"], n["left"], n["moved"], n["same"], stay) == ADDS_COUNTS[k, sim]
    assert len(tails) - stay == n["left"]  # (a c that leaves sorts behind every other stored entry: always a tail row)
    assert len(out[0]) + len(quiet) == 59


def test_adds_3_covers_every_kind(synth, oracle):
    """across the cases: every kind, a same-position row whose bits changed, and tail rows that stay and that leave"""
    new_bits = stay = leave = 0
    for (k, sim) in ADDS_COUNTS:
        case = uc.adds_3(synth, k)
        out, kinds, quiet, lists = _with_lists(oracle, case, sim)
        for v, s, p, pr, kind in zip(out[0], out[1], out[2], out[3], kinds):
            L0, L1 = lists[int(v)]
            new_bits += kind == "same" and _bits([L0[1][pr]]) != _bits([s])
            if uc.is_tail(k, int(pr), int(p), L0, L1, case.q):
                stay += p >= 0
                leave += p < 0
    assert new_bits > 0 and stay > 0 and leave > 0


@pytest.mark.parametrize("k", [59, 300])
@pytest.mark.parametrize("sim", [uc.COS, uc.JAC])
def test_adds_3_short_lists(synth, oracle, k, sim):
    """no user is outside a list: every other user is reported, nobody enters or leaves"""
    case = uc.adds_3(synth, k)
    out, kinds, quiet = uc.expected(oracle, case, sim, with_kinds=True)
    assert len(out[0]) == 59 and not quiet and set(kinds) <= {"moved", "same"} and (out[4] == -1).all()


@pytest.mark.parametrize("k,sim", sorted(ADDS_COUNTS))
def test_guarantee_for_unreported_users(synth, oracle, k, sim):
    """L1 == L0 in ids and similarity bits, and the kNN predictions on the changer's items and its added items are those on train"""
    case = uc.adds_3(synth, k)
    kind = uc.sim_kind(oracle, sim)
    out, kinds, quiet = uc.expected(oracle, case, sim, with_kinds=True)
    assert len(quiet) > 10
    m0, m1 = oracle.Model(*case.train), oracle.Model(*case.aug)
    items = np.concatenate([uc._rows(case.train, case.q)[0], case.items]).tolist()
    for v, L0, L1 in quiet:
        assert L0[0] == L1[0] and _bits(L0[1]) == _bits(L1[1]), v
        p0, p1 = m0.pipeline(kind, k), m1.pipeline(kind, k)
        assert _bits([p0.predict(v, int(i)) for i in items]) == _bits([p1.predict(v, int(i)) for i in items]), v


@pytest.mark.parametrize("sim", [uc.COS, uc.JAC])
def test_zero_weight(synth, oracle, sim):
    case = uc.zero_weight(synth)
    z = case.note["planted"]
    rows, _ = uc.lists_of(oracle, case.train, case.q, case.items, case.ratings, case.k, sim)
    L0, L1 = next((a, b) for v, a, b in rows if v == z)
    p = L0[0].index(case.q)
    assert L1[0].index(case.q) == p and _bits([L0[1][p], L1[1][p]]) == _bits([0.0, 0.0])
    out = uc.expected(oracle, case, sim)
    assert z not in out[0].tolist() and len(out[0]) == 59  # every other user holds c in its list of U - 1
    assert len(uc.expected_for(oracle, case.train, case.q, [], [], case.k, sim)[0]) == 0


def test_tie_at_the_cut(oracle, synth):
    before, after = uc.tie(synth, oracle)
    for case in (before, after):
        v, x, c = case.note["bystander"], case.note["copy_of"], case.q
        m = oracle.Model(*case.aug)
        assert _bits([m.users_avg(c)]) == _bits([m.users_avg(x)])
        ids, sims = m.pipeline(oracle.SIM_COSINE, case.k + 1).neighbors(v)
        ids = ids.tolist()
        assert {ids[case.k - 1], ids[case.k]} == {c, x} and _bits([sims[case.k - 1]]) == _bits([sims[case.k]])
        first = c if case.note["side"] == "before" else x
        assert ids[case.k - 1] == first
        out = uc.expected(oracle, case, uc.COS)
        row = out[0].tolist().index(v) if v in out[0].tolist() else -1
        if case.note["side"] == "before":
            assert row >= 0 and out[2][row] == case.k - 1  # c holds the last cell, x is out
        else:
            assert row < 0 or out[2][row] == -1            # x holds it: c is not in v's list on aug


@pytest.mark.parametrize("k", uc.EDGE_KS)
def test_list_edge_positions(synth, oracle, k):
    """on the fit of 140 users the changer stands, in full lists on train, at positions 0, 63 and 64 (where the list has them) and
    at the last one"""
    train = uc.scaled(synth, uc.EDGE_USERS)
    c = uc.edge_changer(oracle, train, k)
    m = oracle.Model(*train)
    seen = set()
    for v in m.user_iteration_order().tolist():
        ids = m.pipeline(oracle.SIM_COSINE, k).neighbors(v)[0].tolist() if v != c else []
        assert v == c or len(ids) == k
        if c in ids:
            seen.add(ids.index(c))
    assert uc.edge_positions(k) <= seen


@pytest.mark.parametrize("n_users", uc.EDGE_FITS)
def test_dense_index_edges(synth, oracle, n_users):
    """the changers of the U-edge cases stand at dense index 63, 64 (where the fit has it) and U - 1, and at k = U - 1 users at
    those indices are reported"""
    train = uc.scaled(synth, n_users)
    order = uc.dense_order(oracle, train)
    for at in uc.edge_indices(n_users):
        c = order[at]
        items, ratings = uc.added_rows(train, c)
        out = uc.expected_for(oracle, train, c, items, ratings, n_users - 1, uc.COS)
        assert len(out[0]) >= n_users - 4  # (every list holds c; a user that shares no item with it is the zero-weight exception)
        assert {order[x] for x in uc.edge_indices(n_users) if x != at} <= set(out[0].tolist())
