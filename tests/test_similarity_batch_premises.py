"""The inputs of tests/test_gpu_similarity_batch.py can catch a wrong pair kernel (no GPU): on tests/similarity_pairs.case()
the oracle's fresh-closure similarity equals the literal closures of tests/scala_model.py on every pair, and the pair list
separates the left fold in the first argument's item order from every other way of adding the same products — a pairwise
tree, 64 per-lane partial sums, the reverse order, the other argument's order, ascending items for a <= 4-rating first
argument, fused multiply-add — and holds the Jaccard NaN."""
from fractions import Fraction

import numpy as np
import pytest

from tests import scala_model, similarity_pairs
from tests.similarity_pairs import bits


@pytest.fixture(scope="module")
def case():
    return similarity_pairs.case()


@pytest.fixture(scope="module")
def model(oracle, case):
    return oracle.Model(*case.train)


@pytest.fixture(scope="module")
def cosine(oracle, case, model):
    """the oracle's fresh-closure adjusted cosine of every pair"""
    return np.array([model.fresh_similarity(oracle.SIM_COSINE, u, v) for u, v in case.pairs])


@pytest.fixture(scope="module")
def products(case, model):
    """per pair: pre(u, i) * pre(v, i) over the common items in the item-set order of u (a <= 4-item set iterates in file
    order, a larger one in trie order), and the same products in ascending trie order"""
    pre = {(int(u), int(i)): float(p) for u, i, p in zip(case.train[0], case.train[1], model.preprocessed())}
    out = []
    for u, v in case.pairs:
        u_items = scala_model.scala_order([i for i, _ in case.rows.get(u, [])])
        v_items = set(i for i, _ in case.rows.get(v, []))
        both = [i for i in u_items if i in v_items]
        trie = similarity_pairs.item_orders(both)[1]
        out.append(([pre[u, i] * pre[v, i] for i in both], [pre[u, i] * pre[v, i] for i in trie]))
    return out


def _fold(xs):
    acc = 0.0
    for x in xs:
        acc = acc + x
    return acc


def _tree(xs):
    if len(xs) <= 1:
        return xs[0] if xs else 0.0
    h = len(xs) // 2
    return _tree(xs[:h]) + _tree(xs[h:])


def _lanes(xs):
    return _fold([_fold(xs[l::64]) for l in range(64)])


def _fresh_literal(case, make):
    """the literal closure `make(ratings)` on every pair, each on a closure that has seen neither (u, v) nor (v, u)"""
    ratings = list(zip(case.train[0].tolist(), case.train[1].tolist(), case.train[2].tolist()))
    closures, out = [], []
    for u, v in case.pairs:
        key = frozenset((u, v))
        for c in closures:
            if key not in c[1]:
                break
        else:
            c = (make(ratings), set())
            closures.append(c)
        c[1].add(key)
        out.append(c[0](u, v))
    return np.array(out)


def _same(a, b):
    """bit for bit; a NaN equals a NaN (the literal model's is Python's)"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a[~nan]), bits(b[~nan]))


def test_case_is_what_it_claims(case):
    lengths = sorted(len(case.rows[u]) for u in case.crafted)
    for n in (1, 2, 3, 4) + similarity_pairs.PIECE_EDGE_ROWS + (similarity_pairs.LONG_ROW,):
        assert n in lengths
    sets = {u: frozenset(i for i, _ in case.rows[u]) for u in case.crafted}
    assert any(sets[u] == sets[v] and len(sets[u]) >= 130 for u in case.crafted for v in case.crafted if u < v)
    assert any(not (sets[u] & sets[v]) and len(sets[u]) > 4 and len(sets[v]) > 4 for u in case.crafted for v in case.crafted if u < v)
    assert (case.train[2] * 16 != np.round(case.train[2] * 16)).mean() > 0.5  # non-dyadic ratings
    file_items = {}
    for u, i in zip(case.train[0].tolist(), case.train[1].tolist()):
        file_items.setdefault(u, []).append(i)
    for u in case.tiny:
        got = file_items[u]
        assert len(got) <= 4
        asc, trie = similarity_pairs.item_orders(got)
        if len(got) >= 3:
            assert got != asc and got != trie, u
    pairs = case.pairs
    known = set(case.train[0].tolist())
    assert set((u, v) for u in case.crafted for v in case.crafted) <= set(pairs)
    assert any((u in known) != (v in known) for u, v in pairs) and any(u not in known and v not in known for u, v in pairs)
    assert len(set(pairs)) < len(pairs)
    assert any(pairs[j + 1] == (pairs[j][1], pairs[j][0]) and pairs[j][0] != pairs[j][1] for j in range(len(pairs) - 1))


def test_oracle_equals_literal_closures(oracle, case, model, cosine):
    """(a)"""
    assert _same(cosine, _fresh_literal(case, scala_model.adjusted_cosine_similarity_function))
    jac = np.array([model.fresh_similarity(oracle.SIM_JACCARD, u, v) for u, v in case.pairs])
    assert _same(jac, _fresh_literal(case, scala_model.jaccard_coefficient))


def test_products_fold_to_the_oracle(cosine, products):
    assert _same(cosine, [_fold(p) for p, _ in products])


@pytest.mark.parametrize("other", [_tree, _lanes, lambda xs: _fold(xs[::-1])], ids=["tree", "lanes", "reverse"])
def test_long_folds_depend_on_their_order(products, other):
    """(b) among the pairs with >= 128 common items at least half get other bits from another summation"""
    long_ones = [p for p, _ in products if len(p) >= 128]
    differ = sum(bits(_fold(p)) != bits(other(p)) for p in long_ones)
    assert len(long_ones) >= 20 and 2 * differ >= len(long_ones), (differ, len(long_ones))


def test_given_order_shows(case, products):
    """(c) <= 4-rating first users with >= 3 common items: file order against ascending items"""
    differ = sum(len(case.rows.get(u, ())) <= 4 and len(p) >= 3 and bits(_fold(p)) != bits(_fold(t))
                 for (u, _), (p, t) in zip(case.pairs, products))
    assert differ >= 8, differ


def test_argument_order_shows(case, cosine):
    """(d) no memo across pairs is observable: sim(u, v) and sim(v, u) differ for some pair"""
    at = {}
    for j, p in enumerate(case.pairs):
        at.setdefault(p, j)
    assert any((v, u) in at and bits(cosine[j]) != bits(cosine[at[v, u]]) for (u, v), j in at.items())


def test_jaccard_of_two_absent_users_is_nan(oracle, case, model):
    """(e)"""
    known = set(case.train[0].tolist())
    both_absent = [(u, v) for u, v in case.pairs if u not in known and v not in known]
    assert both_absent and all(np.isnan(model.fresh_similarity(oracle.SIM_JACCARD, u, v)) for u, v in both_absent)


def test_fused_multiply_add_shows(case, model, cosine):
    """(f) s = fma(a, b, s) instead of s = s + a * b changes some pair's bits"""
    pre = {(int(u), int(i)): float(p) for u, i, p in zip(case.train[0], case.train[1], model.preprocessed())}
    differ = 0
    for (u, v), want in list(zip(case.pairs, cosine))[: 40 * len(case.crafted)]:
        u_items = scala_model.scala_order([i for i, _ in case.rows.get(u, [])])
        v_items = set(i for i, _ in case.rows.get(v, []))
        both = [i for i in u_items if i in v_items]
        if not 2 <= len(both) <= 64:
            continue
        s = 0.0
        for i in both:
            s = float(Fraction(pre[u, i]) * Fraction(pre[v, i]) + Fraction(s))  # one rounding
        differ += bits(s) != bits(want)
    assert differ >= 1
