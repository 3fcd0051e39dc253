"""What the committed call sequences of tests/call_sequences.py can tell apart (CPU, oracle only): each deliberately wrong
model of the handle — wrong in one clause of include/knncf.h — must answer some op of the sequences differently from
HandleModel, in bits or ids; every sequence holds every call kind, derived from the Engine methods; and no op is left out.
The counts are printed (pytest -s) per case and wrong model."""
import importlib
import inspect

import pytest

from tests import call_sequences as cs

_counts = {}


def _differs(oracle, case, wrong):
    key = (case.name, wrong)
    if key not in _counts:
        _counts[key] = cs.differing_ops(oracle, case, wrong)
    return _counts[key]


@pytest.fixture(scope="module")
def engine_methods(pkg):
    kn = importlib.import_module(pkg.__name__ + ".knncf")
    return [n for n, f in inspect.getmembers(kn.Engine, inspect.isfunction) if not n.startswith("_")]


def test_counts_table(oracle):
    """prints, per case, how many of the 60 ops each wrong model changes"""
    print("\ncase      " + " ".join(f"{w:>18}" for w in cs.WRONG_MODELS))
    for case in cs.MEMO_CASES:
        print(f"{case.name:<10}" + " ".join(f"{len(_differs(oracle, case, w)):>18}" for w in cs.WRONG_MODELS))


@pytest.mark.parametrize("case", cs.MEMO_CASES, ids=lambda c: c.name)
def test_stateless_engine_differs_in_three_ops_of_every_sequence(oracle, case):
    """an engine that drops the memo before every call: at least 3 ops of EVERY memo sequence (the condition of the seed
    search)"""
    assert len(_differs(oracle, case, "stateless")) >= 3, case.name


@pytest.mark.parametrize("case", cs.MEMO_CASES, ids=lambda c: c.name)
def test_jaccard_has_no_order(oracle, case):
    """the Jaccard coefficient is a ratio of two counts: the same sequence under it cannot tell the stateless engine apart,
    which is why the premises above are stated under the adjusted cosine"""
    ops = case.ops(oracle)
    good = cs.play_on_model(case.model(oracle, "jaccard"), ops)
    bad = cs.play_on_model(case.model(oracle, "jaccard", wrong="stateless"), ops)
    assert all(cs.same(b, g) for g, b in zip(good, bad))


@pytest.mark.parametrize("wrong, drop", [("keeps_after_reset", "reset_neighbors"), ("keeps_after_sweep", "mae_sweep")])
def test_never_dropping_engine_differs_after_the_drop(oracle, wrong, drop):
    """the old pipeline kept across reset_neighbors / across mae_sweep: a later op differs in at least one sequence"""
    hits = []
    for case in cs.MEMO_CASES:
        ops = case.ops(oracle)
        first = min(j for j, op in enumerate(ops) if op.kind == drop)
        d = _differs(oracle, case, wrong)
        assert all(j > first or (j == first and drop == "mae_sweep") for j in d), (case.name, d, first)
        hits += [(case.name, j) for j in d if j > first]
    assert hits, wrong


def test_read_only_call_that_builds_differs_later(oracle):
    """a query, similarity_batch or explain_personalized for a fitted user that also evaluates the user's neighbourhood: the
    call's own answer is right, a LATER op differs"""
    hits = []
    for case in cs.MEMO_CASES:
        ops = case.ops(oracle)
        d = _differs(oracle, case, "read_only_builds")
        readers = [j for j, op in enumerate(ops) if op.kind in ("similarity_batch", "explain_personalized", "explain_personalized_batch")
                   or "_q" in op.kind]
        hits += [(case.name, j) for j in d if any(r < j for r in readers)]
    assert hits


def test_sorted_batch_differs(oracle):
    """neighbors_batch, recommend_batch and knn_similarity_batch evaluated in sorted instead of given order"""
    assert any(_differs(oracle, case, "sorted_batches") for case in cs.MEMO_CASES)


def test_every_engine_method_has_a_kind(engine_methods):
    """a family added to the Engine without a model method fails here instead of being skipped silently"""
    for name in engine_methods:
        kind = cs.kind_of(name)
        assert (kind is None) == (name in cs.NOT_MODELLED), name
        if kind is not None:
            assert kind in cs.KINDS and callable(getattr(cs.HandleModel, kind)) and callable(getattr(cs.Player, kind)), name
    kinds = {cs.kind_of(n) for n in engine_methods} - {None}
    assert kinds == set(cs.KINDS), (kinds ^ set(cs.KINDS))
    for kind in cs.DEVICE_FORMS:
        assert f"{kind}_device" in engine_methods, kind
    assert {n[:-7] for n in engine_methods if n.endswith("_device")} == set(cs.DEVICE_FORMS)


def _check_coverage(ops, refusals, short_fit, what):
    assert {op.kind for op in ops} >= set(cs.KINDS) - ({"fit"} if what.startswith("life") else set()), (what, set(cs.KINDS) - {op.kind for op in ops})
    statuses = {(k.split("_q")[0] if "_q" in k else k, s) for k, s in refusals}
    assert any(s == cs.E_UNSUPPORTED and "_q" in k for k, s in refusals), (what, "a query whose mean is negative")
    assert any(s == cs.E_INVALID and "_q" in k for k, s in refusals), (what, "a revise that removes an unrated item")
    fitted = any(s == cs.E_UNSUPPORTED and "_q" not in k for k, s in refusals)
    assert fitted == short_fit, (what, "Personalized with the adjusted cosine on a fit with a <= 4-rating user", statuses)


@pytest.mark.parametrize("case", cs.MEMO_CASES, ids=lambda c: c.name)
def test_memo_sequences_hold_every_kind_and_refusal(oracle, case):
    ops = case.ops(oracle)
    assert len(ops) == cs.N_OPS
    assert [repr(op) for op in ops] == [repr(op) for op in case.ops(oracle)]  # deterministic
    assert all("\n" not in repr(op) for op in ops)
    assert {op.form for op in ops} == {"host", "device"}
    _check_coverage(ops, cs.refusals_in(ops, lambda: case.model(oracle)), True, case.name)
    # the fitted Personalized forms are refused under the cosine only: under Jaccard the same ops are answered
    assert not [k for k, s in cs.refusals_in(ops, lambda: case.model(oracle, "jaccard")) if "_q" not in k]
    # the query forms are answered where the fitted forms refuse
    out = cs.play_on_model(case.model(oracle), ops)
    assert any(op.kind in ("predict_q", "recommend_q", "explain_q") and op.args[1] == cs.PRED_PERSONALIZED and not isinstance(o, cs.Refused)
               for op, o in zip(ops, out)), case.name


def test_memo_fits_are_as_described(oracle):
    import numpy as np

    for case in cs.MEMO_CASES:
        tr = case.train()
        users, counts = np.unique(tr[0], return_counts=True)
        assert len(users) == 40 and len(np.unique(tr[1])) == 12 and 160 <= len(tr[0]) <= 190 and (counts <= 4).sum() >= 18
        assert cs.K_ALL >= len(users) - 1


@pytest.mark.parametrize("life", range(len(cs.LIVES)))
def test_lives_hold_every_kind_variant_and_refusal(oracle, life):
    fit, k0, pool = cs.LIVES[life]
    ops = cs.life_ops(oracle, life)
    model = lambda: cs.HandleModel(oracle, fit.train, oracle.SIM_COSINE, k0)
    _check_coverage(ops, cs.refusals_in(ops, model), model().short_fit, f"life {life}")
    for what in cs.QUERY_WHATS:
        for tail in ("", "_batch"):
            seen = {(op.args[0], op.args[1]) for op in ops if op.kind == f"{what}_q{tail}"}
            want = {(f, p) for f in cs.FAMILIES for p in ((cs.PRED_KNN,) if what == "neighbors" else (cs.PRED_KNN, cs.PRED_PERSONALIZED))}
            assert seen >= want, (life, what, tail, want - seen)
    # query batches on both sides of the split between the two similarity kernels
    out = cs.play_on_model(model(), ops)
    answerable = {sum(not isinstance(x, cs.Refused) for x in o) for op, o in zip(ops, out) if op.kind.endswith("_q_batch")}
    assert {cs.QB_DUAL_MIN - 1, cs.QB_DUAL_MIN} <= answerable, (life, sorted(answerable))
