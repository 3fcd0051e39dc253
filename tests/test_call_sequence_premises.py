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
    """the ops that the wrong model changes: in the answer under the adjusted cosine, and for the wrong models of
    cs.WRONG_AFTER_APPEND in the answer or in the set of built lists under Jaccard (where the memo fits carry lists)"""
    key = (case.name, wrong)
    if key not in _counts:
        late = wrong in cs.WRONG_AFTER_APPEND
        _counts[key] = cs.differing_ops(oracle, case, wrong, sim="jaccard" if late else "cosine", with_built=late)
    return _counts[key]


def _public(cls):
    return [n for n, f in inspect.getmembers(cls, inspect.isfunction) if not n.startswith("_")]


@pytest.fixture(scope="module")
def engine_methods(pkg):
    kn = importlib.import_module(pkg.__name__ + ".knncf")
    return _public(kn.Engine)


@pytest.fixture(scope="module")
def wrapper_methods(pkg):
    """{class name: public methods} of every public class of knncf.py that wraps an engine: its constructor takes one"""
    kn = importlib.import_module(pkg.__name__ + ".knncf")
    found = {}
    for name, c in inspect.getmembers(kn, inspect.isclass):
        if c.__module__ != kn.__name__ or name.startswith("_") or c is kn.Engine:
            continue
        params = list(inspect.signature(c.__init__).parameters.values())[1:]
        if any(p.name == "engine" or p.annotation is kn.Engine for p in params):
            found[name] = _public(c)
    return found


def test_counts_table(oracle):
    """prints, per case, how many of the ops each wrong model changes"""
    print("\ncase      " + " ".join(f"{w:>{max(18, len(w))}}" for w in cs.WRONG_MODELS))
    for case in cs.MEMO_CASES:
        print(f"{case.name:<10}" + " ".join(f"{len(_differs(oracle, case, w)):>{max(18, len(w))}}" for w in cs.WRONG_MODELS))


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


def _played(oracle, case, sim):
    model = case.model(oracle, sim)
    return model, cs.play_on_model(model, case.ops(oracle))


@pytest.mark.parametrize("wrong", cs.WRONG_AFTER_APPEND)
def test_wrong_fit_after_an_append_differs_later(oracle, wrong):
    """an append that keeps every built list, one that keeps the old fit's statistics and Personalized answers, and an entered
    call that builds nothing: each shows in an op AFTER the first append or entered call of some sequence, in the answer or in
    the set of built lists"""
    starts = ("append",) if wrong.startswith("append") else cs.ENTERED
    hits = []
    for case in cs.MEMO_CASES:
        ops = case.ops(oracle)
        first = min(j for j, op in enumerate(ops) if op.kind in starts)
        d = _differs(oracle, case, wrong)
        assert all(j >= first for j in d), (case.name, d, first)
        hits += [(case.name, j) for j in d if j > first]
    assert hits, wrong
    if wrong == "entered_builds_nothing":  # ... and in what a later append carries
        assert any(case.ops(oracle)[j].kind == "append" for case in cs.MEMO_CASES
                   for j in cs.differing_ops(oracle, case, wrong, sim="jaccard"))


@pytest.mark.parametrize("case", cs.MEMO_CASES, ids=lambda c: c.name)
def test_memo_appends_carry_and_drop(oracle, case):
    """under Jaccard some append of every sequence meets built lists, keeps some and drops some; under the adjusted cosine every
    append of a memo fit (users of <= 4 ratings) is a plain refit; one append of every sequence is refused and leaves no trace"""
    model, out = _played(oracle, case, "jaccard")
    assert any(a["carried"] >= 1 and a["dropped"] >= 1 for a in model.appends), (case.name, model.appends)
    assert all(a["carried"] + a["dropped"] == a["built"] for a in model.appends)
    cosine, out_c = _played(oracle, case, "cosine")
    assert cosine.appends and all(a["plain"] and a["carried"] == 0 for a in cosine.appends), (case.name, cosine.appends)
    ops = case.ops(oracle)
    for o in (out, out_c):
        refused = [x for op, x in zip(ops, o) if op.kind == "append" and isinstance(x, cs.Refused)]
        assert [x.status for x in refused] == [cs.E_DUPLICATE], case.name
    assert len(model.appends) == len(cosine.appends) == sum(op.kind == "append" for op in ops) - 1 >= 3
    # the rows come in all three shapes: a fitted changer, a newcomer, both interleaved
    fitted = set(case.train()[0].tolist())
    shapes = set()
    for op, x in zip(ops, out):
        if op.kind == "fit":
            fitted = set(op.args[0].train[0].tolist())
        if op.kind == "append" and not isinstance(x, cs.Refused):
            users = list(dict.fromkeys(op.args[0].tolist()))
            new = [u for u in users if u not in fitted]
            assert all(u > cs.NEWCOMER for u in new) and len(new) <= 1
            shapes.add("both" if new and len(users) > 1 else "newcomer" if new else "changer")
            fitted |= set(users)
    assert shapes == set(cs.APPEND_SHAPES), (case.name, shapes)


def test_entered_calls_meet_missing_and_complete_tables(oracle):
    """some entered call finds every list built (M empty) and in every sequence one finds lists to build (M not empty), under
    Jaccard; under the adjusted cosine the memo fits refuse the entered calls and nothing is built"""
    missing = []
    for case in cs.MEMO_CASES:
        model, _ = _played(oracle, case, "jaccard")
        assert max(model.entered_missing) > 0, (case.name, model.entered_missing)
        missing += model.entered_missing
        cosine, out = _played(oracle, case, "cosine")
        assert cosine.entered_missing == []
        assert all(isinstance(x, cs.Refused) and x.status == cs.E_UNSUPPORTED for op, x in zip(case.ops(oracle), out) if op.kind in cs.ENTERED)
    assert 0 in missing, missing


@pytest.mark.parametrize("life", range(len(cs.LIVES)))
def test_lives_append_early_and_carry(oracle, life):
    """every life has an accepted append in the first half of its body; on the fits without short rows (A, B, D) some append
    under the adjusted cosine keeps lists and drops lists; on the memo fit C every append is a plain refit"""
    fit, k0, _ = cs.LIVES[life]
    ops = cs.life_ops(oracle, life)
    model = cs.HandleModel(oracle, fit.train, oracle.SIM_COSINE, k0)
    out = cs.play_on_model(model, ops)
    body = ops[2:]
    accepted = [j for j, (op, x) in enumerate(zip(body, out[2:])) if op.kind == "append" and not isinstance(x, cs.Refused)]
    assert accepted and accepted[0] < len(body) // 2, (life, accepted, len(body))
    if model.short_fit:
        assert all(a["plain"] for a in model.appends), (life, model.appends)
    else:
        assert any(a["carried"] >= 1 and a["dropped"] >= 1 for a in model.appends), (life, model.appends)
        assert max(model.entered_missing) > 0, (life, model.entered_missing)


def test_every_engine_method_has_a_kind(engine_methods, wrapper_methods):
    """a family added to the Engine, or in a class beside it that wraps one, without a model method fails here instead of being
    skipped silently"""
    for name in engine_methods:
        kind = cs.kind_of(name)
        assert (kind is None) == (name in cs.NOT_MODELLED), name
        if kind is not None:
            assert kind in cs.KINDS and callable(getattr(cs.HandleModel, kind)) and callable(getattr(cs.Player, kind)), name
    kinds = {cs.kind_of(n) for n in engine_methods} - {None}
    assert {"BystanderQueries", "EnteredQueries", "Appends"} <= set(wrapper_methods), sorted(wrapper_methods)
    for owner, names in wrapper_methods.items():
        assert names, owner
        for name in names:
            kind = cs.kind_of(name, owner)
            assert kind in cs.KINDS and callable(getattr(cs.HandleModel, kind)) and callable(getattr(cs.Player, kind)), (owner, name)
            assert kind not in kinds, (owner, name, "the kind of another class's method")
        kinds |= {cs.kind_of(n, owner) for n in names}
    for kind in cs.BYSTANDER:  # both families of every bystander kind exist
        what, tail = kind[len("bystander_"):].replace("_batch", ""), "_batch" if kind.endswith("_batch") else ""
        assert {f"{what}_{fam}{tail}" for fam in cs.BYSTANDER_FAMILIES} <= set(wrapper_methods["BystanderQueries"]), kind
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
    # (of the kinds beside the Engine's only what the generator plants is refused: the duplicate append, and a query inside a batch
    # of entered or bystander queries that is invalid as such)
    beside = ("append",) + cs.ENTERED + cs.BYSTANDER
    jaccard = cs.refusals_in(ops, lambda: case.model(oracle, "jaccard"))
    assert not [k for k, s in jaccard if "_q" not in k and k not in beside]
    assert {(k, s) for k, s in jaccard if k in beside} <= {("append", cs.E_DUPLICATE)} | {(k, cs.E_INVALID) for k in beside if k.endswith("_batch")}
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
