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
    cs.WRONG_AFTER_APPEND, cs.WRONG_AFTER_AMEND and "bystander_revised_builds" in the answer or in the set of built lists under
    Jaccard (where the memo fits carry lists)"""
    key = (case.name, wrong)
    if key not in _counts:
        late = wrong in cs.WRONG_MODELS[5:]  # (the models of an append, an entered call, an amend and the revised bystanders)
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
    for models in (cs.WRONG_MODELS[:8], cs.WRONG_MODELS[8:]):
        print("\ncase      " + " ".join(f"{w:>{max(18, len(w))}}" for w in models))
        for case in cs.MEMO_CASES:
            print(f"{case.name:<10}" + " ".join(f"{len(_differs(oracle, case, w)):>{max(18, len(w))}}" for w in models))


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
    appends = [a for a in model.appends if a["kind"] == "append"]  # (model.appends holds the accepted amends too)
    assert any(a["carried"] >= 1 and a["dropped"] >= 1 for a in appends), (case.name, appends)
    assert all(a["carried"] + a["dropped"] == a["built"] for a in model.appends)
    cosine, out_c = _played(oracle, case, "cosine")
    appends_c = [a for a in cosine.appends if a["kind"] == "append"]
    assert appends_c and all(a["plain"] and a["carried"] == 0 for a in appends_c), (case.name, appends_c)
    ops = case.ops(oracle)
    for o in (out, out_c):
        refused = [x for op, x in zip(ops, o) if op.kind == "append" and isinstance(x, cs.Refused)]
        assert [x.status for x in refused] == [cs.E_DUPLICATE], case.name
    assert len(appends) == len(appends_c) == sum(op.kind == "append" for op in ops) - 1 >= 3
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
        if op.kind == "amend" and not isinstance(x, cs.Refused):  # (its newcomer joins; the user that leaves is no changer later)
            fitted |= set(op.args[2].tolist())
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
    appends = [a for a in model.appends if a["kind"] == "append"]
    if model.short_fit:
        assert all(a["plain"] for a in appends), (life, appends)
    else:
        assert any(a["carried"] >= 1 and a["dropped"] >= 1 for a in appends), (life, appends)
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
    for kind in cs.BYSTANDER:  # every family of every bystander kind exists: "revised" is the *_with method with removed=
        what, tail = kind[len("bystander_"):].replace("_batch", ""), "_batch" if kind.endswith("_batch") else ""
        for fam in cs.BYSTANDER_FAMILIES:
            owner, name, with_removed = cs.method_of(cs.Op(kind, (fam, (0, [], [], []))))
            assert owner == "BystanderQueries" and name in wrapper_methods[owner], (kind, fam)
            assert with_removed == (fam == "revised") and name == f"{what}_{'with' if fam == 'revised' else fam}{tail}"
    assert kinds == set(cs.KINDS), (kinds ^ set(cs.KINDS))
    for kind in cs.DEVICE_FORMS:
        assert f"{kind}_device" in engine_methods, kind
    assert {n[:-7] for n in engine_methods if n.endswith("_device")} == set(cs.DEVICE_FORMS)


def _takes_removed(pkg):
    """{(class, method): whether `removed` is optional} of every public method of Engine and of the wrapper classes whose
    signature has a parameter `removed` — the keyword or argument that switches the method to a knncf_revise_* entry point — or
    whose name says *_revised*"""
    kn = importlib.import_module(pkg.__name__ + ".knncf")
    found = {}
    for owner, c in inspect.getmembers(kn, inspect.isclass):
        if c.__module__ != kn.__name__ or owner.startswith("_"):
            continue
        for name in _public(c):
            p = inspect.signature(getattr(c, name)).parameters.get("removed")
            if p is not None:
                found[owner, name] = p.default is not inspect.Parameter.empty
            elif "_revised" in name:  # (the batch forms take the removals inside their queries)
                found[owner, name] = False
    return found


def test_every_method_with_removed_is_played_both_ways(oracle, pkg, wrapper_methods):
    """a method's name says nothing about a keyword that switches its C entry point (knncf_update_* to knncf_revise_*): every
    public method with a parameter `removed` is played in EVERY life with removals and, where the parameter is optional, without"""
    takes = _takes_removed(pkg)
    by, en = ("BystanderQueries", "EnteredQueries")
    assert {(by, f"{w}_with{t}") for w in ("neighbors", "predict") for t in ("", "_batch")} <= set(takes)
    assert {(en, "entered_with"), (en, "entered_with_batch")} <= set(takes) and all(takes[o, n] for o, n in takes if o in (by, en))
    revised = {("Engine", f"{w}_revised{t}") for w in cs.QUERY_WHATS for t in ("", "_batch")}
    assert revised <= set(takes) and not any(takes[x] for x in revised)
    assert set(takes) == revised | {x for x in takes if x[0] in (by, en)}, "a method with `removed` that no call kind plays"
    for life in range(len(cs.LIVES)):
        seen = {cs.method_of(op) for op in cs.life_ops(oracle, life)} - {None}
        for (owner, name), optional in takes.items():
            assert (owner, name, True) in seen, (life, owner, name, "never played with removals")
            if optional:
                assert (owner, name, False) in seen, (life, owner, name, "never played without removals")
        # a query with removals is what the flag says: the Player passes removed= exactly then
        for op in cs.life_ops(oracle, life):
            m = cs.method_of(op)
            if m is not None and m[0] == en:
                queries = op.args[0] if op.kind.endswith("_batch") else [op.args[0]]
                assert m[2] == any(len(q[1]) for q in queries)


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
    # (of the kinds beside the Engine's only what the generator plants is refused: the duplicate append, the amends with a bad
    # removal or a duplicate row, and a query inside a batch of entered or bystander queries that is invalid as such)
    beside = ("append", "amend") + cs.ENTERED + cs.BYSTANDER
    jaccard = cs.refusals_in(ops, lambda: case.model(oracle, "jaccard"))
    assert not [k for k, s in jaccard if "_q" not in k and k not in beside]
    planted = {("append", cs.E_DUPLICATE), ("amend", cs.E_INVALID), ("amend", cs.E_DUPLICATE)}
    assert {(k, s) for k, s in jaccard if k in beside} <= planted | {(k, cs.E_INVALID) for k in beside if k.endswith("_batch")}
    assert planted <= jaccard
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
    # the three bystander families of every bystander kind, and the entered `with` forms with and without removals
    for kind in cs.BYSTANDER:
        assert {op.args[0] for op in ops if op.kind == kind} >= set(cs.BYSTANDER_FAMILIES), (life, kind)
    for kind in ("entered_with", "entered_with_batch"):
        assert {cs.method_of(op)[2] for op in ops if op.kind == kind} == {False, True}, (life, kind)
    # query batches on both sides of the split between the two similarity kernels
    out = cs.play_on_model(model(), ops)
    answerable = {sum(not isinstance(x, cs.Refused) for x in o) for op, o in zip(ops, out) if op.kind.endswith("_q_batch")}
    assert {cs.QB_DUAL_MIN - 1, cs.QB_DUAL_MIN} <= answerable, (life, sorted(answerable))


# ---- knncf_amend and the removed= forms ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrong", cs.WRONG_AFTER_AMEND)
def test_wrong_amend_differs_after_the_first_amend(oracle, wrong):
    """an amend that keeps every built list, one whose S comes from the update reports of the rows alone, one that keeps the
    removed rows, one that re-rates in place, and one after which the user that left is still there: each shows in an op AFTER the
    first amend of some sequence — in the answer or in the set of built lists — and in none before it.  (Half-star sums are exact
    in fp64, so a re-rating in place shows only where the row's place is read: in the order of a <= 4-rating user's fold and in
    the rank of tied deviations; seeds 0 .. 29 of every memo fit were searched, and it shows in most of them.)"""
    hits = []
    for case in cs.MEMO_CASES:
        ops = case.ops(oracle)
        first = min(j for j, op in enumerate(ops) if op.kind == "amend")
        d = _differs(oracle, case, wrong)
        assert all(j >= first for j in d), (case.name, d, first)
        hits += [(case.name, j) for j in d if j > first]
    assert hits, wrong


def test_revised_bystander_call_that_builds_differs_later(oracle):
    """read_only_builds restricted to the revised bystander forms: the call's own answer is right, a LATER op differs"""
    hits = []
    for case in cs.MEMO_CASES:
        ops = case.ops(oracle)
        d = _differs(oracle, case, "bystander_revised_builds")
        readers = [j for j, op in enumerate(ops) if op.kind in cs.BYSTANDER and op.args[0] == "revised"]
        assert readers and all(j >= readers[0] for j in d), (case.name, d, readers)
        hits += [(case.name, j) for j in d if any(r < j for r in readers) and j not in readers]
    assert hits


def _amends(ops, out):
    return [(op, x) for op, x in zip(ops, out) if op.kind == "amend"]


@pytest.mark.parametrize("case", cs.MEMO_CASES, ids=lambda c: c.name)
def test_memo_amends_hold_every_shape_and_refusal(oracle, case):
    """every memo sequence plays every amend shape and every refusal once, each with its status under both similarities; a refused
    amend and the trivial one leave model.appends as it was; the shapes are what their names say"""
    import numpy as np

    ops = case.ops(oracle)
    assert sorted(op.shape for op in ops if op.kind == "amend") == sorted(cs.AMEND_SHAPES + tuple(cs.AMEND_REFUSALS))
    assert {"not_a_row": cs.E_INVALID, "twice": cs.E_INVALID, "duplicate": cs.E_DUPLICATE, "both_wrong": cs.E_INVALID} == cs.AMEND_REFUSALS
    for sim in ("jaccard", "cosine"):
        model = case.model(oracle, sim)
        for op in ops:
            before, train, built = list(model.appends), model.train, set(model.built)
            users, items = set(model.known_users), set(model.known_items)
            x = model.call(op)
            if op.kind != "amend":
                continue
            ru, ri, u, i, r = op.args
            if op.shape in cs.AMEND_REFUSALS:
                assert isinstance(x, cs.Refused) and x.status == cs.AMEND_REFUSALS[op.shape], (case.name, sim, op)
                assert model.appends == before and model.train is train and model.built == built and model.definition == []
                if op.shape == "twice":
                    assert len(set(zip(ru.tolist(), ri.tolist()))) < len(ru)
                if op.shape == "both_wrong":  # without its bad removal the call is a duplicate, without its duplicate row E_INVALID
                    pairs = set(zip(train[0].tolist(), train[1].tolist()))
                    good = np.asarray([p in pairs for p in zip(ru.tolist(), ri.tolist())])
                    assert not good.all() and good.any()
                    again = case.model(oracle, sim)
                    again.fit(train)
                    assert again.amend(ru[good], ri[good], u, i, r).status == cs.E_DUPLICATE
                continue
            assert not isinstance(x, cs.Refused), (case.name, sim, op)
            if op.shape == "trivial":
                assert len(ru) == len(u) == 0 and x[:2] == (len(built), 0) and model.appends == before and model.train is train
                continue
            a = model.appends[-1]
            assert model.appends[:-1] == before and a["kind"] == "amend" and x[:2] == (a["carried"], a["dropped"])
            assert a["left_users"] == len(users - model.known_users) and a["left_items"] == len(items - model.known_items)
            if op.shape == "remover":
                assert len(u) == 0 and 1 <= len(ru) <= 2 and len(set(ru.tolist())) == 1
            if op.shape == "rerate":
                assert len(u) == 1 and (int(u[0]), int(i[0])) in set(zip(ru.tolist(), ri.tolist())) and 1 <= len(ru) <= 2
            if op.shape == "mixed":
                new = set(u.tolist()) - users
                assert len(set(u.tolist())) == 3 and len(new) == 1 and min(new) > cs.NEWCOMER and len(set(ru.tolist())) == 1
                assert set(ru.tolist()) < set(u.tolist()) and u.tolist() != sorted(u.tolist())  # a remover that re-rates; interleaved
            if op.shape == "leaver":
                assert a["left_users"] == 1 and a["plain"] and a["carried"] == 0 and len(u) == 0
            if op.shape == "lone_item":
                assert a["left_items"] == 1 and a["left_users"] == 0 and len(ru) == 1 and len(u) == 0


def test_memo_amends_carry_drop_and_shrink(oracle):
    """under Jaccard some amend of every memo sequence carries lists and drops lists, the amend of a lone item carries in some
    sequence while num_items shrinks; under the adjusted cosine every amend of a memo fit (users of <= 4 ratings) is plain"""
    lone = []
    for case in cs.MEMO_CASES:
        model, _ = _played(oracle, case, "jaccard")
        amends = [a for a in model.appends if a["kind"] == "amend"]
        assert any(a["carried"] >= 1 and a["dropped"] >= 1 for a in amends), (case.name, amends)
        assert any(a["plain"] and a["left_users"] == 1 for a in amends), (case.name, amends)
        lone += [a for a in amends if a["left_items"] == 1]
        cosine, _ = _played(oracle, case, "cosine")
        amends_c = [a for a in cosine.appends if a["kind"] == "amend"]
        assert len(amends_c) == len(amends) == len(cs.AMEND_SHAPES) - 1
        assert all(a["plain"] and a["carried"] == 0 for a in amends_c), (case.name, amends_c)
    assert len(lone) == len(cs.MEMO_CASES) and any(a["carried"] >= 1 and not a["plain"] for a in lone), lone


@pytest.mark.parametrize("life", range(len(cs.LIVES)))
def test_lives_amend_early_carry_and_shrink(oracle, life):
    """every life has an amend that shrinks the fit in the first half of its body, a trivial one and two refused ones; on the fits
    without short rows some amend under the adjusted cosine keeps lists and drops lists"""
    fit, k0, _ = cs.LIVES[life]
    ops = cs.life_ops(oracle, life)
    model = cs.HandleModel(oracle, fit.train, oracle.SIM_COSINE, k0)
    out = cs.play_on_model(model, ops)
    body = ops[2:]
    shapes = [op.shape for op in body if op.kind == "amend"]
    assert {"leaver", "trivial", "not_a_row", "duplicate"} < set(shapes) and len(shapes) == len(set(shapes)), (life, shapes)
    assert set(shapes) >= ({"rerate"} if len(set(fit.train[0].tolist())) > 1000 else {"rerate", "mixed", "lone_item"}), (life, shapes)
    shrinks = [j for j, op in enumerate(body) if op.kind == "amend" and op.shape in cs.AMEND_SHRINKS]
    assert shrinks[0] < len(body) // 2, (life, shrinks, len(body))
    for op, x in _amends(ops, out):
        want = cs.AMEND_REFUSALS.get(op.shape)
        assert (x.status == want) if want else not isinstance(x, cs.Refused), (life, op)
    amends = [a for a in model.appends if a["kind"] == "amend"]
    assert any(a["left_users"] == 1 for a in amends) and ("lone_item" not in shapes or any(a["left_items"] == 1 for a in amends))
    if model.short_fit:
        assert all(a["plain"] for a in amends), (life, amends)
    else:
        assert any(a["carried"] >= 1 and a["dropped"] >= 1 for a in amends), (life, amends)
