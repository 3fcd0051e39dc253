"""KNNCF_PRED_PERSONALIZED on the query families at the header and in the binding, without a GPU: the three family texts name
the predictor, the new block states the contract, the explanations still call it out of scope, and the Python wrappers pass the
predictor they are given (PRED_KNN by default)."""
import importlib
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _comment(title):
    """the comment block that starts with `title`, its line starts removed"""
    text = open(os.path.join(ROOT, "include", "knncf.h")).read()
    block = text[text.index(title):]
    return " ".join(re.sub(r"\n \*", " ", block[:block.index("*/")]).split())


@pytest.mark.parametrize("title", ["---- fold-in queries: one user that is NOT in the fitted training set",
                                   "---- Batched fold-in queries: many users outside the fit in one call",
                                   "---- Update queries: a user that may be IN the fit",
                                   "---- Revise queries: a user of the fit who REMOVED or RE-RATED items"])
def test_family_texts_name_the_predictor(title):
    assert "KNNCF_PRED_PERSONALIZED" in _comment(title)


def test_contract_block():
    block = _comment("---- Personalized queries: KNNCF_PRED_PERSONALIZED on the query families")
    for phrase in ("predictor(aug, weightedSumDeviation(aug, S))", "predict/Personalized.scala:61-72", ":508-524", "S(u, u)",
                   "no fused multiply-add", "exactly 1.0", "4 or fewer ratings are accepted", "handle's k plays no part",
                   "predict_ms", "prep_ms", "do not depend on C", "KNNCF_E_UNSUPPORTED"):
        assert phrase in block, phrase
    # the chunk rule's text says what this mode allocates beside the budget
    assert "transposed similarities" in _comment("---- Batched fold-in queries: many users outside the fit in one call")


def test_explanations_stay_out_of_scope():
    block = _comment("Explanations of query predictions: the terms behind")
    assert re.search(r"OUT OF SCOPE", block) and re.search(r"KNNCF_PRED_PERSONALIZED explanations", block)


def test_wrappers_take_a_predictor(pkg):
    kn = importlib.import_module(pkg.__name__ + ".knncf")
    for stem in ("for", "with", "revised"):
        for name in (f"predict_{stem}", f"recommend_{stem}", f"predict_{stem}_batch", f"recommend_{stem}_batch"):
            p = inspect.signature(getattr(kn.Engine, name)).parameters["predictor"]
            assert p.default == kn.PRED_KNN, name
        assert "predictor" not in inspect.signature(getattr(kn.Engine, f"neighbors_{stem}")).parameters

    class Lib:
        def __getattr__(self, name):
            def call(h, predictor, *rest):
                seen.append((name, predictor))
                return kn.OK
            return call

    seen = []
    e = kn.Engine.__new__(kn.Engine)
    e._lib, e._h, e.k, e.device = Lib(), None, 10, 0
    its, rts = [1, 2], [3.0, 4.0]
    e.predict_for(5, its, rts, [3], predictor=kn.PRED_PERSONALIZED)
    e.recommend_with(5, its, rts, 2, predictor=kn.PRED_PERSONALIZED)
    e.recommend_revised(5, [7], its, rts, 2, predictor=kn.PRED_PERSONALIZED)
    e.predict_revised_batch([(5, [7], its, rts)], [[3]], predictor=kn.PRED_PERSONALIZED)
    e.recommend_for_batch([(5, its, rts)], 2, predictor=kn.PRED_PERSONALIZED)
    e.predict_with(5, its, rts, [3])
    assert seen == [("knncf_query_predict", kn.PRED_PERSONALIZED), ("knncf_update_recommend", kn.PRED_PERSONALIZED),
                    ("knncf_revise_recommend", kn.PRED_PERSONALIZED), ("knncf_revise_predict_batch", kn.PRED_PERSONALIZED),
                    ("knncf_query_recommend_batch", kn.PRED_PERSONALIZED), ("knncf_update_predict", kn.PRED_KNN)]
