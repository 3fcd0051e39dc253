"""The width of the dense head is a cost decision, never a result: the neighbour lists and the MAE with the cost model's
head (head_items = 0) equal those with a forced head on either side of it (the re-rank is exact), and the model picks a
multiple of 64."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _fit(kn, d, head_items):
    e = kn.Engine(k=30, head_items=head_items)
    e.fit(d.train.users, d.train.items, d.train.ratings)
    mae = e.mae(kn.PRED_KNN, d.test.users, d.test.items, d.test.ratings)
    users = np.unique(d.train.users)
    ids, sims, counts = e.neighbors_batch(users)
    head = int(e.timings()["head_items"])
    e.close()
    assert counts.min() >= 0
    return mae, ids, np.ascontiguousarray(sims), head


def test_model_head_and_forced_heads_agree(kn, synth):
    d = synth.syn_scaled(3000, 2500, 400_000, seed=77)
    mae0, ids0, sims0, head0 = _fit(kn, d, 0)
    assert head0 > 0 and head0 % 64 == 0, head0
    n_items = len(np.unique(d.train.items))
    below, above = max(64, head0 - 128), min(head0 + 192, (n_items // 64) * 64)
    assert below != head0 or above != head0
    for forced in (below, above):
        mae, ids, sims, head = _fit(kn, d, forced)
        assert head == forced
        assert np.array_equal(ids, ids0), forced
        assert np.array_equal(sims.view(np.int64), sims0.view(np.int64)), forced
        assert mae == mae0, (forced, mae, mae0)
