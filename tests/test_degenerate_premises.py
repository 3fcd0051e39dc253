"""The premises of tests/test_gpu_degenerate_rows.py, from the oracle alone (no GPU): every generator of tests/degenerate.py,
at the exact parameters the GPU tests use, really produces the rows that leave the engine's ordinary path — and ordinary rows
beside them.  The engine's limits appear as LITERALS: a product change that moves one of them must fail here, visibly, instead
of silently turning the GPU tests into ordinary-row tests."""
import numpy as np
import pytest

from tests import degenerate as dg

SHORTLIST_CAP = 16_384   # api.cpp shortlist_cap(k, U) for k <= 4096 and U > 16 384: more candidates overflow the shortlist
STORE_COLUMNS = 65_536   # engine.h select_gcap(k) x 8 for k <= 512: 8192 provisional groups of 8 columns
HIST_LO = -0.125         # select.hip HIST_LO: a k-th largest value below it puts the final threshold in bin 0
HIST_HI = HIST_LO + 1.0  # values at or above it clamp into the top bin
K = dg.K


@pytest.fixture(scope="module")
def model(oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = oracle.Model(*dg.case(name).train)
        return made[name]

    return get


def _rows(model, name, users, k):
    """the oracle's neighbour similarities of `users`, [len(users), k], descending"""
    t = model(name).knn_table(k, users=users)
    assert t.rows == len(users) and t.width == k
    return t.sims.copy()  # (t.sims is a view of the table's memory, freed with t)


@pytest.mark.parametrize("name,floor", [("cold40", SHORTLIST_CAP), ("cold160", SHORTLIST_CAP), ("cold_wide", STORE_COLUMNS)])
def test_cold_rows_tie_at_zero_beyond_the_limits(model, oracle, name, floor):
    c = dg.case(name)
    U = c.num_users
    assert U - 1 > floor
    cold = c.groups["cold"]
    assert len(cold) <= 200  # (what one build may send through the per-row exact path)
    sims = _rows(model, name, cold, U - 1)
    zeros = (sims == 0.0).sum(axis=1)
    assert zeros.min() > floor and zeros.min() > U - 100
    assert (sims[:, K - 1] == 0.0).all() and (sims[:, K] == 0.0).all()
    # the same from the per-pair closure, for one row
    m, u = model(name), int(cold[0])
    others = np.unique(c.train[0])
    others = others[others != u][:: max(1, U // 2000)]
    assert sum(m.fresh_similarity(oracle.SIM_COSINE, u, int(v)) == 0.0 for v in others) >= len(others) - 100
    # and no common item at all with a background user: the Jaccard coefficient is 0 as well
    assert all(m.fresh_similarity(oracle.SIM_JACCARD, u, int(v)) == 0.0 for v in dg.ordinary_sample(name)[:50])


@pytest.mark.parametrize("name", ["cold40", "clones"])
def test_constant_rows_are_all_zero(model, name):
    """zero deviations, zero norm: a constant user's cosine row is 0.0 in EVERY column — in the 20 480-user case that is a
    shortlist overflow like a cold row's, which the GPU test counts among its fallback rows"""
    c = dg.case(name)
    U = c.num_users
    const = c.groups["constant"]
    assert len(const) == 50
    sims = _rows(model, name, const, U - 1)
    assert (sims == 0.0).all()
    assert (U - 1 > SHORTLIST_CAP) == (name == "cold40")
    # they rate background items: members of other users' rater lists, with test rows of their own
    assert np.isin(const, c.test[0]).all()
    if name == "clones":  # ... and of other users' neighbour lists where a list reaches down to 0.0
        t = model(name).knn_table(1000, users=c.groups["background"])
        assert np.isin(t.ids, const).any()


@pytest.mark.parametrize("k", [300, 1000])
def test_clone_rows_are_cut_inside_a_tie(model, k):
    c = dg.case("clones")
    clones = c.groups["clones"]
    assert len(clones) == 4 * 700
    sims = _rows(model, "clones", clones, k + 1)
    assert (sims[:, k - 1] == sims[:, k]).all()  # rank k and rank k + 1 hold the same fp64 value
    # the tie that rank k cuts is hundreds of users wide (k = 300: inside the row's own prototype group, whose norms — folded
    # in an order that depends on the raw user id — differ by an ulp, so its 699 values of about 1.0 form two or three large
    # ties; k = 1000: inside another prototype's group)
    wide = _rows(model, "clones", clones, 1500)
    assert ((wide == wide[:, k - 1:k]).sum(axis=1) >= 100).all()
    # the 699 other copies of the row's prototype: about 1.0, above the histogram's range; everybody else far below
    assert (np.abs(wide[:, :699] - 1.0) < 1e-12).all() and wide[:, :699].min() >= HIST_HI and wide[:, 699].max() < 0.5
    # copies are scattered over the raw id range (dense indices are HashSet ranks of the raw ids)
    for g in range(4):
        ids = c.groups[f"clones{g}"]
        assert ids.min() < c.num_users // 20 and ids.max() > c.num_users - c.num_users // 20


@pytest.mark.parametrize("name", ["camps12k", "camps20k"])
def test_camp_a_rows_end_below_the_histogram(model, name):
    c = dg.case(name)
    U = c.num_users
    camp_a = c.groups["camp_a"]
    assert len(camp_a) == 100 < K
    sims = _rows(model, name, camp_a, K)
    assert sims[:, K - 1].max() < HIST_LO
    assert sims[:, len(camp_a) - 2].min() > 0.0  # the camp itself on top
    # "everything qualifies" fits the shortlist at 12 000 users and overflows it at 20 480
    assert (U - 1 > SHORTLIST_CAP) == (name == "camps20k")
    assert U - 1 <= STORE_COLUMNS


@pytest.mark.parametrize("name", list(dg.CASES))
def test_ordinary_rows_stay_ordinary(model, name):
    users = dg.ordinary_sample(name)
    assert len(users) >= 12
    sims = _rows(model, name, users, K)
    assert sims[:, K - 1].min() > 0.0
    if name == "clones":  # k = 1000 too: both mirrored pairs of prototypes on the positive side
        assert (_rows(model, name, users, 1000)[:, 999] >= 0.0).all()


def test_generators_are_deterministic_and_well_formed():
    a, b = dg.CASES["clones"](), dg.CASES["clones"]()
    for x, y in zip(a.train + a.test, b.train + b.test):
        assert np.array_equal(x, y)
    for name in dg.CASES:
        c = dg.case(name)
        for cols in (c.train, c.test):
            assert cols[0].dtype == np.int32 and cols[1].dtype == np.int32 and cols[2].dtype == np.float64
            assert set(np.unique(cols[2]).tolist()) <= {1.0, 2.0, 3.0, 4.0, 5.0}
        assert np.bincount(np.unique(c.train[0], return_inverse=True)[1]).min() >= 5
        planted = [g for g in c.groups if g not in ("background", "camp_b")]
        for g in planted:  # every planted user has a test row on an item somebody rated: its neighbourhood gets built
            rows = np.isin(c.test[0], c.groups[g]) & np.isin(c.test[1], c.train[1])
            assert np.isin(c.groups[g], c.test[0][rows]).all(), (name, g)
