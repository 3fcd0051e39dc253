"""The fused set-up kernels of the fit (prep.hip k_user_setup: a user's segment sorted by item and by tuple hash, folded and
normalised on chip) against the oracle bit for bit, on the planted users of tests/fused_setup_cases.py: one per row length on
either side of every padded size of the sort network, of its lane / register / LDS strides and of the three size classes.

Compared through the calls of tests/test_gpu_setup_edges.py: the WHOLE arrays of knncf_shard_view_get — user means and norms,
normalized deviations and preprocessed ratings in canonical order — the kNN predictions of the test rows and the planted
users' neighbour lists.  The same users then take every other path — the global sorts, the unfused chain (one rating off the
dyadic grid; two shard handles), a re-fit of one handle — and the two failures that the kernels report through the status
word.  tests/test_fused_setup_premises.py proves the sets' premises on the CPU."""
import numpy as np
import pytest

from tests import fused_setup_cases as fc
from tests import setup_edges as se
from tests.test_gpu_k_classes import _trace
from tests.test_gpu_setup_edges import (K, _Ref, _check_knn, _check_shard_predictions, _check_view, _fit, _hooks, _prep_line,
                                        _same_bits, _shards, _view, kn)  # noqa: F401  (kn: the module-scoped fixture)

pytestmark = pytest.mark.gpu


class _CaseRef(_Ref):
    """_Ref over a case that is not one of setup_edges.CASES"""

    def __init__(self, oracle, c):
        self.oracle = oracle
        self.case = c
        self.model = m = oracle.Model(*c.train)
        self.order = m.user_iteration_order()
        self.avg = np.array([m.users_avg(int(u)) for u in self.order])
        self.norm = np.array([m.user_weight(int(u)) for u in self.order])
        canon = se.canonical(c.train, self.order)
        self.dev = m.normalized_deviations()[canon]
        self.pre = m.preprocessed()[canon]
        self.ptr = np.concatenate([[0], np.cumsum(np.bincount(se.rank_of(self.order, c.train[0]), minlength=len(self.order)))])
        self.lengths = se.lengths_of(c.train)
        self._knn = None


@pytest.fixture(scope="module")
def refs(oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _CaseRef(oracle, getattr(fc, name)())
        return made[name]

    return get


def _lists(c, **kw):
    return _prep_line(mid=c.facts["mid"], long=c.facts["long"], **kw)


def test_planted_lengths_on_the_fused_path(kn, pkg, refs, monkeypatch, capfd):
    ref = refs("planted")
    _hooks(monkeypatch)
    e, prep, _ = _fit(kn, ref.case, capfd)
    assert prep == _lists(ref.case, uf=0)
    _check_view(pkg, e, ref)
    _check_knn(kn, e, ref)
    e.close()


def test_global_sorts_give_the_same_arrays(kn, pkg, refs, monkeypatch, capfd):
    """KNNCF_DEBUG_GLOBAL_HASH_ORDER: the radix sorts and the unfused fold chain; equal to the oracle and to the fused path"""
    ref = refs("planted")
    _hooks(monkeypatch, global_order=True)
    g, prep, _ = _fit(kn, ref.case, capfd)
    assert prep == _prep_line(order="global", uf=0)
    vg = _check_view(pkg, g, ref)
    _check_knn(kn, g, ref)
    _hooks(monkeypatch)
    f, prep, _ = _fit(kn, ref.case, capfd)
    assert prep == _lists(ref.case, uf=0)
    vf = _view(pkg, f)
    for key in ("user_avg", "user_norm", "dev", "pre"):
        _same_bits(vf[key], vg[key], key)
    g.close()
    f.close()


def test_one_non_dyadic_rating_takes_the_unfused_chain(kn, pkg, refs, monkeypatch, capfd):
    ref = refs("non_dyadic")
    _hooks(monkeypatch)
    e, prep, _ = _fit(kn, ref.case, capfd)
    assert prep == _lists(ref.case, uf=1)
    _check_view(pkg, e, ref)
    _check_knn(kn, e, ref)
    e.close()


def test_mean_of_one_with_a_rating_below_fails(kn, monkeypatch, capfd):
    """scale() == 0 inside the fused kernel still reaches the host as KNNCF_E_NONFINITE; the handle fits the clean set after"""
    c = fc.planted()
    _hooks(monkeypatch)
    e = kn.Engine(k=K)
    capfd.readouterr()
    with pytest.raises(kn.KnncfError) as ex:
        e.fit(*fc.with_mean_one_user(c))
    assert ex.value.status == kn.E_NONFINITE
    prep, = [ln for ln in _trace(capfd) if ln.startswith("prep ")]
    assert prep == _lists(c, uf=0)
    e.close()


@pytest.mark.parametrize("length", fc.DUPLICATE_LENGTHS)
def test_duplicate_pair_fails(kn, pkg, refs, monkeypatch, capfd, length):
    """one (user, item) pair twice in a one-wave segment and in a 512-thread one, on the fused path: KNNCF_E_DUPLICATE, and the
    handle fits the clean set afterwards"""
    ref = refs("planted")
    c = ref.case
    user = {v: k for k, v in c.facts["lengths"].items()}[length]
    _hooks(monkeypatch)
    e = kn.Engine(k=K)
    capfd.readouterr()
    with pytest.raises(kn.KnncfError) as ex:
        e.fit(*se.with_duplicate(c, user))
    assert ex.value.status == kn.E_DUPLICATE
    prep, = [ln for ln in _trace(capfd) if ln.startswith("prep ")]
    assert prep == _lists(c, uf=0)
    e.fit(*c.train)
    _check_view(pkg, e, ref)
    e.close()


def test_two_shards_stay_on_the_unfused_chain(kn, pkg, refs, monkeypatch, capfd):
    ref = refs("planted")
    _hooks(monkeypatch)
    engines, tr, te, preps = _shards(kn, pkg, ref, 2, capfd)
    assert preps == [_lists(ref.case, uf=1)] * 2
    _check_shard_predictions(kn, ref, engines, tr, te)
    for e in engines:
        e.close()


def test_refit_with_a_smaller_set(kn, pkg, refs, monkeypatch, capfd):
    """one handle, the planted set and then a smaller one: no LDS, cursor or list state of the first fit shows in the second"""
    big, small = refs("planted"), refs("smaller")
    _hooks(monkeypatch)
    e, prep, _ = _fit(kn, big.case, capfd)
    assert prep == _lists(big.case, uf=0)
    _check_view(pkg, e, big)
    capfd.readouterr()
    e.fit(*small.case.train)
    prep, = [ln for ln in _trace(capfd) if ln.startswith("prep ")]
    assert prep == _lists(small.case, uf=0)
    _check_view(pkg, e, small)
    _check_knn(kn, e, small)
    e.close()
