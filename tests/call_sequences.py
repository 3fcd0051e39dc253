"""Random call sequences on one handle and the stateful model they are checked against (helper of
test_call_sequence_premises.py, test_gpu_call_sequences.py and scripts/fuzz_sequences.py).  Pure CPU: nothing here loads the
engine; play() drives whatever Engine it is handed.

HandleModel is ONE oracle.Model plus ONE Pipeline for the kNN memo plus k, and one method per call kind that returns what the
handle must answer and advances the pipeline as include/knncf.h says the call leaves the handle.  A pair with a <= 4-rating
user is summed in the order of the first closure that evaluated it, so every later answer depends on the order in
which the earlier calls built their neighbourhoods: the model plays that history, the sequences are drawn where it shows.

A call kind is an Engine method with "_device" taken off; the thirty query methods ({neighbors, predict, recommend, explain,
recommend_explain}_{for, with, revised}[_batch]) are the ten kinds *_q / *_q_batch, the family being an argument; the five
statistic getters are the kind `statistics`.  The classes beside Engine that wrap one give the kinds `append` and `amend`
(Appends), entered / entered_batch / entered_with / entered_with_batch (EnteredQueries; a query of the last two with removals
is played with removed=, knncf_revise_entered*) and bystander_{neighbors, predict}[_batch] (BystanderQueries, the family an
argument: "for", "with", or "revised" for the *_with methods with removed=).  kind_of() maps a method name, method_of() an op to
the method and keyword it is played through, NOT_MODELLED names the methods left out.

HandleModel.built is the set of raw ids whose neighbourhood the handle has built since the last drop, kept by the rules the
header states per call; the GPU tests compare it with the build numbers of the parsed checkpoint after every op."""
import hashlib
import re
from dataclasses import dataclass, field

import numpy as np

from tests import amend_cases as am
from tests import append_cases as ac
from tests import bystander_cases as bc
from tests import entered_cases as ec
from tests import explain_model
from tests import personalized_explain_model as pm
from tests import personalized_query_cases as pc
from tests import query_explain_cases as qc
from tests import revise_cases as rc
from tests import revise_entered_cases as rec
from tests import update_entered_cases as uc
from tests.test_oracle_semantics import _cols, _no_zero_scale, _random_case

OK, E_INVALID, E_NONFINITE, E_DUPLICATE, E_STATE, E_UNSUPPORTED = 0, -1, -2, -3, -6, -7
APPEND_MAX_CHANGERS = 128                       # KNNCF_APPEND_MAX_CHANGERS
PRED_BASELINE, PRED_KNN, PRED_PERSONALIZED = 3, 5, 6
SUM_ORDER, BY_WEIGHT = explain_model.SUM_ORDER, explain_model.BY_WEIGHT
MAE_TOL = 1e-9
ABSENT_USERS = (2_000_000_011, 2_000_000_029)   # ids no fit holds
ABSENT_ITEM = 2_000_000_017
NEW_USER = 3_000_000                            # fold-in users: NEW_USER + j, in no fit (small: the oracle's tables span the ids)
NEW_ITEM = 5_003                                # unknown to every fit, given by some queries
NEWCOMER = 3_020_000                            # appended newcomers: NEWCOMER + j, a range no query id uses
APPEND_ITEM = 5_100                             # items that an append brings into the fit: APPEND_ITEM + j (NEW_ITEM itself must
                                                # stay unknown to every fit: the queries rely on it)
QB_DUAL_MIN = 32                                # answerable queries from which a batch takes the dual similarity kernel
FAMILIES = ("for", "with", "revised")
QUERY_WHATS = ("neighbors", "predict", "recommend", "explain", "recommend_explain")

# what the handle keeps: these advance the memo; the drops replace it; everything else only reads
ENTERED = ("entered", "entered_batch", "entered_with", "entered_with_batch")  # build every missing list, then only read
MUTATING = ("neighbors", "neighbors_batch", "predict", "predict_batch", "mae", "recommend", "recommend_batch", "knn_similarity",
            "knn_similarity_batch", "explain", "explain_batch") + ENTERED
DROPS = ("set_k", "reset_neighbors", "mae_sweep", "fit")
REFITS = ("append", "amend")  # replace the fit as `fit` does, and keep some lists
BYSTANDER = ("bystander_neighbors", "bystander_neighbors_batch", "bystander_predict", "bystander_predict_batch")
BYSTANDER_FAMILIES = ("for", "with", "revised")  # "revised": the *_with methods with removed=
APPEND_SHAPES = ("changer", "newcomer", "both")
AMEND_SHAPES = ("remover", "rerate", "mixed", "leaver", "lone_item", "trivial")  # accepted amends
AMEND_REFUSALS = {"not_a_row": E_INVALID, "twice": E_INVALID, "duplicate": E_DUPLICATE, "both_wrong": E_INVALID}
AMEND_SHRINKS = ("leaver", "lone_item")
CHECKPOINT = ("neighbors_save", "neighbors_load")
STATISTICS = ("global_avg", "user_avg", "item_avg", "item_avg_dev", "item_avg_dev_rdd")
NOT_MODELLED = {
    "close": "ends the handle",
    "timings": "counters, no answer of the fit", "reset_timings": "counters, no answer of the fit",
    "shard_view": "shard handles are out of scope (queries and explanations are refused on them)",
    "shard_commit": "shard handles are out of scope (queries and explanations are refused on them)",
}
DEVICE_FORMS = ("fit", "similarity_batch", "explain_batch", "mae", "mae_sweep")  # kinds with an Engine.<kind>_device


def kind_of(method, owner="Engine"):
    """the call kind of a public method of Engine or of a class beside it that wraps one, None for one of NOT_MODELLED"""
    if owner == "BystanderQueries":
        m = re.fullmatch(r"(neighbors|predict)_(for|with)(_batch)?", method)
        return f"bystander_{m.group(1)}{m.group(3) or ''}" if m else method
    if owner != "Engine":
        return method  # (Appends.append, EnteredQueries.entered*: the kind is the method; anything else is no kind of KINDS)
    if method in NOT_MODELLED:
        return None
    name = method[:-len("_device")] if method.endswith("_device") else method
    if name in STATISTICS:
        return "statistics"
    m = re.fullmatch(r"(recommend_explain|neighbors|predict|recommend|explain)_(for|with|revised)(_batch)?", name)
    if m:
        return f"{m.group(1)}_q{m.group(3) or ''}"
    return name


def is_read_only(kind):
    return kind not in MUTATING and kind not in DROPS and kind not in REFITS and kind != "neighbors_load"


# ---- ops ---------------------------------------------------------------------------------------------------------------------
def _plain(x):
    if isinstance(x, np.ndarray):
        return x.tolist() if x.size <= 256 else f"<{x.size} values from {x.flat[0]}>"
    if isinstance(x, (tuple, list)):
        return type(x)(_plain(y) for y in x)
    if isinstance(x, np.generic):
        return x.item()
    return x


@dataclass
class Fit:
    """a named train set (LIVES, or the case's own fit as "same"), so that an op's repr stays one line"""
    name: str
    train: tuple

    def __repr__(self):
        return f"Fit({self.name!r})"


@dataclass
class Op:
    kind: str
    args: tuple
    form: str = "host"  # "host" or "device", where the kind has both
    shape: str = field(default="", compare=False)  # the generator's name for what it drew (the shape of an amend), for the premises

    def __repr__(self):
        return f"Op({self.kind!r}, {_plain(self.args)!r}, {self.form!r})"


@dataclass
class Refused:
    status: int


@dataclass
class Approx:
    """a value compared within MAE_TOL (the mae scalars; the predictions behind them are compared in bits)"""
    value: object


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64).tolist()


def same(got, want):
    """ids ==, float bit views ==, Approx within MAE_TOL, containers element by element"""
    if isinstance(want, Approx):
        g = got.value if isinstance(got, Approx) else got
        return bool(np.all(np.abs(np.asarray(g, dtype=np.float64) - np.asarray(want.value, dtype=np.float64)) <= MAE_TOL))
    if isinstance(want, Refused):
        return isinstance(got, Refused) and got.status == want.status
    if isinstance(got, (Refused, Approx)):
        return False
    if isinstance(want, (tuple, list)):
        return isinstance(got, (tuple, list)) and len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    if want is None or got is None:
        return want is None and got is None
    g, w = np.asarray(got), np.asarray(want)
    if g.shape != w.shape:
        return False
    if w.dtype.kind == "f" or g.dtype.kind == "f":
        return bits(g) == bits(w)
    return g.tolist() == w.tolist()


def unpad(out, cap, with_predictions=True):
    """the padded explain outputs (raters [m, cap], sims, devs, counts, sums [m, 2][, predictions]) as one tuple per row, cut
    to the row's min(count, cap) terms"""
    raters, sims, devs, counts, sums = out[:5]
    rows = []
    for j in range(len(counts)):
        t = min(int(counts[j]), cap)
        row = (np.asarray(raters).reshape(len(counts), -1)[j, :t], np.asarray(sims).reshape(len(counts), -1)[j, :t],
               np.asarray(devs).reshape(len(counts), -1)[j, :t], int(counts[j]), np.asarray(sums).reshape(-1, 2)[j])
        rows.append(row + ((float(out[5][j]),) if with_predictions else ()))
    return rows


# ---- the model ---------------------------------------------------------------------------------------------------------------
class HandleModel:
    """wrong: "" for the reference, or one of WRONG_MODELS — a deliberately wrong engine of the premises test"""

    def __init__(self, oracle, train, sim, k, wrong=""):
        self.oracle, self.sim, self.k, self.wrong = oracle, sim, int(k), wrong
        self.saved = None
        self.appends, self.entered_missing = [], []  # what every accepted append carried; |M| of every entered call that could build
        self.fit(train)

    # ---- plumbing ----
    def call(self, op):
        """the op's answer.  Afterwards self.definition is None, or — for the kinds that are DEFINED by older calls (append, entered*) —
        the list of ops through those older calls that leaves a handle in the same state: what a replaying handle plays instead"""
        if self.wrong == "stateless":
            self._closures()  # (the summation history is gone; which lists exist is not a matter of order and stays)
        self.definition = None
        out = getattr(self, op.kind)(*op.args)
        if op.kind in MUTATING and op.kind not in ENTERED:  # (an entered call logs the neighbors_batch it is defined by)
            self.log.append(op)
        return out

    def _closures(self):
        """fresh closures: one pipeline, and the term model that shares its memo"""
        self.p = self.m.pipeline(self.sim, self.k)
        self.tm = explain_model.TermModel(self.oracle, self.m, self.sim, self.k, pipeline=self.p)

    def _drop(self):
        """fresh closures and no list built"""
        self._closures()
        self.log = []
        self.built = set()

    def _builds(self, users):
        """the known users of `users` have their neighbourhood built from here on"""
        self.built |= {int(u) for u in np.asarray(users).reshape(-1).tolist() if int(u) in self.known_users}

    def _sim_name(self):
        return ac.COS if self.sim == self.oracle.SIM_COSINE else ac.JAC

    def replica(self):
        """the model of a second handle that loaded this one's checkpoint: a new pipeline onto which the mutating calls so far
        are replayed (Pipeline has no clone)"""
        r = HandleModel(self.oracle, self.train, self.sim, self.k, self.wrong)
        for op in self.log:
            r.call(op)
        r.saved = None if self.saved is None else list(self.saved)
        return r

    def _known(self, u):
        return int(u) in self.known_users

    def _in_order(self, keys, one):
        """[one(j) for every position j of keys], evaluated in the given order — by the wrong model "sorted_batches" in the
        order of the sorted keys"""
        order = np.argsort(keys, kind="stable") if self.wrong == "sorted_batches" else range(len(keys))
        out = {int(j): one(int(j)) for j in order}
        return [out[j] for j in range(len(keys))]

    # ---- knncf_fit: a new Model, fresh closures; a checkpoint of another fit no longer loads ----
    def fit(self, train):
        train = train.train if isinstance(train, Fit) else train
        self.train = (np.ascontiguousarray(train[0], np.int32), np.ascontiguousarray(train[1], np.int32),
                      np.ascontiguousarray(train[2], np.float64))
        self._refit(self.oracle.Model(*self.train), caches=True)

    def _refit(self, m, caches):
        """everything that follows the fit, from self.train and its Model m.  caches: the statistics and the Personalized answers
        move to the new fit too (they do not under the wrong model "append_keeps_fit_caches")"""
        self.m = m
        users, counts = np.unique(self.train[0], return_counts=True)
        self.known_users, self.known_items = set(users.tolist()), set(np.unique(self.train[1]).tolist())
        self.short_fit = bool(counts.min() <= 4)
        assert all(self.m.users_avg(int(u)) >= 0 for u in users), "the model has no clause for fitted users with a negative mean"
        if caches:
            self.mc, self.items_c = m, self.known_items  # the fit behind the statistics getters and the Personalized predictor
            self._ptm = None
        self.train_key = hashlib.sha1(b"".join(a.tobytes() for a in self.train)).hexdigest()
        self.saved = None
        self._drop()

    # ---- knncf_set_k: "change k (== getSimilarity(train, k, ...) with a new k); drops the memo" ----
    def set_k(self, k):
        self.k = int(k)
        self.saved = None
        self._drop()

    # ---- knncf_reset_neighbors: "drop the getNeighbors/getSimilarity memo (== constructing fresh closures)" ----
    def reset_neighbors(self):
        if self.wrong != "keeps_after_reset":
            self._drop()

    # ---- knncf_mae_sweep: every k from fresh closures; "On return the neighbour memo is dropped, as knncf_reset_neighbors
    # drops it, and the handle's k is unchanged" ----
    def mae_sweep(self, ks, users, items, ratings):
        maes, preds = [], []
        for k in ks:
            m, per = self.m.pipeline(self.sim, int(k)).mae(users, items, ratings, True)
            maes.append(m)
            preds.append(per)
        if self.wrong != "keeps_after_sweep":
            self._drop()
        return Approx(np.asarray(maes)), np.asarray(preds)

    # ---- knncf_neighbors_save: read-only; knncf_neighbors_load: "afterwards getNeighbors / getSimilarity / predictions use the
    # loaded lists" — the state at the save, i.e. fresh closures onto which the mutating calls up to the save are replayed ----
    def neighbors_save(self):
        self.saved = list(self.log)

    def neighbors_load(self):
        assert self.saved is not None, "the generator loads only what was saved under this fit and k"
        log = self.saved
        self._drop()
        for op in log:
            getattr(self, op.kind)(*op.args)
        self.log = list(log)

    # ---- knncf_neighbors: getNeighbors(train, k, sim)(u), memoised ----
    def neighbors(self, u):
        self._builds([u])
        return self.p.neighbors(int(u))

    # ---- knncf_neighbors_batch: "numbers every user it is asked about", in the given order, repeated users included ----
    def neighbors_batch(self, users):
        users = np.asarray(users)
        self._builds(users)
        return self._in_order(users, lambda j: self.p.neighbors(int(users[j])))

    # ---- knncf_predict / knncf_predict_batch / knncf_mae: KNNCF_PRED_KNN evaluates the rows in order on the handle's closures;
    # KNNCF_PRED_PERSONALIZED: "The kNN state (neighbour lists, their build numbers) is not touched", "Cosine needs > 4 ratings
    # per user" else KNNCF_E_UNSUPPORTED; the baseline has no closure ----
    def _predictions(self, predictor, users, items, ratings=None):
        users, items = np.asarray(users, np.int32), np.asarray(items, np.int32)
        ratings = np.zeros(len(users)) if ratings is None else np.asarray(ratings, np.float64)
        if predictor == PRED_KNN:
            self._builds_rows(users, items)
            return self.p.mae(users, items, ratings, True)
        if predictor == PRED_BASELINE:
            return self.mc.mae(self.oracle.KIND_BASELINE, users, items, ratings, True)
        assert predictor == PRED_PERSONALIZED
        if self._personalized_refused():
            return None
        return self.mc.pipeline(self.sim, -1).mae(users, items, ratings, True)

    def _builds_rows(self, users, items):
        """the rows of a kNN prediction or explanation where the reference's lazy closure is evaluated (explain_model.TermModel.row):
        the user is known and the item has raters"""
        self._builds([u for u, i in zip(np.asarray(users).tolist(), np.asarray(items).tolist()) if int(i) in self.known_items])

    def _personalized_refused(self):
        return self.short_fit and self.sim == self.oracle.SIM_COSINE

    def predict(self, predictor, u, i):
        got = self._predictions(predictor, [u], [i])
        return Refused(E_UNSUPPORTED) if got is None else float(got[1][0])

    def predict_batch(self, predictor, users, items):
        got = self._predictions(predictor, users, items)
        return Refused(E_UNSUPPORTED) if got is None else got[1]

    def mae(self, predictor, users, items, ratings):
        got = self._predictions(predictor, users, items, ratings)
        return Refused(E_UNSUPPORTED) if got is None else (Approx(got[0]), got[1])

    # ---- knncf_recommend / knncf_recommend_batch: "as if knncf_recommend had been called for users[0], users[1], ... in this
    # order"; KNNCF_PRED_KNN builds "only where the reference evaluates it: the user is in train and its mean is not negative";
    # "the other predictors leave the neighbour table alone" ----
    def recommend(self, predictor, u, n):
        if predictor == PRED_KNN:
            self._builds([u])  # (a known user; fit() has asserted that no mean is negative)
            return self.p.recommend(int(u), int(n))
        if predictor == PRED_BASELINE:
            return self.mc.recommend(self.oracle.KIND_BASELINE, int(u), int(n))
        if self._personalized_refused():
            return Refused(E_UNSUPPORTED)
        return self.mc.pipeline(self.sim, -1).recommend(int(u), int(n))

    def recommend_batch(self, predictor, users, n):
        if predictor == PRED_PERSONALIZED and self._personalized_refused():
            return Refused(E_UNSUPPORTED)
        users = np.asarray(users)
        return self._in_order(users, lambda j: self.recommend(predictor, users[j], n))

    # ---- knncf_knn_similarity / knncf_knn_similarity_batch: "leaves what knncf_neighbors_batch over us' leaves", us' having
    # an absent id wherever us[j] or vs[j] is absent from train: nothing is built for such a pair, its answer is +0.0 ----
    def knn_similarity(self, u, v):
        if not (self._known(u) and self._known(v)):
            return 0.0
        self._builds([u])
        return self.p.knn_similarity(int(u), int(v))

    def knn_similarity_batch(self, us, vs):
        us, vs = np.asarray(us), np.asarray(vs)
        return np.asarray(self._in_order(us, lambda j: self.knn_similarity(us[j], vs[j])))

    # ---- knncf_explain / knncf_explain_batch: "Missing neighbourhoods are built as predict_batch(PRED_KNN, users, items) builds
    # them": TermModel asks the shared pipeline in row order, only where the reference's lazy closure would ----
    def explain(self, u, i, cap, order):
        return self.explain_batch([u], [i], cap, order)[0]

    def explain_batch(self, users, items, cap, order):
        self._builds_rows(users, items)
        return unpad(qc.expected(self.tm.rows(users, items), cap, order), cap)

    # ---- read-only from here on: answers from fresh closures, the pipeline is untouched ----
    def _reads(self, u, revised_bystander=False):
        """the wrong models whose read-only calls build: a fitted user's neighbourhood is evaluated on the handle's closures
        (every read-only call, or the revised bystander forms alone)"""
        if (self.wrong == "read_only_builds" or (revised_bystander and self.wrong == "bystander_revised_builds")) and self._known(u):
            self._builds([u])
            self.p.neighbors(int(u))

    # knncf_similarity / knncf_similarity_batch: "Every pair is answered on a closure of its OWN", us[j] the first argument
    def similarity(self, u, v):
        return self.m.fresh_similarity(self.sim, int(u), int(v))

    def similarity_batch(self, us, vs):
        out = np.asarray([self.similarity(u, v) for u, v in zip(us, vs)])
        for u in us:
            self._reads(u)
        return out

    # the fit's statistics: (global_avg, user_avg(u), item_avg_dev(i)[, item_avg(i), item_avg_dev_rdd(i) for an item of the fit])
    def statistics(self, u, i):
        m = self.mc
        ua = m.users_avg(int(u))
        dev = m.items_avg_dev(int(i))
        out = (m.average(), m.average() if ua is None else ua, 0.0 if dev is None else dev)
        if int(i) in self.known_items:  # (what the player asks for: the items of the fit as it stands)
            out += tuple(0.0 if x is None else x for x in (m.items_avg(int(i)), m.items_avg_dev_spark(int(i))))
        return out

    # knncf_explain_personalized*: "KNNCF_E_UNSUPPORTED exactly where the fitted KNNCF_PRED_PERSONALIZED refuses"; read-only
    def explain_personalized(self, u, i, cap, order):
        out = self.explain_personalized_batch([u], [i], cap, order)
        return out if isinstance(out, Refused) else out[0]

    def explain_personalized_batch(self, users, items, cap, order):
        if self._personalized_refused():
            return Refused(E_UNSUPPORTED)
        if self._ptm is None:
            self._ptm = pm.PersonalTermModel(self.oracle, self.mc, self.sim)
        out = unpad(qc.expected(self._ptm.rows(users, items), cap, order), cap)
        for u in users:
            self._reads(u)
        return out

    # knncf_query_* / knncf_update_* / knncf_revise_*: "every result equals, bit for bit, the reference's on aug with fresh
    # closures whose first evaluation is `user`'s"; "Read-only on the handle".  A query is (user, removed, items, ratings).
    def _query_status(self, fam, query):
        q, removed, items, ratings = query
        mine = self.train[1][self.train[0] == q]
        if fam == "for" and (self._known(q) or len(items) == 0):
            return E_INVALID
        if len(removed) and not set(_plain(removed)) <= set(mine.tolist()):
            return E_INVALID  # "a removed item that the user did not rate in train"
        aug = rc.aug_of(self.train, q, removed, items, ratings)
        rows = aug[2][aug[0] == q]
        if len(rows) == 0:
            return E_INVALID
        if rows.sum() / len(rows) < 0:
            return E_UNSUPPORTED  # "a negative mean of the combined rows"
        return OK

    def _query(self, what, fam, predictor, query, *params):
        """one query's answer (Refused for a per-query refusal); fitted-form refusals of Personalized do not apply: "Train users
        with 4 or fewer ratings are accepted\""""
        q, removed, items, ratings = query
        q, removed = int(q), np.asarray(removed, np.int32)
        st = self._query_status(fam, (q, removed, items, ratings))
        if st != OK:
            return Refused(st)
        aug = rc.aug_of(self.train, q, removed, items, ratings)
        try:
            m = self.oracle.Model(*aug)
        except self.oracle.OracleError as ex:  # "KNNCF_E_NONFINITE for a non-finite deviation": scale() == 0 on the user's rows in aug
            if ex.status not in (E_NONFINITE, E_DUPLICATE):  # (a duplicate: only a wrong model's fit can hold the row already)
                raise
            return Refused(ex.status)
        if predictor == PRED_KNN:
            p = m.pipeline(self.sim, self.k)
            near = p.neighbors(q)  # first evaluation: the query user's
            tm = explain_model.TermModel(self.oracle, m, self.sim, self.k, pipeline=p)
        else:
            tm = pm.PersonalTermModel(self.oracle, m, self.sim)
        explained = lambda its, cap, order, preds: unpad(qc.expected([tm.row(q, int(i)) for i in its], cap, order), cap, preds)
        if what == "neighbors":
            out = near
        elif what == "predict":
            out = np.asarray([p.predict(q, int(i)) for i in params[0]]) if predictor == PRED_KNN else \
                np.asarray(pc.oracle_answers(self.oracle, aug, q, self.sim, params[0], [])[0])
        elif what in ("recommend", "recommend_explain"):
            out = p.recommend(q, params[0]) if predictor == PRED_KNN else pc.oracle_answers(self.oracle, aug, q, self.sim, [], [params[0]])[1][0]
            if what == "recommend_explain":
                out = (out[0], out[1], explained(out[0], params[1], params[2], False))
        else:
            out = explained(params[0], params[1], params[2], True)
        self._reads(q)
        return out

    def _query_batch(self, what, fam, predictor, queries, *params):
        per_query = what in ("predict", "explain")  # the requested items come one list per query
        return [self._query(what, fam, predictor, query, *((params[0][b],) + params[1:] if per_query else params))
                for b, query in enumerate(queries)]

    # ---- knncf_append: "every later call on the handle answers bit for bit as a handle on which knncf_fit(aug) was called"; "The
    # handle is left in the state that knncf_fit(aug) followed by knncf_neighbors_batch over K in ascending raw id leaves";
    # "knncf_append is the call without removals" ----
    def append(self, users, items, ratings):
        assert len(users), "the generator appends at least one row"
        none = np.empty(0, np.int32)
        return self._amend("append", none, none, users, items, ratings)

    # ---- knncf_amend: "aug is built in two steps: train in file order without the removed rows; then the n rows in the given
    # order.  Everything else is knncf_append's contract, read on this aug"; "Precedence: the argument checks, then the removal
    # checks, then the duplicate, then the non-finite deviation"; "n_removed == 0 && n == 0 is KNNCF_OK and touches nothing" ----
    def amend(self, removed_users, removed_items, users, items, ratings):
        return self._amend("amend", removed_users, removed_items, users, items, ratings)

    def _wrong_aug(self, case):
        """aug under the wrong models that build it otherwise (None: the reference's)"""
        gone = list(zip(case.removed_users.tolist(), case.removed_items.tolist()))
        rows = list(zip(case.users.tolist(), case.items.tolist()))
        tu, ti, tr = (a.copy() for a in case.train)
        pairs = list(zip(tu.tolist(), ti.tolist()))
        if self.wrong == "amend_keeps_removed_rows":  # aug = train ++ rows: only what is rated again goes
            keep = np.asarray([not (p in gone and p in rows) for p in pairs], dtype=bool)
            add = np.ones(len(rows), dtype=bool)
        elif self.wrong == "amend_rerates_in_place":  # a re-rated row keeps its file position
            keep = np.asarray([not (p in gone and p not in rows) for p in pairs], dtype=bool)
            add = np.asarray([p not in gone for p in rows], dtype=bool)
            for p, r in zip(rows, case.ratings.tolist()):
                if p in gone:
                    tr[pairs.index(p)] = r
        elif self.wrong == "amend_leaver_stays":  # the rows of a user that would leave stay
            left = set(tu.tolist()) - set(case.aug[0].tolist())
            keep = np.asarray([not (p in gone and p[0] not in left) for p in pairs], dtype=bool)
            add = np.ones(len(rows), dtype=bool)
        else:
            return None
        return (np.concatenate([tu[keep], case.users[add]]).astype(np.int32), np.concatenate([ti[keep], case.items[add]]).astype(np.int32),
                np.concatenate([tr[keep], case.ratings[add]]).astype(np.float64))

    def _amend(self, kind, removed_users, removed_items, users, items, ratings):
        ru, ri = np.asarray(removed_users, np.int32), np.asarray(removed_items, np.int32)
        users, items = np.asarray(users, np.int32), np.asarray(items, np.int32)
        ratings = np.asarray(ratings, np.float64)
        self.definition = []
        if len(ru) == 0 and len(users) == 0:
            return (len(self.built), 0, np.empty(0, np.int32))  # the trivial call: a saved checkpoint still loads
        train_pairs = set(zip(self.train[0].tolist(), self.train[1].tolist()))
        gone = list(zip(ru.tolist(), ri.tolist()))
        if not set(gone) <= train_pairs or len(set(gone)) < len(gone) or (len(gone) == len(train_pairs) and len(users) == 0):
            return Refused(E_INVALID)  # "is not a train row", "listed twice", "an aug without any row"
        pairs = list(zip(users.tolist(), items.tolist()))
        if len(set(pairs)) < len(pairs) or set(pairs) & (train_pairs - set(gone)):
            return Refused(E_DUPLICATE)  # "the handle answers exactly as before the call"
        case = am.Amend(kind, self.train, ru, ri, users, items, ratings, self.k)
        aug = (self._wrong_aug(case) if kind == "amend" else None) or case.aug
        try:
            m = self.oracle.Model(*aug)
        except self.oracle.OracleError as ex:
            if ex.status not in (E_NONFINITE, E_DUPLICATE):  # (a duplicate: only a wrong model's fit can hold the row already)
                raise
            return Refused(ex.status)
        sim, built = self._sim_name(), sorted(self.built)
        assert len(self.known_users) >= 5 and len(self.known_items) >= 5, "the model has no clause for fits that the update queries refuse"
        negative = any(aug[2][aug[0] == c].sum() < 0 for c, _, _, _ in case.changers)  # "a negative mean of its combined rows"
        plain = (am.is_plain(case, sim) or (sim == ac.COS and self.short_fit) or negative or len(case.changers) > APPEND_MAX_CHANGERS)
        left = sorted(self.known_users - set(aug[0].tolist()))
        # the new fit's set order, a user that left "where its id would stand in that order"
        order = bc.trie_sorted(self.oracle, set(m.user_iteration_order().tolist()) | set(left)) if left else m.user_iteration_order().tolist()
        if plain or not built:
            keep, gone_lists = [], [v for v in order if v in self.built]
        else:
            if self.wrong == "amend_reports_as_update" and kind == "amend":  # the removals ignored: what the rows alone report
                new = np.asarray([p not in train_pairs for p in pairs], dtype=bool)  # (a re-rating would be a duplicate there)
                find = lambda: ac.stale(self.oracle, ac.Append(kind, self.train, users[new], items[new], ratings[new], self.k), sim)
            else:
                find = lambda: am.stale(self.oracle, case, sim)
            stale = _memo(("stale", self.wrong == "amend_reports_as_update" and kind == "amend", self.train_key, ru.tobytes(), ri.tobytes(),
                           users.tobytes(), items.tobytes(), ratings.tobytes(), self.k, sim), find)
            keep, gone_lists = sorted(self.built - stale), [v for v in order if v in self.built and v in stale]
            if self.wrong == f"{kind}_keeps_every_list":
                keep, gone_lists = built, []
        if self.wrong == "amend_leaver_stays" and kind == "amend":  # ... and its list with them
            keep = sorted(set(keep) | (set(self.built) & (self.known_users - set(case.aug[0].tolist()))))
            gone_lists = [v for v in gone_lists if v not in keep]
        left_items = len(self.known_items - set(aug[1].tolist()))
        self.appends.append({"kind": kind, "plain": bool(plain), "built": len(built), "carried": len(keep), "dropped": len(gone_lists),
                             "left_users": len(left), "left_items": left_items})
        self.train = aug
        self._refit(m, caches=not (self.wrong == "append_keeps_fit_caches" and kind == "append"))
        self.definition = [Op("fit", (Fit("aug", aug),))]
        if keep:
            op = Op("neighbors_batch", (np.asarray(keep, np.int32),))
            self.neighbors_batch(*op.args)
            self.log, self.definition = [op], self.definition + [op]
        return (len(keep), len(gone_lists), np.asarray(gone_lists, np.int32))

    # ---- knncf_query_entered* / knncf_update_entered*: "Let M be the train users whose neighbourhood the handle has not built, in
    # ascending raw id.  When the call passes its handle-level checks, n_queries > 0 and M is not empty, it first builds them in ONE
    # batch and LEAVES THE HANDLE IN THE STATE THAT knncf_neighbors_batch OVER M LEAVES IT IN ... whether or not any query is
    # answerable"; refused on "a KNNCF_SIM_COSINE handle whose train set has a user with 4 or fewer ratings" ----
    def _entered(self, fam, queries):
        self.definition = []
        if self._personalized_refused():  # (the same condition: the adjusted cosine on a fit with a <= 4-rating user)
            return Refused(E_UNSUPPORTED)
        missing = sorted(self.known_users - self.built)
        if len(queries):
            self.entered_missing.append(len(missing))
        if missing and len(queries) and self.wrong != "entered_builds_nothing":
            op = Op("neighbors_batch", (np.asarray(missing, np.int32),))
            self.neighbors_batch(*op.args)
            self.log.append(op)
            self.definition = [op]
        out = []
        for q, removed, items, ratings in queries:
            q, items, ratings = int(q), np.asarray(items, np.int32), np.asarray(ratings, np.float64)
            st = self._query_status(fam, (q, removed, items, ratings))
            if st != OK:
                out.append(Refused(st))
                continue
            removed = np.asarray(removed, np.int32)
            key = ("entered", fam, self.train_key, q, removed.tobytes(), items.tobytes(), ratings.tobytes(), self.k, self._sim_name())
            if len(removed):  # knncf_revise_entered*: the removals in front of the rows
                want = lambda *a: rec.expected_for(self.oracle, self.train, q, removed, *a[3:])
            else:
                want = ec.expected_for if fam == "for" else uc.expected_for
            try:
                out.append(_memo(key, lambda: want(self.oracle, self.train, q, items, ratings, self.k, self._sim_name())))
            except self.oracle.OracleError as ex:
                if ex.status not in (E_NONFINITE, E_DUPLICATE):  # (a duplicate: only a wrong model's fit can hold the row already)
                    raise
                out.append(Refused(ex.status))
        return out

    def entered(self, query):
        out = self._entered("for", [query])
        return out if isinstance(out, Refused) else out[0]

    def entered_batch(self, queries):
        return self._entered("for", queries)

    def entered_with(self, query):
        out = self._entered("with", [query])
        return out if isinstance(out, Refused) else out[0]

    def entered_with_batch(self, queries):
        return self._entered("with", queries)

    # ---- knncf_query_bystander_* / knncf_update_bystander_*: "Every row is answered on closures of its own over aug whose first
    # evaluation is the row's"; "a query with a row whose others[r] == users[b] gets KNNCF_E_INVALID"; read-only ----
    def _bystander(self, what, fam, query, others, pred_items=None):
        q, removed, items, ratings = query
        q = int(q)
        st = self._query_status(fam, (q, removed, items, ratings))
        if st == OK and q in set(np.asarray(others).tolist()):
            st = E_INVALID
        if st != OK:
            return Refused(st)
        try:
            m = self.oracle.Model(*rc.aug_of(self.train, q, removed, items, ratings))
        except self.oracle.OracleError as ex:
            if ex.status not in (E_NONFINITE, E_DUPLICATE):  # (a duplicate: only a wrong model's fit can hold the row already)
                raise
            return Refused(ex.status)
        self._reads(q, revised_bystander=fam == "revised")
        if what == "neighbors":
            return [m.pipeline(self.sim, self.k).neighbors(int(v)) for v in others]
        return np.asarray([m.pipeline(self.sim, self.k).predict(int(v), int(i)) for v, i in zip(others, pred_items)], np.float64)

    def bystander_neighbors(self, fam, query, others):
        return self._bystander("neighbors", fam, query, others)

    def bystander_predict(self, fam, query, others, pred_items):
        return self._bystander("predict", fam, query, others, pred_items)

    def bystander_neighbors_batch(self, fam, queries, others):
        return [self._bystander("neighbors", fam, query, others[b]) for b, query in enumerate(queries)]

    def bystander_predict_batch(self, fam, queries, others, pred_items):
        return [self._bystander("predict", fam, query, others[b], pred_items[b]) for b, query in enumerate(queries)]


_memo_cache = {}


def _memo(key, make):
    """make() once per key: the sequences are played many times (premises, both similarities, every GPU test) and the oracle's
    side of an append or an entered query on a large fit costs seconds"""
    if key not in _memo_cache:
        _memo_cache[key] = make()
    return _memo_cache[key]


def _bind_queries():
    for what in QUERY_WHATS:
        setattr(HandleModel, f"{what}_q", lambda self, *a, _w=what: self._query(_w, *a))
        setattr(HandleModel, f"{what}_q_batch", lambda self, *a, _w=what: self._query_batch(_w, *a))


_bind_queries()
KINDS = tuple(sorted(n for n in vars(HandleModel) if not n.startswith("_") and n not in ("call", "replica")))
# the last three differ where the new fit of an append or the lists that an entered call builds matter: under Jaccard on the memo
# fits (under the adjusted cosine every append there is a plain refit and every entered call refused), in an answer or in `built`
WRONG_MODELS = ("stateless", "keeps_after_reset", "keeps_after_sweep", "read_only_builds", "sorted_batches",
                "append_keeps_every_list", "append_keeps_fit_caches", "entered_builds_nothing",
                "amend_keeps_every_list", "amend_reports_as_update", "amend_keeps_removed_rows", "amend_rerates_in_place",
                "amend_leaver_stays", "bystander_revised_builds")
WRONG_AFTER_APPEND = WRONG_MODELS[5:8]
WRONG_AFTER_AMEND = WRONG_MODELS[8:13]  # each wrong in one clause of "Amend": they show after the first amend, under Jaccard


def method_of(op):
    """(owner class, method, whether removals are passed) of the binding call through which the Player plays an op of a kind
    whose method takes `removed`; None for the other kinds"""
    tail = "_batch" if op.kind.endswith("_batch") else ""
    if "_q" in op.kind:
        return ("Engine", f"{op.kind[:op.kind.index('_q')]}_{op.args[0]}{tail}", op.args[0] == "revised")
    if op.kind in BYSTANDER:
        what, fam = op.kind[len("bystander_"):].replace("_batch", ""), op.args[0]
        return ("BystanderQueries", f"{what}_{'with' if fam == 'revised' else fam}{tail}", fam == "revised")
    if op.kind in ("entered_with", "entered_with_batch"):
        queries = op.args[0] if tail else [op.args[0]]
        return ("EnteredQueries", op.kind, any(len(q[1]) for q in queries))
    return None


# ---- playing an op on an Engine ------------------------------------------------------------------------------------------------
class Player:
    """plays ops on one Engine and returns each answer in the model's shape.  kn: the knncf module; tmp: a directory for the
    checkpoint of neighbors_save / neighbors_load."""

    def __init__(self, kn, engine, tmp, name="e", train=None):
        self.kn, self.e, self.path = kn, engine, f"{tmp}/{name}_sequence.nbr"
        self._stands(np.empty(0, np.int32) if train is None else train[0], np.empty(0, np.int32) if train is None else train[1])

    def _stands(self, users, items):
        """the player's own record of the (user, item) rows as they stand in the handle's fit: what the statistics getters of an item
        are asked for follows it, also when an amend takes an item out"""
        self.row_users, self.row_items = np.asarray(users, np.int32).copy(), np.asarray(items, np.int32).copy()
        self.known_items = set(np.unique(self.row_items).tolist())

    def _dev(self, a, dtype):
        import torch

        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(torch.device("cuda", self.e.device))

    def play(self, op):
        try:
            return getattr(self, op.kind)(op.form == "device", *op.args)
        except self.kn.KnncfError as ex:
            return Refused(ex.status)

    @staticmethod
    def _lists(ids, vals, counts):
        return [(ids[b, :counts[b]], vals[b, :counts[b]]) for b in range(len(counts))]

    def fit(self, dev, train):
        t = train.train if isinstance(train, Fit) else train
        if dev:
            self.e.fit_device(self._dev(t[0], np.int32), self._dev(t[1], np.int32), self._dev(t[2], np.float64))
        else:
            self.e.fit(*t)
        self._stands(t[0], t[1])

    def set_k(self, dev, k):
        self.e.set_k(int(k))

    def reset_neighbors(self, dev):
        self.e.reset_neighbors()

    def neighbors_save(self, dev):
        self.e.neighbors_save(self.path)

    def neighbors_load(self, dev):
        self.e.neighbors_load(self.path)

    def mae_sweep(self, dev, ks, users, items, ratings):
        if not dev:
            maes, preds = self.e.mae_sweep(ks, users, items, ratings, predictions=True)
            return Approx(maes), preds
        import torch

        out = torch.full((len(ks), len(users)), float("nan"), dtype=torch.float64, device=torch.device("cuda", self.e.device))
        sums, count = self.e.mae_sweep_device(ks, self._dev(users, np.int32), self._dev(items, np.int32), self._dev(ratings, np.float64), out)
        assert count == len(users)
        return Approx(sums / count), out.cpu().numpy()

    def neighbors(self, dev, u):
        return self.e.neighbors(int(u))

    def neighbors_batch(self, dev, users):
        return self._lists(*self.e.neighbors_batch(users))

    def predict(self, dev, predictor, u, i):
        return self.e.predict(predictor, int(u), int(i))

    def predict_batch(self, dev, predictor, users, items):
        return self.e.predict_batch(predictor, users, items)

    def mae(self, dev, predictor, users, items, ratings):
        """the host form has no prediction output: the predictions behind it are predict_batch's over the same rows, which
        builds nothing more"""
        if not dev:
            return Approx(self.e.mae(predictor, users, items, ratings)), self.e.predict_batch(predictor, users, items)
        import torch

        out = torch.full((len(users),), float("nan"), dtype=torch.float64, device=torch.device("cuda", self.e.device))
        s, c = self.e.mae_device(predictor, self._dev(users, np.int32), self._dev(items, np.int32), self._dev(ratings, np.float64), out)
        assert c == len(users)
        return Approx(s / c), out.cpu().numpy()

    def recommend(self, dev, predictor, u, n):
        return self.e.recommend(predictor, int(u), int(n))

    def recommend_batch(self, dev, predictor, users, n):
        return self._lists(*self.e.recommend_batch(predictor, np.asarray(users, np.int32), int(n)))

    def knn_similarity(self, dev, u, v):
        return self.e.knn_similarity(int(u), int(v))

    def knn_similarity_batch(self, dev, us, vs):
        return self.e.knn_similarity_batch(np.asarray(us, np.int32), np.asarray(vs, np.int32))

    def similarity(self, dev, u, v):
        return self.e.similarity(int(u), int(v))

    def similarity_batch(self, dev, us, vs):
        if not dev:
            return self.e.similarity_batch(np.asarray(us, np.int32), np.asarray(vs, np.int32))
        import torch

        out = torch.full((len(us),), float("nan"), dtype=torch.float64, device=torch.device("cuda", self.e.device))
        return self.e.similarity_batch_device(self._dev(us, np.int32), self._dev(vs, np.int32), out).cpu().numpy()

    def statistics(self, dev, u, i):
        e = self.e
        out = (e.global_avg(), e.user_avg(int(u)), e.item_avg_dev(int(i)))
        if int(i) in self.known_items:
            out += (e.item_avg(int(i)), e.item_avg_dev_rdd(int(i)))
        return out

    @staticmethod
    def _single(out, cap):
        raters, sims, devs, count, sums, pred = out
        return (raters, sims, devs, int(count), np.asarray(sums), float(pred))

    def explain(self, dev, u, i, cap, order):
        return self._single(self.e.explain(int(u), int(i), cap, order), cap)

    def explain_personalized(self, dev, u, i, cap, order):
        return self._single(self.e.explain_personalized(int(u), int(i), cap, order), cap)

    def explain_batch(self, dev, users, items, cap, order):
        if not dev:
            return unpad(self.e.explain_batch(users, items, cap, order), cap)
        import torch

        n, d = len(users), torch.device("cuda", self.e.device)
        raters = torch.full((n, cap), -1, dtype=torch.int32, device=d)
        sims, devs = (torch.full((n, cap), float("nan"), dtype=torch.float64, device=d) for _ in range(2))
        counts = torch.zeros(n, dtype=torch.int32, device=d)
        sums, preds = torch.zeros((n, 2), dtype=torch.float64, device=d), torch.zeros(n, dtype=torch.float64, device=d)
        terms = (raters, sims, devs) if cap > 0 else (None, None, None)
        self.e.explain_batch_device(self._dev(users, np.int32), self._dev(items, np.int32), cap, *terms, counts, sums, preds, order)
        return unpad([t.cpu().numpy() for t in (raters, sims, devs, counts, sums, preds)], cap)

    def explain_personalized_batch(self, dev, users, items, cap, order):
        return unpad(self.e.explain_personalized_batch(users, items, cap, order), cap)

    # the query families
    @staticmethod
    def _fam_args(fam, query):
        q, removed, items, ratings = query
        items, ratings = np.asarray(items, np.int32), np.asarray(ratings, np.float64)
        return (int(q), np.asarray(removed, np.int32), items, ratings) if fam == "revised" else (int(q), items, ratings)

    def _q(self, what, dev, fam, predictor, query, *params):
        args, kw = self._fam_args(fam, query), ({} if what == "neighbors" else {"predictor": predictor})
        out = getattr(self.e, f"{what}_{fam}")(*args, *params, **kw)
        if what == "explain":
            return unpad(out, params[1])
        if what == "recommend_explain":
            return (out[0], out[1], unpad(out[2:], params[1], False))
        return out

    def _qb(self, what, dev, fam, predictor, queries, *params):
        kw = {} if what == "neighbors" else {"predictor": predictor}
        if what in ("predict", "explain"):
            params = ([np.asarray(x, np.int32) for x in params[0]],) + params[1:]
        outs, st = getattr(self.e, f"{what}_{fam}_batch")([self._fam_args(fam, q) for q in queries], *params, **kw)
        rows = []
        for out, s in zip(outs, st.tolist()):
            if s != OK:
                rows.append(Refused(s))
            elif what == "explain":
                rows.append(unpad(out, params[1]))
            elif what == "recommend_explain":
                rows.append((out[0], out[1], unpad(out[2:], params[1], False)))
            else:
                rows.append(out)
        return rows


    # the classes beside Engine
    def append(self, dev, users, items, ratings):
        carried, dropped, ids = self.kn.Appends(self.e).append(users, items, ratings, return_dropped=True)
        self._stands(np.concatenate([self.row_users, users]), np.concatenate([self.row_items, items]))
        return (carried, dropped, ids)

    def amend(self, dev, removed_users, removed_items, users, items, ratings):
        carried, dropped, ids = self.kn.Appends(self.e).amend(removed_users, removed_items, users, items, ratings, return_dropped=True)
        key = lambda u, i: (np.asarray(u, np.int64) << 32) | (np.asarray(i, np.int64) & 0xFFFFFFFF)
        keep = ~np.isin(key(self.row_users, self.row_items), key(removed_users, removed_items))
        self._stands(np.concatenate([self.row_users[keep], np.asarray(users, np.int32)]),
                     np.concatenate([self.row_items[keep], np.asarray(items, np.int32)]))
        return (carried, dropped, ids)

    @staticmethod
    def _removed_kw(op_kind, arg, batch):
        """the removed= keyword of a *_with method: absent without removals (the update call), one sequence per query in a batch —
        an empty one for a query without removals"""
        queries = arg if batch else [arg]
        if not method_of(Op(op_kind, (arg,)))[2]:
            return {}
        return {"removed": [np.asarray(q[1], np.int32) for q in queries] if batch else np.asarray(arg[1], np.int32)}

    def _entered(self, fam, batch, arg):
        eq = self.kn.EnteredQueries(self.e)
        name = "entered" if fam == "for" else "entered_with"
        kw = self._removed_kw(name + ("_batch" if batch else ""), arg, batch) if fam == "with" else {}
        if not batch:
            return tuple(getattr(eq, name)(*self._fam_args(fam, arg), **kw))
        outs, st = getattr(eq, name + "_batch")([self._fam_args(fam, q) for q in arg], **kw)
        return [tuple(out) if s == OK else Refused(s) for out, s in zip(outs, st.tolist())]

    def entered(self, dev, query):
        return self._entered("for", False, query)

    def entered_batch(self, dev, queries):
        return self._entered("for", True, queries)

    def entered_with(self, dev, query):
        return self._entered("with", False, query)

    def entered_with_batch(self, dev, queries):
        return self._entered("with", True, queries)

    def _by(self, kind, fam, arg, batch):
        """(the BystanderQueries method, the query arguments, the removed= keyword) of a bystander op: the family "revised" is the
        *_with method with removed= (one sequence per query in a batch, an empty one for a query without removals)"""
        owner, name, with_removed = method_of(Op(kind, (fam, arg)))
        short = "with" if fam == "revised" else fam
        queries = arg if batch else [arg]
        kw = {}
        if with_removed:
            kw = {"removed": [np.asarray(q[1], np.int32) for q in queries] if batch else np.asarray(arg[1], np.int32)}
        args = [self._fam_args(short, q) for q in queries]
        return getattr(self.kn.BystanderQueries(self.e), name), args if batch else args[0], kw

    def bystander_neighbors(self, dev, fam, query, others):
        fn, args, kw = self._by("bystander_neighbors", fam, query, False)
        return fn(*args, np.asarray(others, np.int32), **kw)

    def bystander_predict(self, dev, fam, query, others, pred_items):
        fn, args, kw = self._by("bystander_predict", fam, query, False)
        return fn(*args, np.asarray(others, np.int32), np.asarray(pred_items, np.int32), **kw)

    def bystander_neighbors_batch(self, dev, fam, queries, others):
        fn, args, kw = self._by("bystander_neighbors_batch", fam, queries, True)
        outs, st = fn(args, [np.asarray(x, np.int32) for x in others], **kw)
        return [out if s == OK else Refused(s) for out, s in zip(outs, st.tolist())]

    def bystander_predict_batch(self, dev, fam, queries, others, pred_items):
        fn, args, kw = self._by("bystander_predict_batch", fam, queries, True)
        outs, st = fn(args, [np.asarray(x, np.int32) for x in others], [np.asarray(x, np.int32) for x in pred_items], **kw)
        return [out if s == OK else Refused(s) for out, s in zip(outs, st.tolist())]


def _bind_player():
    for what in QUERY_WHATS:
        setattr(Player, f"{what}_q", lambda self, *a, _w=what: self._q(_w, *a))
        setattr(Player, f"{what}_q_batch", lambda self, *a, _w=what: self._qb(_w, *a))


_bind_player()


# ---- the generator -----------------------------------------------------------------------------------------------------------
class _Draw:
    def __init__(self, rng, model, k_pool, batch_sizes, fits, life=False):
        self.rng, self.model, self.k_pool, self.batch_sizes, self.fits, self.life = rng, model, k_pool, batch_sizes, fits, life
        self.big_pairs = {"similarity_batch", "knn_similarity_batch"} if life else set()
        self.new_user, self.k = NEW_USER, model.k
        self.newcomer, self.append_item = NEWCOMER, APPEND_ITEM
        self.set_train(model.train)

    def set_train(self, train):
        self.train = train
        self.users, counts = np.unique(train[0], return_counts=True)
        self.items = np.unique(train[1])
        assert NEW_ITEM not in self.items and ABSENT_ITEM not in self.items and not np.isin(ABSENT_USERS, self.users).any()
        assert not ((self.users > NEW_USER) & (self.users < NEW_USER + 10_000)).any() and NEWCOMER > NEW_USER + 10_000
        self.count = dict(zip(self.users.tolist(), counts.tolist()))
        raters = np.unique(train[1], return_counts=True)[1]
        self.lone = self.items[raters == 1]    # items of one rater: kept for the amend that takes such an item out of the fit
        self.common = self.items[raters > 1]   # what the appends and the other amends draw their items from
        short = self.users[counts <= 4]
        self.short = short if len(short) else self.users
        self.hot = self._order_shows(train, short) if len(short) else self.users

    def _order_shows(self, train, short):
        """the co-raters of the <= 4-rating users whose list depends on who evaluated their pairs first: the users whose
        neighbours, asked after everybody else's, differ from fresh closures' (all co-raters where the fit is too large to ask)"""
        co = np.unique(train[0][np.isin(train[1], train[1][np.isin(train[0], short)])])
        if len(self.users) > 400:
            return co
        o = self.model.oracle
        sim = o.SIM_COSINE  # (where the order shows; the ops do not depend on the handle's similarity)
        m = o.Model(*train)
        hot, first = set(), set()
        for k in self.k_pool:
            fresh = {int(v): m.pipeline(sim, int(k)).neighbors(int(v)) for v in co}
            for u in short:  # u's neighbourhood first, then v's: the pair (u, v) is summed in u's order
                p = m.pipeline(sim, int(k))
                p.neighbors(int(u))
                moved = {int(v) for v in co if v != u and not same(p.neighbors(int(v)), fresh[int(v)])}
                if moved:
                    first.add(int(u))
                    hot |= moved
        if first:
            self.short = np.asarray(sorted(first), np.int32)
        return np.asarray(sorted(hot), np.int32) if hot else co

    def user(self):
        x = self.rng.random()
        if x < 0.08:
            return int(self.rng.choice(ABSENT_USERS))
        return int(self.rng.choice(self.short if x < 0.4 else self.hot if x < 0.85 else self.users))

    def fitted(self, min_rows=1):
        for _ in range(100):
            u = self.user()
            if self.count.get(u, 0) >= min_rows:
                return u
        return int(self.users[np.argmax([self.count[int(u)] for u in self.users])])

    def item(self):
        return ABSENT_ITEM if self.rng.random() < 0.06 else int(self.rng.choice(self.items))

    def users_n(self, n):
        return np.asarray([self.user() for _ in range(n)], np.int32)

    def rows(self, n):
        return (self.users_n(n), np.asarray([self.item() for _ in range(n)], np.int32), self.rng.integers(1, 6, n).astype(np.float64))

    def size(self):
        return int(self.rng.integers(30, 60)) if self.life else int(self.rng.integers(3, 10))

    def explain_args(self):
        return int(self.rng.choice([0, 1, 3, 64])), int(self.rng.choice([SUM_ORDER, BY_WEIGHT]))

    def query(self, fam, refusal=None):
        """(user, removed, items, ratings) of family fam; refusal: None, "negative_mean" or "removes_unrated\""""
        rng = self.rng
        none = np.empty(0, np.int32)
        if refusal == "negative_mean" or fam == "for" or (fam == "with" and rng.random() < 0.3):
            self.new_user += 1
            n = int(rng.integers(1, 7))
            items = rng.choice(self.items, min(n, len(self.items)), replace=False).astype(np.int32)
            if rng.random() < 0.3:
                items[-1] = NEW_ITEM
            ratings = rng.integers(1, 6, len(items)).astype(np.float64)
            if refusal == "negative_mean":
                ratings = -ratings
            return (self.new_user, none, items, ratings)
        q = self.fitted(2 if fam == "revised" else 1)
        mine = self.train[1][self.train[0] == q]
        free = np.setdiff1d(self.items, mine)
        if refusal == "removes_unrated":
            return (q, np.asarray([ABSENT_ITEM if len(free) == 0 or rng.random() < 0.5 else int(rng.choice(free))], np.int32), none, np.empty(0))
        n_new = int(rng.integers(0, 4))
        items = rng.choice(free, min(n_new, len(free)), replace=False).astype(np.int32)
        if rng.random() < 0.25:
            items = np.append(items, NEW_ITEM).astype(np.int32)
        removed = none
        if fam == "revised":
            removed = rng.choice(mine, int(rng.integers(1, min(3, len(mine)))), replace=False).astype(np.int32)
            if rng.random() < 0.5:  # re-rate the first removed item
                items = np.append(items, removed[0]).astype(np.int32)
        return (q, removed, items, rng.integers(1, 6, len(items)).astype(np.float64))

    def pred_items(self, query):
        own = self.train[1][self.train[0] == query[0]][:2]
        return np.concatenate([[self.item() for _ in range(4)], own, query[1][:1], query[2][:1], [ABSENT_ITEM]]).astype(np.int32)

    def append_rows(self, shape):
        """(users, items, ratings) of an append.  "changer": a fitted user adds 1-3 items it has not rated; "newcomer": a new user
        of 5-7 rows, sometimes with an item new to the fit; "both": the two interleaved; "duplicate": a changer's rows and a row
        of train again, which is refused; "newcomer_item": a newcomer that brings an item for sure.  Items come from those of more
        than one rater, so that an item of one rater stays one.  An accepted append (the oracle can scale aug) becomes the train
        set of the later ops."""
        rng, o = self.rng, self.model.oracle
        for _ in range(50):
            parts = []
            if shape in ("changer", "both", "duplicate"):
                c = self.fitted()
                free = np.setdiff1d(self.common, self.train[1][self.train[0] == c])
                n = min(int(rng.integers(1, 4)), len(free))
                if n == 0:
                    continue
                parts.append((c, rng.choice(free, n, replace=False).astype(np.int32), rng.integers(1, 6, n).astype(np.float64)))
            if shape in ("newcomer", "both", "newcomer_item"):
                self.newcomer += 1
                items = rng.choice(self.common, min(int(rng.integers(5, 8)), len(self.common)), replace=False).astype(np.int32)
                if rng.random() < 0.4 or shape == "newcomer_item":
                    self.append_item += 1
                    items[int(rng.integers(0, len(items)))] = self.append_item
                parts.append((self.newcomer, items, rng.integers(1, 6, len(items)).astype(np.float64)))
            u, i, r = ac.interleave(parts)
            rows = (np.asarray(u, np.int32), np.asarray(i, np.int32), np.asarray(r, np.float64))
            aug = tuple(np.concatenate([a, b]).astype(a.dtype) for a, b in zip(self.train, rows))
            try:
                o.Model(*aug)
            except o.OracleError:
                continue  # (a scale() == 0 input: drawn again)
            if shape == "duplicate":  # (the duplicate is all that is wrong with the rows)
                t, at = int(rng.integers(0, len(self.train[0]))), int(rng.integers(0, len(u) + 1))
                return tuple(np.insert(a, at, self.train[x][t] if x < 2 else 3.0).astype(a.dtype) for x, a in enumerate(rows))
            self.set_train(aug)
            return rows
        raise AssertionError(("no acceptable append", shape))

    def _own(self, c):
        at = self.train[0] == c
        return self.train[1][at], self.train[2][at]

    def _original(self, min_rows=1):
        """a fitted user of the first fit (no appended newcomer) of at least min_rows rows"""
        for _ in range(200):
            u = self.fitted(min_rows)
            if u < NEWCOMER and self.count.get(u, 0) >= min_rows:
                return u
        raise AssertionError(("no fitted user of so many rows", min_rows))

    def _removals_of(self, c, n):
        """n train items of c that other users rated too, in a random order"""
        mine = self._own(c)[0]
        mine = mine[np.isin(mine, self.common)]
        return self.rng.choice(mine, min(n, len(mine)), replace=False).astype(np.int32)

    def _other_value(self, v):
        return float(v - 2 if v >= 3 else v + 2)

    def amend_rows(self, shape):
        """(removed users, removed items, users, items, ratings) of an amend.
        "remover": a fitted user of more than 6 rows removes 1-2 of them; "rerate": a removal and a row on the same item (half of
        them with the same value), sometimes a second removal; "mixed": a remover that re-rates, a fitted user that only adds and a
        newcomer (sometimes with a new item), rows interleaved, removals shuffled; "leaver": a fitted user — a <= 4-rating one where
        the fit has some — removes all its rows; "lone_item": the only rating of an item goes, and the item with it; "trivial":
        nothing.  Refused and without a trace: "not_a_row" (an item the user did not rate; in every other draw the call's own
        newcomer), "twice" (a removal listed twice), "duplicate" (a row on an unremoved train row), "both_wrong" (a bad removal
        and a duplicate row: the removal checks come first).  An accepted draw — aug keeps 5 users and 5 items, no fitted user's
        mean is negative, the oracle can scale it — becomes the train set of the later ops."""
        rng, o = self.rng, self.model.oracle
        none, nof = np.empty(0, np.int32), np.empty(0, np.float64)
        if shape == "trivial":
            return (none, none, none, none, nof)
        self.amend_draws = getattr(self, "amend_draws", 0) + 1
        for _ in range(50):
            rm, parts = [], []  # [(user, item)], [(user, items, ratings)]
            if shape in ("remover", "twice"):
                c = self._original(7)
                rm = [(c, int(i)) for i in self._removals_of(c, int(rng.integers(1, 3)))]
                if shape == "twice":
                    rm.insert(int(rng.integers(0, len(rm) + 1)), rm[int(rng.integers(0, len(rm)))])
            elif shape in ("rerate", "duplicate", "both_wrong"):
                c = self._original(3)
                gone = self._removals_of(c, 1 + int(rng.random() < 0.5))
                if len(gone) == 0:
                    continue
                rm = [(c, int(i)) for i in gone]
                mine, vals = self._own(c)
                v = float(vals[mine == gone[0]][0])
                parts = [(c, gone[:1], np.asarray([v if rng.random() < 0.5 else self._other_value(v)]))]
                if shape != "rerate":  # a row on a train row of c that stays
                    stays = np.setdiff1d(mine, gone)
                    parts[0] = (c, np.append(gone[:1], rng.choice(stays)).astype(np.int32), np.append(parts[0][2], 3.0))
                if shape == "both_wrong":
                    free = np.setdiff1d(self.items, mine)
                    rm.append((c, int(rng.choice(free)) if len(free) else ABSENT_ITEM))
            elif shape == "not_a_row":
                if self.amend_draws % 2:
                    c = self.fitted()
                    free = np.setdiff1d(self.items, self._own(c)[0])
                    rm = [(c, int(rng.choice(free)) if len(free) and rng.random() < 0.7 else ABSENT_ITEM)]
                else:  # the removal names the call's own newcomer
                    self.newcomer += 1
                    items = rng.choice(self.common, min(5, len(self.common)), replace=False).astype(np.int32)
                    parts = [(self.newcomer, items, rng.integers(1, 6, len(items)).astype(np.float64))]
                    rm = [(self.newcomer, int(items[0]))]
            elif shape == "mixed":
                a = self._original(5)
                gone = self._removals_of(a, int(rng.integers(2, 4)))
                b = self._original()
                free = np.setdiff1d(self.common, self._own(b)[0])
                if len(gone) < 2 or b == a or len(free) == 0:
                    continue
                rm = [(a, int(i)) for i in gone]
                mine, vals = self._own(a)
                parts.append((a, gone[:1], np.asarray([self._other_value(float(vals[mine == gone[0]][0]))])))
                n = min(int(rng.integers(1, 4)), len(free))
                parts.append((b, rng.choice(free, n, replace=False).astype(np.int32), rng.integers(1, 6, n).astype(np.float64)))
                self.newcomer += 1
                items = rng.choice(self.common, min(int(rng.integers(5, 8)), len(self.common)), replace=False).astype(np.int32)
                if rng.random() < 0.4:
                    self.append_item += 1
                    items[int(rng.integers(0, len(items)))] = self.append_item
                parts.insert(1, (self.newcomer, items, rng.integers(1, 6, len(items)).astype(np.float64)))  # (between the two: its rows
                rm = [rm[j] for j in rng.permutation(len(rm))]                                              # interleave with theirs)
            elif shape == "leaver":
                few = [int(u) for u in self.users if self.count[int(u)] <= 4 and u < NEWCOMER]
                c = int(rng.choice(few)) if few else self._original()
                mine = self._own(c)[0]
                if np.isin(mine, self.lone).any():
                    continue
                rm = [(c, int(i)) for i in mine[rng.permutation(len(mine))]]
            elif shape == "lone_item":
                assert len(self.lone), "no item of one rater: the slot lies behind a newcomer append that brings one"
                i = int(rng.choice(self.lone))
                c = int(self.train[0][self.train[1] == i][0])
                assert self.count[c] > 1
                rm = [(c, i)]
            else:
                raise AssertionError(shape)
            if not rm:
                continue
            u, i, r = ac.interleave(parts) if parts else ([], [], [])
            call = (np.asarray([x[0] for x in rm], np.int32), np.asarray([x[1] for x in rm], np.int32),
                    np.asarray(u, np.int32), np.asarray(i, np.int32), np.asarray(r, np.float64))
            if shape in AMEND_REFUSALS:
                return call
            aug = am.Amend(shape, self.train, *call, self.k).aug
            if len(np.unique(aug[0])) < 5 or len(np.unique(aug[1])) < 5:
                continue
            try:
                m = o.Model(*aug)
            except o.OracleError:
                continue  # (a scale() == 0 input: drawn again)
            if any(m.users_avg(int(x)) < 0 for x in np.unique(aug[0])):
                continue
            self.set_train(aug)
            return call
        raise AssertionError(("no acceptable amend", shape))

    def bystander_rows(self, query, refused=False):
        """(others, pred_items) of a bystander query: fitted users (an absent id among them at times) other than the query's user
        — but for a refused query, which names its own user — and an item each"""
        n = int(self.rng.integers(2, 7))
        others = [u for u in self.users_n(n + 2).tolist() if u != query[0]][:n]
        if refused:
            others.insert(int(self.rng.integers(0, len(others) + 1)), int(query[0]))
        items = [self.item() if self.rng.random() < 0.7 else int(query[2][0]) if len(query[2]) else NEW_ITEM for _ in others]
        return np.asarray(others, np.int32), np.asarray(items, np.int32)

    def op(self, kind, variant=None):
        """one op of `kind`; variant: a predictor, a (family, predictor) pair or a refusal where the slot fixes one"""
        rng, d = self.rng, self
        form = "device" if kind in DEVICE_FORMS and rng.random() < 0.5 else "host"
        pred3 = lambda: variant if variant is not None else int(rng.choice([PRED_KNN, PRED_KNN, PRED_KNN, PRED_BASELINE, PRED_PERSONALIZED]))
        if kind == "fit":
            return Op(kind, (self.fits[int(rng.integers(0, len(self.fits)))],), form)
        if kind == "set_k":
            self.k = int(rng.choice([k for k in self.k_pool if k != self.k]))
            return Op(kind, (self.k,))
        if kind in ("reset_neighbors", "neighbors_save", "neighbors_load"):
            return Op(kind, ())
        if kind == "mae_sweep":
            ks = sorted(set(int(x) for x in rng.choice(self.k_pool + [1, 3], 3)))
            return Op(kind, (ks,) + d.rows(d.size()), form)
        if kind == "neighbors":
            return Op(kind, (d.user(),))
        if kind == "neighbors_batch":
            return Op(kind, (d.users_n(d.size()),))
        if kind == "predict":
            return Op(kind, (pred3(), d.user(), d.item()))
        if kind == "predict_batch":
            return Op(kind, (pred3(),) + d.rows(d.size())[:2])
        if kind == "mae":
            return Op(kind, (pred3(),) + d.rows(d.size()), form)
        if kind == "recommend":
            return Op(kind, (pred3(), d.user(), int(rng.integers(1, 6))))
        if kind == "recommend_batch":
            return Op(kind, (pred3(), d.users_n(d.size()), int(rng.integers(1, 6))))
        if kind in ("knn_similarity", "similarity"):
            return Op(kind, (d.user(), d.user()))
        if kind in ("knn_similarity_batch", "similarity_batch"):
            n = d.size()
            if kind in self.big_pairs:  # once per life: more pairs than a chunk of LIFE_WORKSPACE holds, through the host form
                self.big_pairs.discard(kind)
                n, form = LIFE_WORKSPACE // 2 // 16 + 100, "host"
                return Op(kind, (rng.choice(self.users, n).astype(np.int32), rng.choice(self.users, n).astype(np.int32)), form)
            return Op(kind, (d.users_n(n), d.users_n(n)), form)
        if kind == "statistics":
            return Op(kind, (d.user(), d.item()))
        if kind in ("explain", "explain_personalized"):
            return Op(kind, (d.user(), d.item()) + d.explain_args())
        if kind in ("explain_batch", "explain_personalized_batch"):
            if variant == "cap64":  # more rows than the host form's term scratch of LIFE_WORKSPACE holds at this cap
                return Op(kind, d.rows(150)[:2] + (64, int(rng.choice([SUM_ORDER, BY_WEIGHT]))), "host")
            return Op(kind, d.rows(d.size())[:2] + d.explain_args(), form)
        if kind == "append":
            return Op(kind, d.append_rows(variant or APPEND_SHAPES[int(rng.integers(0, 3))]))
        if kind == "amend":
            shape = variant or AMEND_SHAPES[int(rng.integers(0, 3))]
            return Op(kind, d.amend_rows(shape), shape=shape)
        if kind in ENTERED:
            fam = "with" if "with" in kind else "for"
            drawn = "revised" if variant == "removed" else fam  # entered_with*(..., removed=...): the queries of the revise family
            if not kind.endswith("_batch"):
                return Op(kind, (d.query(drawn),))
            queries = [d.query(drawn) for _ in range(int(rng.choice(self.batch_sizes)))]
            if drawn == "revised" and rng.random() < 0.5:  # a query without removals inside the revise call
                queries[-1] = d.query("with")
            if rng.random() < 0.5:  # a refused query inside the batch: a fitted user as a newcomer, an absent one without rows
                at = len(queries) // 2
                gone = queries[at][1]  # (with removals: "any removal for a user absent from train")
                queries[at] = (d.fitted(),) + queries[at][1:] if fam == "for" else (int(rng.choice(ABSENT_USERS)), gone, gone[:0], np.empty(0))
            return Op(kind, (queries,))
        if kind in BYSTANDER:
            fam = variant if variant is not None else BYSTANDER_FAMILIES[int(rng.integers(0, 3))]
            predict = "predict" in kind
            if not kind.endswith("_batch"):
                query = d.query(fam)
                rows = d.bystander_rows(query)
                return Op(kind, (fam, query) + (rows if predict else rows[:1]))
            queries = [d.query(fam) for _ in range(int(rng.choice(self.batch_sizes)))]
            if fam == "revised" and rng.random() < 0.5:  # a query without removals inside the revise call
                queries[-1] = d.query("with")
            refused = len(queries) // 2 if rng.random() < 0.5 else -1  # a query that names its own user among its rows
            rows = [d.bystander_rows(q, refused=b == refused) for b, q in enumerate(queries)]
            return Op(kind, (fam, queries, [x[0] for x in rows]) + (([x[1] for x in rows],) if predict else ()))
        what, batch = kind[:kind.index("_q")], kind.endswith("_batch")
        refusal = variant if isinstance(variant, str) else None
        fam, predictor = variant[:2] if isinstance(variant, tuple) else (FAMILIES[int(rng.integers(0, 3))], int(rng.choice([PRED_KNN, PRED_PERSONALIZED])))
        if isinstance(variant, tuple) and len(variant) == 3:  # variant[2] answerable queries and a refused one
            queries = [d.query(fam) for _ in range(variant[2])] + [d.query(fam, "negative_mean")]
            params = {"neighbors": (), "predict": ([d.pred_items(q) for q in queries],), "recommend": (3,),
                      "explain": ([d.pred_items(q) for q in queries], 3, BY_WEIGHT)}[what]
            return Op(kind, (fam, predictor, queries) + params)
        if refusal == "removes_unrated":
            fam = "revised"
        if what == "neighbors":
            predictor = PRED_KNN
        queries = [d.query(fam, refusal if b == 0 else None) for b in range(int(rng.choice(self.batch_sizes)) + (refusal is not None) if batch else 1)]
        if batch and refusal is None and rng.random() < 0.5:
            queries[len(queries) // 2] = d.query(fam, "negative_mean")  # a refused query inside a batch
        if what == "neighbors":
            params = ()
        elif what == "predict":
            params = ([d.pred_items(q) for q in queries],) if batch else (d.pred_items(queries[0]),)
        elif what == "recommend":
            params = (int(rng.integers(1, 6)),)
        elif what == "explain":
            params = (([d.pred_items(q) for q in queries],) if batch else (d.pred_items(queries[0]),)) + d.explain_args()
        else:
            params = (int(rng.integers(1, 6)),) + d.explain_args()
        return Op(kind, (fam, predictor, queries if batch else queries[0]) + params)


REFUSALS = ("negative_mean", "removes_unrated", "personalized_fitted")


def sequence(seed, model, n_ops, k_pool=(2, 6), fits=None, batch_sizes=(2, 3, 5), every_variant=False):
    # (n_ops None with every_variant: every slot and eight more)
    """a deterministic list of n_ops Ops for a handle in the state of `model` (its fit and k): every kind of KINDS at least once,
    each refusal once, the rest drawn with a preference for the calls that advance the memo; ids are drawn from the fit with a
    preference for <= 4-rating users and their co-raters, a few absent ids among them.  every_variant: every (family, predictor)
    of every query kind and every predictor of the fitted predictor kinds gets a slot of its own (the lives)."""
    rng = np.random.default_rng(seed)
    fits = fits if fits is not None else [Fit("same", model.train)]
    d = _Draw(rng, model, list(k_pool), list(batch_sizes), fits, life=every_variant)
    slots = [(kind, None) for kind in KINDS if kind not in CHECKPOINT]
    slots += [("predict_q", "negative_mean"), ("recommend_q_batch", "negative_mean"), ("explain_q", "removes_unrated"),
              ("neighbors_q_batch", "removes_unrated"), ("predict_batch", PRED_PERSONALIZED), ("recommend", PRED_PERSONALIZED),
              ("mae", PRED_KNN), ("predict_batch", PRED_KNN), ("recommend_batch", PRED_KNN)]
    # appends: the slot of the kind is a newcomer that brings an item of its own (which the "lone_item" amend later takes out again),
    # one is a fitted changer's, one is refused and leaves no trace, and in the memo sequences a fourth one interleaves a changer and
    # a newcomer (on the 2 100 users of a life the oracle's side of an append costs seconds)
    slots += [("append", "changer"), ("append", "duplicate")] + ([] if every_variant else [("append", "both")])
    slots[slots.index(("append", None))] = ("append", "newcomer_item")
    # amends: every shape and every refusal once in the memo sequences; the lives leave out the lone remover and two refusals, and
    # a life on more than 1 000 users (the oracle's side costs seconds per changer there) keeps one changer that carries, what
    # shrinks and what is refused
    slots.remove(("amend", None))
    if not every_variant:
        slots += [("amend", x) for x in AMEND_SHAPES + tuple(AMEND_REFUSALS)]
    elif len(d.users) > 1000:
        slots += [("amend", x) for x in ("rerate", "leaver", "trivial", "not_a_row", "duplicate")]
    else:
        slots += [("amend", x) for x in ("rerate", "mixed", "leaver", "lone_item", "trivial", "not_a_row", "duplicate")]
    # the entered_with forms once more with removals (knncf_revise_entered*)
    slots += [("entered_with", "removed"), ("entered_with_batch", "removed")]
    if every_variant:
        slots = [s for s in slots if s[0] not in BYSTANDER] + [(kind, fam) for kind in BYSTANDER for fam in BYSTANDER_FAMILIES]
        for what in QUERY_WHATS:
            for fam in FAMILIES:
                for predictor in (PRED_KNN,) if what == "neighbors" else (PRED_KNN, PRED_PERSONALIZED):
                    slots += [(f"{what}_q", (fam, predictor)), (f"{what}_q_batch", (fam, predictor))]
        slots += [(kind, predictor) for kind in ("predict", "mae", "recommend_batch") for predictor in (PRED_BASELINE, PRED_PERSONALIZED)]
        slots += [("predict_q_batch", ("with", PRED_KNN, QB_DUAL_MIN - 1)), ("recommend_q_batch", ("for", PRED_PERSONALIZED, QB_DUAL_MIN)),
                  ("explain_q_batch", ("revised", PRED_KNN, QB_DUAL_MIN)), ("neighbors_q_batch", ("for", PRED_KNN, QB_DUAL_MIN - 1)),
                  ("explain_batch", "cap64"), ("explain_personalized_batch", "cap64")]
        n_ops = len(slots) + 10 if n_ops is None else n_ops
    assert len(slots) + 2 <= n_ops, (len(slots), n_ops)
    extra = ["neighbors", "neighbors_batch", "predict_batch", "mae", "recommend", "recommend_batch", "knn_similarity",
             "knn_similarity_batch", "explain", "explain_batch", "neighbors", "knn_similarity"]
    while len(slots) + 2 < n_ops:
        slots.append((extra[int(rng.integers(0, len(extra)))], PRED_KNN if rng.random() < 0.8 else None))
    order = rng.permutation(len(slots))
    slots = [slots[j] for j in order]
    # the fit changes with an accepted append and with an accepted amend other than the trivial one
    accepted = lambda s: (s[0] == "append" and s[1] != "duplicate") or (s[0] == "amend" and s[1] in AMEND_SHAPES and s[1] != "trivial")

    def swap(a, b):
        slots[a], slots[b] = slots[b], slots[a]

    if every_variant:  # an accepted append in the first half, so that a full pass of kinds runs on the appended fit
        first = min(j for j, s in enumerate(slots) if accepted(s) and s[0] == "append")
        if first >= len(slots) // 2:
            swap(int(rng.integers(0, len(slots) // 2)), first)
    if ("amend", "lone_item") in slots:  # behind the newcomer whose item it removes
        brings, lone = slots.index(("append", "newcomer_item")), slots.index(("amend", "lone_item"))
        if lone < brings:
            swap(lone, brings)
            brings, lone = lone, brings
        if any(s[0] == "fit" for s in slots[brings:lone]):  # (a fit takes the newcomer and its item away again)
            swap(lone, brings + 1)
    if every_variant:  # ... and an amend that shrinks the fit there too: every kind runs on a fit smaller than the one before
        first = min(j for j, s in enumerate(slots) if s[0] == "amend" and s[1] in AMEND_SHRINKS)
        if first >= len(slots) // 2:
            free = [j for j in range(len(slots) // 2) if slots[j][0] not in REFITS + ("fit",)]
            swap(free[int(rng.integers(0, len(free)))], slots.index(("amend", "leaver")))
    # the checkpoint: a save, and its load before the next call after which it no longer loads (set_k, fit, an accepted append or
    # amend)
    at = int(rng.integers(1, max(2, len(slots) // 2)))
    ends = [j for j in range(at, len(slots)) if slots[j][0] in ("set_k", "fit") or accepted(slots[j])]
    end = ends[0] if ends else len(slots)
    load_at = int(rng.integers(at, end + 1))
    slots = slots[:at] + [("neighbors_save", None)] + slots[at:load_at] + [("neighbors_load", None)] + slots[load_at:]
    ops = []
    for kind, variant in slots:
        op = d.op(kind, variant)
        if kind == "fit":
            d.set_train(op.args[0].train)
        ops.append(op)
    return ops


def refusals_in(ops, model_factory):
    """the refusals a sequence meets, by playing it on a model: {(kind, status)}"""
    model = model_factory()
    seen = set()
    for op in ops:
        out = model.call(op)
        flat = out if isinstance(out, list) else [out]
        for x in flat:
            if isinstance(x, Refused):
                seen.add((op.kind, x.status))
    return seen


# ---- the committed cases -----------------------------------------------------------------------------------------------------
N_OPS = 84


def memo_fit(seed, half=True):
    """the shape of test_gpu_handle_reuse._tiny_case pushed further: about 40 users (18 of them with <= 4 ratings), 12 items,
    170 ratings, sparse raw ids, whole or half stars"""
    rng = np.random.default_rng(7300 + seed)
    while True:
        rows = _random_case(rng, n_users=22, n_items=12, n_ratings=130, half=half, tiny_rows=18)
        if _no_zero_scale(rows):
            break
    u, i, r = _cols(rows)
    return np.asarray(u, np.int32), np.asarray(i, np.int32), np.asarray(r, np.float64)


@dataclass
class Case:
    """one order-sensitive fit, the handle's first k and the seed of its sequence.  The ops do not depend on the similarity:
    they are drawn where the adjusted cosine's order shows and are played under both similarities (the Jaccard coefficient has
    no summation order, so under it the sequence checks the state that is not a matter of bits: lists, copies, scratch)."""
    name: str
    fit_seed: int
    k: int
    seed: int

    def train(self):
        return memo_fit(self.fit_seed)

    def k_pool(self):
        return [2, 6, K_ALL]

    def model(self, oracle, sim="cosine", wrong=""):
        return HandleModel(oracle, self.train(), sim_of(oracle, sim), self.k, wrong)

    def ops(self, oracle):
        return sequence(self.seed, self.model(oracle), N_OPS, k_pool=self.k_pool())


def sim_of(oracle, name):
    return {"cosine": oracle.SIM_COSINE, "jaccard": oracle.SIM_JACCARD}[name]


K_ALL = 60  # >= U - 1 of every memo fit (40 users)
# fit and sequence seeds searched on the CPU (differing_ops over the sequence seeds 0 .. 29 of each fit) so that the premises of
# test_call_sequence_premises.py hold
MEMO_CASES = [
    Case("k2-a", 20, 2, 3),
    Case("k2-b", 13, 2, 23),
    Case("k6", 4, 6, 23),
    Case("kall", 5, K_ALL, 11),
]


# ---- one handle through several fits ------------------------------------------------------------------------------------------
def _big_ids(train):
    """the rows with large raw ids, as test_gpu_handle_reuse._split(big=True) makes them: outside the direct id tables"""
    from types import SimpleNamespace as NS

    from tests.test_gpu_handle_reuse import _split

    rows = NS(users=train[0], items=train[1], ratings=train[2])
    return _split(NS(train=rows, test=rows), 0, big=True)[0]


def _lives():
    a = pc.wide_set(seed=31, n_users=300, n_items=120, per_user=17)     # 5 100 ratings
    b = pc.wide_set(seed=23, n_users=2100, n_items=300, per_user=19)    # 39 900 ratings, past the Personalized table's 2048 users
    fit_a = Fit("A", a)
    # (fit, the life's first k, the k that set_k moves between): k = 1000 on B gives kcap > 512, the id-sorted prediction path
    return [(fit_a, 50, [10, 50]), (Fit("B", b), 1000, [10, 1000]), (Fit("C", memo_fit(20)), 6, [2, 6, K_ALL]),
            (Fit("D", _big_ids(a)), 50, [10, 50]), (fit_a, 10, [10, 50])]


LIVES = _lives()
# a workspace with which the chunk rules of include/knncf.h give several chunks in the lives: 5 queries per chunk on A
# (tests/query_helpers._workspace_for), hence budget = 153 601 bytes: pairs 9 600 (budget / 16), recommend rows 13 on A and D and 5
# on B (budget / (96 * num_items)), explained rows 117 at cap 64 (budget / (20 * cap + 28)), Personalized ones 59, queries 5
# on A and D and 1 on B
LIFE_WORKSPACE = 2 * 5 * (64 * 300 + 96 * 120) + 2


def life_ops(oracle, life):
    """the ops of one life: the fit, the life's k, then a shuffled pass over every kind, family and predictor"""
    fit, k0, pool = LIVES[life]
    model = HandleModel(oracle, fit.train, oracle.SIM_COSINE, k0)
    body = sequence(9100 + life, model, None, k_pool=pool, fits=[fit], batch_sizes=(2, 3), every_variant=True)
    return [Op("fit", (fit,), "device" if life % 2 else "host"), Op("set_k", (k0,))] + body


def play_on_model(model, ops):
    return [model.call(op) for op in ops]


def play_with_built(model, ops):
    """[(answer, the built users after the op in ascending raw id)]"""
    return [(model.call(op), sorted(model.built)) for op in ops]


def differing_ops(oracle, case, wrong, ops=None, sim="cosine", with_built=False):
    """indices of the ops whose expected output — with_built: or the set of built lists after it — differs between the reference
    model and the wrong one"""
    ops = case.ops(oracle) if ops is None else ops
    play = play_with_built if with_built else play_on_model
    good, bad = play(case.model(oracle, sim), ops), play(case.model(oracle, sim, wrong=wrong), ops)
    return [j for j, (g, b) in enumerate(zip(good, bad)) if not same(b, g)]
