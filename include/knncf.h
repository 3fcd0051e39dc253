/*
 * knncf.h — C ABI of the MI355X-native kNN collaborative-filtering engine.
 *
 * The reference (EloDoyard/movie-recommender-system) has no FFI boundary: its
 * hot path is a set of Scala functions in
 *   src/main/scala/shared/predictions.scala
 * that take a Seq[Rating]/RDD[Rating] and return (Int,Int)=>Double closures,
 * called by predict.Baseline, predict.Personalized, predict.kNN and
 * distributed.DistributedBaseline.  This header is the boundary a JNI shim
 *  binds instead: one handle == one set of those closures
 * (including their memo state), plain pointers and sizes only.
 *
 * Conventions: every function returns a status (0 ok, negative error; text via
 * knncf_last_error).  Ids are the RAW user/item ids of the rating files, in
 * and out.  Host-pointer and device-pointer variants exist for the bulk calls;
 * "_device" pointers must live on the handle's HIP device, and their contents
 * must be COMPLETE when the call is made: the engine works on private
 * non-blocking HIP streams and cannot order itself after the caller's
 * producer stream (synchronise that stream, or wait on its event, first);
 * results written to caller-provided device buffers are complete on return.
 * A handle is not thread-safe; different handles may be used from different
 * threads and on different devices (per-device kernel state is keyed by device
 * ordinal); the calling thread's current device is restored on return.  The library owns all device memory it allocates.  There is no
 * CPU fallback: without a usable gfx950 device knncf_create fails.
 */
#ifndef KNNCF_H
#define KNNCF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KNNCF_OK 0
#define KNNCF_E_INVALID (-1)     /* bad argument */
#define KNNCF_E_NONFINITE (-2)   /* scale() == 0: non-finite deviation (reference would emit NaN) */
#define KNNCF_E_DUPLICATE (-3)   /* duplicate (user,item) training rows */
#define KNNCF_E_NOMEM (-4)
#define KNNCF_E_HIP (-5)         /* HIP runtime error */
#define KNNCF_E_STATE (-6)       /* call order, e.g. query before fit */
#define KNNCF_E_UNSUPPORTED (-7)
#define KNNCF_E_NODEVICE (-8)    /* no gfx950 device / HIP runtime unavailable */

/* similarity functions of shared/predictions.scala */
#define KNNCF_SIM_COSINE 0  /* adjustedCosineSimilarityFunction :407-433 */
#define KNNCF_SIM_ONE 1     /* similarityOne :400 */
#define KNNCF_SIM_JACCARD 2 /* jaccardCoefficient :440-464 */

/* predictors (the closures the entry points build) */
#define KNNCF_PRED_GLOBAL_AVG 0   /* computeAvgRating :101 */
#define KNNCF_PRED_USER_AVG 1     /* computeUserAvg :120 */
#define KNNCF_PRED_ITEM_AVG 2     /* computeItemAvg :141 */
#define KNNCF_PRED_BASELINE 3     /* computePrediction :205-237 */
#define KNNCF_PRED_BASELINE_RDD 4 /* baselinePredictorSpark :362-391 */
#define KNNCF_PRED_KNN 5          /* predictor(train, weightedSumDeviation(train, getSimilarity(train, k, sim))) predict/kNN.scala:43-44;
                                     sim = the handle's similarity: the adjusted cosine or the Jaccard coefficient (any number of users:
                                     both go through the MFMA GEMM + sparse tail + exact re-rank); similarityOne: KNNCF_E_UNSUPPORTED */
#define KNNCF_PRED_PERSONALIZED 6 /* predictor(train, weightedSumDeviation(train, sim)) predict/Personalized.scala:61-72, sim = the
                                     handle's similarity itself, no neighbourhood cut, at any number of users.  Cosine / Jaccard:
                                     U <= 2048 keeps a U x U table of the non-zero similarities (built once per fit); beyond, each
                                     call builds the exact fp64 similarity rows of the test users block by block (row scratch:
                                     R x U x 8 B, R sized from workspace_bytes / 2 or a quarter of free memory) and folds each
                                     test row over its item's raters in file order; the first such call after a fit also keeps
                                     20 B x n of per-rating copies (rater + deviation in file order, fp64 preprocessed rating in
                                     item order), charged to prep_ms.  Timings: the row build counts as rerank_ms, the row sort
                                     and the folds as predict_ms.  Cosine needs > 4 ratings per user, and shard
                                     handles are refused: KNNCF_E_UNSUPPORTED.  The kNN state (neighbour lists, their build
                                     numbers) is not touched. */

#define KNNCF_FLAG_VERIFY_BOUND 1u /* check |approx - exact| <= eps on every re-ranked pair (debug) */
/* The similarity GEMM is only a filter in front of the exact fp64 re-rank.  Default operand type is fp16
 * (11-bit significand, same MFMA rate as bf16): its rigorous error band is 8x narrower, so the shortlists
 * are ~k instead of ~3k and the re-rank is 3.6x cheaper (measured).  |pre| <= 1, so fp16's range is ample.
 * This flag selects bf16 operands (the north_star's literal wording); results are identical either way. */
#define KNNCF_FLAG_BF16_FILTER 4u
#define KNNCF_FLAG_F32_PANEL 8u /* keep the similarity panel in fp32 (default fp16: half the HBM traffic, band + 2^-11) */
#define KNNCF_FLAG_OVERLAP 2u      /* double-buffer the row blocks: GEMM/tail of block b+1 overlap select/re-rank of block b */

typedef struct knncf_handle knncf_handle;

typedef struct knncf_config {
    uint32_t struct_size;    /* = sizeof(knncf_config) */
    int32_t device;          /* HIP device ordinal */
    int32_t k;               /* neighbourhood size of KNNCF_PRED_KNN (predict/kNN.scala:44 uses 300) */
    int32_t similarity;      /* KNNCF_SIM_* */
    int32_t shard_rank;      /* users are block-partitioned over shard_count handles (one per GPU); */
    int32_t shard_count;     /* this handle owns block shard_rank.  1 = everything. */
    int64_t workspace_bytes; /* cap for the similarity panel + dense operand panels; 0 = auto */
    uint32_t flags;          /* KNNCF_FLAG_* */
    uint32_t head_items;     /* hybrid similarity: the head_items most-rated items go through the dense MFMA
                                GEMM, the sparse tail is accumulated per panel row in LDS (fixed point).  0 = cost model,
                                KNNCF_HEAD_ALL = every item dense */
} knncf_config;
#define KNNCF_HEAD_ALL 0xffffffffu

/* per-stage device timings of the last fit / neighbour build / predict, milliseconds */
typedef struct knncf_timings {
    double prep_ms;     /* K0-K3 (and K4 when a call needed it): id compaction, CSR/CSC, means, deviations, norms */
    double densify_ms;  /* CSR -> 16-bit operand panels */
    double gemm_ms;     /* K5 similarity GEMM (all launches) */
    double tail_ms;     /* K5 sparse tail when run as its own pass (0: fused into select_ms) */
    double select_ms;   /* K6 threshold + shortlist */
    double rerank_ms;   /* K6b exact fp64 re-rank + top-k sort */
    double predict_ms;  /* K7-K9 prediction + MAE */
    int64_t gemm_launches;
    double gemm_flops_executed;    /* 2*M*N*K summed over launches */
    double gemm_flops_algorithmic; /* 2 * pairs * I_c for the rows built */
    int64_t shortlist_total;       /* sum of shortlist sizes */
    int64_t fallback_rows;         /* rows re-done by the exact fallback */
    double max_bound_violation;    /* KNNCF_FLAG_VERIFY_BOUND: max(|approx-exact| - eps), <= 0 when the bound holds */
    int64_t head_items;            /* dense head width used by the last build */
    double tail_pair_updates;      /* sum over tail items of (raters in panel) x (raters) */
    double rerank_row_bytes;       /* K6b algorithmic traffic: 12 B x ratings of every re-ranked candidate */
    double select_row_bytes;       /* K6 algorithmic traffic: panel entry size x (rows x users) similarity panel entries read */
    int64_t select_launches;       /* row-block launches of select / re-rank (the symmetric GEMM is ONE launch for all of them) */
} knncf_timings;

const char* knncf_version(void);
const char* knncf_status_string(int status);

int knncf_create(const knncf_config* cfg, knncf_handle** out);
void knncf_destroy(knncf_handle* h);
const char* knncf_last_error(const knncf_handle* h);

/* ---- fit: everything the reference's kNN closures compute eagerly (K0-K3) -- */
/* Rows are the collected Array[Rating] in FILE ORDER (the reference's summation
 * order and fallbacks depend on it).  Arrays are copied.
 * K4 — the per-item maps of the baseline predictors (itemsAvg :134, itemsAvgDev
 * :176-186, getItemsAvgDev :336-343) — is not part of the kNN closures
 * (weightedSumDeviation :489-548, predictor :557-585 never evaluate them): the
 * reference builds those maps when computeItemAvg / computePrediction / the Spark
 * forms are constructed, and the handle builds them on the first call that reads
 * them (knncf_item_avg*, KNNCF_PRED_ITEM_AVG / BASELINE / BASELINE_RDD, and
 * PERSONALIZED with similarityOne), charged to prep_ms of that call.
 * Rating domain: any finite double is accepted (the loader's toDouble yields any); nothing assumes the star scale [0.5, 5].
 * A non-finite rating (NaN, +inf, -inf) gives a non-finite deviation and the fit returns KNNCF_E_NONFINITE, like a zero
 * scale().  A fitted user whose mean is negative is predicted as the global average by every predictor, exactly like a
 * user unknown to train: usersAvg.getOrElse(u, -1.0) < 0.0 at :572-573 (and :226 for the baseline) does not tell them apart. */
int knncf_fit(knncf_handle* h, const int32_t* users, const int32_t* items,
              const double* ratings, int64_t n);
int knncf_fit_device(knncf_handle* h, const int32_t* d_users, const int32_t* d_items,
                     const double* d_ratings, int64_t n);

int knncf_num_users(const knncf_handle* h, int32_t* out);
int knncf_num_items(const knncf_handle* h, int32_t* out);

/* ---- scalar queries mirroring the JSON answers ---------------------------- */
int knncf_global_avg(knncf_handle* h, double* out);                 /* average :94 */
int knncf_user_avg(knncf_handle* h, int32_t user, double* out);     /* computeUserAvg(train)(user, _) */
int knncf_item_avg(knncf_handle* h, int32_t item, double* out);     /* computeItemAvg(train)(_, item) */
int knncf_item_avg_dev(knncf_handle* h, int32_t item, double* out); /* computeItemAvgDev(train)(_, item) :193 */
int knncf_item_avg_dev_rdd(knncf_handle* h, int32_t item, double* out); /* itemsAvgDevSpark(train)(_, item) :350 */
/* the similarity function on a fresh closure: sim(train)(u, v) */
int knncf_similarity(knncf_handle* h, int32_t u, int32_t v, double* out);
/* getSimilarity(train, k, sim)(u, v): sim if v is one of u's k nearest, else 0 :634-648 */
int knncf_knn_similarity(knncf_handle* h, int32_t u, int32_t v, double* out);
/* getNeighbors(train, k, sim)(u): ids and similarities in reference order :603-616.
 * Shard handles (shard_count > 1) whose train set has a user with <= 4 ratings: KNNCF_E_UNSUPPORTED for a user whose
 * neighbourhood knncf_mae* / knncf_predict_batch* have not built yet.  Such a build would be numbered on this shard only,
 * and a <= 4-rating pair is summed in the order that numbering decides: the shards could disagree with each
 * other and with a single handle.  Query after the replicated mae / predict call, which numbers every user on every shard.
 * The same holds for knncf_neighbors_batch. */
int knncf_neighbors(knncf_handle* h, int32_t u, int32_t cap, int32_t* ids, double* sims,
                    int32_t* count);
/* getNeighbors for users[0..n) at once ("as if called in this order"): row j of ids / sims ([n * cap]) receives
 * min(counts[j], cap) entries.  Neighbourhoods that do not exist yet are built in ONE batch on the device — the bulk
 * door for exporting or verifying whole neighbour tables (knncf_neighbors costs a device round trip per user). */
int knncf_neighbors_batch(knncf_handle* h, const int32_t* users, int64_t n, int32_t cap, int32_t* ids,
                          double* sims, int32_t* counts);
int knncf_predict(knncf_handle* h, int predictor, int32_t user, int32_t item, double* out);

/* recommendations(train, predictor)(user, n) shared/predictions.scala:651-674 (called by
 * recommend/Recommender.scala:85-88 with n = 3): every train item `user` has not rated, predicted with `predictor`,
 * ordered by (prediction descending, raw item id ascending); the first min(n, #unrated) are written, *count of them.
 * An unknown user has rated nothing (every prediction is the global average: pure id order).
 * This is knncf_recommend_batch over the one user (*count = its counts[0]): the same code, the same handle state afterwards and
 * the same statuses, shard handles included.  An unfitted handle (KNNCF_E_STATE) and a bad argument (count null, n < 0, a null
 * output with n > 0: KNNCF_E_INVALID) leave *count alone; past these two checks *count = 0 is written before anything else
 * can fail. */
int knncf_recommend(knncf_handle* h, int predictor, int32_t user, int32_t n, int32_t* items,
                    double* predictions, int32_t* count);

/* ---- Bulk similarities: knncf_similarity / knncf_knn_similarity for many pairs in one device pass ----------------------------
 * knncf_similarity_batch: out[j] equals what knncf_similarity(h, us[j], vs[j], ..) writes, bit for bit (the bits of a NaN
 * included), j < n.  Every pair is answered on a closure of its OWN: the batch keeps no memo across its pairs, (v, u) after
 * (u, v) is computed with v as the first argument, and a pair listed twice is computed twice.  (A "one closure across the batch"
 * mode, in which an earlier pair's memo decides a later pair's summation order, is not offered.)  Adjusted cosine :415-432: the
 * left fold from 0.0 of pre(u, i) * pre(v, i) over the common items in the item-set order of u, the FIRST argument — ascending
 * trie order when u has more than 4 train ratings, u's file order otherwise; multiply and add round separately.  u == v is an
 * ordinary pair (S(u, u), close to but not 1.0); a user absent from train gives 0.0.  Jaccard :446-463: |I(u) & I(v)| /
 * (|I(u)| + |I(v)| - |I(u) & I(v)|) as Double / Int; an absent user has the empty set, so one absent user gives 0.0 and two give
 * 0.0 / 0 = NaN.  KNNCF_SIM_ONE: every out[j] = 1.0.
 * Status: KNNCF_E_STATE before a fit; KNNCF_E_INVALID for n < 0 or a null pointer with n > 0; n == 0 is KNNCF_OK and touches
 * nothing; a call that fails these checks writes nothing.  Shard handles are accepted exactly where knncf_similarity accepts
 * them (after knncf_shard_commit every shard holds every user's preprocessed ratings).  The call only reads the handle: the
 * neighbour table, its build numbers, the call epoch and the knncf_neighbors_save file stay as they were.  knncf_get_timings:
 * the pair kernels are charged to rerank_ms.
 * Chunks.  The host forms answer the pairs in chunks of consecutive positions, [0, C), [C, 2 C), ..., the last one possibly
 * shorter, through scratch that the handle owns (two ids and one double per pair):
 *     C = max(1, budget / 16)
 *     budget = workspace_bytes / 2 if workspace_bytes > 0, else min(48 GiB, free device memory / 4)
 * The results do not depend on C, and a call on a handle that has answered the same shape before allocates no device memory.
 * knncf_similarity_batch_device: the same over device arrays (raw ids, looked up on the device; d_out [n] doubles), one pass
 * into the caller's buffer with no scratch.  Inputs must be complete at the call, outputs are complete on return.
 * knncf_knn_similarity_batch: getSimilarity(train, k, sim)(us[j], vs[j]) :634-648.  out[j] equals what a loop of
 * knncf_knn_similarity over the pairs in this order returns, bit for bit: 0.0 + sim when vs[j] is in the list of us[j] (.sum
 * from 0.0: a similarity of -0.0 comes back as +0.0), 0.0 otherwise, and 0.0 for us[j] == vs[j] and when either id is absent
 * from train.  Order and handle state.  The reference builds the neighbourhood of us[j] only when BOTH ids are in train, and so
 * does this call.  The missing neighbourhoods are built in ONE batch.  Let us' be us with a raw id absent from train in every
 * position where us[j] or vs[j] is absent from train: THE HANDLE IS LEFT IN THE STATE THAT knncf_neighbors_batch OVER us'
 * LEAVES IT IN: the same lists, the same build numbers (call, position j), the same knncf_neighbors_save file.  The lookup runs
 * on the device, in the id-sorted copy of the lists (made when it is not current); only out comes back.
 * Status: KNNCF_E_STATE before a fit; KNNCF_E_INVALID for n < 0 or a null pointer with n > 0; KNNCF_E_UNSUPPORTED on a
 * KNNCF_SIM_ONE handle, as knncf_knn_similarity; KNNCF_E_INVALID when a us[j] in train (with vs[j] in train) is owned by another
 * shard; a neighbourhood that is not built yet is refused on a shard whose train set has a <= 4-rating user, as
 * knncf_neighbors_batch refuses it.  All of these are checked for the whole call before anything is built or written; n == 0
 * is KNNCF_OK.  The chunk rule above applies.  knncf_get_timings: builds are charged as in knncf_neighbors_batch, the lookup to
 * predict_ms.  There is no device form: the builds are numbered on the host, from the pairs' positions. */
int knncf_similarity_batch(knncf_handle* h, const int32_t* us, const int32_t* vs, int64_t n, double* out);
int knncf_similarity_batch_device(knncf_handle* h, const int32_t* d_us, const int32_t* d_vs, int64_t n, double* d_out);
int knncf_knn_similarity_batch(knncf_handle* h, const int32_t* us, const int32_t* vs, int64_t n, double* out);

/* ---- Batched recommendations: knncf_recommend for many users of the fit in one call ------------------------------------------
 * Row b of out_items / out_preds ([n_users * n], row stride n) receives exactly what
 * knncf_recommend(h, predictor, users[b], n, ...) writes, bit for bit, and counts[b] its *count = min(n, #items users[b] has
 * not rated) (0 for a user who rated every train item); cells of a row beyond counts[b] are left untouched.  A raw id absent
 * from train is a valid row (nothing rated, every prediction the global average: the first n items in raw-id order); the same
 * user may occur several times, the rows are independent.  Every predictor is accepted where knncf_recommend accepts it
 * (KNNCF_PRED_KNN on a KNNCF_SIM_ONE handle: KNNCF_E_UNSUPPORTED, ...).
 * Order and handle state.  The call behaves as if knncf_recommend had been called for users[0], users[1], ... in this order
 * on this handle: a neighbourhood that does not exist yet is built and numbered by the call, and a pair with a <= 4-rating
 * user is summed in the order that numbering decides.  KNNCF_PRED_KNN builds and numbers the neighbourhood of
 * users[b] only where the reference evaluates it: the user is in train and its mean is not negative (the predictor answers a
 * negative mean with the global average, :573, before it looks at a neighbour).  The missing neighbourhoods are built in ONE
 * batch, and THE HANDLE IS LEFT IN THE STATE THAT knncf_neighbors_batch OVER THE SAME users LEAVES IT IN ONCE THOSE WHOSE MEAN
 * IS NEGATIVE ARE TAKEN OUT OF THEM (the other predictors leave the neighbour table alone): the same lists, the same build
 * numbers (call, position in users), the same knncf_neighbors_save file.  knncf_neighbors_batch itself numbers every user it
 * is asked about.  (A loop of single calls numbers its builds (call, 0), one call each: the same order, hence the same lists
 * and sums, under different numbers.)
 * Status: KNNCF_E_STATE before a fit; KNNCF_E_INVALID for a null pointer with n_users > 0, n_users < 0, n < 0 or an unknown
 * predictor; n_users == 0 or n == 0 is KNNCF_OK (n == 0: counts[b] = 0 for every b) and touches nothing else.  Shard
 * handles: every known user must be owned by the shard and an unknown user is answered by shard 0 only (KNNCF_E_STATE
 * otherwise, for the whole call, before anything is built); a neighbourhood that is not built yet is refused on a shard
 * whose train set has a <= 4-rating user, as knncf_neighbors_batch refuses it (KNNCF_E_UNSUPPORTED) — by knncf_recommend
 * too: such a list would be built under a number that the other shards never see.  A call that fails
 * these checks builds nothing and writes nothing.
 * Chunks.  The users are answered in chunks of consecutive rows, [0, C), [C, 2 C), ..., the last one possibly shorter:
 *     C = max(1, min(1024, budget / (96 * num_items), (2^31 - 1) / num_items))
 *     budget = workspace_bytes / 2 if workspace_bytes > 0, else min(48 GiB, free device memory / 4)
 * The results do not depend on C, and a call on a handle that has answered the same shape before allocates no device memory.
 * Every predictor sends the chunk's C x num_items rows through the prediction batch that knncf_predict_batch runs (there is no
 * threshold on the chunk size: a chunk of one, which is what knncf_recommend asks for, takes the same path).  n <= 32 then
 * selects each row's n best without sorting; larger n (up to and beyond num_items) orders each row completely.
 * knncf_get_timings: neighbour builds are charged as in knncf_neighbors_batch, everything else as predict_ms. */
int knncf_recommend_batch(knncf_handle* h, int predictor, const int32_t* users, int64_t n_users, int32_t n,
                          int32_t* out_items, double* out_preds, int32_t* counts);

/* ---- Explanations: the neighbour terms behind KNNCF_PRED_KNN predictions ---------------------------------------------------
 * A kNN prediction is a short sum over the neighbours who rated the item: weightedSumDeviation shared/predictions.scala:504-548
 * maps the item's raters x, in training file order, to simVal :513-517 and folds (num + dev * sim, den + |sim|) from
 * (0.0, 0.0) :520-524.  The TERMS of row j = (users[j], items[j]) are the elements of simVal whose similarity is non-zero, each
 * with three parts: the rater's raw id x.user, getSimilarity(train, k, sim)(users[j], x.user) :634-648, and x's normalized
 * deviation on the item.  A neighbour of the list whose similarity is exactly 0.0 (k >= num_users - 1, disjoint users) is NOT a
 * term, and the user is never its own term.
 * Outputs per row: counts[j] = the number of terms (it may exceed cap); the first min(counts[j], cap) terms, in `order`, in
 * row j of raters / sims / devs ([n * cap], row stride cap; cells beyond them are left untouched); sums[2 j], sums[2 j + 1] =
 * num and den of the fold over ALL terms in summation order (independent of order and cap); predictions[j] =
 * knncf_predict(h, KNNCF_PRED_KNN, users[j], items[j]) bit for bit.  sums and predictions may be null; with cap == 0 the three
 * term arrays may be null.
 * Row kinds.  A user unknown to train (or one whose mean is negative, :573): count 0, sums (0, 0), prediction = the global
 * average.  A known user on an item that is unknown to train or that no neighbour rated: count 0, sums (0, 0), wsd = 0.0
 * :527-529.
 * Properties.  With counts[j] <= cap and KNNCF_EXPLAIN_SUM_ORDER the caller's left fold of the returned terms,
 * (num + devs * sims, den + |sims|) from (0.0, 0.0), gives sums bit for bit (no fused multiply-add).  With ua = knncf_user_avg
 * and wsd = den > 0 ? num / den : 0.0, the combine :578, ua + wsd * scale(ua + wsd, ua), gives predictions[j] bit for bit.
 * KNNCF_EXPLAIN_BY_WEIGHT returns a permutation of the same terms.
 * Handle state.  Neighbourhoods that do not exist yet are built by the call exactly as
 * knncf_predict_batch(h, KNNCF_PRED_KNN, users, items, n, ...) builds them — once for the whole call, before any chunk — and
 * THE HANDLE IS LEFT IN THE STATE THAT knncf_predict_batch OVER THE SAME ROWS LEAVES IT IN: the same lists, the same build
 * numbers, the same knncf_neighbors_save file.  knncf_explain is the batch of one row.  knncf_get_timings: builds are charged
 * as usual, the explain kernel as predict_ms.
 * Status: KNNCF_E_STATE before a fit; KNNCF_E_UNSUPPORTED for a KNNCF_SIM_ONE handle (as knncf_predict) and for a shard
 * handle (shard_count > 1): SHARDED EXPLANATIONS ARE OUT OF SCOPE, as are explanations of KNNCF_PRED_PERSONALIZED by these
 * calls: knncf_explain* has no predictor argument and explains KNNCF_PRED_KNN only; the Personalized predictions of fitted users
 * have knncf_explain_personalized* ("Explanations of Personalized predictions" below), and the explanations of fold-in /
 * update / revise queries are the knncf_*_explain* calls below ("Explanations of query predictions"); KNNCF_E_INVALID for a null pointer that is needed, n < 0, cap < 0, an unknown order or
 * n >= 2^32 - 1.  n == 0 is KNNCF_OK and touches nothing.  A call that fails these checks builds nothing and writes nothing.
 * Chunks.  The device form is one pass into the caller's buffers (every pointer on the handle's device, inputs complete at
 * the call, outputs complete on return).  The host form answers consecutive row ranges [0, C), [C, 2 C), ... through
 * handle-owned device scratch:
 *     C = max(1, budget / (20 * cap + 28))
 *     budget = workspace_bytes / 2 if workspace_bytes > 0, else min(48 GiB, free device memory / 4)
 * The results do not depend on C, and a call on a handle that has answered the same shape before allocates no device memory. */
#define KNNCF_EXPLAIN_SUM_ORDER 0  /* the order of the fold :520-524 = training file order of the item's raters */
#define KNNCF_EXPLAIN_BY_WEIGHT 1  /* |similarity| descending, equal magnitudes in summation order */
int knncf_explain(knncf_handle* h, int32_t user, int32_t item, int32_t order, int32_t cap, int32_t* raters, double* sims,
                  double* devs, int32_t* count, double* sums, double* prediction);
int knncf_explain_batch(knncf_handle* h, const int32_t* users, const int32_t* items, int64_t n, int32_t order, int32_t cap,
                        int32_t* raters, double* sims, double* devs, int32_t* counts, double* sums, double* predictions);
int knncf_explain_batch_device(knncf_handle* h, const int32_t* d_users, const int32_t* d_items, int64_t n, int32_t order,
                               int32_t cap, int32_t* d_raters, double* d_sims, double* d_devs, int32_t* d_counts,
                               double* d_sums, double* d_predictions);

/* ---- Explanations of Personalized predictions: the terms behind KNNCF_PRED_PERSONALIZED for users as the fit holds them ------
 * KNNCF_PRED_PERSONALIZED, predictor(train, weightedSumDeviation(train, sim)) predict/Personalized.scala:61-72, has no
 * neighbourhood cut: its prediction folds EVERY rating of the item, 10^4 .. 10^5 terms for a popular one.  These calls answer
 * "which few users carried this prediction".  order (KNNCF_EXPLAIN_SUM_ORDER / KNNCF_EXPLAIN_BY_WEIGHT), cap and the outputs
 * are those of knncf_explain_batch: counts[j] = the number of terms of row j (it may exceed cap); the first min(counts[j], cap)
 * terms, in `order`, in row j of raters / sims / devs ([n * cap], row stride cap; cells beyond them are left untouched);
 * sums and predictions may be null; with cap == 0 the three term arrays may be null.  knncf_explain_personalized is the batch
 * of one row.
 * Terms of row j = (u, i) = (users[j], items[j]).  The elements of simVal shared/predictions.scala:513-517, built with S = the
 * handle's similarity itself (adjustedCosineSimilarityFunction(train) or jaccardCoefficient(train)), whose similarity is not
 * exactly 0.0: (the rater's raw id, S(u, rater), the rater's normalized deviation on i), over all ratings of i in train, in file
 * order.  Unlike the kNN explanations THE USER IS ITS OWN TERM when (u, i) is a training pair: weight S(u, u), at its file
 * place.  KNNCF_EXPLAIN_BY_WEIGHT is |similarity| descending, equal magnitudes in summation order.
 * Properties.  sums[2 j], sums[2 j + 1] = num and den of the fold :520-524 over ALL terms in summation order (independent of
 * order and cap).  With counts[j] <= cap and KNNCF_EXPLAIN_SUM_ORDER the caller's left fold of the returned terms,
 * (num + dev * sim, den + |sim|) from (0.0, 0.0) with the multiply and the add separate (no fused multiply-add), gives sums bit
 * for bit: the raters that are no terms add +-0.0 to sums that start at +0.0.  predictions[j] equals
 * knncf_predict(h, KNNCF_PRED_PERSONALIZED, users[j], items[j]) bit for bit, at every number of users; the combine :578 of
 * knncf_user_avg with (den > 0 ? num / den : 0.0) gives predictions[j].  KNNCF_EXPLAIN_BY_WEIGHT returns the first
 * min(count, cap) elements of its total order, a permutation of the KNNCF_EXPLAIN_SUM_ORDER terms when count <= cap; among
 * equal magnitudes that the cap cuts through, the earliest in summation order are kept.  It selects the cap heaviest terms
 * without ordering the item's raters and ranks only those, so its cost grows with the raters and with min(count, cap)^2 / 256,
 * not with the square of the raters; cap >= count ranks every term, which is the caller's choice.
 * Row kinds.  A user unknown to train, or one whose mean is negative (:573): count 0, sums (0, 0), prediction = the global
 * average.  A known user on an item unknown to train, or on an item whose raters all have similarity 0.0: count 0, sums
 * (0, 0), prediction = the user's mean.
 * Status: KNNCF_E_STATE before a fit; KNNCF_E_UNSUPPORTED exactly where the fitted KNNCF_PRED_PERSONALIZED refuses — a shard
 * handle (SHARDED EXPLANATIONS ARE OUT OF SCOPE), or the adjusted cosine with a train user of 4 or fewer ratings — and on a
 * KNNCF_SIM_ONE handle: every weight is 1.0 there and every rater is a term, so there is nothing to explain;
 * KNNCF_E_INVALID for a null pointer that is needed, n < 0, cap < 0, an unknown order or n >= 2^32 - 1.  n == 0 is KNNCF_OK and
 * touches nothing.  A call that fails these checks writes nothing.
 * Handle state.  Read-only on the kNN state: the neighbour table, the build numbers, the epoch and the knncf_neighbors_save
 * bytes stay as they were.  The first call after a fit builds the handle's file-order rater copies (20 bytes per train rating,
 * charged to prep_ms as the streamed KNNCF_PRED_PERSONALIZED path charges them; a refit drops them).  knncf_get_timings: the
 * similarity rows are charged as rerank_ms, everything else as predict_ms.
 * Blocks and sub-ranges.  One path at every number of users: the rows are sorted by (user, item) and the distinct users that
 * have a row on a train item are cut into equal blocks of at most budget / (8 * num_users) users, whose exact fp64 similarity
 * rows are built per block (as knncf_predict_batch does beyond 2048 users).  Within a block the explain kernel runs over
 * consecutive sub-ranges of
 *     R = max(1, budget / (40 * cap + 28))
 *     budget = workspace_bytes / 2 if workspace_bytes > 0, else min(48 GiB, free device memory / 4)
 * rows: 20 * cap + 28 bytes of outputs per row, which come back in one copy, and 20 * cap bytes in which
 * KNNCF_EXPLAIN_BY_WEIGHT stages the selected terms before it ranks them.  The results depend neither on the blocks nor on R,
 * and a call on a handle that has answered the same shape before allocates no device memory.
 * OUT OF SCOPE: a device-pointer form, shard handles, KNNCF_SIM_ONE, and Personalized explanations of fold-in / update / revise
 * queries (knncf_*_explain* below keep refusing KNNCF_PRED_PERSONALIZED).  Those have calls of their own:
 * knncf_*_explain_personalized* ("Explanations of Personalized query predictions" below).  The query families can also have
 * their recommendations and the terms behind them from one call: knncf_*_recommend_explain* ("Recommendations with their
 * explanations" below). */
int knncf_explain_personalized(knncf_handle* h, int32_t user, int32_t item, int32_t order, int32_t cap, int32_t* raters, double* sims,
                               double* devs, int32_t* count, double* sums, double* prediction);
int knncf_explain_personalized_batch(knncf_handle* h, const int32_t* users, const int32_t* items, int64_t n, int32_t order,
                                     int32_t cap, int32_t* raters, double* sims, double* devs, int32_t* counts, double* sums,
                                     double* predictions);

/* ---- fold-in queries: one user that is NOT in the fitted training set ------
 * recommend/Recommender.scala:64-88 appends a person's ratings to the data (data.union(personal), :68) and asks for
 * that person's recommendations.  These calls answer for such a query user `user` (a raw id absent from train) with
 * ratings (items[j], ratings[j]), j < n_ratings, WITHOUT a refit: every result equals, bit for bit, the reference's on
 * aug = train ++ [Rating(user, items[j], ratings[j]) for j in order] with fresh closures whose first evaluation is the
 * query user's:
 *   knncf_query_neighbors  getNeighbors(aug, k, sim)(user) :603-616 — min(k, U) entries, *count of them, the first
 *                          min(cap, *count) written;
 *   knncf_query_predict    predictor(aug, weightedSumDeviation(aug, getSimilarity(aug, k, sim)))(user, pred_items[j])
 *                          :489-585 for any item id (rated by the user, unknown to train, ...);
 *   knncf_query_recommend  recommendations(aug, that predictor)(user, n) :651-674.
 * KNNCF_SIM_COSINE / KNNCF_SIM_JACCARD handles with predictor KNNCF_PRED_KNN (above) or KNNCF_PRED_PERSONALIZED (no
 * neighbourhood cut: "Personalized queries" below), single shard, >= 5 train users, at most
 * 65536 query ratings (KNNCF_E_UNSUPPORTED otherwise, also for a query whose mean rating is negative); KNNCF_E_STATE
 * before a fit; KNNCF_E_INVALID if `user` occurs in train, a pointer is null or n_ratings <= 0; KNNCF_E_DUPLICATE if
 * the query repeats an item; KNNCF_E_NONFINITE for a non-finite deviation (as knncf_fit).  Read-only on the handle:
 * the neighbour table, its build history and everything knncf_neighbors / knncf_mae / knncf_neighbors_save observe
 * stay as they were.  Each call is the batched call below with one query (a chunk of one, no chunk rule), except that the
 * query's status is the call's return value and knncf_last_error reads "query: <reason>". */
int knncf_query_neighbors(knncf_handle* h, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings,
                          int32_t cap, int32_t* ids, double* sims, int32_t* count);
int knncf_query_predict(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings,
                        int64_t n_ratings, const int32_t* pred_items, int64_t m, double* out);
int knncf_query_recommend(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings,
                          int64_t n_ratings, int32_t n, int32_t* out_items, double* out_preds, int32_t* count);

/* ---- Batched fold-in queries: many users outside the fit in one call -------------------------------------------------------
 * n_queries independent queries, CSR-style: query b is (users[b], items[offsets[b] .. offsets[b + 1]), ratings[...]) with
 * offsets[0] == 0, offsets non-decreasing, fewer than 2^31 ratings in all.
 *   knncf_query_neighbors_batch   ids / sims [n_queries * cap]: row b = knncf_query_neighbors of query b, counts[b] its *count;
 *   knncf_query_predict_batch     out[pred_offsets[b] .. pred_offsets[b + 1]) = knncf_query_predict of query b on
 *                                 pred_items[pred_offsets[b] ..) (pred_offsets: a CSR like offsets);
 *   knncf_query_recommend_batch   out_items / out_preds [n_queries * n]: row b = knncf_query_recommend of query b, counts[b] its
 *                                 *count.
 * Row b is the single call's answer, bit for bit.  The queries are independent: each is answered on aug_b = train ++ the rows
 * of query b alone, fresh closures, first evaluation the query user's; the other queries of the batch are not part of aug_b, so
 * the same raw user id may occur in several queries, and permuting the queries permutes the rows and changes nothing else.
 * statuses[b] is the status the single call would return for query b: KNNCF_OK, KNNCF_E_INVALID (the user occurs in train, or
 * the query is empty), KNNCF_E_DUPLICATE, KNNCF_E_NONFINITE, KNNCF_E_UNSUPPORTED (negative mean, more than 65536 ratings).  A
 * failed query gets counts[b] = 0, its output row is left untouched, and it does not disturb the other queries.
 * The return value reports what is wrong with the call or the handle, as the single calls do: KNNCF_E_STATE before a fit;
 * KNNCF_E_UNSUPPORTED for KNNCF_SIM_ONE, a shard handle, fewer than 5 train users or a predictor other than KNNCF_PRED_KNN
 * and KNNCF_PRED_PERSONALIZED;
 * KNNCF_E_INVALID for a null pointer, n_queries < 0, cap or n < 0, or offsets that are not a CSR.  n_queries == 0 is KNNCF_OK
 * and touches nothing.  After a call with failed queries knncf_last_error names the first failed query and its reason.
 * Read-only on the handle, as the single calls.
 * Chunks.  The batch is answered in chunks of consecutive queries, [0, C), [C, 2 C), ..., the last one possibly shorter:
 *     C = max(1, min(64, budget / (64 * num_users + 96 * num_items), (2^31 - 1) / max(num_users, num_items)))
 *     budget = workspace_bytes / 2 if workspace_bytes > 0, else min(48 GiB, free device memory / 4)
 * so a call makes ceil(n_queries / C) chunks.  (The gathered neighbour ratings of a chunk are allocated beside that as they
 * are needed; a chunk whose neighbours hold 2^32 - 1 ratings or more fails the call with KNNCF_E_UNSUPPORTED.  With
 * KNNCF_PRED_PERSONALIZED nothing is gathered; the transposed similarities of a chunk, 8 * num_users * (the power of two >= C)
 * bytes, and the handle's file-order rater copies, 20 bytes per train rating, are allocated beside the budget instead.)  Failed queries
 * keep their place in their chunk.  A chunk with fewer than 32 answerable queries runs the one-query similarity kernel once
 * per query; larger ones read every train row once for the whole chunk.  The results do not depend on C. */
int knncf_query_neighbors_batch(knncf_handle* h, const int32_t* users, const int64_t* offsets, const int32_t* items,
                                const double* ratings, int64_t n_queries, int32_t cap, int32_t* ids, double* sims, int32_t* counts,
                                int32_t* statuses);
int knncf_query_predict_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets, const int32_t* items,
                              const double* ratings, int64_t n_queries, const int64_t* pred_offsets, const int32_t* pred_items,
                              double* out, int32_t* statuses);
int knncf_query_recommend_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets, const int32_t* items,
                                const double* ratings, int64_t n_queries, int32_t n, int32_t* out_items, double* out_preds,
                                int32_t* counts, int32_t* statuses);

/* ---- Update queries: a user that may be IN the fit, with additional ratings ------------------------------------------------
 * The fold-in calls above refuse a user that occurs in train.  These answer for any `user`: (items[j], ratings[j]), j <
 * n_ratings, are the rows the user has rated IN ADDITION to whatever train holds for it, and with
 *     aug = train ++ [Rating(user, items[j], ratings[j]) for j in order]
 * (data.union(personal), recommend/Recommender.scala:68 — nothing there requires the person to be new) every result equals,
 * bit for bit, the reference's on aug with fresh closures whose first evaluation is `user`'s, WITHOUT a refit:
 *   knncf_update_neighbors  getNeighbors(aug, k, sim)(user) :603-616.  (allUsers - u) :608 drops a user of the fit from its
 *                           own candidates, so *count is min(k, U - 1) for a user of the fit and min(k, U) for any other;
 *   knncf_update_predict    predictor(aug, weightedSumDeviation(aug, getSimilarity(aug, k, sim)))(user, pred_items[j]) :489-585;
 *   knncf_update_recommend  recommendations(aug, that predictor)(user, n) :651-674: the user's own items, train and
 *                           additional, are the rated ones.
 * The argument lists, the batched forms (CSR offsets, per-query statuses, counts, untouched rows of failed queries, the
 * handle-level return values), the chunk rule with its formula, the split at 32 answerable queries between the two similarity
 * kernels and "the results do not depend on C" are exactly those of knncf_query_* / knncf_query_*_batch; a batch may mix users
 * of the fit and others and may name the same user several times with different additional rows (each query has its own aug).
 * For a user absent from train the answer is the knncf_query_* answer bit for bit: the same code runs.
 * n_ratings == 0 (items / ratings may then be null) is valid for a user of the fit: the fresh-closure answer on train itself,
 * whatever the handle has memoised for that user (after other calls knncf_neighbors(user) may own fewer of its pairs and
 * differ in the last bits).  For a user absent from train it stays KNNCF_E_INVALID.
 * Statuses: KNNCF_E_DUPLICATE if an additional item repeats another additional item or an item the user rated in train (the
 * reference has no operation that replaces a rating); KNNCF_E_NONFINITE for a non-finite deviation; KNNCF_E_UNSUPPORTED for
 * a negative mean of the combined rows or more than 65536 combined rows (the user's train rows plus the additional ones); and
 * as for knncf_query_*: KNNCF_SIM_COSINE / KNNCF_SIM_JACCARD, KNNCF_PRED_KNN or KNNCF_PRED_PERSONALIZED ("Personalized queries"
 * below), single shard, >= 5 train users (KNNCF_E_UNSUPPORTED), KNNCF_E_STATE before a fit, KNNCF_E_INVALID for null pointers, negative sizes or bad CSR offsets.
 * Read-only on the handle: the neighbour table, its build numbers and epoch and what knncf_neighbors_save writes stay as they
 * were; the user's own stored list is neither read nor replaced, and the additional rows do not enter the fit. */
int knncf_update_neighbors(knncf_handle* h, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings,
                           int32_t cap, int32_t* ids, double* sims, int32_t* count);
int knncf_update_predict(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings,
                         int64_t n_ratings, const int32_t* pred_items, int64_t m, double* out);
int knncf_update_recommend(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings,
                           int64_t n_ratings, int32_t n, int32_t* out_items, double* out_preds, int32_t* count);
int knncf_update_neighbors_batch(knncf_handle* h, const int32_t* users, const int64_t* offsets, const int32_t* items,
                                 const double* ratings, int64_t n_queries, int32_t cap, int32_t* ids, double* sims, int32_t* counts,
                                 int32_t* statuses);
int knncf_update_predict_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets, const int32_t* items,
                               const double* ratings, int64_t n_queries, const int64_t* pred_offsets, const int32_t* pred_items,
                               double* out, int32_t* statuses);
int knncf_update_recommend_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets, const int32_t* items,
                                 const double* ratings, int64_t n_queries, int32_t n, int32_t* out_items, double* out_preds,
                                 int32_t* counts, int32_t* statuses);

/* ---- Revise queries: a user of the fit who REMOVED or RE-RATED items, possibly with additional ratings -----------------------
 * The update calls above can only add rows.  These take, in front of the additional rows, the raw ids of train items of `user`
 * whose rows are taken out: removed_items[0 .. n_removed) (batched: the CSR removed_offsets / removed_items, like offsets:
 * removed_offsets[0] == 0, non-decreasing, fewer than 2^31 removed items in all).  With
 *     aug = [r for r in train, in file order, unless r.user == user and r.item is in removed_items]
 *           ++ [Rating(user, items[j], ratings[j]) for j in order]
 * every result equals, bit for bit, the reference's on aug with fresh closures whose first evaluation is `user`'s, WITHOUT a
 * refit: knncf_revise_neighbors = getNeighbors(aug, k, sim)(user) :603-616, knncf_revise_predict = the kNN predictor :489-585,
 * knncf_revise_recommend = recommendations :651-674.  Removing rows of `user` changes only that user's mean, deviations, norm
 * and preprocessed ratings; nobody else's quantities move.
 *   The user set of aug.  A user of the fit that keeps at least one row, train or additional, stays in allUsers: *count of
 *     the neighbours is min(k, U - 1).  A user of the fit whose train rows are all removed and who gives no additional row is
 *     not in aug: KNNCF_E_INVALID, like an empty fold-in query.
 *   Row-size class.  The <= 4-rating regime (given-order folding) is decided by the user's row count in aug: train rows minus
 *     removed plus additional.  The surviving train rows come first, in file order; the additional rows come behind them.
 *   An item that leaves aug: the user was its only rater in train, it is removed and not given again.  It is no longer in
 *     ratings.map(_.item).toSet :667, so it is no candidate of the recommendations, whose *count is
 *     min(n, #items of aug - #items the user rates in aug); knncf_revise_predict on it answers the user's mean exactly (no
 *     raters, den = 0), as for any item unknown to aug.
 *   A removed item that other users rate becomes an unrated item of the user: it is a candidate again, and its prediction folds
 *     the neighbours' ratings as for any other item.
 *   Re-rating.  An item may occur in removed_items and among the additional rows of the same query: its train row is replaced.
 *     An additional row on a train item of the user that is NOT removed stays KNNCF_E_DUPLICATE, as does a repeat inside the
 *     additional rows.
 *   Per-query refusals beyond those of knncf_update_*, status KNNCF_E_INVALID: a removed item that the user did not rate in
 *     train (this includes an id unknown to train, and any removal for a user absent from train), and a removed item listed
 *     twice.  knncf_last_error names the query and the reason, like the other per-query failures.
 * Everything else is as knncf_update_* documents it, read on the rows the user has in aug: KNNCF_E_NONFINITE, KNNCF_E_UNSUPPORTED
 * for a negative mean of the user's rows in aug; the cap of 65536 rows, which counts the user's train rows, REMOVED ONES
 * INCLUDED, plus the additional rows, because all of them are seeded; the handle-level return values, the CSR checks (for
 * removed_offsets too), n_queries == 0, untouched rows and counts[b] = 0 for failed queries; the chunk rule with its formula
 *     C = max(1, min(64, budget / (64 * num_users + 96 * num_items), (2^31 - 1) / max(num_users, num_items)))
 * and the split at 32 answerable queries between the two similarity kernels.  The results do not depend on C.  Read-only on
 * the handle: the neighbour table, its build numbers and epoch and what knncf_neighbors_save writes stay as they were.
 * n_removed == 0 (removed_items may then be null) gives the knncf_update_* answer bit for bit: the same code runs.
 * predictor: KNNCF_PRED_KNN as described here, or KNNCF_PRED_PERSONALIZED ("Personalized queries" below) on the same aug. */
int knncf_revise_neighbors(knncf_handle* h, int32_t user, const int32_t* removed_items, int64_t n_removed, const int32_t* items,
                           const double* ratings, int64_t n_ratings, int32_t cap, int32_t* ids, double* sims, int32_t* count);
int knncf_revise_predict(knncf_handle* h, int predictor, int32_t user, const int32_t* removed_items, int64_t n_removed,
                         const int32_t* items, const double* ratings, int64_t n_ratings, const int32_t* pred_items, int64_t m,
                         double* out);
int knncf_revise_recommend(knncf_handle* h, int predictor, int32_t user, const int32_t* removed_items, int64_t n_removed,
                           const int32_t* items, const double* ratings, int64_t n_ratings, int32_t n, int32_t* out_items,
                           double* out_preds, int32_t* count);
int knncf_revise_neighbors_batch(knncf_handle* h, const int32_t* users, const int64_t* removed_offsets, const int32_t* removed_items,
                                 const int64_t* offsets, const int32_t* items, const double* ratings, int64_t n_queries, int32_t cap,
                                 int32_t* ids, double* sims, int32_t* counts, int32_t* statuses);
int knncf_revise_predict_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* removed_offsets,
                               const int32_t* removed_items, const int64_t* offsets, const int32_t* items, const double* ratings,
                               int64_t n_queries, const int64_t* pred_offsets, const int32_t* pred_items, double* out,
                               int32_t* statuses);
int knncf_revise_recommend_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* removed_offsets,
                                 const int32_t* removed_items, const int64_t* offsets, const int32_t* items, const double* ratings,
                                 int64_t n_queries, int32_t n, int32_t* out_items, double* out_preds, int32_t* counts,
                                 int32_t* statuses);

/* ---- Personalized queries: KNNCF_PRED_PERSONALIZED on the query families -----------------------------------------------------
 * knncf_query_predict / _recommend, knncf_update_predict / _recommend, knncf_revise_predict / _recommend and their _batch
 * forms accept predictor == KNNCF_PRED_PERSONALIZED on KNNCF_SIM_COSINE and KNNCF_SIM_JACCARD handles.  With aug exactly as
 * each family defines it above, every result equals, bit for bit, the reference's
 *     predictor(aug, weightedSumDeviation(aug, S))(user, item)   and   recommendations(aug, that predictor)(user, n)
 * with S = adjustedCosineSimilarityFunction(aug) or jaccardCoefficient(aug) (predict/Personalized.scala:61-72,
 * shared/predictions.scala:407-464, :489-585, :651-674) on fresh closures on which only the query user u is ever the first
 * argument.  No neighbourhood cut and no refit.
 *   Terms of a row (u, i).  ALL ratings of i in aug, in aug's file order (:508-524), each adding num = num + dev * s and
 *     den = den + |s| from (0.0, 0.0) — the multiply and the add are separate, no fused multiply-add.  Raters with s == 0 add
 *     +-0 and are not skipped.
 *   The user's own rating is a term.  Unlike KNNCF_PRED_KNN, where getSimilarity(u, u) is 0, S(u, u) is not zero.  Its value is
 *     S(u, u) on aug: for the cosine the left fold from 0.0 of pre(u, j) * pre(u, j) over u's items of aug in u's item-set
 *     order (:418-426: the trie order of the item ids, the given order when u has at most 4 rows in aug) — close to but not
 *     1.0 (1.0000000000000002, 0.9999999999999869, ...); for Jaccard exactly 1.0 (:454-458).
 *   Where the own term sits.  At its place in aug's file order: a surviving train row of a fitted user at its train file
 *     position, with u's deviation ON AUG (the mean changed); an additional row, or any row of a fold-in user, last; a removed
 *     row is no term; a re-rated item has its train row taken out and its additional row at the end.  The position shows in
 *     the last bits of (num, den).
 *   An item that only u rates in aug (unknown to train, given in the additional rows) has exactly one term: num = 0.0 +
 *     dev(u, i) * S(u, u), den = 0.0 + |S(u, u)|.  knncf_*_predict on it therefore does not answer the mean, as KNNCF_PRED_KNN
 *     does there.  An item unknown to aug (an id never seen, or the item that leaves aug under a revise query) answers the
 *     mean exactly, as does an item nobody rates with a non-zero similarity (den > 0 fails :527, the deviation is 0.0).
 *   Train users with 4 or fewer ratings are accepted.  (The fitted KNNCF_PRED_PERSONALIZED refuses them for the adjusted cosine
 *     because a pair's summation order there depends on the call history; here the closures are fresh and u is the first
 *     argument of every pair, so the order is u's, as in the kNN queries.)
 *   The handle's k plays no part: two handles that differ only in k give the same bits.  knncf_update_* with n_ratings == 0
 *     for a fitted user gives the fresh-closure Personalized answer on train itself.
 * Everything else stays as the families document it: per-query statuses, handle-level return values, CSR checks, n_queries ==
 * 0, the cap of 65536 rows, the negative-mean refusal, >= 5 train users, KNNCF_SIM_ONE and shard handles refused, untouched
 * rows of failed queries, the chunk rule C with its formula, the split at 32 answerable queries between the two similarity
 * kernels, and "the results do not depend on C".  Read-only on the handle in the sense of the other families: the neighbour
 * table, its build numbers, its epoch and the knncf_neighbors_save bytes stay as they were.  The first such call after a fit
 * builds the handle's file-order rater copies (20 bytes per train rating, charged to prep_ms as the fitted
 * KNNCF_PRED_PERSONALIZED path charges them; a refit drops them); they and the transposed similarities of a chunk (8 *
 * num_users * the power of two >= C bytes) are allocated beside the chunk budget.  knncf_get_timings: the new fold is charged
 * to predict_ms.  A repeated call of the same shape allocates nothing.
 * Not part of this: knncf_*_explain* with KNNCF_PRED_PERSONALIZED (KNNCF_E_UNSUPPORTED, below), the *_neighbors calls (they
 * have no predictor), every other predictor (KNNCF_E_UNSUPPORTED).  The terms behind these predictions are what
 * knncf_*_explain_personalized* return ("Explanations of Personalized query predictions" below). */

/* ---- Explanations of query predictions: the terms behind knncf_query_predict / knncf_update_predict / knncf_revise_predict ---
 * knncf_explain* above explains a prediction for a user as the fit holds it.  These explain what the three query families
 * predict: for a person whose ratings are not, or no longer, what the fit holds, WITHOUT a refit.  One implementation serves
 * the six calls: a revise query without removals is an update query, an update query for a user absent from train is a
 * fold-in query.
 * Arguments.  The query arguments are exactly those of the matching knncf_*_predict / knncf_*_predict_batch call, the
 * pred_offsets / pred_items CSR included.  Row j of the call is one requested (query, raw item): m rows in the single forms,
 * m = pred_offsets[n_queries] in the batched ones, in the order of pred_items.  order, cap and the outputs are those of
 * knncf_explain_batch: counts[j] = the number of terms of row j (it may exceed cap); the first min(counts[j], cap) terms, in
 * `order`, in row j of raters / sims / devs ([m * cap], row stride cap; the cells beyond them are left untouched);
 * sums[2 j], sums[2 j + 1] = num and den of the fold over ALL terms; predictions[j] = the matching knncf_*_predict answer for
 * that row, bit for bit.  sums and predictions may be null; with cap == 0 the three term arrays may be null.
 * Terms.  With aug as the family defines it, the terms of row (query user u, item i) are the elements of simVal :513-517 on
 * aug — fresh closures, first evaluation u's — whose similarity is non-zero: (rater's raw id, getSimilarity(aug, k, sim)(u,
 * rater), the rater's normalized deviation on i).  KNNCF_EXPLAIN_SUM_ORDER is aug's file order of the item's raters; every
 * term is a train user, so that is train file order.  KNNCF_EXPLAIN_BY_WEIGHT is |similarity| descending, equal magnitudes in
 * summation order.  It follows that the user is never its own term, even when it rates i itself in aug; that a listed
 * neighbour whose similarity is exactly 0.0 is no term; and that an item unknown to train, an item that leaves aug under a
 * revise query and an item no neighbour rated get count 0, sums (0, 0) and the query's mean, exactly, as prediction.
 * Properties, as for knncf_explain: with counts[j] <= cap and KNNCF_EXPLAIN_SUM_ORDER the caller's left fold of the returned
 * terms (num + dev * sim, den + |sim| from (0.0, 0.0), no fused multiply-add) gives sums bit for bit, and the combine :578 of
 * the query's mean with (den > 0 ? num / den : 0.0) gives predictions[j]; the query's mean is the answer for an unknown item.
 * KNNCF_EXPLAIN_BY_WEIGHT returns a permutation of the same terms.
 * Statuses.  Per-query statuses, the handle-level return values, the CSR checks and n_queries == 0 are those of the
 * knncf_*_predict_batch call of the same family; so are the chunk rule C, the split at 32 answerable queries, "read-only on
 * the handle" and "the results do not depend on C".  In addition: KNNCF_E_INVALID for cap < 0, an unknown order, or a needed
 * output pointer that is null; a failed query gets counts[j] = 0 on each of its rows and nothing else of those rows is written;
 * a single call returns the query's status (and has set counts = 0 on every row when that is a per-query refusal).
 * Row sub-ranges inside a chunk.  The term scratch of one launch holds
 *     R = max(1, budget / (20 * cap + 28))
 *     budget = workspace_bytes / 2 if workspace_bytes > 0, else min(48 GiB, free device memory / 4)
 * rows (the budget of the other batched calls).  A chunk with more requested rows runs the explain kernel over consecutive
 * sub-ranges of R rows; the chunk's fold results stay in place between the launches.  The results do not depend on R, and a
 * call on a handle that has answered the same shape before allocates no device memory.
 * OUT OF SCOPE here as above: KNNCF_PRED_PERSONALIZED explanations (KNNCF_E_UNSUPPORTED, as the explain calls answer for any
 * predictor but KNNCF_PRED_KNN), sharded explanations (a shard handle: KNNCF_E_UNSUPPORTED), and a fused "recommend and
 * explain in one pass" call: explain the items knncf_*_recommend returned with a second call.  (Users as the fit holds them have
 * knncf_explain_personalized* above for KNNCF_PRED_PERSONALIZED; the query families have knncf_*_explain_personalized* below,
 * "Explanations of Personalized query predictions".)  That fused call has entry points of its own, which leave these calls
 * as they are: knncf_*_recommend_explain* ("Recommendations with their explanations" below). */
int knncf_query_explain(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings,
                        const int32_t* pred_items, int64_t m, int32_t order, int32_t cap, int32_t* raters, double* sims, double* devs,
                        int32_t* counts, double* sums, double* predictions);
int knncf_update_explain(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings,
                         const int32_t* pred_items, int64_t m, int32_t order, int32_t cap, int32_t* raters, double* sims, double* devs,
                         int32_t* counts, double* sums, double* predictions);
int knncf_revise_explain(knncf_handle* h, int predictor, int32_t user, const int32_t* removed_items, int64_t n_removed,
                         const int32_t* items, const double* ratings, int64_t n_ratings, const int32_t* pred_items, int64_t m,
                         int32_t order, int32_t cap, int32_t* raters, double* sims, double* devs, int32_t* counts, double* sums,
                         double* predictions);
int knncf_query_explain_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets, const int32_t* items,
                              const double* ratings, int64_t n_queries, const int64_t* pred_offsets, const int32_t* pred_items,
                              int32_t order, int32_t cap, int32_t* raters, double* sims, double* devs, int32_t* counts, double* sums,
                              double* predictions, int32_t* statuses);
int knncf_update_explain_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets, const int32_t* items,
                               const double* ratings, int64_t n_queries, const int64_t* pred_offsets, const int32_t* pred_items,
                               int32_t order, int32_t cap, int32_t* raters, double* sims, double* devs, int32_t* counts, double* sums,
                               double* predictions, int32_t* statuses);
int knncf_revise_explain_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* removed_offsets,
                               const int32_t* removed_items, const int64_t* offsets, const int32_t* items, const double* ratings,
                               int64_t n_queries, const int64_t* pred_offsets, const int32_t* pred_items, int32_t order, int32_t cap,
                               int32_t* raters, double* sims, double* devs, int32_t* counts, double* sums, double* predictions,
                               int32_t* statuses);

/* ---- Explanations of Personalized query predictions: the terms behind KNNCF_PRED_PERSONALIZED on the query families -----------
 * knncf_query_predict / knncf_update_predict / knncf_revise_predict with predictor == KNNCF_PRED_PERSONALIZED ("Personalized
 * queries" above) fold every rating of the item in aug.  These six calls answer "which few users carried this prediction" for
 * them, as knncf_explain_personalized* does for users as the fit holds them.  NEW CALLS, NOT A LIFTED REFUSAL:
 * knncf_*_explain* above keep answering KNNCF_E_UNSUPPORTED for KNNCF_PRED_PERSONALIZED.
 * Arguments.  Exactly those of the matching knncf_*_explain / knncf_*_explain_batch call without `int predictor`
 * (knncf_explain_personalized* has none either): the query, the requested items (m of them, or the pred_offsets / pred_items
 * CSR), order, cap and the outputs.  Row j of the call is one requested (query, raw item).
 * Terms of row (u, i).  With aug exactly as each family defines it and S = adjustedCosineSimilarityFunction(aug) or
 * jaccardCoefficient(aug) on fresh closures whose first argument is only ever the query user u: the elements of simVal
 * shared/predictions.scala:513-517 on aug whose similarity is not exactly 0.0, over ALL ratings of i in aug, in aug's file order,
 * each (the rater's raw id, S(u, rater), the rater's normalized deviation on i).
 * THE USER IS ITS OWN TERM when it rates i in aug, as in the Personalized query predictions: weight S(u, u) on aug (for the
 * cosine close to but not 1.0, for Jaccard exactly 1.0), u's deviation ON AUG, rater id = the query's `user`.  Its place follows
 * the row it comes from: a surviving train row stands at its train file place; an additional row stands last, after every train
 * row, and so does any row of a fold-in user and a re-rated item; a removed row is no term.
 * Orders.  KNNCF_EXPLAIN_SUM_ORDER is that file order.  KNNCF_EXPLAIN_BY_WEIGHT is |similarity| descending, equal magnitudes in
 * summation order; when cap cuts through a group of equal magnitudes, the earliest in summation order are kept.
 * Outputs.  counts[j] = the number of terms (it may exceed cap); the first min(counts[j], cap) terms, in `order`, in row j of
 * raters / sims / devs (row stride cap; cells beyond the terms are left untouched).  sums and predictions may be null; with
 * cap == 0 the three term arrays may be null.  sums[2 j], sums[2 j + 1] = num and den of the fold :520-524 over all of the
 * item's ratings in aug, independent of order and cap.  With counts[j] <= cap and KNNCF_EXPLAIN_SUM_ORDER the caller's left fold
 * of the returned terms, (num + dev * sim, den + |sim|) from (0.0, 0.0) with the multiply and the add separate (no fused
 * multiply-add), gives sums bit for bit: the raters that are no terms add +-0.0 to sums that start at +0.0.  The combine :578
 * of the query's mean with (den > 0 ? num / den : 0.0) gives predictions[j], which equals the matching
 * knncf_*_predict(..., KNNCF_PRED_PERSONALIZED, ...) answer bit for bit.
 * Row kinds.  An item unknown to aug (an id never seen, or the item that leaves aug under a revise query): count 0, sums
 * (0, 0), the query's mean exactly.  An item only u rates in aug (an additional item unknown to train, or the re-rated lone
 * item): exactly one term, u's own.  A query with S(u, u) == 0.0 (the cosine with every deviation zero, e.g. a one-rating
 * fold-in user): count 0 on every row and the mean as every prediction.  An item whose raters all have similarity 0.0: count 0
 * and the mean.
 * Everything else is as "Personalized queries" documents it: per-query statuses and handle-level return values, the CSR checks,
 * n_queries == 0, the cap of 65536 rows, the negative-mean refusal, >= 5 train users, KNNCF_SIM_ONE and shard handles refused,
 * train users with 4 or fewer ratings accepted, the handle's k without a part, the chunk rule C, the split at 32 answerable
 * queries between the two similarity kernels, and "the results do not depend on C".  In addition, as knncf_*_explain*:
 * KNNCF_E_INVALID for cap < 0, an unknown order, or a needed output pointer that is null; a failed query gets counts[j] = 0 on
 * each of its rows and nothing else of those rows is written; a single call returns the query's status.
 * Row sub-ranges inside a chunk.  The explain kernel runs over consecutive sub-ranges of
 *     R = max(1, budget / (40 * cap + 28))
 *     budget = workspace_bytes / 2 if workspace_bytes > 0, else min(48 GiB, free device memory / 4)
 * rows (the budget of the other batched calls; the formula of knncf_explain_personalized*: 20 * cap + 28 bytes of outputs per
 * row, which come back in one copy, and 20 * cap bytes in which KNNCF_EXPLAIN_BY_WEIGHT stages the selected terms before it
 * ranks them).  The chunk's fold results stay in place between the launches.  The results do not depend on R, and a call on a
 * handle that has answered the same shape before allocates no device memory.
 * Handle state.  Read-only in the sense of the other families: the neighbour table, its build numbers, its epoch and the
 * knncf_neighbors_save bytes stay as they were.  The first call after a fit builds the handle's file-order rater copies
 * (prep_ms); knncf_get_timings: the fold and the explain kernel are charged to predict_ms.
 * OUT OF SCOPE: a device-pointer form, shard handles, KNNCF_SIM_ONE, a fused "recommend and explain in one pass" call, and the
 * command-line tool.  The fused call has entry points of its own, which take KNNCF_PRED_PERSONALIZED as well:
 * knncf_*_recommend_explain* ("Recommendations with their explanations" below). */
int knncf_query_explain_personalized(knncf_handle* h, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings,
                                     const int32_t* pred_items, int64_t m, int32_t order, int32_t cap, int32_t* raters, double* sims,
                                     double* devs, int32_t* counts, double* sums, double* predictions);
int knncf_update_explain_personalized(knncf_handle* h, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings,
                                      const int32_t* pred_items, int64_t m, int32_t order, int32_t cap, int32_t* raters, double* sims,
                                      double* devs, int32_t* counts, double* sums, double* predictions);
int knncf_revise_explain_personalized(knncf_handle* h, int32_t user, const int32_t* removed_items, int64_t n_removed,
                                      const int32_t* items, const double* ratings, int64_t n_ratings, const int32_t* pred_items,
                                      int64_t m, int32_t order, int32_t cap, int32_t* raters, double* sims, double* devs,
                                      int32_t* counts, double* sums, double* predictions);
int knncf_query_explain_personalized_batch(knncf_handle* h, const int32_t* users, const int64_t* offsets, const int32_t* items,
                                           const double* ratings, int64_t n_queries, const int64_t* pred_offsets,
                                           const int32_t* pred_items, int32_t order, int32_t cap, int32_t* raters, double* sims,
                                           double* devs, int32_t* counts, double* sums, double* predictions, int32_t* statuses);
int knncf_update_explain_personalized_batch(knncf_handle* h, const int32_t* users, const int64_t* offsets, const int32_t* items,
                                            const double* ratings, int64_t n_queries, const int64_t* pred_offsets,
                                            const int32_t* pred_items, int32_t order, int32_t cap, int32_t* raters, double* sims,
                                            double* devs, int32_t* counts, double* sums, double* predictions, int32_t* statuses);
int knncf_revise_explain_personalized_batch(knncf_handle* h, const int32_t* users, const int64_t* removed_offsets,
                                            const int32_t* removed_items, const int64_t* offsets, const int32_t* items,
                                            const double* ratings, int64_t n_queries, const int64_t* pred_offsets,
                                            const int32_t* pred_items, int32_t order, int32_t cap, int32_t* raters, double* sims,
                                            double* devs, int32_t* counts, double* sums, double* predictions, int32_t* statuses);

/* ---- Recommendations with their explanations: the top n of a query and the terms behind each, in one pass over the fit -------
 * A serving layer wants both together: n recommended items, each with the few users that carried its prediction.
 * knncf_*_recommend followed by knncf_*_explain* on the returned items repeats the upload, the similarity pass over every train
 * row, the top-k selection and the fold.  These six calls run the explain kernel over the rows the selection just produced: one
 * implementation, three families, single and batched.  NEW CALLS: no refusal of the explain calls above is lifted.
 * Arguments.  Those of the matching knncf_*_recommend / knncf_*_recommend_batch call up to n, then order and cap as the explain
 * calls take them, the recommend outputs, and the explain outputs without a predictions array.  predictor is KNNCF_PRED_KNN or
 * KNNCF_PRED_PERSONALIZED, as the recommend calls accept them.
 * Recommendation outputs.  out_items / out_preds ([n_queries * n], row stride n), counts[b] and statuses[b] are exactly what
 * knncf_*_recommend_batch writes for the same arguments, bit for bit: the cells past counts[b] are untouched, a refused query
 * gets counts[b] = 0 and its row is untouched, and the return values are the same.
 * Explanation rows.  Row (b, j) with j < counts[b] is explain row r = b * n + j.  It receives term_counts[r], sums[2 r] and
 * sums[2 r + 1], and the first min(term_counts[r], cap) terms in `order` at raters / sims / devs [r * cap ..]: each of these is
 * what the matching explain call — knncf_*_explain_batch for KNNCF_PRED_KNN, knncf_*_explain_personalized_batch for
 * KNNCF_PRED_PERSONALIZED — writes for that query with pred_items = its recommended items.  The row's cells past its terms are
 * untouched.  Every explain cell of a row j >= counts[b] is untouched; that includes every row of a refused query.
 * NO PREDICTIONS ARRAY: out_preds[r] already is the explained prediction — the selection and the explain kernels read the same
 * prediction cell of the chunk.
 * Term properties.  Those of "Explanations of query predictions" and "Explanations of Personalized query predictions" above hold
 * row for row and are not restated here: the caller's left fold of the returned terms gives sums, the combine :578 of the
 * query's mean with them gives out_preds[r], the user is its own term under KNNCF_PRED_PERSONALIZED and never under
 * KNNCF_PRED_KNN, and KNNCF_EXPLAIN_BY_WEIGHT orders equal magnitudes in summation order.
 * Statuses.  Per-query statuses, the handle-level refusals (before a fit, KNNCF_SIM_ONE, a shard handle, fewer than 5 train
 * users, any other predictor), the CSR checks and n_queries == 0 are those of knncf_*_recommend_batch.  In addition
 * KNNCF_E_INVALID for cap < 0 and for an unknown order, as in the explain calls, for a null term_counts with n > 0, and for a
 * null raters / sims / devs with n > 0 and cap > 0.  sums may be null.  n == 0 is KNNCF_OK with counts[b] = 0.  A call that
 * fails these checks writes nothing, except that a single form has set *count = 0, as knncf_*_recommend does.  A single form
 * returns the query's status.
 * Chunks.  The chunk rule C is that of the families ("Batched fold-in queries").  Inside a chunk the explain kernel runs over
 * consecutive sub-ranges of R rows of the chunk's recommended rows (slot after slot, j ascending), by the existing rules:
 *     R = max(1, budget / (20 * cap + 28))   for KNNCF_PRED_KNN
 *     R = max(1, budget / (40 * cap + 28))   for KNNCF_PRED_PERSONALIZED
 *     budget = workspace_bytes / 2 if workspace_bytes > 0, else min(48 GiB, free device memory / 4)
 * The rows are formed on the device from the selection's cells, so there is no host round trip between the selection and the
 * first explain launch; a chunk whose rows fit in R has one stream synchronisation after the similarity stage, a chunk with
 * more rows one per sub-range.  The results depend on neither C nor R, and a call on a handle that has answered the same shape
 * before allocates no device memory.
 * Handle state.  Read-only in the sense of the other families: the neighbour table, its build numbers, its epoch and the
 * knncf_neighbors_save bytes stay as they were.  With KNNCF_PRED_PERSONALIZED the first call after a fit builds the handle's
 * file-order rater copies (prep_ms); knncf_get_timings: everything else is charged to predict_ms.
 * OUT OF SCOPE: a fused call for users as the fit holds them (their neighbour lists are memoised: knncf_recommend_batch then
 * knncf_explain_batch repeats no pass), device-pointer forms, shard handles, KNNCF_SIM_ONE, returning the neighbour list from
 * the same pass, and the command-line tool. */
int knncf_query_recommend_explain(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings,
                                  int64_t n_ratings, int32_t n, int32_t order, int32_t cap, int32_t* out_items, double* out_preds,
                                  int32_t* count, int32_t* raters, double* sims, double* devs, int32_t* term_counts, double* sums);
int knncf_update_recommend_explain(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings,
                                   int64_t n_ratings, int32_t n, int32_t order, int32_t cap, int32_t* out_items, double* out_preds,
                                   int32_t* count, int32_t* raters, double* sims, double* devs, int32_t* term_counts, double* sums);
int knncf_revise_recommend_explain(knncf_handle* h, int predictor, int32_t user, const int32_t* removed_items, int64_t n_removed,
                                   const int32_t* items, const double* ratings, int64_t n_ratings, int32_t n, int32_t order,
                                   int32_t cap, int32_t* out_items, double* out_preds, int32_t* count, int32_t* raters, double* sims,
                                   double* devs, int32_t* term_counts, double* sums);
int knncf_query_recommend_explain_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets,
                                        const int32_t* items, const double* ratings, int64_t n_queries, int32_t n, int32_t order,
                                        int32_t cap, int32_t* out_items, double* out_preds, int32_t* counts, int32_t* raters,
                                        double* sims, double* devs, int32_t* term_counts, double* sums, int32_t* statuses);
int knncf_update_recommend_explain_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets,
                                         const int32_t* items, const double* ratings, int64_t n_queries, int32_t n, int32_t order,
                                         int32_t cap, int32_t* out_items, double* out_preds, int32_t* counts, int32_t* raters,
                                         double* sims, double* devs, int32_t* term_counts, double* sums, int32_t* statuses);
int knncf_revise_recommend_explain_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* removed_offsets,
                                         const int32_t* removed_items, const int64_t* offsets, const int32_t* items,
                                         const double* ratings, int64_t n_queries, int32_t n, int32_t order, int32_t cap,
                                         int32_t* out_items, double* out_preds, int32_t* counts, int32_t* raters, double* sims,
                                         double* devs, int32_t* term_counts, double* sums, int32_t* statuses);

/* ---- Bystander queries: a FITTED user's kNN answers once a newcomer has joined the data --------------------------------------
 * recommend/Recommender.scala:68-89 asks two things of aug = data.union(personal): the newcomer's top n (knncf_query_recommend)
 * and predictor(aug, ...)(1, 1), the prediction of a user who was in the data all along.  The newcomer is one more candidate of
 * that user's neighbour list, one more rater (the last in file order) of every item it rated, and it shifts average(aug).  These
 * calls answer for such bystanders WITHOUT a refit.
 * A query is a fold-in query exactly as above: a raw id `user` absent from train with rows (items[j], ratings[j]), and aug =
 * train ++ those rows in order.  A ROW of the query names a bystander, a raw user id others[r] != user, and in the predict forms
 * a raw item pred_items[r].  Every row is answered on closures of its own over aug whose first evaluation is the row's, bit for
 * bit:
 *   knncf_query_bystander_neighbors  getNeighbors(aug, k, sim)(others[r]) :596-617 into row r of ids / sims (row stride cap): raw
 *                                    ids, the newcomer's own id where it is a neighbour; counts[r] = the list's length, which may
 *                                    exceed cap: min(k, U) for a user of the fit (U - 1 train users and the newcomer), and for a
 *                                    user unknown to aug the first min(k, U + 1) users of aug in set order with similarity +0.0,
 *                                    as knncf_neighbors answers on train.  Cells past the written entries are untouched.
 *   knncf_query_bystander_predict    out[r] = predictor(aug, weightedSumDeviation(aug, getSimilarity(aug, k, sim)))(others[r],
 *                                    pred_items[r]) :489-585 for any item id.  A bystander unknown to aug or with a negative
 *                                    mean gets average(aug) :573: the fit's running total of the train ratings in file order,
 *                                    continued over the query's ratings in the given order, divided by n + n_ratings.
 * The bystander owns every pair: S(v, x) folds the common items in v's item-set order (file order for a v of <= 4 ratings),
 * also for x = the newcomer.  Rows are independent; the same bystander may occur many times.
 * Batch forms.  Query b is (users[b], items / ratings [offsets[b], offsets[b + 1])) as in "Batched fold-in queries"; its rows
 * are others / pred_items [row_offsets[b], row_offsets[b + 1]) (row_offsets: a CSR like pred_offsets, fewer than 2^31 rows), and
 * ids / sims / counts / out are indexed by row.  The single forms are the batch of one query and return the query's status.
 * Statuses.  Per-query statuses and the return values are those of knncf_query_predict_batch, and in addition a query with a
 * row whose others[r] == users[b] gets KNNCF_E_INVALID (ask knncf_query_predict), a query with a bystander of more than 65536
 * train ratings KNNCF_E_UNSUPPORTED.  predictor must be KNNCF_PRED_KNN (KNNCF_E_UNSUPPORTED otherwise).  KNNCF_E_INVALID for
 * cap < 0.  A failed query leaves its rows of out / ids / sims untouched and gets counts = 0 on its rows.  n_queries == 0, or a
 * query without rows, is fine and writes nothing (the query still gets its status).
 * Chunks.  The unit is a SLOT.  An answerable query takes one slot for its own prepared row, plus one per distinct bystander that
 * is known to train and — in the predict forms — whose mean is not negative; the other bystanders need none.
 *     C = max(2, min(64, budget / (64 * num_users + 96 * num_items), (2^31 - 1) / max(num_users, num_items)))
 *     budget = workspace_bytes / 2 if workspace_bytes > 0, else min(48 GiB, free device memory / 4)
 * Queries are packed into chunks of C slots in order; a query with more bystanders than fit beside its own slot continues in the
 * next chunk, where its row is prepared again.  (The gathered neighbour ratings are allocated beside the budget, as in "Batched
 * fold-in queries".)  The results do not depend on C, and a call on a handle that has answered the same shape before allocates
 * no device memory.
 * Handle state.  Read-only in the sense of the other families: the neighbour table, its build numbers, its epoch and the
 * knncf_neighbors_save bytes stay as they were.  knncf_get_timings: charged as the fold-in calls charge theirs.
 * OUT OF SCOPE: a `user` that is in the fit (update queries: "Bystanders of update queries" below; revise queries:
 * "Bystanders of revise queries" below); KNNCF_PRED_PERSONALIZED and the other predictors;
 * recommendations and explanations for a bystander; device-pointer forms; shard handles and knncf_group_*.  ("Which fitted
 * users does the newcomer enter" is knncf_query_entered, below.) */
int knncf_query_bystander_neighbors(knncf_handle* h, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings,
                                    const int32_t* others, int64_t m, int32_t cap, int32_t* ids, double* sims, int32_t* counts);
int knncf_query_bystander_predict(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings,
                                  int64_t n_ratings, const int32_t* others, const int32_t* pred_items, int64_t m, double* out);
int knncf_query_bystander_neighbors_batch(knncf_handle* h, const int32_t* users, const int64_t* offsets, const int32_t* items,
                                          const double* ratings, int64_t n_queries, const int64_t* row_offsets, const int32_t* others,
                                          int32_t cap, int32_t* ids, double* sims, int32_t* counts, int32_t* statuses);
int knncf_query_bystander_predict_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets,
                                        const int32_t* items, const double* ratings, int64_t n_queries, const int64_t* row_offsets,
                                        const int32_t* others, const int32_t* pred_items, double* out, int32_t* statuses);

/* ---- Bystanders of update queries: a FITTED user's kNN answers once another user, fitted or not, has added ratings ------------
 * Most ratings come from users the fit knows.  When fitted user c rates more items its mean moves, and with it every deviation
 * and the norm: every S(v, c) changes, c can climb, sink, enter or leave the list of any other user v, and the terms c gives
 * to v's folds change on the items it rated long ago too.  These calls answer for such v WITHOUT a refit.
 * A query is an update query exactly as knncf_update_* defines it: any raw id `user` with ADDITIONAL rows (items[j],
 * ratings[j]), aug = train ++ those rows in order.  A ROW names a bystander others[r] != user, the predict forms a raw item
 * pred_items[r] beside it.  Every row is answered on closures of its own over aug whose first evaluation is the row's — the
 * bystander owns every pair — bit for bit:
 *   knncf_update_bystander_neighbors  getNeighbors(aug, k, sim)(others[r]) :596-617: raw ids, row stride cap, counts[r] = the
 *                                     list's length (may exceed cap), cells past the written ones untouched.  A fitted `user`
 *                                     is an ordinary train candidate at its place in set order: min(k, U - 1) for a fitted
 *                                     bystander; for a bystander unknown to aug the first min(k, |users(aug)|) users of aug
 *                                     in set order with +0.0, |users(aug)| = U for a fitted `user`, U + 1 otherwise.
 *   knncf_update_bystander_predict    predictor(aug, weightedSumDeviation(aug, getSimilarity(aug, k, sim)))(others[r],
 *                                     pred_items[r]) :489-585 for any item id; a bystander unknown to aug or with a negative
 *                                     mean gets average(aug) :573, the fit's running total continued over the additional
 *                                     ratings in the given order, over n + n_ratings.
 * What a fitted changer c does to bystander v:
 *   S(v, c) on aug, owned by v: the left fold from 0.0 of pre_v(i) * pre_c^aug(i) over the common items in v's item-set order
 *     (ascending dense item for a v of more than 4 train ratings, else v's file order); Jaccard |I(v) & I(c)| / (|I(v)| +
 *     |I(c)| - |I(v) & I(c)|) with |I(c)| counting all of c's items on aug.  Every other S(v, x) is the train value.
 *   The list: that value replaces the train value in v's similarity row before the list is cut.  c keeps its place in set
 *     order; a c that leaves a full list is replaced by the next candidate.
 *   The fold: where c is in v's list its terms carry its deviations on aug and the list's similarity; a train row of c stays
 *     at its train file row, an additional row comes behind every train row in the given order.
 *   An item unknown to train that c rates in an additional row has exactly one rater in aug: the one-term fold 0.0 + dev_c(i) *
 *     S(v, c) over 0.0 + |S(v, c)| where c is in v's list, v's mean exactly otherwise.
 * A `user` absent from train is the fold-in case: the answers are knncf_query_bystander_*'s bit for bit, except that an empty
 * query is KNNCF_E_INVALID as in knncf_update_*.  n_ratings == 0 for a fitted `user` is valid and aug is train: every row is then
 * knncf_update_neighbors / knncf_update_predict of the bystander without rows.  Users of 4 or fewer ratings are accepted on both
 * sides and both similarities: the closures are fresh.
 * Batch forms, outputs, untouched rows: those of knncf_query_bystander_*.  A failed query gets counts = 0 on its rows.
 * Per-query statuses: those of knncf_update_predict_batch (KNNCF_E_DUPLICATE, also against the user's train items;
 * KNNCF_E_NONFINITE; KNNCF_E_UNSUPPORTED for a negative mean of the combined rows or more than 65536 of them; KNNCF_E_INVALID for
 * an empty query of an absent user), and KNNCF_E_INVALID for a row with others[r] == users[b], KNNCF_E_UNSUPPORTED for a
 * bystander of more than 65536 train ratings.  Refusals of the handle: those of knncf_query_bystander_*_batch.
 * Chunks: the slots and C of "Bystander queries".  The changer's own slot is an update slot (its train rows seeded, then the
 * additional rows), each distinct bystander that needs the device takes an update slot without rows; a query with more
 * bystanders than fit beside its own slot continues in the next chunk, where its row is prepared again.  A chunk may mix fitted
 * changers and newcomers.  Results do not depend on C; a repeated call of the same shape allocates no device memory.
 * Handle state: read-only, as "Bystander queries".  knncf_get_timings: charged as the fold-in calls charge theirs.
 * OUT OF SCOPE: removals (bystanders of revise queries: "Bystanders of revise queries" below); the entered question for update
 * queries is served by knncf_update_entered* ("Entered queries of update
 * queries" below), which rebuilds a user's full row through these calls only where the stored list cannot decide;
 * KNNCF_PRED_PERSONALIZED and the other predictors; recommendations and explanations for a bystander; device-pointer forms; shard
 * handles and knncf_group_*; the command-line tool. */
int knncf_update_bystander_neighbors(knncf_handle* h, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings,
                                     const int32_t* others, int64_t m, int32_t cap, int32_t* ids, double* sims, int32_t* counts);
int knncf_update_bystander_predict(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings,
                                   int64_t n_ratings, const int32_t* others, const int32_t* pred_items, int64_t m, double* out);
int knncf_update_bystander_neighbors_batch(knncf_handle* h, const int32_t* users, const int64_t* offsets, const int32_t* items,
                                           const double* ratings, int64_t n_queries, const int64_t* row_offsets, const int32_t* others,
                                           int32_t cap, int32_t* ids, double* sims, int32_t* counts, int32_t* statuses);
int knncf_update_bystander_predict_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets,
                                         const int32_t* items, const double* ratings, int64_t n_queries, const int64_t* row_offsets,
                                         const int32_t* others, const int32_t* pred_items, double* out, int32_t* statuses);

/* ---- Bystanders of revise queries: a FITTED user's kNN answers once another user has removed or re-rated items ---------------
 * A user of the fit who deletes a rating, or rates an item again, changes its mean, its deviations and its norm like one who
 * adds ratings — and takes terms OUT of other users' folds.  These calls are knncf_update_bystander_* for such a user WITHOUT a
 * refit; the argument lists are those calls' with the removals in front of the additional rows, where knncf_revise_* puts them.
 * A query is a revise query exactly as knncf_revise_* defines it: any raw id `user`, the train items it takes out
 * (removed_items), its additional rows (items[j], ratings[j]);
 *     aug = train without the removed rows of `user`, in file order, ++ the additional rows in order.
 * A ROW names a bystander others[r] != user, the predict forms a raw item beside it.  Every row is answered on closures of its
 * own over aug whose first evaluation is the row's — the bystander owns every pair — bit for bit: getNeighbors(aug, k,
 * sim)(others[r]) and the kNN predictor, as "Bystanders of update queries" describes them.  Row outputs, counts, untouched cells,
 * slots and chunks (a revise query that continues in the next chunk has its revise row prepared again), per-query and
 * handle-level statuses, read-only handle state and timings: everything knncf_update_bystander_* documents holds unchanged.
 * What a fitted changer c with removals does to bystander v:
 *   S(v, c) and the list: as for an update query, with c's row on aug (live train rows in file order, then the additional
 *     rows).  c stays a user of aug: the list lengths are those of the update case.
 *   The fold: c's term on an item stands where c's row of that item stands in aug's file order.  A live train row stays at
 *     its train file row with the deviation on aug; a removed row is no term; a re-rated item has its train row gone and its
 *     additional row behind every train row.
 *   An item that leaves aug (c was its only train rater, removed it and did not give it again) has no rater: the prediction
 *     is the bystander's mean exactly, as for an item unknown to aug.  A lone item that c re-rates has exactly one rater, the
 *     last of aug: the one-term fold where c is in v's list, v's mean otherwise.
 *   average(aug), the answer for a bystander unknown to aug or with a negative mean: the left fold from 0.0 of the SURVIVING
 *     train ratings in file order, continued over the additional ratings in the given order, over n - n_removed + n_ratings.
 *     It is no continuation of the fit's running total.  On a fit whose ratings are all dyadic (multiples of 1/16: every
 *     MovieLens file) every partial sum is exact and the surviving fold is the total minus the removed ratings; on any other
 *     fit a predict call folds the file again on the device — one dependent chain over the n train ratings, what the fit's own
 *     sequential sum costs — once per query that has removals AND a row answered with the average.
 * Per-query statuses: those of knncf_update_bystander_*, and the refusals of knncf_revise_* on top — KNNCF_E_INVALID for a
 * removed item the user did not rate in train, a removed item listed twice, any removal for a user absent from train, and a
 * fitted user left without a row; the 65536-row cap counts the removed rows too.  KNNCF_E_INVALID for n_removed < 0, null
 * removed items with n_removed > 0, and removed_offsets that are null, do not start at 0 or decrease.
 * n_removed == 0 in every query of a call gives the knncf_update_bystander_* answer bit for bit through the same code.
 * KNNCF_DEBUG_TRACE_DISPATCH prints, after the `bystander` line of a chunk that holds a changer with removals,
 *     knncf-dispatch bystander-revise slots=<such changer slots> removed=<their removed items> refold=<sequential folds>
 * OUT OF SCOPE: removals in knncf_append (knncf_amend takes them; the entered question for revise queries is served by
 * knncf_revise_entered*: "Entered queries of revise queries" below); prefix checkpoints
 * that would shorten the sequential fold; KNNCF_PRED_PERSONALIZED and the other predictors; device-pointer forms; shard handles
 * and knncf_group_*; the command-line tool. */
int knncf_revise_bystander_neighbors(knncf_handle* h, int32_t user, const int32_t* removed_items, int64_t n_removed,
                                     const int32_t* items, const double* ratings, int64_t n_ratings, const int32_t* others, int64_t m,
                                     int32_t cap, int32_t* ids, double* sims, int32_t* counts);
int knncf_revise_bystander_predict(knncf_handle* h, int predictor, int32_t user, const int32_t* removed_items, int64_t n_removed,
                                   const int32_t* items, const double* ratings, int64_t n_ratings, const int32_t* others,
                                   const int32_t* pred_items, int64_t m, double* out);
int knncf_revise_bystander_neighbors_batch(knncf_handle* h, const int32_t* users, const int64_t* removed_offsets,
                                           const int32_t* removed_items, const int64_t* offsets, const int32_t* items,
                                           const double* ratings, int64_t n_queries, const int64_t* row_offsets, const int32_t* others,
                                           int32_t cap, int32_t* ids, double* sims, int32_t* counts, int32_t* statuses);
int knncf_revise_bystander_predict_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* removed_offsets,
                                         const int32_t* removed_items, const int64_t* offsets, const int32_t* items,
                                         const double* ratings, int64_t n_queries, const int64_t* row_offsets, const int32_t* others,
                                         const int32_t* pred_items, double* out, int32_t* statuses);

/* ---- Entered queries: which fitted users' neighbour lists a newcomer joins ---------------------------------------------------
 * Under KNNCF_PRED_KNN a fitted user v's predictions change when a newcomer joins only if the newcomer enters
 * getNeighbors(aug, k, sim)(v) (the shift of average(aug) matters only to users who are answered with it).  These calls name
 * those v in one pass over the fit, where knncf_query_bystander_neighbors would take one slot per fitted user.
 * A query is a fold-in query exactly as knncf_query_neighbors_batch defines it: the raw id users[b] is absent from train, its rows
 * are the CSR offsets / items / ratings, and aug_b = train ++ those rows in order.  Queries are independent.
 * Which users are reported.  Fitted user v is ENTERED by query b iff users[b] occurs in getNeighbors(aug_b, k, sim)(v) :596-617,
 * the list evaluated on closures of v's own, so that v owns every pair.  For every accepted handle this equals, bit for bit,
 * "users[b] occurs in the row that knncf_query_bystander_neighbors answers for (query b, v) with cap = k".
 * Outputs.  Row b of out_users / out_sims / out_pos / out_displaced ([n_queries * cap], row stride cap) receives the first
 * min(counts[b], cap) entered users of query b in the fit's user set order (dense order, the order allUsers iterates).  counts[b]
 * is the number of entered users and may exceed cap.  Cells past the written ones are untouched.  With cap == 0 the four arrays
 * may be null: a count-only call.  Per entered user v:
 *   out_users      the raw id of v
 *   out_sims       S(v, q) as it stands in v's list — the cell knncf_query_bystander_neighbors writes, the bits of a +-0.0
 *                  included.  Adjusted cosine: the left fold from 0.0 of pre(v, i) * pre(q, i) over the common items in dense-item
 *                  order, multiply and add separate.  Jaccard: |I(v) & I(q)| / (|I(v)| + |I(q)| - |I(v) & I(q)|), |I(q)| with q's
 *                  items unknown to train.
 *   out_pos        the 0-based position of q in v's list on aug_b
 *   out_displaced  the raw id that is in getNeighbors(train, k, sim)(v) and no longer in the list on aug_b: the last entry of a
 *                  full list; -1 when the list grew (k >= num_users, where every fitted user is entered)
 * Place rule.  An entry (x, s_x) of v's stored list goes before q iff its order key is smaller (similarity descending, -0.0 with
 * +0.0), or the keys are equal and x comes before q in the set order of aug's users (q's rank: the lower bound of its trie key
 * over the fit's user keys).  q is entered iff fewer than take = min(k, num_users) entries go before it.  A fitted user with a
 * negative mean is reported like any other: getNeighbors does not look at the mean.
 * Refusals of the handle: those of knncf_query_neighbors_batch — KNNCF_E_STATE before a fit; KNNCF_E_UNSUPPORTED for
 * KNNCF_SIM_ONE, a shard handle, fewer than 5 train users; KNNCF_E_INVALID for null pointers, n_queries < 0, cap < 0, bad CSR
 * offsets; n_queries == 0 is KNNCF_OK and touches nothing — and one more: KNNCF_E_UNSUPPORTED on a KNNCF_SIM_COSINE handle whose
 * train set has a user with 4 or fewer ratings (there a pair's summation order depends on who owns it, SURVEY N6, and the stored
 * lists are not the fresh-closure lists).  Jaccard handles are accepted with such users: a ratio of counts has no order.
 * Per-query statuses: exactly those of knncf_query_neighbors_batch (the user occurs in train or the query is empty, a duplicate
 * item, a non-finite deviation, a negative mean, more than 65536 ratings).  A failed query gets counts[b] = 0, its rows are
 * untouched, and it does not disturb the others; knncf_last_error names the first failed query.  The single form is the batch of
 * one and returns the query's status; it has set *count = 0 first, once the argument checks pass.
 * Handle state.  NOT read-only.  Let M be the train users whose neighbourhood the handle has not built, in ascending raw id.
 * When the call passes its handle-level checks, n_queries > 0 and M is not empty, it first builds them in ONE batch and LEAVES
 * THE HANDLE IN THE STATE THAT knncf_neighbors_batch OVER M LEAVES IT IN: the same lists, the same build numbers (call, position
 * in M), the same knncf_neighbors_save file — whether or not any query is answerable.  With M empty the call touches nothing.
 * knncf_get_timings: the build is charged as knncf_neighbors_batch charges it, the rest as the fold-in calls charge theirs.
 * Chunks.  C of "Batched fold-in queries", one slot per query.  The entered-list scratch (20 bytes * min(cap, num_users) + 4 per
 * slot, at most 20 bytes * num_users) is allocated beside the budget, as the gathered ratings are.  The results do not depend on
 * C, and a repeated call of the same shape allocates no device memory.
 * OUT OF SCOPE: newcomers that are in the fit (their bystanders' lists: "Bystanders of update queries" above; the entered
 * question for them: "Entered queries of update queries" below; for revise queries: "Entered queries of revise queries" below); KNNCF_PRED_PERSONALIZED; cosine fits with users of 4
 * or fewer ratings; an ordering by similarity; device-pointer forms; shard handles and knncf_group_*; the command-line tool. */
int knncf_query_entered(knncf_handle* h, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings,
                        int32_t cap, int32_t* out_users, double* out_sims, int32_t* out_pos, int32_t* out_displaced,
                        int32_t* count);
int knncf_query_entered_batch(knncf_handle* h, const int32_t* users, const int64_t* offsets, const int32_t* items,
                              const double* ratings, int64_t n_queries, int32_t cap, int32_t* out_users, double* out_sims,
                              int32_t* out_pos, int32_t* out_displaced, int32_t* counts, int32_t* statuses);

/* ---- Entered queries of update queries: whose kNN lists a user's new ratings change ------------------------------------------
 * The entered question for a changer that may be IN the fit: when fitted user c rates more items, which other fitted users'
 * cached kNN answers are stale?  One pass over the fit, where knncf_update_bystander_neighbors would take one slot per fitted user.
 * A query is an update query exactly as knncf_update_neighbors_batch defines it: any raw id c = users[b] with ADDITIONAL rows,
 * aug_b = train ++ those rows.  Queries are independent.
 * Which users are reported.  For a fitted v != c let L0 = getNeighbors(train, k, sim)(v) and L1 = getNeighbors(aug_b, k, sim)(v)
 * :596-617, each evaluated on closures of v's own, so that v owns every pair.  v is REPORTED iff c occurs in L0 or in L1, with
 * two exceptions: (a) a fitted c with n_ratings == 0 — aug is train; the query is valid (KNNCF_OK) and reports nothing; (b) c
 * stands in both lists at the same position with a similarity of +-0.0 of identical bits — a zero weight, no term of any fold.
 * Guarantee for an unreported v: L1 == L0 in ids and similarity bits, and every KNNCF_PRED_KNN prediction of v on aug_b equals
 * its prediction on train bit for bit — but for users answered with the global average, as in "Entered queries".
 * Outputs.  Row b of the five arrays ([n_queries * cap], row stride cap) receives the first min(counts[b], cap) reported users of
 * query b in the fit's user set order.  counts[b] is the number of reported users and may exceed cap.  Cells past the written
 * ones are untouched.  With cap == 0 every output array may be null: a count-only call.  Per reported user v:
 *   out_users  the raw id of v
 *   out_sims   S(v, c) on aug_b, owned by v, whether or not c is in L1; where c is in L1, the bits of that cell
 *   out_pos    the 0-based position of c in L1, -1 if c left
 *   out_prev   the 0-based position of c in L0, -1 if c entered
 *   out_other  entered: the raw id that drops out of L0, -1 where the list grew; left: the raw id that comes into L1 (its last
 *              cell); otherwise -1
 * A c absent from train is the fold-in case: out_users / out_sims / out_pos / out_other are knncf_query_entered's answer bit for
 * bit, out_prev = -1.  An empty query of an absent user stays KNNCF_E_INVALID, as in knncf_update_*.
 * Tail rows.  A reported v whose stored list is full and in which c, stored on train, now sorts behind every other stored entry
 * cannot be decided from the stored list: whether c keeps the last cell depends on v's best candidate outside it.  Such rows
 * within cap are resolved through knncf_update_bystander_neighbors_batch internally (one update slot per tail row); a
 * count-only call and tail rows beyond cap cost nothing.  Per-query statuses are those of knncf_update_neighbors_batch, and
 * one more: KNNCF_E_UNSUPPORTED when a tail user within cap has more than 65536 train ratings — counts[b] = 0 and the rows
 * untouched, as for every failed query (a query's rows are written once all of them are resolved).
 * Refusals of the handle and handle state: those of knncf_query_entered_batch.  NOT read-only: the missing lists M are built
 * first, in one batch in ascending raw id, which leaves the state knncf_neighbors_batch over M leaves; a KNNCF_SIM_COSINE handle
 * whose train set has a user of 4 or fewer ratings is refused, Jaccard is accepted.
 * The single form is the batch of one and returns the query's status; it has set *count = 0 once the argument checks pass.
 * Chunks.  C of "Batched fold-in queries", one slot per query in phase 1 (24 bytes * min(cap, num_users) + 4 per slot of answer
 * scratch beside the budget); the tail rows of a chunk then travel as "Bystanders of update queries" describes.  Results do not
 * depend on C; a repeated call of the same shape allocates no device memory.
 * OUT OF SCOPE: revise queries (a changer that also removes train rows: "Entered queries of revise queries" below);
 * KNNCF_PRED_PERSONALIZED; cosine fits with users of 4 or fewer ratings; device-pointer forms; shard handles and knncf_group_*;
 * the command-line tool. */
int knncf_update_entered(knncf_handle* h, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings,
                         int32_t cap, int32_t* out_users, double* out_sims, int32_t* out_pos, int32_t* out_prev,
                         int32_t* out_other, int32_t* count);
int knncf_update_entered_batch(knncf_handle* h, const int32_t* users, const int64_t* offsets, const int32_t* items,
                               const double* ratings, int64_t n_queries, int32_t cap, int32_t* out_users, double* out_sims,
                               int32_t* out_pos, int32_t* out_prev, int32_t* out_other, int32_t* counts, int32_t* statuses);

/* ---- Entered queries of revise queries: whose kNN lists a user's removals change ----------------------------------------------
 * The entered question for a changer that also takes ratings OUT: when fitted user c deletes a rating, or rates an item again,
 * its mean, every deviation and its norm move — which other fitted users' cached kNN answers are stale?  One pass over the fit,
 * where knncf_revise_bystander_neighbors would take one slot per fitted user.  The argument lists are knncf_update_entered*'s
 * with the removals in front of the additional rows, where knncf_revise_bystander_* puts them.
 * A query is a revise query exactly as knncf_revise_* defines it: c = users[b], the train items it takes out (removed_items rows
 * [removed_offsets[b], removed_offsets[b + 1])), its additional rows;
 *     aug_b = train without c's rows on the removed items, in file order, ++ the additional rows in order.
 * Queries are independent.
 * Which users are reported: as "Entered queries of update queries" above.  For a fitted v != c, L0 = getNeighbors(train, k,
 * sim)(v) and L1 = getNeighbors(aug_b, k, sim)(v) on closures of v's own; v is REPORTED iff c occurs in L0 or in L1, with two
 * exceptions: (a) a fitted c with n_removed == 0 AND n_ratings == 0 — aug is train; KNNCF_OK, nothing reported.  A fitted c that
 * only removes is an ordinary query: aug is not train; (b) c stands in both lists at the same position with a similarity of
 * +-0.0 of identical bits.  Only (b) silences a row: a re-rating with the SAME value is an ordinary query too (the row moves
 * behind every train row, and the bits of c's mean may move with it), and equal non-zero bits at the same position are reported.
 * Guarantee for an unreported v: L1 == L0 in ids and similarity bits, and every KNNCF_PRED_KNN prediction of v on aug_b equals
 * its prediction on train bit for bit — but for users answered with the global average.
 * Outputs, their set order, counts[b] that may exceed cap, untouched cells, cap == 0 as a count-only call with null arrays, tail
 * rows and the single form (the batch of one; *count = 0 once the argument checks pass): those of knncf_update_entered*.
 *   out_sims   S(v, c) on aug_b, owned by v: the left fold in v's dense-item order over c's row on aug, whatever c's size class
 *              there.  A FITTED COSINE CHANGER THAT FALLS TO 4 OR FEWER ROWS ON aug_b IS ACCEPTED: v owns the pair and has more
 *              than 4 ratings on the accepted handles, so the fold order is v's (c's own answers, knncf_revise_neighbors, fold
 *              such a pair in c's given order: their bits may differ from out_sims).
 * An item that leaves aug (c was its only train rater, removed it and did not give it again) changes no list: nobody else rated
 * it, so it was a term of no pair.
 * Tail rows within cap are resolved through knncf_revise_bystander_neighbors_batch internally with the query's removed items
 * (knncf_update_bystander_neighbors_batch for a call whose queries all have n_removed == 0).
 * Per-query statuses: those of knncf_revise_neighbors_batch — KNNCF_E_INVALID for a removed item that c did not rate in train, a
 * removed item listed twice, any removal for a user absent from train, a fitted user left without a row (and an empty query of
 * an absent user); KNNCF_E_DUPLICATE for an additional row on an unremoved train item or a repeated item; KNNCF_E_NONFINITE;
 * KNNCF_E_UNSUPPORTED for a negative mean on aug or more than 65536 rows, removed rows included — and KNNCF_E_UNSUPPORTED when a
 * tail user within cap has more than 65536 train ratings.  A failed query gets counts[b] = 0 and untouched rows.
 * Refusals of the handle and handle state: those of knncf_update_entered_batch.  NOT read-only: the missing lists M are built
 * first, in one batch in ascending raw id, which leaves the state knncf_neighbors_batch over M leaves.  A KNNCF_SIM_COSINE handle
 * whose TRAIN set has a user of 4 or fewer ratings is refused, Jaccard is accepted.  KNNCF_E_INVALID for n_removed < 0, null
 * removed items with n_removed > 0, and removed_offsets that are null, do not start at 0 or decrease.
 * n_removed == 0 in every query of a call gives the knncf_update_entered* answer bit for bit through the same code and with the
 * same trace lines.  KNNCF_DEBUG_TRACE_DISPATCH prints, after the `entered_update` line of a chunk that holds a changer with
 * removals,
 *     knncf-dispatch entered_revise slots=<changer slots with removals> removed=<their removed items> small=<fitted slots of <= 4 rows on aug>
 * Chunks.  C of "Batched fold-in queries", one revise slot per query in phase 1 and the answer scratch of the update form; the
 * tail rows of a chunk then travel as "Bystanders of revise queries" describes.  Results do not depend on C; a repeated call of
 * the same shape allocates no device memory.
 * OUT OF SCOPE: removals in knncf_append (knncf_amend takes them: "Amend" below); KNNCF_PRED_PERSONALIZED; cosine fits with
 * train users of 4 or fewer ratings; device-pointer forms; shard handles and knncf_group_*; the command-line tool. */
int knncf_revise_entered(knncf_handle* h, int32_t user, const int32_t* removed_items, int64_t n_removed, const int32_t* items,
                         const double* ratings, int64_t n_ratings, int32_t cap, int32_t* out_users, double* out_sims,
                         int32_t* out_pos, int32_t* out_prev, int32_t* out_other, int32_t* count);
int knncf_revise_entered_batch(knncf_handle* h, const int32_t* users, const int64_t* removed_offsets,
                               const int32_t* removed_items, const int64_t* offsets, const int32_t* items, const double* ratings,
                               int64_t n_queries, int32_t cap, int32_t* out_users, double* out_sims, int32_t* out_pos,
                               int32_t* out_prev, int32_t* out_other, int32_t* counts, int32_t* statuses);

/* ---- Append: new ratings into the fit, the kNN lists they cannot change kept ---------------------------------------------------
 * The query families above say what new ratings would change; knncf_append makes the n rows (users[j], items[j], ratings[j])
 * part of the fit.  Rows of several users may interleave; a user may be new or of the fit; items may be new.
 * Answers.  With aug = train ++ the n rows in the given order, every later call on the handle answers bit for bit as a handle
 * on which knncf_fit(aug) was called.
 * Handle state.  B = the users whose neighbour list was built before the call.  S = the changers (the distinct users of the
 * rows) and every fitted user that knncf_update_entered_batch reports on the handle as it stood before the call for the query
 * (changer c, c's rows of the append in order), each changer on its own; a tail row is reported, hence in S.  K = B \ S.  The
 * handle is left in the state that knncf_fit(aug) followed by knncf_neighbors_batch over K in ascending raw id leaves: the same
 * lists, the same build numbers (call 1, position in K), the call counter of the next build, the same knncf_neighbors_save
 * bytes wherever the state defines them.  With K empty that is the state of knncf_fit(aug).  No list outside K is built, not
 * for a user of S and not for a user that had none: the next call that needs one builds it, as after any fit.
 * Why S is enough.  A list of v outside S holds no changer on train; every changer's similarity to v on aug is the one on the
 * changer's own aug (v's rows did not move) and sorts behind v's stored last cell; new users and new items keep the relative
 * set order of the old ones.  So v's list on aug is its list on train.
 * Outputs.  *n_carried = |K|, *n_dropped = |B ∩ S|; dropped receives the first min(*n_dropped, dropped_cap) raw ids of B ∩ S in
 * the new fit's user set order and may be null with dropped_cap == 0; cells past the written ones are untouched.
 * Plain refits.  Nothing is carried (*n_carried = 0, dropped = B; the answers are still those of knncf_fit(aug)) when
 *   - min(k, num_users' - 1) is not the stored lists' length (a user joined a fit with k >= num_users - 1),
 *   - the handle is KNNCF_SIM_COSINE and train or aug has a user of 4 or fewer ratings (as the entered calls refuse it; Jaccard
 *     carries),
 *   - a changer's update query is KNNCF_E_UNSUPPORTED: a negative mean of its combined rows, more than 65536 of them, or a fit
 *     of fewer than 5 users or items,
 *   - the rows have more than KNNCF_APPEND_MAX_CHANGERS distinct users: marking that many costs more than the rebuild it saves
 *     (DESIGN.md "Append" has the measurement behind the constant),
 *   - the handle is KNNCF_SIM_ONE: it has no lists, 0 / 0.
 * Statuses.  KNNCF_E_STATE before a fit; KNNCF_E_UNSUPPORTED on a shard handle; KNNCF_E_INVALID for a null pointer with n > 0
 * (dropped with dropped_cap > 0), n < 0, dropped_cap < 0, null n_carried / n_dropped; KNNCF_E_DUPLICATE when a row repeats a
 * (user, item) of train or of the rows; KNNCF_E_NONFINITE for a non-finite deviation.  After any of the last three the handle
 * answers exactly as before the call: the new fit is built beside the old one and swapped in on success, so a SECOND copy of the
 * fit's arrays lives on the device during the call.  (The new fit decides from the free device memory at that moment — the old fit's
 * arrays, its per-item rater bitmaps among them, still allocated — whether it builds its own rater bitmaps: near that threshold an
 * appended handle can take the no-bitmap prediction path where knncf_fit(aug) would not.  The answers are the same; the speed is
 * not.)  n == 0 is KNNCF_OK and touches nothing: *n_carried = |B|, *n_dropped = 0.
 * Everything a refit drops is dropped: the Personalized table, the rater copies, the item statistics.
 * Timings: the refit and the carry are charged to prep_ms; the marking runs the update queries' neighbour pass, which charges
 * no stage.
 * Measurement hook: the environment variable KNNCF_DEBUG_APPEND_MAX_CHANGERS, read at every call, replaces the constant below for
 * that call (0: every append is a plain refit); scripts/append_latency.py brackets the crossover with it.  Not for production use.
 * OUT OF SCOPE: removals (knncf_amend below takes them); a device-pointer form; shard handles and knncf_group_*; the
 * command-line tool. */
#define KNNCF_APPEND_MAX_CHANGERS 128
int knncf_append(knncf_handle* h, const int32_t* users, const int32_t* items, const double* ratings, int64_t n,
                 int64_t* n_carried, int64_t* n_dropped, int32_t* dropped, int64_t dropped_cap);

/* ---- Amend: removals and re-ratings into the fit, the kNN lists they cannot change kept -------------------------------------------
 * knncf_append with removals in front: the train rows (removed_users[j], removed_items[j]), j < n_removed, leave the fit, then
 * the n rows join it.  aug is built in two steps: train in file order without the removed rows; then the n rows in the given
 * order.  Everything else is knncf_append's contract, read on this aug.
 * Answers.  Every later call on the handle answers bit for bit as a handle on which knncf_fit(aug) was called.
 * Changers.  The distinct users of the removals and of the rows.  Changer c is the revise query (c, its removed items, its rows
 * of the call in order) on the handle as it stood before the call.
 * Handle state.  B = the users whose neighbour list was built before the call.  S = the changers and every fitted user that
 * knncf_revise_entered_batch reports for that query, each changer on its own; a tail row is reported, hence in S.  K = B \ S.
 * The handle is left in the state that knncf_fit(aug) followed by knncf_neighbors_batch over K in ascending raw id leaves: the
 * lists, the build numbers, the call counter, the knncf_neighbors_save bytes.  Nothing outside K is built.
 * Why S is still enough.  A list that holds c on train is reported for c; S(v, c) on the joint aug reads v's rows, which did
 * not move, and c's rows on c's own aug, so it is the value c's own query saw and sorts behind v's stored last cell; no pair of
 * two non-changers moves — items that leave, users and items that join keep the relative set order of the rest.  Removing rows
 * shifts the file rows of everyone behind them and moves the global and the item averages: the lists read neither, and what
 * does is rebuilt by the refit (DESIGN.md "Amend").
 * Semantics.
 *   - A re-rating is a removal plus a row for the same (user, item): the row moves behind every train row.  A re-rating with the
 *     same value is an ordinary change (the bits of the user's mean may move with the row): the lists of S are dropped.
 *   - A removed item whose only rater was the changer leaves the fit: num_items shrinks, the item is no recommendation candidate
 *     any more and predicts as an unknown item; no list changes because of it.
 *   - A fitted user whose train rows are all removed and who gives no row leaves the fit: num_users shrinks (a plain refit).
 * Outputs.  *n_carried = |K|, *n_dropped = |B ∩ S| and dropped as in knncf_append: the first min(*n_dropped, dropped_cap) raw ids
 * of B ∩ S in the new fit's user set order.  A user that left stands where its id would stand in that order; where the new fit
 * has fewer than 5 users (their order is that of first occurrence) it stands behind them.
 * Plain refits.  Nothing is carried (*n_carried = 0, dropped = B; the answers are still those of knncf_fit(aug)) under every rule
 * of knncf_append, read on the revise queries — the stored list length min(k, num_users' - 1) changes; KNNCF_SIM_ONE; more than
 * KNNCF_APPEND_MAX_CHANGERS changers; a changer's revise query is KNNCF_E_UNSUPPORTED (a negative mean on aug, more than 65536
 * rows with the removed ones included, a fit of fewer than 5 users or items) — and when
 *   - a user leaves the fit (the carry maps every old user into the new fit),
 *   - the handle is KNNCF_SIM_COSINE and train or aug has a user of 4 or fewer ratings, a changer that its removals bring down to
 *     4 rows or fewer included.  Jaccard carries in that case.
 * Statuses.  KNNCF_E_STATE before a fit; KNNCF_E_UNSUPPORTED on a shard handle; KNNCF_E_INVALID for a null pointer that is needed
 * (removed_users / removed_items with n_removed > 0, the rows with n > 0, dropped with dropped_cap > 0, n_carried, n_dropped) or a
 * negative n_removed, n or dropped_cap; KNNCF_E_INVALID for a removal whose (user, item) is not a train row — a user or an item
 * unknown to train and a newcomer of the same call included —, for a removal listed twice, and for an aug without any row;
 * KNNCF_E_DUPLICATE for a row on a (user, item) that aug already holds: an unremoved train row, or one repeated within the rows;
 * KNNCF_E_NONFINITE for a non-finite deviation.  Precedence: the argument checks, then the removal checks, then the duplicate,
 * then the non-finite deviation.  The removal checks are the removal stage's own (every removal must match exactly one train
 * row) and run whether or not the marking runs.  After any refusal the handle is exactly as before the call: the new fit is
 * built beside the old one and swapped in last, as in knncf_append (a SECOND copy of the fit's arrays during the call).
 * Trivial calls.  n_removed == 0 && n == 0 is KNNCF_OK and touches nothing: *n_carried = |B|, *n_dropped = 0.  n_removed == 0 is
 * knncf_append bit for bit through the same code: knncf_append is the call without removals.
 * The removal stage.  The old fit's three file-order arrays are compacted on the device, in tiles of KNNCF_AMEND_TILE rows, into
 * the new fit's: every train row looks its (user, item) up in the sorted table of the removals, a scan of the tiles' survivor
 * counts gives each tile its place, and the surviving rows are written in file order — stable, without atomics.  The old arrays
 * stay intact until the swap; a repeated call of the same shape allocates nothing for this stage.
 * Timings: the removal stage, the refit and the carry are charged to prep_ms.
 * KNNCF_DEBUG_TRACE_DISPATCH prints knncf_append's `append` line for every call and, after it, for a call with removals
 *     knncf-dispatch amend removers=<changers with removals> removed=<n_removed> kept_rows=<train rows that went into aug>
 * KNNCF_DEBUG_APPEND_MAX_CHANGERS applies as in knncf_append.
 * OUT OF SCOPE: carrying when a user leaves (knncf_remove_users below carries: "Remove users"); a device-pointer form; shard handles and knncf_group_*; the command-line tool;
 * KNNCF_PRED_PERSONALIZED state (a refit drops it, as before). */
#define KNNCF_AMEND_TILE 2048
int knncf_amend(knncf_handle* h, const int32_t* removed_users, const int32_t* removed_items, int64_t n_removed,
                const int32_t* users, const int32_t* items, const double* ratings, int64_t n,
                int64_t* n_carried, int64_t* n_dropped, int32_t* dropped, int64_t dropped_cap);

/* ---- Remove users: users leave the fit, the kNN lists that do not hold them kept -----------------------------------------------
 * The n_users fitted users users[j] leave the fit with every row they have.  The caller keeps no rows: the ids are enough.
 * aug = train in file order without every row whose user is in `users`.
 * Answers.  Every later call on the handle answers bit for bit as a handle on which knncf_fit(aug) was called.  These are also
 * the answers of knncf_amend given every row of those users.
 * Handle state.  B = the users whose neighbour list was built before the call.  S = the leavers and every fitted user whose
 * STORED list holds a leaver in one of its min(count, min(k, num_users - 1)) cells, whatever the similarity there, +0.0 and -0.0
 * included.  K = B \ S.  The handle is left in the state that knncf_fit(aug) followed by knncf_neighbors_batch over K in
 * ascending raw id leaves: the same lists, the same build numbers (call 1, position in K), the same call counter, the same
 * knncf_neighbors_save bytes.  Nothing outside K is built.
 * Why the lists that hold a leaver are enough.  A list that does not hold leaver l has l behind its cut: taking l out of
 * allUsers - u changes nothing in front of the cut.  No similarity between two remaining users reads l's rows.  Users and items
 * that leave keep the relative set order of the rest: the trie key of an id does not depend on the set.  So the list of v outside
 * S on aug is its list on train (tests/test_remove_users_premises.py checks it on the oracle; DESIGN.md "Remove users").
 * Outputs.  As knncf_append: *n_carried = |K|, *n_dropped = |B ∩ S|; dropped receives the first min(*n_dropped, dropped_cap) raw
 * ids of B ∩ S in the new fit's user set order, a leaver that had a list standing where its id would stand in that order (where
 * the new fit has fewer than 5 users: behind them, as in knncf_amend).  A leaver without a list is not counted.
 * Plain refits.  Nothing is carried (*n_carried = 0, dropped = B; the answers are still those of knncf_fit(aug)) when
 *   - min(k, num_users' - 1) is not the stored lists' length, or the stored lists were built for another k (knncf_set_k),
 *   - the handle is KNNCF_SIM_ONE: it has no lists, 0 / 0,
 *   - more than KNNCF_APPEND_MAX_CHANGERS leavers are given (KNNCF_DEBUG_APPEND_MAX_CHANGERS applies as in knncf_append),
 *   - train or aug has fewer than 5 users or fewer than 5 items (the id sets change their iteration class there),
 *   - the handle is KNNCF_SIM_COSINE and train has a user of 4 or fewer ratings: the owner rule of such pairs reads the build
 *     numbers.  Jaccard carries.
 * Statuses.  KNNCF_E_STATE before a fit; KNNCF_E_UNSUPPORTED on a shard handle; KNNCF_E_INVALID for a null n_carried or
 * n_dropped, a null users with n_users > 0, a null dropped with dropped_cap > 0, a negative n_users or dropped_cap; KNNCF_E_INVALID
 * for an id that is no user of train, for an id listed twice, and for a call that leaves no row.  Precedence: the arguments, then
 * the ids, then the empty aug.  After any refusal the handle is exactly as before the call: the new fit is built beside the old
 * one and swapped in last, as in knncf_append (a SECOND copy of the fit's arrays during the call).
 * Trivial calls.  n_users == 0 is KNNCF_OK and touches nothing: *n_carried = |B|, *n_dropped = 0.
 * Everything a refit drops is dropped: the Personalized table, the rater copies, the item statistics.
 * The stages.  Removal: the host sorts the ids, looks them up among the fit's users and knows the surviving row count from the row
 * lengths; the device flags every file row of a leaver, in knncf_amend's tiles of KNNCF_AMEND_TILE rows, and compacts the three
 * file-order arrays as knncf_amend does — stable, no atomics; the counted survivors must be the host's number (KNNCF_E_STATE).
 * Marking: one pass over the stored lists, one wave per fitted user, each stored id tested against a bitmap of the leavers (in
 * LDS where it fits; KNNCF_DEBUG_NO_LDS_BITMAPS takes the global-memory variant).  Carry: knncf_append's, through a map in which
 * a leaver is "gone".
 * Timings: the removal, the refit and the carry are charged to prep_ms.
 * KNNCF_DEBUG_TRACE_DISPATCH prints knncf_append's `append` line (changers = the leavers) and after it
 *     knncf-dispatch remove users=<n_users> removed=<rows taken out> kept_rows=<rows of aug>
 *                           holders=<|B ∩ S| without the leavers> bitmap=<lds|global>
 * on one line.
 * OUT OF SCOPE: a device-pointer form; shard handles and knncf_group_*; the command-line tool; leavers mixed with other changers
 * in one call (knncf_amend takes a leaver's rows among its removals and then refits plainly: its own leaver rule is unchanged);
 * the call-sequence model of the tests. */
int knncf_remove_users(knncf_handle* h, const int32_t* users, int64_t n_users,
                       int64_t* n_carried, int64_t* n_dropped, int32_t* dropped, int64_t dropped_cap);

/* ---- batch---------------------------------------------------------------- */
int knncf_predict_batch(knncf_handle* h, int predictor, const int32_t* users,
                        const int32_t* items, int64_t n, double* out);
int knncf_predict_batch_device(knncf_handle* h, int predictor, const int32_t* d_users,
                               const int32_t* d_items, int64_t n, double* d_out);
/* MAE :69-73 over (users, items, ratings) in file order */
int knncf_mae(knncf_handle* h, int predictor, const int32_t* users, const int32_t* items,
              const double* ratings, int64_t n, double* mae);
/* device variant; returns the partial sums of the rows this shard owns
 * (rows of users outside the shard are skipped): mae = sum_abs_err / count
 * after an all-reduce over the shards.  d_pred (optional, may be NULL) receives
 * the per-row predictions of the owned rows (others untouched). */
int knncf_mae_device(knncf_handle* h, int predictor, const int32_t* d_users,
                     const int32_t* d_items, const double* d_ratings, int64_t n,
                     double* sum_abs_err, int64_t* count, double* d_pred);

/* ---- MAE at many k from one neighbour build (predict/kNN.scala:73) -------------------------------------------------
 * predict/kNN.scala:73 maps List(10, 30, 50, 100, 200, 300, 400, 800, 943) to
 * MAE(predictor(train, weightedSumDeviation(train, getSimilarity(train, k, sim))), test), fresh closures per k.
 * getNeighbors :603-616 is a stable sort followed by take(k), so every k's lists are prefixes of the lists at the largest k,
 * built in the same order: one build at kcap = min(max(ks), U-1) answers every k.
 * maes[q] == (knncf_set_k(h, ks[q]), knncf_mae(h, KNNCF_PRED_KNN, ...)), bit for bit.  predictions (optional, may be NULL):
 * [n_k * n], row q holds the per-row predictions at ks[q].
 * ks: strictly ascending, 1 <= ks[q] <= 2048, 1 <= n_k <= 64 (KNNCF_E_INVALID otherwise); values at or above U-1 all give
 * the same column.  KNNCF_E_STATE before a fit and, for the host form, on a shard handle; KNNCF_E_UNSUPPORTED for
 * KNNCF_SIM_ONE.  n == 0: NaN for every k.
 * Handle state: the call ignores the neighbour lists the handle holds (from knncf_mae, knncf_neighbors_load, ...) and builds
 * its own.  On return the neighbour memo is dropped, as knncf_reset_neighbors drops it, and the handle's k is unchanged — the
 * state a knncf_set_k + knncf_mae loop over the same ks would leave behind, except for k.  knncf_get_timings: the one build's
 * stage times, the sweep kernel as predict_ms. */
int knncf_mae_sweep(knncf_handle* h, const int32_t* ks, int32_t n_k, const int32_t* users, const int32_t* items,
                    const double* ratings, int64_t n, double* maes, double* predictions);
/* device form, as knncf_mae_device: per-k partial sums over the rows this shard owns (sum_abs_err[n_k], one count),
 * d_pred optional [n_k * n] (owned rows only) */
int knncf_mae_sweep_device(knncf_handle* h, const int32_t* ks, int32_t n_k, const int32_t* d_users,
                           const int32_t* d_items, const double* d_ratings, int64_t n, double* sum_abs_err,
                           int64_t* count, double* d_pred);

/* ---- multi-GPU exchange (one handle per GPU, collectives done by the host) - */
/* After knncf_fit* on every shard, each shard holds the per-user means / norms
 * (the order-sensitive fp64 folds of K2 / K3) of ITS users only.  The host
 * all-gathers d_user_avg[user_begin, user_end) and d_user_norm[...] (RCCL
 * all-gather over xGMI: 16 B per user) in place, then calls knncf_shard_commit,
 * which recomputes the other users' normalized deviations and preprocessed
 * ratings — elementwise functions of (rating, mean) and (deviation, norm) — bit
 * for bit, so nothing per RATING travels.  (d_dev / d_pre stay in the view: a host
 * that gathers them as well, as the round-1 protocol did, gets the same values
 * written twice.)  Users are block-partitioned in ascending dense order,
 * ceil(num_users / shard_count) per shard.  With shard_count == 1 these are no-ops.
 * One process driving all GPUs binds knncf_group_* below instead. */
typedef struct knncf_shard_view {
    int32_t user_begin, user_end; /* owned dense users [begin, end) */
    int64_t nnz_begin, nnz_end;   /* their entries in the user-major rating arrays */
    int32_t num_users;
    int64_t num_ratings;
    double* d_user_avg;  /* [num_users]   */
    double* d_user_norm; /* [num_users]   */
    double* d_dev;       /* [num_ratings] normalized deviations, user-major order */
    double* d_pre;       /* [num_ratings] preprocessed ratings, user-major order */
} knncf_shard_view;
int knncf_shard_view_get(knncf_handle* h, knncf_shard_view* out);
int knncf_shard_commit(knncf_handle* h);

/* ---- one process, several GPUs: the collectives inside the library ---------- */
/* A group = n shard handles (shard_rank i on devices[i]) + one RCCL communicator per device (ncclCommInitAll) + one
 * HIP stream per device for the collectives; every entry point drives the n GPUs from n host threads.  This is what a
 * JVM binds: ONE call per step instead of a re-implementation of the exchange —
 * distributed/DistributedBaseline.scala:41-47 hands one RDD to Spark the same way.
 *   knncf_group_fit  : knncf_fit on every shard (the host arrays are copied to every device) -> collective status ->
 *                      ncclAllGather of the padded {mean, norm} segments -> knncf_shard_commit on every shard.
 *   knncf_group_mae  : knncf_mae_device on every shard (each predicts the test rows of its own users) -> collective
 *                      status -> ncclAllReduce (sum) of (sum |r - p|, rows) -> mae; shared/predictions.scala:246-268's
 *                      `sum` / `count` actions.
 * cfg->device, shard_rank and shard_count are ignored (the group sets them).  RCCL is loaded at the first
 * knncf_group_create (dlopen of librccl.so.1: the library itself does not link it); KNNCF_E_UNSUPPORTED if it is absent,
 * KNNCF_E_RCCL for a failing RCCL call.  A group is not thread-safe. */
#define KNNCF_E_RCCL (-9)
typedef struct knncf_group knncf_group;
int knncf_group_create(const knncf_config* cfg, const int32_t* devices, int32_t n_devices, knncf_group** out);
void knncf_group_destroy(knncf_group* g);
const char* knncf_group_last_error(const knncf_group* g);
int knncf_group_size(const knncf_group* g, int32_t* n_devices);
/* the shard handle of rank i (owned by the group): scalar queries, knncf_neighbors of ITS users, timings */
int knncf_group_handle(knncf_group* g, int32_t rank, knncf_handle** out);
int knncf_group_fit(knncf_group* g, const int32_t* users, const int32_t* items, const double* ratings, int64_t n);
int knncf_group_mae(knncf_group* g, int predictor, const int32_t* users, const int32_t* items, const double* ratings,
                    int64_t n, double* mae);
/* every shard predicts the rows of its own users; out[0..n) receives all of them */
int knncf_group_predict_batch(knncf_group* g, int predictor, const int32_t* users, const int32_t* items, int64_t n, double* out);

/* ---- loader and on-disk cache --------------------------------- */
/* `load` shared/predictions.scala:35-49 as a multithreaded host parser: the line is split on `separator` (literal),
 * columns are trimmed, a line is kept iff column 0 parses as an Int (headers are dropped silently); columns 1 and 2
 * of a kept line must parse (the reference throws; here: KNNCF_E_INVALID with "<path>:<line>: ..." in err).  Rows
 * come back in FILE ORDER.  threads <= 0: one per hardware thread.  Release with knncf_free_ratings. */
typedef struct knncf_ratings {
    int64_t n;
    int32_t* users;
    int32_t* items;
    double* ratings;
} knncf_ratings;
int knncf_load_file(const char* path, const char* separator, int threads, knncf_ratings* out, char* err, int err_cap);
void knncf_free_ratings(knncf_ratings* r);
/* The same with a binary cache beside it (at ml-25m the text parse takes seconds, the fit 6 ms): the parsed
 * triples in FILE ORDER — the order is part of the semantics — stamped with the source file's size, modification time and
 * the separator, closed by a checksum.  A cache that matches `path` as it is now is read instead of parsing (*from_cache
 * = 1); a missing, stale, truncated or corrupt one is ignored and rewritten (tmp file + rename) after the parse.  The CSR /
 * CSC are not cached: K0 rebuilds them on the GPU faster than they could be read back.  cache_path == NULL: plain
 * knncf_load_file.  A cache that cannot be written is not an error. */
int knncf_load_file_cached(const char* path, const char* separator, int threads, const char* cache_path, knncf_ratings* out,
                           int* from_cache, char* err, int err_cap);

/* The Recommender's personal-ratings file, recommend/Recommender.scala:40-54 ("id,title,rating" CSV): every row's
 * (id, title) in file order — the header row as (0, "header") — and the rows with a non-zero rating as ratings of
 * `user` (the reference uses 944), ready to be appended to the training rows (`data.union(personal)` :68).  Rows with
 * an empty rating column are unrated; a non-numeric id / rating fails loudly (the reference throws).  Release with
 * knncf_free_personal. */
typedef struct knncf_personal {
    int64_t n_rows;
    int32_t* row_ids;      /* [n_rows] */
    char** row_names;      /* [n_rows] NUL-terminated, owned by the struct */
    char* name_storage;
    knncf_ratings ratings; /* the non-zero ratings, file order */
} knncf_personal;
int knncf_load_personal(const char* path, int32_t user, knncf_personal* out, char* err, int err_cap);
void knncf_free_personal(knncf_personal* p);

/* Checkpoint / resume of the expensive part of a fit: the U x k neighbour table (ids, fp64 similarities, build
 * sequence numbers).  save: every neighbourhood built so far.  load: the handle must be fitted on the same training
 * rows with the same k and similarity (checked with a fingerprint of the users, row extents and means and of every
 * rating's item and value in row order: KNNCF_E_STATE otherwise; a file of the older format "KNNCFNB1", whose fingerprint
 * left out the ratings, is refused with KNNCF_E_INVALID); afterwards getNeighbors / getSimilarity / predictions use the loaded lists and only
 * users that were not built at save time are built on demand. */
int knncf_neighbors_save(knncf_handle* h, const char* path);
int knncf_neighbors_load(knncf_handle* h, const char* path);

/* ---- introspection for bench / tests -------------------------------------- */
int knncf_get_timings(const knncf_handle* h, knncf_timings* out);
int knncf_reset_timings(knncf_handle* h);
/* drop the getNeighbors/getSimilarity memo (== constructing fresh closures) */
int knncf_reset_neighbors(knncf_handle* h);
/* change k (== getSimilarity(train, k, ...) with a new k); drops the memo */
int knncf_set_k(knncf_handle* h, int32_t k);

#ifdef __cplusplus
}
#endif
#endif
