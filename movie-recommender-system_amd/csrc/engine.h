// engine.h — internal state of one knncf handle and the launcher interface between the host
// orchestrator (api.cpp) and the kernel translation units.  gfx950 only.
#pragma once

#include <string>
#include <vector>

#include "common.h"

namespace knncf {

typedef __bf16 bf16_t;

// columns of a similarity row that select.hip holds in LDS at a time (prep.hip tabulates the tile crossings)
// provisional store of select.hip per similarity row: groups of 8 columns (36 B each); the capacity scales with k
inline int32_t select_gcap(int32_t k) { return 8192 * (int32_t)((k + 511) / 512 > 1 ? (k + 511) / 512 : 1); }
// (SELECT_TCOLS appears as a literal in tests/test_boundary_premises.py and tests/boundary_shapes.py: move together)
static constexpr int SELECT_TCOLS = 16384;  // <= 2^14: it_pack keeps the BYTE address of the column's LDS cell inside its tile in 16 bits
static_assert(SELECT_TCOLS <= 16384 && (SELECT_TCOLS & (SELECT_TCOLS - 1)) == 0, "it_pack: 16-bit cell byte address");

// ---- sort_util.hip (stable LSD radix sort / sorted-unique, hand-written; K0 plumbing) ----
struct SortWorkspace {
    DArr<char> tmp;
    DArr<size_t> count;  // unique_u32's per-tile counts and result cell (raw storage; kept: a hipFree per call synchronises the device)
};
void sort_pairs_u64_u32(SortWorkspace& ws, const uint64_t* kin, uint64_t* kout, const uint32_t* vin,
                        uint32_t* vout, size_t n, int end_bit, hipStream_t st);
void sort_keys_u32(SortWorkspace& ws, const uint32_t* kin, uint32_t* kout, size_t n, hipStream_t st);
void sort_pairs_u32_u32(SortWorkspace& ws, const uint32_t* kin, uint32_t* kout, const uint32_t* vin, uint32_t* vout, size_t n,
                        int end_bit, hipStream_t st);
// out must hold n entries; returns the number of distinct values (synchronises the stream)
size_t unique_u32(SortWorkspace& ws, const uint32_t* sorted_in, uint32_t* out, size_t n, hipStream_t st);

// ---- prep.hip: K0-K4 -------------------------------------------------------------------
struct Train {
    int64_t n = 0;
    int32_t U = 0, I = 0;
    // raw rows, file order
    DArr<int32_t> user_raw, item_raw;
    DArr<double> rating;
    // dense ids: trie keys of the distinct raw ids, in dense order (see dense_lookup)
    DArr<uint32_t> ukeys, ikeys;
    DArr<int32_t> uid, iid;  // raw id of dense index
    // raw id -> dense index as a direct table (MovieLens ids are small non-negative integers): one gather per row instead
    // of a hash + binary search; empty (n = 0) when an id is negative or >= 2^24 — then dense_lookup is used
    DArr<int32_t> u_table, i_table;
    int32_t u_table_n = 0, i_table_n = 0;
    // canonical user-major order ("position" p): users ascending, inside a user items ascending.
    // dense item index == rank in HashSet iteration order, so ascending p inside a user IS the
    // reference's summation order N2 for users with > 4 ratings.
    DArr<int64_t> u_ptr;     // [U+1]
    DArr<int32_t> s_user;    // [n]
    DArr<int32_t> s_col;     // [n]
    DArr<uint32_t> s_t;      // [n] file row of position p
    DArr<double> s_rating;   // [n]
    DArr<double> s_dev;      // [n] computeNormalizeDeviation :155-169
    DArr<double> s_pre;      // [n] preprocessedRating :470-481
    // fold orders (permutations of positions)
    DArr<uint32_t> perm_uf;  // (user, file order)            usersAvg :113
    DArr<uint32_t> perm_uh;  // (user, HashMap order, N4)      usersWeights :474
    DArr<int64_t> i_ptr;     // [I+1]
    DArr<double> user_avg, user_norm;  // [U]
    // K4 (itemsAvg :134, itemsAvgDev :176-186, getItemsAvgDev :336-343): built on first use by prep_item_stats — the kNN
    // path of the reference never evaluates them
    DArr<double> item_avg, item_dev_hash, item_dev_file;  // [I]
    bool item_stats_ready = false;
    // item-major copies for the sparse tail of the hybrid similarity (fp32 is enough: it only filters)
    DArr<int32_t> it_user;   // [n] dense user of the q-th entry in (item, user ascending) order
    DArr<uint32_t> it_pack;  // [n] the sparse tail's 4-byte entry: value field (16 bits, high) | byte address of the LDS cell of (user mod SELECT_TCOLS) — prep.hip: k_item_major
    DArr<double> it_dev;     // [n] normalized deviation of that entry (prediction gathers)
    DArr<uint32_t> it_t;     // [n] training file row of that entry (order of ratedI(i) :508-517)
    // per-item rater bitmaps over the dense user index + per-word exclusive rank prefixes: "did user x rate
    // item i, and where is that rating" is one 8-byte read (+ one on a hit) instead of a binary search
    int64_t ib_words = 0;        // 64-bit words per item row = ceil(U / 64); 0 = not built (too large)
    DArr<uint64_t> item_bits;    // [I * ib_words]
    DArr<uint32_t> item_rank;    // [I * ib_words]
    // where each item's rater list crosses the column tiles of select.hip: it_tile[i][t] = first entry q of item i
    // with it_user[q] >= t * SELECT_TCOLS (t = 0 .. tile_stride-1; the last one is the list's end)
    int32_t tile_stride = 0;
    DArr<uint32_t> it_tile;      // [I * tile_stride]
    DArr<int32_t> pop_item;  // [I] dense items by descending number of raters
    std::vector<int64_t> pop_count;  // host: rater counts in that order
    double global_avg = 0.0;
    double total = 0.0;  // the left fold of the ratings in file order that global_avg divides (average :18): bystander queries continue it
    bool exact_total = false;  // every rating is dyadic (k_check_dyadic): total and every partial sum of it are exact (k_exact_sum)
    int32_t own_lo = 0, own_hi = 0;  // owned dense users [lo, hi)
    int64_t own_p0 = 0, own_p1 = 0;  // their positions in the canonical order (everything when not sharded)
    // the handle's similarity is jaccardCoefficient :440-464: the similarity stage then counts common items — 0/1 operand
    // panels, tail entries of value 1 — instead of summing products of preprocessed ratings
    bool jaccard = false;
};

// status word bits written by kernels
enum : uint32_t { ST_NONFINITE = 1u, ST_DUPLICATE = 2u, ST_NOT_DYADIC = 4u, ST_LONG_ROW = 16u };

struct PrepScratch {
    SortWorkspace sort;
    DArr<uint64_t> k64_a, k64_b;
    DArr<uint32_t> v32_a, v32_b, k32_a, k32_b;
    DArr<int32_t> du_row, di_row;
    DArr<uint32_t> perm_f;
    DArr<uint32_t> status;  // [4] device status words
    DArr<int32_t> idrange;  // [4] min / max raw user id, min / max raw item id
    DArr<uint32_t> ucnt, utile;  // [U] ratings per user (then the scatter cursors), [U / 2048] their sums per tile
    DArr<int32_t> long_rows;  // [2 (U + 1)] users whose segment is sorted by the list classes of k_user_setup
    DArr<double> dsum;      // small reduction scratch
    DArr<uint4> rec;        // [2 n] (preprocessed rating, deviation | user, file row) records: one 32-byte gather per entry
    // second stream of the fit: the per-user LDS sorts of the few long rows run beside those of everybody else
    hipStream_t aux = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_commit = nullptr;
    // prep_commit leaves its second part (item-major copies, tile table, rater bitmaps) running on `aux`: whoever reads
    // those (select.hip, predict.hip) or re-uses this scratch for more than a sort (prep_item_stats) joins first
    bool commit_pending = false;
    DArr<uint32_t> perm_iu;  // [n] positions in (item, user ascending) order
    void join_commit(hipStream_t st);
    void ensure_aux();
    void release_all();
    PrepScratch() = default;
    PrepScratch(const PrepScratch&) = delete;
    PrepScratch& operator=(const PrepScratch&) = delete;
    ~PrepScratch();
};

// K0 + K1 + owned part of K2/K3.  Throws Error on invalid data.
void prep_fit(Train& tr, PrepScratch& sc, int32_t shard_rank, int32_t shard_count, hipStream_t st);
// sharded handles, after the exchange of the per-user (mean, norm): the deviations and preprocessed ratings of the users
// this shard does NOT own — pure elementwise functions of (rating, the user's mean) and (deviation, the user's norm), so
// every rank recomputes them bit for bit instead of receiving 16 B per rating over xGMI
void prep_complete_rows(Train& tr, PrepScratch& sc, hipStream_t st);
// item-major copies, rater bitmaps, popularity order (need every user's deviations: after the shards' exchange)
void prep_commit(Train& tr, PrepScratch& sc, hipStream_t st);
// K4: the per-item statistics of the baseline predictors (after prep_commit; sets tr.item_stats_ready)
void prep_item_stats(Train& tr, PrepScratch& sc, hipStream_t st);

// raw test ids -> dense (-1 = absent from train)
void launch_dense_ids(const Train& tr, const int32_t* d_users, const int32_t* d_items, int64_t n,
                      int32_t* d_du, int32_t* d_di, hipStream_t st);

// ---- gemm.hip: densify + K5 ------------------------------------------------------------
// rows[r] = dense user of panel row r (nullptr: panel row r == user row_begin + r)
// (tr.jaccard: every present entry is written as 1.0 — the 0/1 panel whose GEMM counts common items)
void launch_densify(const Train& tr, const int32_t* d_rows, int32_t row_begin, int32_t n_rows,
                    const int32_t* d_colmap, bf16_t* panel, int64_t ld, int64_t panel_rows, bool fp16,
                    hipStream_t st);
// colmap[item] = column of the dense head panel (popularity rank < H) or -1 (tail)
void launch_colmap(const Train& tr, int32_t H, int32_t* d_colmap, hipStream_t st);
// C[M][ldc] (fp32 or fp16) = A[M][K] * B[N][K]^T, 16-bit in / fp32 accumulate; M, N multiples of 256, K of 64
// clamp: fp16 C entries are clamped to [-1, 1] before rounding (adjusted cosine: the exact value lies there); false for
// the counting GEMM of the Jaccard path (counts <= 2048 are exact in fp16)
void launch_gemm_nt(const bf16_t* A, const bf16_t* B, void* C, bool c_fp16, int64_t M, int64_t N, int64_t K,
                    int64_t lda, int64_t ldb, int64_t ldc, bool fp16, bool clamp, hipStream_t st);

// the whole symmetric matrix at once: C[N][ldc] = B B^T computed on and above the diagonal (256 x 256 tiles in the order of
// the tile list) and mirrored below it; the stored values are bit for bit those of launch_gemm_nt(B, B, ...)
void gemm_sym_tile_list(int32_t n_tiles, std::vector<uint32_t>& out);
void launch_gemm_sym(const bf16_t* B, void* C, bool c_fp16, int64_t N, int64_t K, int64_t ldb, int64_t ldc, bool fp16, bool clamp,
                     const uint32_t* d_tile_list, int64_t n_listed, hipStream_t st);

// ---- select.hip: K6 + K6b --------------------------------------------------------------
struct NeighborTable {
    int32_t k = 0;     // requested k
    int32_t kcap = 0;  // min(k, U-1): stored neighbours per user
    DArr<int32_t> idx;   // [U * kcap] dense neighbour ids, reference order
    DArr<double> sim;    // [U * kcap]
    DArr<int32_t> uidx;  // [U * kcap] the same neighbours sorted by dense id: built on demand (probe_args) for the prediction
    DArr<double> usim;   // [U * kcap]   kernels that probe in global memory; the item-grouped kernel streams idx / sim as they are
    bool by_id_valid = false;  // uidx / usim hold the current lists
    DArr<int32_t> cnt;   // [U] 0 until built
    DArr<int64_t> seq;   // [U] build sequence number (memo history); -1 = not built
};

struct SelectScratch {
    DArr<int32_t> cand_idx;   // [rows * cap]
    DArr<float> cand_approx;  // [rows * cap] (KNNCF_FLAG_VERIFY_BOUND)
    DArr<int32_t> cand_cnt;   // [rows] (> cap == overflow)
    DArr<float> cand_eps;     // [rows] the error band of the row's approximate similarities
    DArr<int32_t> grp_v0;     // [rows * select_gcap(k)] provisional groups: first column
    DArr<float> grp_x;        // [rows * select_gcap(k) * 8] their 8 values
    DArr<double> stats;       // [4]: max bound violation, ...
    DArr<uint32_t> row_entries;  // [rows] ratings of the row's shortlisted candidates (re-rank traffic accounting)
    DArr<double> row_exact;   // fallback: [U] exact similarities of one row
    DArr<uint64_t> fb_keys_a, fb_keys_b;
    DArr<uint32_t> fb_vals_a, fb_vals_b;
};

// per panel row: S[r][:] += sparse tail (items with colmap < 0), then threshold + shortlist:
// candidates v with S[r][v] >= T_r - 2 eps_r; eps_r = eps_opnd * ||head part of row r|| + eps_rest + per-row terms
// per-row tail entry lists for the current head (select.hip: k_tail_entries); device pointers
struct TailEntries {
    const int32_t* cnt = nullptr;   // [U]
    const int32_t* item = nullptr;  // [n], row u's entries at u_ptr[u] ..
    const float* x = nullptr;       // [n]
    const float* tail_abs = nullptr;  // [U]
    const float* head_sq = nullptr;   // [U]
    const float* row_len = nullptr;   // Jaccard handles: [row_len_size(U)] |I(v)| as float
};
int64_t row_len_size(int32_t U);
void launch_row_len(const Train& tr, float* d_out, hipStream_t st);
void launch_tail_entries(const Train& tr, const int32_t* d_colmap, int32_t* te_cnt, int32_t* te_item, float* te_x,
                         float* row_tail_abs, float* row_head_sq, hipStream_t st);
// s_by_user: S is the whole matrix and row r's similarities are S[d_row_user[r]] (symmetric path); else S[r]
void launch_tail_select(const Train& tr, const int32_t* d_colmap, const TailEntries& te, bool has_tail, const void* S, bool s_by_user, bool s_fp16, int64_t lds,
                        int32_t n_rows, const int32_t* d_row_user, int32_t k, float eps_opnd, float eps_rest, int32_t cap,
                        int32_t* cand_idx, float* cand_approx, int32_t* cand_cnt, float* cand_eps, int32_t* grp_v0, float* grp_x,
                        int32_t gcap, hipStream_t st, bool anticipate = true, const int32_t* d_row_srow = nullptr);
// (d_row_srow: row-block panels — the panel row of launch row r when it is not r itself: the re-select of a subset of a block)
// (anticipate = false: the emission thresholds are the plain k-th largest value seen so far — api.cpp re-runs the rows of a
// build whose anticipated thresholds overshot too often that way)
// the first n_heavy rows of a re-rank launch as P slices of their shortlists + a merge (rerank.hip)
struct SliceScratch {
    DArr<int32_t> part_idx, part_cnt;
    DArr<uint32_t> entries;
    DArr<double> part_sim;
};
struct Slices {  // (kernel argument)
    int32_t n_heavy, P;
    int32_t* part_idx;
    double* part_sim;
    int32_t* part_cnt;
    uint32_t* entries;
};
// exact fp64 similarities of the shortlists in reference order, stable top-k; n_heavy > 0: the first n_heavy rows as `slices`
// slices each (2 <= slices, slices * k <= 8192; sc holds their partial lists)
void launch_rerank(const Train& tr, NeighborTable& nt, int32_t n_rows, const int32_t* d_row_user,
                   int32_t cap, const int32_t* cand_idx, const float* cand_approx,
                   const int32_t* cand_cnt, const float* cand_eps, double* d_stats, uint32_t* d_row_entries, bool verify,
                   hipStream_t st, int32_t n_heavy = 0, int32_t slices = 1, SliceScratch* sc = nullptr);
// exact similarities of one user against everyone (fallback + scalar queries)
void launch_exact_row(const Train& tr, const NeighborTable& nt, int32_t user, int64_t user_seq,
                      double* d_out, hipStream_t st);
// Personalized (no k): per user the ids (ascending, the user itself included) and fp64 values of every non-zero
// adjusted-cosine / Jaccard similarity; d_idx / d_sim hold U x U cells, d_cnt the list lengths
void launch_full_rows(const Train& tr, bool jaccard, int32_t* d_idx, double* d_sim, int32_t* d_cnt, hipStream_t st);
// fresh-closure similarity of one pair (owner order = u): writes *d_out
void launch_exact_pair(const Train& tr, int32_t u, int32_t v, double* d_out, hipStream_t st);

// ---- predict.hip: K7-K9 ----------------------------------------------------------------
// id-sorted copies of the lists of the given users (d_row_user == nullptr: of every user)
void launch_sort_neighbors(NeighborTable& nt, int32_t U, int32_t n_rows, const int32_t* d_row_user, hipStream_t st);
// What the kNN term kernels (knn_terms.h) probe: "which of u's neighbours rated item i, and where".  Kernel argument, embedded
// in PredArgs, ExplainArgs and SweepArgs.
struct ProbeArgs {
    // neighbour table: lists of kcap cells per user, nbr_cnt[u] of them filled
    const int32_t* nbr_idx;
    const double* nbr_sim;
    const int32_t* nbr_cnt;
    int32_t kcap;
    // item-major rows, raters ascending
    const int64_t* i_ptr;
    const int32_t* it_user;
    const double* it_dev;
    const uint32_t* it_t;
    // per-item rater bitmaps (ib_words == 0: not built, binary search instead)
    int64_t ib_words;
    const unsigned long long* item_bits;
    const uint32_t* item_rank;
};
// by_id: the lists sorted by neighbour id, which the kernels that probe in global memory want (neighbouring lanes on neighbouring
// ids share cache sectors) — the copies are made here on first need (0.7 ms per step at the ml-25m shape when it was part of every
// build); else the lists as the re-rank left them (reference order), for the kernels that probe an LDS bitmap
ProbeArgs probe_args(const Train& tr, NeighborTable& nt, bool by_id, hipStream_t st);
// per test row: prediction of `predictor`; rows whose user is outside [own_lo, own_hi) are
// skipped (unknown users belong to shard 0).  d_abs_err[t] = |r - p| or 0 for skipped rows.
void launch_predict(const Train& tr, NeighborTable* nt, int predictor, int64_t n,
                    const int32_t* d_du, const int32_t* d_di, const double* d_ratings,
                    const uint32_t* d_order, bool order_by_item, double* d_pred, double* d_abs_err, uint8_t* d_owned,
                    bool unknown_users_owned, hipStream_t st);
// (key, value) = (dense user / item, or `limit` (= their number) when absent from train; row) of every test row: sorted
// (bits_for(limit + 1) key bits), it is the d_order of the grouped kNN kernels
void launch_user_keys(int64_t n, const int32_t* d_du, uint32_t limit, uint64_t* d_key, uint32_t* d_val, hipStream_t st);
// sharded handles: key = d_src (dense user or item) for the rows of this shard's users, limit + 1 for everybody else's;
// *d_n_owned += number of rows of this shard
void launch_owned_keys(int64_t n, const int32_t* d_src, const int32_t* d_du, int32_t own_lo, int32_t own_hi, bool unknown_owned, uint32_t limit,
                       uint64_t* d_key, uint32_t* d_val, unsigned long long* d_n_owned, hipStream_t st);
// deterministic fixed-shape reduction: sum of d_abs_err and count of d_owned
void launch_reduce_err(const double* d_abs_err, const uint8_t* d_owned, int64_t n, double* d_partials,
                       int64_t* d_counts, int32_t n_blocks, hipStream_t st);

// ---- explain.hip: the neighbour terms behind kNN predictions (knncf_explain*; DESIGN.md "Explanations") ---------------
// Where the explanations of a set of rows are written, by explain.hip for rows of the fit and by foldin.hip for query rows;
// device pointers for a launch, host pointers for the caller's arrays.  Row t: counts[t] = number of terms, the first
// min(count, cap) of them in `order` (KNNCF_EXPLAIN_*) in row t of raters / sims / devs (row stride cap; unused with cap ==
// 0), sums[2 t ..] = (num, den) of the fold over all terms and pred[t] = the KNNCF_PRED_KNN prediction (either may be null).
struct ExplainCells {
    int32_t order, cap;
    int32_t* raters;
    double* sims;
    double* devs;
    int32_t* counts;
    double* sums;
    double* pred;
};
// per row (d_du[t], d_di[t]), t < n: row t of `out` (terms: neighbours of the user with a non-zero similarity that rated the
// item).  nt.kcap <= 2048; makes nt's id-sorted copies when they are not current.
void launch_explain(const Train& tr, NeighborTable& nt, int64_t n, const int32_t* d_du, const int32_t* d_di, const ExplainCells& out,
                    hipStream_t st);

// ---- ksweep.hip: the kNN prediction at several k from one neighbour table (knncf_mae_sweep) ----------------------
// per test row d_order[0 .. n): the kNN prediction at every k = d_ks[q] (ascending, q < n_k <= 64) from the first k entries of the
// row user's reference-order list in nt (kcap <= 2048); rows sorted by dense item.  Cell q * n_total + row of d_pred (may be
// null) / d_abs_err; rows of other shards' users: abs_err 0 in every column, owned 0
void launch_predict_sweep(const Train& tr, NeighborTable& nt, const int32_t* d_ks, int32_t n_k, int64_t n_rows, int64_t n_total,
                          const int32_t* d_du, const int32_t* d_di, const double* d_ratings, const uint32_t* d_order,
                          double* d_pred, double* d_abs_err, uint8_t* d_owned, bool unknown_users_owned, hipStream_t st);

// ---- personalized.hip: PERSONALIZED (no k) with the adjusted cosine / the Jaccard coefficient beyond the U x U table ----
// columns of a similarity row that k_sim_rows accumulates in LDS at a time (fp64: 64 KiB)
static constexpr int PERSONAL_TCOLS = 8192;
// per-handle copies built on the first streamed PERSONALIZED call (api.cpp: ensure_personal_rows), dropped by a re-fit
struct PersonalRows {
    DArr<double> pi_pre;     // [n] preprocessed rating of the q-th entry in (item, user ascending) order (it_user's order)
    DArr<int32_t> pf_user;   // [n] dense rater of the k-th entry in (item, train file row) order (ratedI(i) :508-517)
    DArr<double> pf_dev;     // [n] that rating's normalized deviation
    int32_t tiles = 0;       // ceil(U / PERSONAL_TCOLS)
    DArr<uint32_t> tile;     // [I * (tiles + 1)] tile[i][t] = first entry q of item i with it_user[q] >= t * PERSONAL_TCOLS
    DArr<double> S;          // [R * U] row scratch: the exact similarity rows of one block of users
    DArr<int32_t> users;     // [U] the users whose rows are built, in test-row order
    DArr<int32_t> slot;      // [U] row of S of each built user inside its block
};
// pi_pre, pf_user / pf_dev and the tile table (after prep_commit's second part)
void personalized_prepare(const Train& tr, PrepScratch& sc, PersonalRows& pr, hipStream_t st);
// key = (dense user or U when absent) << bits_for(I) | (dense item or I when absent), value = row
void launch_personal_row_keys(const Train& tr, int64_t n, const int32_t* d_du, const int32_t* d_di, uint64_t* d_key,
                              uint32_t* d_val, hipStream_t st);
// S[r][v] = s(d_users[r], v) for r < n_users and every dense user v
void launch_sim_rows(const Train& tr, const PersonalRows& pr, const int32_t* d_users, int32_t n_users, double* d_S, hipStream_t st);
// predictions of the test rows d_order[0 .. n_rows): a row of a known user on a known item reads the user's row
// d_S[d_slot[user]]
void launch_fold_rows(const Train& tr, const PersonalRows& pr, int64_t n_rows, const uint32_t* d_order, const int32_t* d_du,
                      const int32_t* d_di, const double* d_ratings, const int32_t* d_slot, const double* d_S, double* d_pred,
                      double* d_abs_err, uint8_t* d_owned, hipStream_t st);

// ---- explain_all.hip: the terms behind Personalized predictions of fitted users (knncf_explain_personalized*; DESIGN.md
// "Explanations of Personalized predictions") ----
// bytes per row of a launch that the sub-range rule of knncf.h counts: the outputs in one block (explain_pack) and as much
// again for the term cells that KNNCF_EXPLAIN_BY_WEIGHT stages before it ranks them
inline size_t explain_all_row_bytes(int32_t cap) { return 40 * (size_t)cap + 28; }
// rows d_order[0 .. n_rows) of (d_du, d_di), users of the block whose exact rows are d_S[d_slot[user]], into rows [0, n_rows) of
// `out` (every pointer set; terms: the item's raters whose similarity is non-zero, the user itself included).  d_stage holds
// 20 * n_rows * out.cap bytes and is read and written with KNNCF_EXPLAIN_BY_WEIGHT only.  One launch.
void launch_explain_all(const Train& tr, const PersonalRows& pr, int64_t n_rows, const uint32_t* d_order, const int32_t* d_du,
                        const int32_t* d_di, const int32_t* d_slot, const double* d_S, const ExplainCells& out, double* d_stage,
                        hipStream_t st);

// ---- foldin.hip: kNN queries of users outside the fit (DESIGN.md "Fold-in queries") ----------------------------------
// Chunks of independent queries, every stage one launch over the chunk; a single call is a chunk of one.  The scratch is
// handle-owned; the fit, its neighbour table and its sequence numbers are only read.
static constexpr uint32_t QUERY_ST_NEG_MEAN = 1u << 8;  // status bit beside ST_NONFINITE / ST_DUPLICATE: the query's mean is negative
// revise queries: a removed item that is not a train item of the slot's user / a removed item listed twice
static constexpr uint32_t QUERY_ST_RM_UNRATED = 1u << 9, QUERY_ST_RM_TWICE = 1u << 10;
static constexpr int QB_MAX_CHUNK = 64;  // queries per chunk: one lane of k_query_sim_dual's waves each
static constexpr int QB_DUAL_MIN = 32;   // smaller chunks run k_query_sim once per query instead: measured crossover
// device bytes per query of a chunk that the chunk rule of knncf.h counts
inline int64_t query_batch_bytes(int32_t U, int32_t I) { return 64 * (int64_t)U + 96 * (int64_t)I; }
struct QueryBatchScratch {
    DArr<int32_t> users;               // [C] raw user of each slot
    DArr<int64_t> qo;                  // [C + 1] first row of each slot
    DArr<int32_t> items, slot, di, given_d;  // [n] rows of the chunk, slot after slot
    DArr<double> ratings, dev, pre, pre_d, dev_d;
    DArr<int32_t> self;                // [C] update queries: dense index of the slot's user in the fit, -1 when it is not there
    DArr<int64_t> ao;                  // [C + 1] update queries: first additional row of each slot
    DArr<int32_t> add_items;           // [ao[C]] the additional rows as uploaded (items / ratings hold train rows + these)
    DArr<double> add_ratings;
    // revise queries (a chunk with removed items; n_removed = their number in the chunk answered last, 0: none)
    int64_t n_removed = 0;
    DArr<int64_t> ro, so;              // [C + 1] first removed item / first source row (train rows + additional rows) of each slot
    std::vector<int64_t> h_so;         // host copy of so
    DArr<int32_t> rm_items, rm_slot, rm_gone;  // [ro[C]] raw item, slot, dense item if it leaves aug (else -1) of each removed item
    DArr<uint32_t> rm_mark;            // [so[C]] 1 = this train row of the slot's user is removed
    DArr<uint64_t> bits;               // [C][ceil(I / 64)]
    DArr<int64_t> rank;                // [C][ceil(I / 64) + 1]
    DArr<uint32_t> tbits, trank;       // [2 ceil(I / 64)][64] the bitmaps and prefixes side by side (k_qb_transpose)
    DArr<int64_t> info;                // [C][4] status bits, known items, neighbour ratings
    DArr<double> scal;                 // [C][2] mean, norm
    DArr<double> sim;                  // [C][U]
    DArr<double> suu, simT;            // KNNCF_PRED_PERSONALIZED: [C] S(u, u) on aug; [U][stride] sim transposed, stride = 2^ceil(log2 C)
    DArr<uint64_t> k64_a, k64_b;       // [C * max(U, I)]
    DArr<uint32_t> v32_a, v32_b, s32_a, s32_b;
    DArr<int32_t> nbr_idx;             // [C][take]
    DArr<double> nbr_sim;
    DArr<int64_t> off, ebase;          // [C][take + 1], [C + 1]
    DArr<uint64_t> e_k64_a, e_k64_b;   // [entries of the chunk]
    DArr<uint32_t> e_v32_a, e_v32_b;
    DArr<double> e_dev, e_sim;
    DArr<double> num, den, pred;       // [C][I]
    DArr<uint8_t> rated;
    DArr<uint32_t> by_id;              // [I]
    DArr<int32_t> pick_items, pick_slot, out_items;
    DArr<double> pick_out, out_preds;
    DArr<int64_t> reco_rb;             // [C + 1] first explain row of each slot (foldin_batch_reco_rows)
    // bystander queries (bystander.hip): [C] the changer's slot of each slot (its own index for a changer's slot), the changer's
    // index (U for a newcomer, its dense user for a user of the fit), a newcomer's place in set order, S(v, q), and S(v, q) again
    // where q is in v's list (else +0.0)
    DArr<int32_t> by_qslot, by_qidx, by_qrank;
    DArr<double> by_pair, by_in;
    bool by_chunk = false;             // the chunk answered last was a bystander chunk (QueryChunk::by)
    // bystanders of revise queries: the changer slots whose surviving train ratings are folded (bystander_survivor_totals), the
    // removed file rows of each ([so[C]], a slot's at so[b]) and the folds
    DArr<int32_t> by_rf_slot;
    DArr<uint32_t> by_rf_rows;
    DArr<double> by_rf_out;
    // entered queries (entered.hip): the answers of a chunk in ONE block (entered_pack), 20 * width + 4 bytes per slot
    DArr<double> en_pack;
};
// A chunk of bystander queries (DESIGN.md "Bystander queries"): slot b is either a newcomer's own fold-in slot (h_qslot[b] == b,
// h_self[b] == -1) or a bystander's — a fitted user with no additional row (h_self[b] >= 0) whose newcomer is slot h_qslot[b] of
// the same chunk.  h_qrank[b] = the number of train users in front of slot b's newcomer in set order.
// The changer may instead be a user c of the fit with additional rows (DESIGN.md "Bystanders of update queries"): its own slot
// is an update slot (h_self[b] == dense(c), h_qslot[b] == b).  h_qidx[b] = the index of slot b's changer in neighbour lists: U
// for a newcomer, dense(c) for a fitted one (h_qrank is not read then).  fitted = the chunk's changer slots of the second kind,
// merged = its bystander slots of newcomers (the trace line).
struct ByChunk {
    const int32_t* h_qslot;
    const int32_t* h_qrank;
    const int32_t* h_qidx;
    int32_t fitted, merged;
};
// A packed chunk of C >= 1 non-empty queries on the host, slot after slot: what foldin_batch_neighbors uploads.
struct QueryChunk {
    int32_t C;
    const int32_t* users;  // [C] raw ids
    const int64_t* qo;     // [C + 1] slot b has qo[b + 1] - qo[b] rows in aug
    // self == nullptr (a fold-in chunk; ao is null with it): items / ratings are the chunk's rows [qo[C]].  Otherwise (an update
    // chunk) self[b] is the dense index of slot b's user in the fit or -1, items / ratings are the ADDITIONAL rows [ao[C]] only,
    // and slot b has (train rows of self[b]) + (ao[b + 1] - ao[b]) rows: the train rows are seeded on the device, a fitted user
    // is left out of its own candidates and gets min(k, U - 1) neighbours.
    const int32_t* items;
    const double* ratings;
    const int32_t* self;  // [C]
    const int64_t* ao;    // [C + 1]
    // ro != nullptr with ro[C] > 0 (a revise chunk, which is an update chunk): removed [ro[b], ro[b + 1]) are raw items whose
    // train rows slot b's user drops, at most as many as it has train rows, none for a slot with self[b] < 0; slot b then has
    // (train rows) - (removed items) + (additional rows) rows.  A removal that names no train row of the user, or one twice, sets
    // QUERY_ST_RM_UNRATED / QUERY_ST_RM_TWICE in the slot's status bits; the known items of h_info count the items that left aug.
    const int64_t* ro;
    const int32_t* removed;
    // false (the Personalized and the entered modes): the pass stops after the similarities — no keys, no sorts, bs.nbr_idx /
    // nbr_sim / off are not written and the neighbour ratings of h_info are 0
    bool topk;
    // != nullptr (a bystander chunk: an update chunk with topk; with removals where the changers are revise slots): after the top lists every bystander slot's
    // list takes its newcomer in — index U, min(k, U) entries — and the neighbour ratings of h_info count the newcomer's known
    // items; a newcomer's own slot and the bystander slots of a newcomer whose status is set have 0.  The bystander slots of a
    // fitted changer get S(v, c) on aug into their similarity row ahead of the sorts instead: min(k, U - 1) entries, c among
    // them at index dense(c).  foldin_batch_predictions then gathers the changer's prepared row by its index (bs.by_chunk)
    const ByChunk* by;
};
// prep + similarities + top-k (bs.nbr_idx / nbr_sim [C][min(k, U)]) of the chunk; h_info[4 b ..] = status bits, known items,
// neighbour ratings (0 for a slot whose status is set) of slot b.  Synchronises the stream once.
void foldin_batch_neighbors(const Train& tr, QueryBatchScratch& bs, SortWorkspace& ws, const QueryChunk& q, int32_t k, long long* h_info, hipStream_t st);
// bs.pred / bs.rated [C][I]; h_ebase[C + 1] = exclusive prefix of the slots' neighbour ratings
void foldin_batch_predictions(const Train& tr, QueryBatchScratch& bs, SortWorkspace& ws, int32_t C, int32_t take,
                              const int64_t* h_ebase, hipStream_t st);
void foldin_batch_pick(const Train& tr, QueryBatchScratch& bs, const int32_t* d_items, const int32_t* d_slot, int64_t m,
                       double* d_out, hipStream_t st);
// KNNCF_PRED_PERSONALIZED instead of foldin_batch_predictions, after foldin_batch_neighbors(topk = false) on the chunk of n rows
// (update: it was given h_self): S(u, u) per slot, the transposed similarities, one fold per (slot, item) over all of the
// item's raters in file order (pr: personalized_prepare's pf_user / pf_dev), then bs.pred / bs.rated [C][I].  No round trip.
void foldin_batch_fold_all(const Train& tr, const PersonalRows& pr, QueryBatchScratch& bs, SortWorkspace& ws, int32_t C, int64_t n,
                           bool update, hipStream_t st);
// foldin_batch_pick after foldin_batch_fold_all: an additional item unknown to train has the slot's own term
void foldin_batch_pick_all(const Train& tr, QueryBatchScratch& bs, const int32_t* d_items, const int32_t* d_slot, int64_t m,
                           double* d_out, hipStream_t st);
// after foldin_batch_predictions: the terms behind the predictions of the chunk's rows [r0, r0 + n) of d_items / d_slot, into
// rows [0, n) of `out`: cell 0 is row r0.  One launch.
struct QbExplainRows {
    int32_t take;   // as foldin_batch_predictions took it
    int64_t E;      // h_ebase[C], the chunk's gathered entries
    const int32_t* d_items;
    const int32_t* d_slot;
    int64_t r0, n;
};
void foldin_batch_explain(const Train& tr, QueryBatchScratch& bs, const QbExplainRows& rows, const ExplainCells& out, hipStream_t st);
// after foldin_batch_fold_all (update as it was given there): the terms behind the Personalized predictions of the chunk's rows
// [rows.r0, rows.r0 + rows.n) (rows.take and rows.E are not read), into rows [0, n) of `out` (every pointer set).  d_stage holds
// 20 * rows.n * out.cap bytes and is read and written with KNNCF_EXPLAIN_BY_WEIGHT only.  One launch.
void foldin_batch_explain_all(const Train& tr, const PersonalRows& pr, QueryBatchScratch& bs, const QbExplainRows& rows, bool update,
                              const ExplainCells& out, double* d_stage, hipStream_t st);
// d_items / d_preds [C][n]: slot b's first min(n, I - known) recommendations (the rest untouched)
void foldin_batch_recommend(const Train& tr, QueryBatchScratch& bs, SortWorkspace& ws, int32_t C, int32_t n, int32_t* d_items,
                            double* d_preds, hipStream_t st);
// after foldin_batch_recommend into d_items [C][n]: the recommended cells as the rows the two explain calls above take, in
// bs.pick_items / bs.pick_slot — cell j of slot b is row h_rb[b] + j for j < h_rb[b + 1] - h_rb[b] (h_rb [C + 1]: the exclusive
// prefix of the slots' counts, 0 for a refused slot; every count <= what foldin_batch_recommend wrote for the slot).  One
// upload and one launch, no round trip; nothing with h_rb[C] == 0.
void foldin_batch_reco_rows(QueryBatchScratch& bs, int32_t C, int32_t n, const int64_t* h_rb, const int32_t* d_items, hipStream_t st);

// ---- bystander.hip: what a newcomer adds to the slots of fitted users (knncf_query_bystander_*; DESIGN.md "Bystander queries")
// the chunk's slot map, before any kernel of the chunk
void bystander_upload(QueryBatchScratch& bs, int32_t C, const ByChunk& by, hipStream_t st);
// a chunk with fitted changers, after the similarity kernel and before the keys: S(v, c) per bystander slot, and that value
// into cell dense(c) of the slot's row of bs.sim where c is of the fit
void bystander_place(const Train& tr, QueryBatchScratch& bs, int32_t C, hipStream_t st);
// after k_qb_write: S(v, q) per bystander slot (placed: bystander_place computed it), a newcomer q into v's list, a fitted one
// looked up in it, then bs.off and the neighbour ratings of bs.info (instead of k_qb_offsets)
void bystander_merge(const Train& tr, QueryBatchScratch& bs, int32_t C, int32_t take, bool placed, hipStream_t st);
// k_qb_gather's launch for such a chunk
void bystander_gather(const Train& tr, QueryBatchScratch& bs, int32_t C, int32_t take, hipStream_t st);
// foldin_batch_pick for rows of bystander slots: an item that only the newcomer rates has its one term
void bystander_pick(const Train& tr, QueryBatchScratch& bs, const int32_t* d_items, const int32_t* d_slot, int64_t m, double* d_out,
                    hipStream_t st);
// bystanders of revise queries: h_out[x] = the left fold from 0.0 of the train ratings in file order without the rows that
// changer slot h_slots[x] (a fitted user's, with removals, status clear) of the chunk answered last removed — what average(aug)
// continues over the additional ratings.  tr.exact_total: total - (the removed ratings), exact; otherwise one sequential
// fold over the file per slot.  Synchronises the stream.
void bystander_survivor_totals(const Train& tr, QueryBatchScratch& bs, const int32_t* h_slots, int32_t n_slots, double* h_out,
                               hipStream_t st);

// ---- entered.hip: the fitted users whose neighbour lists a newcomer joins (knncf_query_entered*; DESIGN.md "Entered queries")
// The answers of a chunk of C slots lie in one block, so that one copy brings them back: sims [C * width] as doubles, then
// users, pos, displaced [C * width] and counts [C] as int32 — row s holds the first min(counts[s], width) entered users of slot s
// in dense order.  The same layout over a device or a host address.
struct EnteredPack {
    double* sims;
    int32_t* users;
    int32_t* pos;
    int32_t* displaced;
    int32_t* counts;
};
inline size_t entered_pack_bytes(int32_t C, int32_t width) { return (size_t)C * ((size_t)width * 20 + 4); }
inline EnteredPack entered_pack(double* base, int32_t C, int32_t width) {
    const size_t cells = (size_t)C * (size_t)width;
    EnteredPack o;
    o.sims = base;
    o.users = reinterpret_cast<int32_t*>(base + cells);
    o.pos = o.users + cells; o.displaced = o.pos + cells; o.counts = o.displaced + cells;
    return o;
}
// after foldin_batch_neighbors(topk = false) on a fold-in chunk of C slots, with every list of nt built and take = min(k, U) > 0:
// the answers of the chunk into bs.en_pack (width = min(cap, U) cells per slot; h_qrank[b] = the train users in front of slot b's
// newcomer in set order; h_qo as the chunk was given it).  Three or four launches, no round trip: the caller copies the block
// back.
void entered_chunk(const Train& tr, const NeighborTable& nt, QueryBatchScratch& bs, int32_t C, int32_t take, int32_t width,
                   const int64_t* h_qo, const int32_t* h_qrank, hipStream_t st);
// Entered queries of update queries (knncf_update_entered*; DESIGN.md "Entered queries of update queries"): the same after
// foldin_batch_neighbors(topk = false) on an UPDATE chunk.  h_self[b] = the dense index of slot b's changer in the fit or -1,
// h_qrank[b] = its place in set order (dense(c) for a fitted one).  A slot without additional rows (bs.ao, the chunk's) reports
// nothing.  The block is an EnteredPack followed by prev [C * width] (entered_pack_prev): the changer's position in the
// stored list or -1; `displaced` holds out_other of an entered cell and -1 otherwise.  pos == EN_TAIL marks a cell that the
// stored list cannot decide (a tail row): the caller resolves it.  Up to six launches, no round trip.
// Entered queries of revise queries (knncf_revise_entered*; DESIGN.md "Entered queries of revise queries"): the same call after
// a REVISE chunk.  h_ro [C + 1] = the chunk's removed CSR on the host (all 0 for a chunk without removals, which is an update
// chunk); a fitted slot with removals reports even without additional rows.
static constexpr int32_t EN_TAIL = -2;
inline size_t entered_update_pack_bytes(int32_t C, int32_t width) { return (size_t)C * ((size_t)width * 24 + 4); }
inline int32_t* entered_pack_prev(const EnteredPack& p, int32_t C) { return p.counts + C; }
void entered_update_chunk(const Train& tr, const NeighborTable& nt, QueryBatchScratch& bs, int32_t C, int32_t take, int32_t width,
                          const int64_t* h_qo, const int32_t* h_self, const int64_t* h_ro, const int32_t* h_qrank, hipStream_t st);
// the first stage of entered_update_chunk alone: the chunk's report bitmaps [C][ceil(U / 64)], bit v of row b = fitted user v is
// reported for slot b (tail rows included; a user without a built list is reported whenever the changer is not in it).  They
// lie in the chunk's sort keys until the next chunk.  No trace line, no round trip.
const unsigned long long* entered_update_flags(const Train& tr, const NeighborTable& nt, QueryBatchScratch& bs, int32_t C, int32_t take,
                                               const int64_t* h_qo, const int32_t* h_self, const int32_t* h_qrank, hipStream_t st);

// ---- append.hip: new ratings into the fit, the neighbour lists they cannot change kept (knncf_append; DESIGN.md "Append") ----
// Everything here is over the OLD fit's dense users (U of them, Wu = ceil(U / 64) bitmap words) unless said otherwise.
struct AppendScratch {
    DArr<unsigned long long> stale;  // [Wu] users whose list the append may change: the changers and every reported user
    DArr<unsigned long long> kept, gone;  // [Wu] built and not stale (K) / built and stale (B ∩ S)
    DArr<int64_t> pre;               // [max(U, Wu) + 1] scan cells
    DArr<uint32_t> k_a, k_b, v_a, v_b;  // [U] the users by ascending raw id (keys: the raw id with its sign bit flipped)
    DArr<int32_t> map;               // [U] old dense user -> new dense user
    DArr<int32_t> dropped;           // [min(cap, U)] raw ids of B ∩ S in dense order
    DArr<int64_t> totals;            // [5] |K|, |B ∩ S|; the removal stage's verdict: the surviving rows, the first missed removal or -1;
                                     // knncf_remove_users: the leavers in B ∩ S
    // knncf_remove_users' marking: the leavers as dense users of the old fit
    DArr<unsigned long long> leaver; // [Wu] bit v: dense user v leaves
    DArr<int32_t> leaver_dense;      // [L]
    // knncf_amend's removal stage: the table of removals and, over the old fit's n file rows in tiles of KNNCF_AMEND_TILE, the
    // removed-row bitmap with the tiles' survivor counts and offsets
    DArr<uint64_t> am_keys;          // [n_removed] (user << 32 | item, both as uint32), ascending
    DArr<uint32_t> am_removers;      // [R] the distinct users of the removals, ascending as uint32
    DArr<int64_t> am_roff;           // [R + 1] remover r's keys are am_keys [am_roff[r], am_roff[r + 1])
    DArr<int32_t> am_hits;           // [n_removed] train rows that matched each removal
    DArr<unsigned long long> am_bits;  // [ceil(n / 64)] bit i: file row i is removed
    DArr<int32_t> am_tile_cnt;       // [tiles]
    DArr<int64_t> am_tile_off;       // [tiles + 1]
};
// stale = 0
void append_begin(AppendScratch& as, int32_t U, hipStream_t st);
// stale |= the OR of a chunk's report bitmaps (entered_update_flags) and the chunk's fitted changers (d_self [C], -1: a newcomer)
void append_mark(AppendScratch& as, int32_t U, int32_t C, const unsigned long long* d_bits, const int32_t* d_self, hipStream_t st);
// as.kept / as.gone from nt.seq (all: every built list counts as stale — the plain refit), as.totals, and the first
// min(|B ∩ S|, cap) raw ids of B ∩ S in dense order into as.dropped.  Two launches.
void append_sets(AppendScratch& as, const Train& tr, const NeighborTable& nt, bool all, int64_t cap, hipStream_t st);
// as.map: the place of every old user among new_ukeys [new_U] (the new fit's trie keys in dense order, new_U > 4), -1 for a user
// whose key they do not hold (it left the fit: knncf_remove_users)
void append_remap(AppendScratch& as, const Train& tr, const uint32_t* new_ukeys, int32_t new_U, hipStream_t st);
// the build numbers knncf_neighbors_batch over K in ascending raw id gives: seq[map[v]] = 1 << 32 | rank of uid[v] among K, for
// v in K (map == nullptr: the identity).  One sort of U keys, one single-block scan.
void append_number(AppendScratch& as, SortWorkspace& ws, const Train& tr, const int32_t* d_map, int64_t* d_seq, hipStream_t st);
// the table stays (no user joined): cnt = 0 and seq = -1 for every user outside K
void append_clear(AppendScratch& as, int32_t U, int32_t* d_cnt, int64_t* d_seq, hipStream_t st);
// the table moves: row map[v] of `to` (cleared beforehand: cnt 0, seq -1) = row v of `from` for v in K, ids through the map,
// similarities verbatim; both tables have from.kcap cells per row
void append_carry(AppendScratch& as, int32_t U, const NeighborTable& from, NeighborTable& to, hipStream_t st);
// knncf_amend's removal stage, after append_begin.  The table as the host sorted it (h_keys [n_removed] ascending and distinct,
// n_removed > 0; h_removers [R] and h_roff [R + 1] its CSR by user): the removed-row bitmap of tr's file rows, the tile offsets
// and the verdict in as.totals[2..3] — [2] = the surviving rows, [3] = the first cell of the table that did not match exactly
// one train row, or -1.  Two launches; the host arrays must live until the stream has passed the copies.
void amend_flag(AppendScratch& as, const Train& tr, const uint64_t* h_keys, int64_t n_removed, const uint32_t* h_removers,
                const int64_t* h_roff, int32_t R, hipStream_t st);
// after amend_flag: tr's surviving file rows, in file order, to the front of the three arrays (as.totals[2] cells each); tr's
// own arrays are only read.  No atomics.
void amend_compact(AppendScratch& as, const Train& tr, int32_t* d_user, int32_t* d_item, double* d_rating, hipStream_t st);
// knncf_remove_users' removal stage, after append_begin: amend_flag for whole users.  h_leavers [L] the raw ids of the leavers as
// uint32, ascending and distinct, L > 0: every file row of one of them is flagged; as.totals[2] = the surviving rows, [3] = -1.
// amend_compact follows as after amend_flag.  Two launches; the host array must live until the stream has passed the copy.
void amend_flag_users(AppendScratch& as, const Train& tr, const uint32_t* h_leavers, int32_t L, hipStream_t st);
// knncf_remove_users' marking.  append_leavers: as.leaver / as.leaver_dense from the leavers' dense users h_dense [L] (distinct,
// of [0, U)).  append_holders: stale |= every user whose stored list holds a leaver in one of its min(cnt, kcap) cells, and the
// leavers; one pass over nt.idx, no read-back (in_lds: the bitmap is copied into LDS by every workgroup — ceil(U / 64) * 8 bytes
// must fit).  append_leavers_gone, after append_sets: as.totals[4] = the leavers in B ∩ S.
void append_leavers(AppendScratch& as, int32_t U, const int32_t* h_dense, int32_t L, hipStream_t st);
void append_holders(AppendScratch& as, const Train& tr, const NeighborTable& nt, bool in_lds, hipStream_t st);
void append_leavers_gone(AppendScratch& as, int32_t L, hipStream_t st);

// ---- reco_batch.hip: recommendations :651-674 for users of the fit (knncf_recommend, knncf_recommend_batch; DESIGN.md "Batched
// recommendations") ----
static constexpr int RB_TPB = 256;
static constexpr int RB_TILE = 2048;      // items per workgroup of the tile selection
static constexpr int RB_FAST_N = 32;      // n up to here: arg-min selection; beyond: the segmented full order of foldin.hip
static constexpr int RB_MAX_CHUNK = 1024; // users per chunk at most
// device bytes per user of a chunk that the chunk rule of knncf.h counts
inline int64_t reco_batch_bytes(int32_t I) { return 96 * (int64_t)I; }
struct RecoBatchScratch {
    DArr<int32_t> slot_user, slot_raw;  // [C] dense user (-1: absent from train) and raw id of each slot
    DArr<int32_t> counts;               // [C] min(n, I - #rated)
    DArr<uint32_t> id_rank;             // [I] place of each dense item in ascending raw-id order
    DArr<uint64_t> p_key;               // [C][tiles][n] the tiles' winners: order key, raw-id rank, dense item
    DArr<uint32_t> p_rank, p_item;
    DArr<int32_t> row_users, row_items; // [C][I] (user, item) rows of the prediction batch
};
// by_id = dense items by ascending raw id (k_a / k_b / v_a hold I entries); foldin.hip orders its chunks with it too
void launch_reco_id_order(const Train& tr, SortWorkspace& ws, uint64_t* k_a, uint64_t* k_b, uint32_t* v_a, uint32_t* by_id, hipStream_t st);
// rb.id_rank (bs lends its key buffers and keeps by_id)
void reco_batch_id_rank(const Train& tr, QueryBatchScratch& bs, RecoBatchScratch& rb, SortWorkspace& ws, hipStream_t st);
void reco_batch_rows(const Train& tr, const RecoBatchScratch& rb, int32_t C, int32_t* d_users, int32_t* d_items, hipStream_t st);
// d_rated [C][I], d_info [C][4] (k_qb_take's layout: [1] = rated items), rb.counts
void reco_batch_mark(const Train& tr, const RecoBatchScratch& rb, int32_t C, int32_t n, uint8_t* d_rated, long long* d_info, hipStream_t st);
// n <= RB_FAST_N: d_items / d_preds [C][n], the first rb.counts[s] cells of row s
void reco_batch_select(const Train& tr, RecoBatchScratch& rb, int32_t C, int32_t n, const double* d_pred, const uint8_t* d_rated,
                       int32_t* d_items, double* d_preds, hipStream_t st);

// ---- similarity_batch.hip: many fresh-closure pair similarities in one pass (knncf_similarity_batch*, knncf_knn_similarity_batch;
// DESIGN.md "Bulk similarities") ----
// device bytes per pair of a chunk that the chunk rule of knncf.h counts: two raw ids and one double
static constexpr int64_t PAIR_BYTES = 16;
// d_out[j] = sim(train)(d_us[j], d_vs[j]) on a closure of its own, j < n: raw ids, looked up on the device (adjusted cosine, or the
// Jaccard coefficient with `jaccard`).  One launch; reads the fit only.
void launch_pair_similarity(const Train& tr, bool jaccard, const int32_t* d_us, const int32_t* d_vs, int64_t n, double* d_out,
                            hipStream_t st);
// d_out[j] = 0.0 + the similarity of d_vs[j] in the neighbour list of d_us[j] (raw ids), 0.0 when it is not there or either id is
// absent from train; every list the pairs need exists.  Makes nt's id-sorted copies when they are not current.
void launch_pair_knn_lookup(const Train& tr, NeighborTable& nt, const int32_t* d_us, const int32_t* d_vs, int64_t n, double* d_out,
                            hipStream_t st);

}  // namespace knncf
