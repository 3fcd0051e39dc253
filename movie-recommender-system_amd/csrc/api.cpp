// api.cpp — the C ABI of include/knncf.h: handle, orchestration of K0-K9 on one HIP stream,
// scalar queries.  No CPU arithmetic path exists here: every number an entry point returns was
// produced by the HIP kernels (prep.hip, gemm.hip, select.hip, predict.hip).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <map>
#include <vector>

#include "engine.h"

using namespace knncf;

namespace knncf {
// small kernels of the orchestrator (neighbours.hip)
void launch_first_rows(int64_t n, const int32_t* d_du, const int32_t* d_di, const double* d_user_avg, int32_t own_lo, int32_t own_hi,
                       uint32_t* d_first, hipStream_t st);
void launch_length_keys(int32_t count, const int32_t* d_list, const int64_t* d_u_ptr, int32_t max_len, uint64_t* d_key, hipStream_t st);
void launch_collect_new(int32_t U, const uint32_t* d_first, int64_t* d_seq, int64_t epoch, int32_t own_lo, int32_t own_hi,
                        int32_t* d_list, int32_t* d_count, hipStream_t st);
void launch_fallback_keys(int32_t U, const double* d_exact, uint64_t* d_keys, uint32_t* d_vals, hipStream_t st);
void launch_fallback_write(int32_t user, int32_t take, int32_t kcap, const uint32_t* d_sorted_vals,
                           const double* d_exact, int32_t* nbr_idx, double* nbr_sim, int32_t* nbr_cnt,
                           hipStream_t st);
void launch_jaccard_pair(const Train& tr, int32_t u, int32_t v, double* d_out, hipStream_t st);
}  // namespace knncf

struct StageTimer {
    hipEvent_t a, b;
    double* acc;
};

struct knncf_handle {
    knncf_config cfg{};
    hipStream_t stream = nullptr;
    std::string err;
    Train tr;
    PrepScratch prep;
    bool fitted = false, committed = false;
    int8_t short_rows = -1;  // the train set has a user with <= 4 ratings (1 / 0; -1 = not looked up since the fit)
    NeighborTable nt;
    int64_t epoch = 1;
    // panels
    int64_t U_pad = 0, K_pad = 0;
    DArr<bf16_t> Bpanel;
    bool b_ready = false;
    int32_t head = 0;  // dense head width of the hybrid similarity
    double tail_pairs_full = 0.0;
    DArr<int32_t> colmap;
    // per-row tail entry lists of the current head (rebuilt with the B panel)
    DArr<int32_t> te_cnt, te_item;
    DArr<float> te_x, row_tail_abs, row_head_sq;
    DArr<float> row_len;  // Jaccard handles: |I(v)| as float for select.hip
    // double-buffered row-block panels: a producer stream (densify, GEMM, tail) runs one block ahead
    // of the consumer stream (select, re-rank)
    hipStream_t stream2 = nullptr;
    DArr<bf16_t> Apanel[2];
    DArr<float> S[2];
    DArr<float> S_full;            // symmetric path: the whole U_pad x U_pad similarity panel (raw storage)
    DArr<uint32_t> sym_tiles;      // its tile order (gemm_sym_tile_list), cached per U_pad
    DArr<int32_t> redo_rows;       // users whose select pass is repeated with the plain thresholds (build_neighbors)
    int32_t sym_tiles_n = 0;       // tiles per side the cached list was built for
    hipEvent_t ev_produced[2] = {nullptr, nullptr}, ev_consumed[2] = {nullptr, nullptr}, ev_ready = nullptr;
    int32_t* pinned_cnt = nullptr;
    size_t pinned_cap = 0;
    SelectScratch sel;
    SliceScratch slices;
    NeighborTable pt;       // Personalized (no k): every non-zero similarity of every user (ids ascending, self included)
    bool pt_ready = false;
    PersonalRows prow;      // Personalized (no k) beyond the table: first-use copies + the row scratch (personalized.hip)
    bool prow_ready = false, prow_checked = false;  // the copies are built; the fitted path's refusals were checked
    QueryBatchScratch query_batch;  // fold-in queries (foldin.hip)
    RecoBatchScratch reco_batch;  // knncf_recommend / knncf_recommend_batch (reco_batch.hip); lends query_batch's prediction and sort buffers
    AppendScratch append;   // knncf_append (append.hip)
    DArr<int32_t> build_list, build_count;
    DArr<uint32_t> first_row;
    // test scratch
    DArr<int32_t> t_du, t_di, t_users, t_items;
    DArr<double> t_pred, t_err, t_ratings, t_partial, scalar_out;
    DArr<unsigned long long> scalar_u64;
    DArr<uint8_t> t_owned;
    DArr<int64_t> t_counts;
    DArr<int32_t> sweep_ks;  // [64] the k values of knncf_mae_sweep*
    // one chunk of knncf_explain_batch's host form: [C * cap] terms, [C] counts and predictions, [2 C] sums
    DArr<int32_t> ex_raters, ex_counts;
    DArr<double> ex_sims, ex_devs, ex_sums, ex_pred;
    // one launch of the query explanations (QB_EXPLAIN, QB_EXPLAIN_ALL): the same outputs of its rows in ONE block, 20 * cap + 28 bytes per
    // row, so that one copy brings a sub-range back (explain_pack)
    DArr<double> ex_pack;
    // knncf_explain_personalized* and knncf_*_explain_personalized* with KNNCF_EXPLAIN_BY_WEIGHT: the selected terms of a launch's
    // rows before they are ranked, 20 * cap bytes per row (explain_select.h)
    DArr<double> ex_stage;
    // one chunk of knncf_similarity_batch / knncf_knn_similarity_batch's host forms: [C] raw ids and results (similarity_batch.hip)
    DArr<int32_t> pair_us, pair_vs;
    DArr<double> pair_out;
    // host mirrors for scalar queries
    std::vector<uint32_t> h_ukeys, h_ikeys;
    std::vector<int32_t> h_uid;
    std::vector<int64_t> h_uptr;  // row extents (update queries)
    std::vector<double> h_uavg;   // user means (recommendations: whose neighbourhood the reference builds)
    std::vector<int32_t> h_utable;  // the direct raw id -> dense user table, when the fit has one (bulk kNN similarities)
    knncf_timings tm{};
    std::vector<StageTimer> pending;
    std::vector<hipEvent_t> event_pool;
};

extern "C" { static void build_unbuilt_neighbors(knncf_handle* h); }  // (beside knncf_neighbors_batch, whose batch build it shares)

namespace {

hipEvent_t get_event(knncf_handle* h) {
    if (!h->event_pool.empty()) {
        hipEvent_t e = h->event_pool.back();
        h->event_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    KN_HIP(hipEventCreate(&e));
    return e;
}

struct Stage {  // RAII: times a stage of device work with HIP events on the stream it is launched on
    knncf_handle* h;
    StageTimer t;
    hipStream_t st;
    Stage(knncf_handle* h_, double* acc, hipStream_t st_ = nullptr) : h(h_), st(st_ ? st_ : h_->stream) {
        t.a = get_event(h);
        t.b = get_event(h);
        t.acc = acc;
        (void)hipEventRecord(t.a, st);
    }
    ~Stage() {
        (void)hipEventRecord(t.b, st);
        h->pending.push_back(t);
    }
};

// end of every entry point: the engine's streams are drained (results in caller-provided device buffers are complete on
// return, include/knncf.h) and the stage timers of the call are read
void resolve_timers(knncf_handle* h) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamSynchronize(h->stream2);
    for (auto& t : h->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) *t.acc += ms;
        h->event_pool.push_back(t.a);
        h->event_pool.push_back(t.b);
    }
    h->pending.clear();
}

template <class F>
int guarded(knncf_handle* h, F&& f) {
    if (!h) return KNNCF_E_INVALID;
    // the calling thread's current device is restored on every path (a JVM thread may drive several handles)
    struct DeviceGuard {
        int prev = -1;
        ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    } guard;
    try {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) {
            // (a thread without a usable HIP context, e.g. after a sticky error: nothing to restore, and the failure — if it
            // persists — becomes this call's status instead of the call running on whatever device is current)
            (void)hipGetLastError();
            KN_HIP(hipSetDevice(h->cfg.device));
        } else if (cur != h->cfg.device) {
            guard.prev = cur;
            KN_HIP(hipSetDevice(h->cfg.device));
        }
        f();
        resolve_timers(h);
        return KNNCF_OK;
    } catch (const Error& e) {
        h->err = e.what();
        (void)hipStreamSynchronize(h->stream);
        (void)hipStreamSynchronize(h->stream2);
        (void)hipGetLastError();
        h->pending.clear();
        return e.status;
    } catch (const std::bad_alloc&) {
        h->err = "host allocation failed";
        return KNNCF_E_NOMEM;
    } catch (const std::exception& e) {
        h->err = e.what();
        return KNNCF_E_INVALID;
    }
}

void require_fitted(knncf_handle* h, bool committed = true) {
    KN_REQUIRE(h->fitted, KNNCF_E_STATE, "call knncf_fit first");
    if (committed) KN_REQUIRE(h->committed, KNNCF_E_STATE, "sharded handle: call knncf_shard_commit after the exchange");
}

void load_host_ids(knncf_handle* h) {
    if (!h->h_ukeys.empty() || h->tr.U == 0) return;
    Train& tr = h->tr;
    h->h_ukeys.resize(tr.U);
    h->h_ikeys.resize(tr.I);
    h->h_uid.resize(tr.U);
    KN_HIP(hipMemcpyAsync(h->h_ukeys.data(), tr.ukeys.p, tr.U * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    KN_HIP(hipMemcpyAsync(h->h_ikeys.data(), tr.ikeys.p, tr.I * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    KN_HIP(hipMemcpyAsync(h->h_uid.data(), tr.uid.p, tr.U * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    KN_HIP(hipStreamSynchronize(h->stream));
}

int32_t dense_user(knncf_handle* h, int32_t raw) {
    load_host_ids(h);
    return dense_lookup(h->h_ukeys.data(), h->tr.U, raw);
}
// ratings of dense user du in train
int64_t train_row_length(knncf_handle* h, int32_t du) {
    if (h->h_uptr.empty()) {
        h->h_uptr.resize((size_t)h->tr.U + 1);
        KN_HIP(hipMemcpyAsync(h->h_uptr.data(), h->tr.u_ptr.p, h->h_uptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        KN_HIP(hipStreamSynchronize(h->stream));
    }
    return h->h_uptr[du + 1] - h->h_uptr[du];
}
// mean of dense user du in train
double train_user_avg(knncf_handle* h, int32_t du) {
    if (h->h_uavg.empty()) {
        h->h_uavg.resize((size_t)h->tr.U);
        KN_HIP(hipMemcpyAsync(h->h_uavg.data(), h->tr.user_avg.p, h->h_uavg.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        KN_HIP(hipStreamSynchronize(h->stream));
    }
    return h->h_uavg[du];
}
int32_t dense_item(knncf_handle* h, int32_t raw) {
    load_host_ids(h);
    return dense_lookup(h->h_ikeys.data(), h->tr.I, raw);
}

// the train set has a user with <= 4 ratings: looked up once per fit
bool has_short_rows(knncf_handle* h) {
    if (h->short_rows < 0) {
        Train& tr = h->tr;
        std::vector<int64_t> ptr((size_t)tr.U + 1);
        KN_HIP(hipMemcpyAsync(ptr.data(), tr.u_ptr.p, ptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        KN_HIP(hipStreamSynchronize(h->stream));
        h->short_rows = 0;
        for (int32_t u = 0; u < tr.U; ++u)
            if (ptr[u + 1] - ptr[u] <= 4) { h->short_rows = 1; break; }
    }
    return h->short_rows == 1;
}

// A neighbour query that builds a list numbers that build on the queried shard only (the other shards never see the call).
// With a <= 4-rating user in train the owner rule of rerank.hip (pair_sim: seq_v < seq_u) reads those numbers on every shard,
// so such a query would let the shards disagree on a pair's summation order: refused.  The mae / predict path
// numbers every user on every shard (ensure_neighbors_for_rows) and stays open.
void require_shard_numbering(knncf_handle* h) {
    if (h->cfg.shard_count == 1) return;
    KN_REQUIRE(!has_short_rows(h), KNNCF_E_UNSUPPORTED,
               "neighbours: on a shard handle whose train set has a user with <= 4 ratings, a neighbourhood that knncf_mae / "
               "knncf_predict_batch has not built yet cannot be built by a query (its build number would exist on this shard only)");
}

template <class T>
T fetch(knncf_handle* h, const T* d, int64_t idx) {
    T v;
    KN_HIP(hipMemcpyAsync(&v, d + idx, sizeof(T), hipMemcpyDeviceToHost, h->stream));
    KN_HIP(hipStreamSynchronize(h->stream));
    return v;
}

void reset_neighbors(knncf_handle* h) {
    Train& tr = h->tr;
    NeighborTable& nt = h->nt;
    nt.k = h->cfg.k;
    nt.kcap = std::max(0, std::min(nt.k, tr.U - 1));
    size_t cells = (size_t)tr.U * (size_t)std::max(nt.kcap, 1);
    nt.idx.ensure(cells);
    nt.sim.ensure(cells);
    nt.by_id_valid = false;  // (uidx / usim: made by launch_predict when a kernel wants them)
    nt.cnt.ensure(tr.U);
    nt.seq.ensure(tr.U);
    KN_HIP(hipMemsetAsync(nt.cnt.p, 0, tr.U * sizeof(int32_t), h->stream));
    KN_HIP(hipMemsetAsync(nt.seq.p, 0xff, tr.U * sizeof(int64_t), h->stream));  // -1
    h->epoch = 1;
}

// per-pair error bound of the bf16 GEMM entry, excluding the per-row accumulation term that
// select.hip adds from the row length: both operands rounded to bf16 (u = 2^-8, via fp32),
// products exact in fp32, sum |x y| <= ||x|| ||y|| <= 1
// split in two: the relative operand-rounding part (2u + u^2), which select.hip scales by the norm of the row's
// head part (sum_head |x y| <= ||x_head|| ||y_head|| <= ||x_head||), and the absolute rest
float gemm_eps_operand(bool fp16) {
    const double u = ldexp(1.0, fp16 ? -11 : -8) * 1.001;  // bf16: 8 significant bits; fp16: 11
    return (float)(2 * u + u * u);
}
float gemm_eps_rest(bool fp16) {
    // the tail's fp32 operand/product roundings (3 * 2^-24 of sum |x y| <= 1); fp16: |pre| <= 1, below 2^-14 the
    // grid is absolute, 2^-25 per operand: sum (|x| + |y|) 2^-25 <= 2 sqrt(n) 2^-25 < 6e-6 for n < 10^4
    // + the tail's row-side factor travels with its 6 low mantissa bits replaced (select.hip: piece descriptors):
    //   relative 2^-17 of sum |x y| <= 1
    return (float)(4e-7 + (fp16 ? 6e-6 : 0.0) + 8e-6);
}

// per-row shortlist storage: rows whose error band holds more candidates than this take the exact
// fallback.  Heavy raters have compressed similarity distributions (many candidates inside the
// bf16 band), so the store is generous; the re-rank consumes it in LDS-sized chunks.
int32_t shortlist_cap(int32_t k, int32_t U) {
    int64_t want = std::max<int64_t>(16384, 4 * (int64_t)k);
    int64_t cap = 64;
    while (cap < want) cap <<= 1;
    int64_t upper = 64;
    while (upper < U) upper <<= 1;
    return (int32_t)std::min(cap, upper);
}

// Width H of the dense head of the hybrid similarity.  Cost model (measured rates, MI355X): a dense
// column costs 2 * rows * U flops on the MFMA GEMM; a tail item with c raters costs c^2 * rows / U
// LDS accumulator updates in k_tail_select.  Items are in descending popularity, so the optimum is a prefix.
int32_t choose_head(knncf_handle* h, int32_t rows_total, bool symmetric) {
    Train& tr = h->tr;
    const int32_t I = tr.I;
    const std::vector<int64_t>& c = tr.pop_count;
    std::vector<double> tail_sq((size_t)I + 1, 0.0);
    for (int32_t j = I - 1; j >= 0; --j) tail_sq[j] = tail_sq[j + 1] + (double)c[j] * (double)c[j];
    int32_t H;
    if (h->cfg.head_items == KNNCF_HEAD_ALL) {
        H = I;
    } else if (h->cfg.head_items > 0) {
        H = (int32_t)std::min<int64_t>(h->cfg.head_items, I);
    } else {
        // marginal rates measured on MI355X at the ml-25m shape (head sweeps 192 .. 1024, profiles/README.md; re-measured in
        // round 3 with the overlapped GEMM and the 6-VALU drain: 0.0195 ms per dense column on the symmetric path = 2.7e15
        // full-square flops per second, 4.2e-13 s per tail pair product — the optimum stays at 384 / 256): full-square
        // flops per second bought by one more dense column — the symmetric launch computes half of them — and tail pair
        // products per second through k_tail_select.  Re-measured with the re-scheduled k-loop of k_gemm_nt_ov
        // (profiles/gemm_kloop_syn25m_1gpu.json).  Symmetric, head sweep 256 .. 768 of the step: the launch is 0.7 ms shorter
        // at every width, a column costs 0.0164 ms on average and 0.0189 ms between 384 and 448 (2.8e15 .. 3.2e15; 2.6e15 by
        // gemm_bench on a slower device), the tail gives back 0.0178 ms there — 384 stays the fastest head by 0.16 ms per
        // step.  Row blocks of 16 384, gemm_bench K = 128 .. 768: 1.3e15 .. 1.4e15 (the parent 1.28e15 in the same job), two
        // sweeps that differ by up to 0.35 ms per launch; no step sweep was run on that path.  Both rates stay as they are.
        const double RATE_DENSE = symmetric ? 2.8e15 : 1.2e15;
        const double RATE_SPARSE = 2.3e12;
        const double frac = (double)rows_total / (double)tr.U;
        const double U_pad = (double)round_up(tr.U, 256);
        double best = 1e300;
        H = I;
        for (int64_t cand = 64;; cand += 64) {
            int32_t hc = (int32_t)std::min<int64_t>(cand, I);
            double cost = 2.0 * rows_total * U_pad * (double)round_up(hc, 64) / RATE_DENSE + tail_sq[hc] * frac / RATE_SPARSE;
            if (cost < best) { best = cost; H = hc; }
            if (hc == I) break;
        }
        // Jaccard handles count common items in the panel: fp16 holds the counts exactly up to 2048 (build_neighbors refuses a
        // wider head unless KNNCF_FLAG_F32_PANEL lifts the limit) — the cost model must not pick what the build then refuses;
        // the tail takes the remaining items and the counts stay exact
        if (tr.jaccard && (h->cfg.flags & KNNCF_FLAG_F32_PANEL) == 0) H = std::min(H, 2048);
    }
    h->tail_pairs_full = tail_sq[H];
    return H;
}

// build the neighbourhoods of the users in h->build_list[0 .. count)
void build_neighbors(knncf_handle* h, int32_t count) {
    Train& tr = h->tr;
    NeighborTable& nt = h->nt;
    if (count <= 0 || nt.kcap <= 0) return;
    KN_REQUIRE(h->cfg.similarity != KNNCF_SIM_ONE, KNNCF_E_UNSUPPORTED,
               "kNN neighbourhoods with similarityOne: every similarity is 1.0, the neighbourhood is the first k users in Set order — not built");
    hipStream_t st = h->stream;
    if (count > 256) {  // (tests/test_boundary_premises.py holds this 256 and the `count * 2 >= U` below as literals: move together)
        // longest rows first (LPT): one workgroup per row in select and re-rank, and the row lengths are heavy-tailed
        // (ml-25m shape: mean 123 ratings, maximum 7485) — a long row dispatched last holds the launch open alone.
        // The order of the list carries no meaning (the users' build sequence numbers are already assigned).
        PrepScratch& sc = h->prep;
        sc.k64_a.ensure(count); sc.k64_b.ensure(count); sc.v32_b.ensure(count);
        launch_length_keys(count, h->build_list.p, tr.u_ptr.p, tr.I, sc.k64_a.p, st);  // (a row holds every item at most once)
        sort_pairs_u64_u32(sc.sort, sc.k64_a.p, sc.k64_b.p, reinterpret_cast<const uint32_t*>(h->build_list.p), sc.v32_b.p, count, bits_for((uint64_t)tr.I), st);
        KN_HIP(hipMemcpyAsync(h->build_list.p, sc.v32_b.p, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    }
    const bool fp16 = (h->cfg.flags & KNNCF_FLAG_BF16_FILTER) == 0;
    const bool s_fp16 = (h->cfg.flags & KNNCF_FLAG_F32_PANEL) == 0;  // similarity panel stored as fp16 (half the HBM traffic)
    h->U_pad = round_up(tr.U, 256);
    const int64_t U_pad = h->U_pad;
    size_t free_b = 0, total_b = 0;
    KN_HIP(hipMemGetInfo(&free_b, &total_b));
    const int64_t s_elem = s_fp16 ? 2 : 4;
    // SYMMETRIC PATH (whole-matrix builds on one GPU): S = B B^T is symmetric, so when (nearly) every user's row is wanted
    // the whole U_pad x U_pad panel is produced by ONE launch that computes the tiles on and above the diagonal and stores
    // each of them twice (gemm.hip: SYM) — half the MFMA work of the row-block launches, the same stored values bit for
    // bit — and the row blocks below only run select + re-rank, reading their rows out of it by dense user index.
    // 288 GB of HBM hold it easily at the ml-25m shape (53 GB as fp16); shapes whose square does not fit (syn-1M: 2 TB)
    // and partial / sharded builds take the row-block path.
    const size_t sym_bytes = (size_t)U_pad * (size_t)U_pad * (size_t)s_elem;
    // (what this handle already holds counts as free: the decision must not flip between two builds of the same shape because
    // the first one allocated — measured: a handle built beside another one's 135 GB sat exactly on the edge, released the
    // 53 GB panel in its second build and spent 1.5 s re-allocating)
    size_t own = h->S_full.bytes() + h->sel.cand_idx.bytes() + h->sel.cand_approx.bytes() + h->sel.grp_v0.bytes() + h->sel.grp_x.bytes();
    for (int s = 0; s < 2; ++s) own += h->S[s].bytes() + h->Apanel[s].bytes();
    // (`count * 2 >= U`: a literal of tests/test_boundary_premises.py — move together)
    bool use_sym = h->cfg.shard_count == 1 && (int64_t)count * 2 >= tr.U && U_pad / 256 < 65536 &&
                   sym_bytes <= (free_b + own) / 3 && !getenv("KNNCF_DEBUG_NO_SYMMETRIC_GEMM");
    if (use_sym) {
        try {
            h->S_full.ensure((sym_bytes + 3) / 4);
        } catch (const Error& e) {  // (fragmented / shared device: the row-block path needs far less in one piece)
            if (e.status != KNNCF_E_NOMEM) throw;
            (void)hipGetLastError();
            use_sym = false;
        }
    }
    if (!h->b_ready) {
        // hybrid similarity: the H most-rated items are dense MFMA columns, the rest a sparse tail
        h->head = choose_head(h, count, use_sym);
        h->K_pad = round_up(h->head, 64);
        size_t need = (size_t)U_pad * h->K_pad * sizeof(bf16_t);
        KN_REQUIRE(need < free_b + h->Bpanel.bytes(), KNNCF_E_UNSUPPORTED,
                   "dense bf16 user panel does not fit in HBM; lower head_items");
        Stage s(h, &h->tm.densify_ms);
        h->colmap.ensure(tr.I);
        launch_colmap(tr, h->head, h->colmap.p, st);
        h->Bpanel.ensure((size_t)U_pad * h->K_pad);
        launch_densify(tr, nullptr, 0, tr.U, h->colmap.p, h->Bpanel.p, h->K_pad, U_pad, fp16, st);
        if (tr.jaccard) {
            // the counting GEMM stores exact integers: fp16 holds them up to 2048 (KNNCF_FLAG_F32_PANEL lifts the limit)
            KN_REQUIRE(!s_fp16 || h->head <= 2048, KNNCF_E_UNSUPPORTED, "Jaccard: more than 2048 dense head items need KNNCF_FLAG_F32_PANEL");
            h->row_len.ensure((size_t)row_len_size(tr.U));
            launch_row_len(tr, h->row_len.p, st);
        }
        if (h->head < tr.I) {
            h->te_cnt.ensure(tr.U); h->te_item.ensure(tr.n); h->te_x.ensure(tr.n);
            h->row_tail_abs.ensure(tr.U); h->row_head_sq.ensure(tr.U);
            launch_tail_entries(tr, h->colmap.p, h->te_cnt.p, h->te_item.p, h->te_x.p, h->row_tail_abs.p, h->row_head_sq.p, st);
        }
        h->b_ready = true;
        KN_HIP(hipMemGetInfo(&free_b, &total_b));
    }
    const int64_t K_pad = h->K_pad;
    const int32_t head = h->head;
    h->tm.head_items = head;
    if (use_sym) {
        const int32_t n_tiles = (int32_t)(U_pad / 256);
        if (h->sym_tiles_n != n_tiles) {
            std::vector<uint32_t> list;
            gemm_sym_tile_list(n_tiles, list);
            h->sym_tiles.ensure(list.size());
            KN_HIP(hipMemcpyAsync(h->sym_tiles.p, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            KN_HIP(hipStreamSynchronize(st));
            h->sym_tiles_n = n_tiles;
        }
        const int64_t n_listed = (int64_t)n_tiles * (n_tiles + 1) / 2;
        Stage s(h, &h->tm.gemm_ms);
        launch_gemm_sym(h->Bpanel.p, h->S_full.p, s_fp16, U_pad, h->K_pad, h->K_pad, U_pad, fp16, !tr.jaccard, h->sym_tiles.p, n_listed, st);
        h->tm.gemm_launches += 1;
        h->tm.gemm_flops_executed += 2.0 * 256.0 * 256.0 * (double)n_listed * (double)h->K_pad;
        // ordered pairs (row, other user) of the rows actually wanted x the dense columns (bench.py halves it)
        h->tm.gemm_flops_algorithmic += 2.0 * (double)count * (double)(tr.U - 1) * (double)h->head;
        KN_HIP(hipMemGetInfo(&free_b, &total_b));
    } else {
        h->S_full.release();
    }
    // rows per block from the similarity-panel budget (two slots: the producer stream runs ahead)
    size_t held = 0;
    for (int s = 0; s < 2; ++s) held += h->S[s].bytes() + h->Apanel[s].bytes();
    held += h->sel.cand_idx.bytes() + h->sel.cand_approx.bytes() + h->sel.grp_v0.bytes() + h->sel.grp_x.bytes();
    int64_t budget = h->cfg.workspace_bytes > 0 ? h->cfg.workspace_bytes / 2
                                                : (int64_t)std::min<size_t>((size_t)48 << 30, (free_b + held) / 4);
    // per panel row: the similarity row, the operand row, the shortlist store and the provisional group store
    int64_t per_row = (use_sym ? 0 : U_pad * s_elem + K_pad * 2) + (int64_t)shortlist_cap(nt.k, tr.U) * 8 + (int64_t)select_gcap(nt.k) * 36;
    // When ALL rows fit a third of what is free (at most 96 GB) they are ONE block: at the ml-25m shape 69 GB of shortlist and
    // group stores beside the 53 GB panel, select and re-rank then run as one launch each and a launch's tail of unfinished
    // rows is paid once (0.5 ms per step against two blocks).  Shapes that need several blocks anyway keep the 48 GB
    // budget: allocating more only costs (syn-1M, one shot: 1.7 s of extra hipMalloc time for 96 GB blocks).
    if (h->cfg.workspace_bytes <= 0) {
        const int64_t whole = round_up(count, 256) * per_row;
        if (whole <= (int64_t)std::min<size_t>((size_t)96 << 30, (free_b + held) / 3)) budget = std::max(budget, whole);
    }
    int64_t R = std::max<int64_t>(256, (budget / per_row) / 256 * 256);
    R = std::min<int64_t>(R, round_up(count, 256));
    const int64_t n_blocks = ceil_div(count, R);
    R = round_up(ceil_div(count, n_blocks), 256);  // equal blocks: no short straggler at the end
    // KNNCF_FLAG_OVERLAP: run the producer one block ahead.  Measured on MI355X (ml-25m shape): -5 % step
    // time, but GEMM and re-rank then contend for LDS/CUs (GEMM 890 -> 506 TFLOP/s), so it is opt-in.
    const bool overlap = (h->cfg.flags & KNNCF_FLAG_OVERLAP) != 0;
    const int slots = (overlap && n_blocks > 1 && !use_sym) ? 2 : 1;
    for (int s = 0; s < slots && !use_sym; ++s) {
        h->S[s].ensure((size_t)(R * U_pad * s_elem + 3) / 4);  // DArr<float> used as raw storage
        h->Apanel[s].ensure((size_t)R * K_pad);
    }
    const int32_t cap = shortlist_cap(nt.k, tr.U);
    const bool verify = (h->cfg.flags & KNNCF_FLAG_VERIFY_BOUND) != 0;
    h->sel.cand_idx.ensure((size_t)R * cap);
    h->sel.cand_approx.ensure((size_t)R * cap);
    h->sel.cand_cnt.ensure(R);
    h->sel.cand_eps.ensure(R);
    h->sel.row_entries.ensure(R);
    h->sel.grp_v0.ensure((size_t)R * select_gcap(nt.k));
    h->sel.grp_x.ensure((size_t)R * select_gcap(nt.k) * 8);
    h->sel.stats.ensure(4);
    KN_HIP(hipMemsetAsync(h->sel.stats.p, 0, 4 * sizeof(double), st));  // [0] bound check, [1] candidate row entries
    if (h->pinned_cap < (size_t)count) {
        if (h->pinned_cnt) KN_HIP(hipHostFree(h->pinned_cnt));
        h->pinned_cnt = nullptr;
        h->pinned_cap = 0;
        KN_HIP(hipHostMalloc((void**)&h->pinned_cnt, (size_t)count * sizeof(int32_t), hipHostMallocDefault));
        h->pinned_cap = (size_t)count;
    }
    // fp16 panel storage rounds the dense head once more: the GEMM clamps it to [-1, 1] first (the exact head sum lies
    // there, so clamping only moves towards it), where half an fp16 ulp is at most 2^-12
    const float eps_opnd = gemm_eps_operand(fp16);
    const float eps_rest = gemm_eps_rest(fp16) + (s_fp16 ? 2.45e-4f : 0.f);
    // producer: densify, GEMM.  Without the overlap it is the consumer's stream itself: an event wait across two
    // hardware queues costs ~0.1 ms each time (three blocks per step at ml-25m shape)
    hipStream_t sp = slots > 1 ? h->stream2 : h->stream;
    hipStream_t sc = h->stream;   // consumer: select, exact re-rank
    KN_HIP(hipEventRecord(h->ev_ready, sc));  // everything queued so far (fit, B panel) precedes the producer
    KN_HIP(hipStreamWaitEvent(sp, h->ev_ready, 0));
    // host copy of the build list (dense users in build order), fetched on first need
    std::vector<int32_t> h_rows;
    auto need_h_rows = [&] {
        if (!h_rows.empty()) return;
        h_rows.resize(count);
        KN_HIP(hipMemcpyAsync(h_rows.data(), h->build_list.p, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        KN_HIP(hipStreamSynchronize(st));
    };
    // rows (positions in the build list) whose anticipated thresholds overshot: once more through select + re-rank with the
    // plain thresholds, out of the panel Sp (whole matrix: indexed by user; a row block based at position rb: by block row)
    auto redo_marked = [&](const std::vector<int32_t>& marked, const void* Sp, bool by_user, int64_t rb) {
        need_h_rows();
        std::vector<int32_t> users(marked.size()), srow(marked.size());
        for (size_t j = 0; j < marked.size(); ++j) {
            users[j] = h_rows[marked[j]];
            srow[j] = (int32_t)(marked[j] - rb);
        }
        TailEntries te{h->te_cnt.p, h->te_item.p, h->te_x.p, h->row_tail_abs.p, h->row_head_sq.p, h->row_len.p};
        const int64_t chunk = std::min<int64_t>((int64_t)marked.size(), R);
        h->redo_rows.ensure(2 * (size_t)chunk);
        for (size_t j0 = 0; j0 < marked.size(); j0 += (size_t)R) {  // (the shortlist / group stores hold R rows)
            const int32_t m = (int32_t)std::min<size_t>((size_t)R, marked.size() - j0);
            KN_HIP(hipMemcpyAsync(h->redo_rows.p, users.data() + j0, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, st));
            KN_HIP(hipMemcpyAsync(h->redo_rows.p + chunk, srow.data() + j0, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, st));
            {
                Stage s(h, &h->tm.select_ms);
                launch_tail_select(tr, h->colmap.p, te, head < tr.I, Sp, by_user, s_fp16, U_pad, m, h->redo_rows.p, nt.k, eps_opnd, eps_rest, cap,
                                   h->sel.cand_idx.p, h->sel.cand_approx.p, h->sel.cand_cnt.p, h->sel.cand_eps.p, h->sel.grp_v0.p, h->sel.grp_x.p,
                                   select_gcap(nt.k), st, /*anticipate=*/false, by_user ? nullptr : h->redo_rows.p + chunk);
                h->tm.select_launches += 1;
            }
            {
                Stage s(h, &h->tm.rerank_ms);
                launch_rerank(tr, nt, m, h->redo_rows.p, cap, h->sel.cand_idx.p, h->sel.cand_approx.p, h->sel.cand_cnt.p, h->sel.cand_eps.p,
                              h->sel.stats.p, h->sel.row_entries.p, verify, st);
            }
            std::vector<int32_t> again(m);
            KN_HIP(hipMemcpyAsync(again.data(), h->sel.cand_cnt.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            KN_HIP(hipStreamSynchronize(st));
            for (int32_t j = 0; j < m; ++j) h->pinned_cnt[marked[j0 + j]] = again[j];
        }
    };
    const bool per_block_redo = !use_sym && n_blocks > 1;
    for (int64_t b = 0; b < n_blocks; ++b) {
        const int64_t rb = b * R;
        const int32_t rows = (int32_t)std::min<int64_t>(R, count - rb);
        const int64_t M = round_up(rows, 256);
        const int32_t* d_rows = h->build_list.p + rb;
        const int slot = (int)(b % slots);
        if (b >= slots) KN_HIP(hipStreamWaitEvent(sp, h->ev_consumed[slot], 0));  // S[slot] has been read
        if (!use_sym) {
            Stage s(h, &h->tm.densify_ms, sp);
            launch_densify(tr, d_rows, 0, rows, h->colmap.p, h->Apanel[slot].p, K_pad, M, fp16, sp);
        }
        if (!use_sym) {
            Stage s(h, &h->tm.gemm_ms, sp);
            launch_gemm_nt(h->Apanel[slot].p, h->Bpanel.p, h->S[slot].p, s_fp16, M, U_pad, K_pad, K_pad, K_pad, U_pad, fp16, !tr.jaccard, sp);
            h->tm.gemm_launches += 1;
            h->tm.gemm_flops_executed += 2.0 * (double)M * (double)U_pad * (double)K_pad;
            // SURVEY 8(d) per-unit figure x the units this launch processes: ordered pairs (row, other user)
            // x the dense columns it contracts
            h->tm.gemm_flops_algorithmic += 2.0 * (double)rows * (double)(tr.U - 1) * (double)head;
        }
        KN_HIP(hipEventRecord(h->ev_produced[slot], sp));
        KN_HIP(hipStreamWaitEvent(sc, h->ev_produced[slot], 0));
        TailEntries te{h->te_cnt.p, h->te_item.p, h->te_x.p, h->row_tail_abs.p, h->row_head_sq.p, h->row_len.p};
        h->prep.join_commit(sc);  // the item-major rater lists and the tile table (second part of prep_commit)
        const void* Sblk = use_sym ? (const void*)h->S_full.p : (const void*)h->S[slot].p;
        const int32_t gcap = select_gcap(nt.k);
        // rows [r0, r0 + nr) of this block through select: every per-row store is indexed by the launch row, so a part of the
        // block is the same launch on offset pointers
        auto select_rows = [&](int32_t r0, int32_t nr) {
            // sparse tail (LDS atomics per row tile) + histogram select, fused: one pass over S
            Stage s(h, &h->tm.select_ms, sc);
            const void* Sp = use_sym ? Sblk : (const void*)(static_cast<const char*>(Sblk) + (size_t)r0 * (size_t)U_pad * (size_t)s_elem);
            launch_tail_select(tr, h->colmap.p, te, head < tr.I, Sp, use_sym, s_fp16, U_pad, nr, d_rows + r0, nt.k, eps_opnd, eps_rest, cap,
                               h->sel.cand_idx.p + (size_t)r0 * cap, h->sel.cand_approx.p + (size_t)r0 * cap, h->sel.cand_cnt.p + r0, h->sel.cand_eps.p + r0,
                               h->sel.grp_v0.p + (size_t)r0 * gcap, h->sel.grp_x.p + (size_t)r0 * gcap * 8, gcap, sc);
            h->tm.select_launches += 1;
            h->tm.tail_pair_updates += h->tail_pairs_full * ((double)nr / (double)tr.U);
            h->tm.select_row_bytes += (double)s_elem * (double)nr * (double)tr.U;
        };
        // HEAVY ROWS AS SLICES.  One workgroup per row, rows longest first — but the re-rank of the few heaviest rows (their
        // candidates are heavy raters too: up to 33 x the median row's work at the ml-25m shape, 12 x at the 99.9th percentile,
        // scripts/analysis/row_work_profile.py) outlasts a sharded handle's whole launch: 1.6 - 3.2 ms per shard of config 4 where
        // the work is 1.4.  The top 0.2 % of such a block's rows are therefore re-ranked as P slices of their shortlists + a merge
        // (rerank.hip), P workgroups per row in the same launch: 1.68 ms on every shard (scripts/slice_sweep.sh; 160 rows the
        // same, 640 rows 1.83).  A whole-matrix launch hides that tail by itself, and there the slices' repeated row set-up
        // only costs (+0.2 ms at 256 rows, +0.85 at 2048), so blocks beyond 65 536 rows go unsliced.
        const int32_t slices = std::min<int32_t>(8, 8192 / std::max<int32_t>(nt.kcap, 1));
        // (KNNCF_DEBUG_SLICE_ROWS = n: the first n rows of every block instead — 0 turns slicing off; the small-shape parity tests
        // force it on with this)
        const char* force_slices = getenv("KNNCF_DEBUG_SLICE_ROWS");
        const int32_t n_heavy = slices < 2                         ? 0
                                : force_slices                     ? std::max<int32_t>(0, std::min<int32_t>(rows, atoi(force_slices)))
                                : (rows >= 4096 && rows <= 65536)  ? std::max<int32_t>(16, rows / 512)
                                                                   : 0;
        select_rows(0, rows);
        if (overlap && !per_block_redo) KN_HIP(hipEventRecord(h->ev_consumed[slot], sc));
        {
            Stage s(h, &h->tm.rerank_ms, sc);
            launch_rerank(tr, nt, rows, d_rows, cap, h->sel.cand_idx.p, h->sel.cand_approx.p, h->sel.cand_cnt.p, h->sel.cand_eps.p, h->sel.stats.p,
                          h->sel.row_entries.p, verify, sc, n_heavy, slices, &h->slices);
        }
        if (!overlap) KN_HIP(hipEventRecord(h->ev_consumed[slot], sc));
        if (per_block_redo) KN_HIP(hipMemcpyAsync(h->pinned_cnt + rb, h->sel.cand_cnt.p, rows * sizeof(int32_t), hipMemcpyDeviceToHost, sc));
        if (per_block_redo) {
            // several row blocks (syn-1M, capped workspaces): the block's panel slot is about to be recycled, so rows whose
            // anticipated thresholds overshot are re-selected NOW if they are many (one host round trip per block: the
            // blocks of such builds take tens of milliseconds each)
            KN_HIP(hipStreamSynchronize(sc));
            std::vector<int32_t> marked;
            for (int64_t r = rb; r < rb + rows; ++r)
                if (h->pinned_cnt[r] > cap) marked.push_back((int32_t)r);
            if ((int64_t)marked.size() > std::max<int64_t>(64, rows / 200)) {
                redo_marked(marked, h->S[slot].p, false, rb);
            }
            if (overlap) KN_HIP(hipEventRecord(h->ev_consumed[slot], sc));  // (only now may the producer recycle S[slot])
        }
    }
    // One-launch builds (whole-matrix, or one row block): the device has summed what the host needs to know about the rows
    // (stats[2] shortlist lengths, stats[3] rows to rebuild: k_sum_row_entries), so ONE four-word read-back ends the build; the per-row counts are fetched only if a row has to be rebuilt.
    // (Walking 162 541 counts on the host between the re-rank and the prediction left the GPU idle for 0.25 ms per step.)
    const bool summary = !per_block_redo;
    unsigned long long four[4] = {0, 0, 0, 0};
    nt.by_id_valid = false;  // (the id-sorted copies are made by launch_predict when a kernel wants them)
    if (summary) KN_HIP(hipMemcpyAsync(four, h->sel.stats.p, sizeof(four), hipMemcpyDeviceToHost, sc));
    KN_HIP(hipStreamSynchronize(sc));
    KN_HIP(hipStreamSynchronize(sp));
    auto take_stats = [&](const unsigned long long* w) {
        h->tm.rerank_row_bytes += 12.0 * (double)w[1];
        if (verify && w[0] != 0) {
            double shifted;
            memcpy(&shifted, &w[0], sizeof(double));
            h->tm.max_bound_violation = std::max(h->tm.max_bound_violation, shifted - 4.0);
        }
    };
    if (summary && four[3] == 0) {  // every list is final
        h->tm.shortlist_total += (double)four[2];
        take_stats(four);
        return;
    }
    if (summary) {
        KN_HIP(hipMemcpyAsync(h->pinned_cnt, h->sel.cand_cnt.p, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        KN_HIP(hipStreamSynchronize(st));
    }
    // select.hip anticipates its emission thresholds and marks a row whose guess overshot (like one whose stores overflowed)
    // for the exact fallback below — a 7-sigma event per row when the dense user order is a pseudo-random column sample,
    // which HashSet ranks of the raw ids are.  Should a data set defeat that (many rows marked), the marked rows are not sent
    // through the per-row exact path (milliseconds each, a U-sized sort each) but once more through select + re-rank with the
    // plain thresholds (redo_marked): the anticipation can then cost at most one extra pass.  Whole-matrix builds and
    // one-block row-block builds do it here (the similarity panel is still there); builds of several row blocks did it per
    // block, before the block's panel slot was recycled (above).
    if (summary) {
        std::vector<int32_t> marked;
        for (int64_t r = 0; r < count; ++r)
            if (h->pinned_cnt[r] > cap) marked.push_back((int32_t)r);
        if ((int64_t)marked.size() > std::max<int64_t>(64, count / 200)) redo_marked(marked, use_sym ? (const void*)h->S_full.p : (const void*)h->S[0].p, use_sym, 0);
    }
    // rows whose shortlist overflowed: exact row + stable descending sort (rare)
    for (int64_t r = 0; r < count; ++r) {
        h->tm.shortlist_total += std::min(h->pinned_cnt[r], cap);
        if (h->pinned_cnt[r] > cap) {
            need_h_rows();
            Stage s(h, &h->tm.rerank_ms);
            int32_t u = h_rows[r];
            h->sel.row_exact.ensure(tr.U);
            h->sel.fb_keys_a.ensure(tr.U); h->sel.fb_keys_b.ensure(tr.U);
            h->sel.fb_vals_a.ensure(tr.U); h->sel.fb_vals_b.ensure(tr.U);
            int64_t seq_u = fetch(h, nt.seq.p, u);
            launch_exact_row(tr, nt, u, seq_u, h->sel.row_exact.p, st);
            launch_fallback_keys(tr.U, h->sel.row_exact.p, h->sel.fb_keys_a.p, h->sel.fb_vals_a.p, st);
            sort_pairs_u64_u32(h->prep.sort, h->sel.fb_keys_a.p, h->sel.fb_keys_b.p, h->sel.fb_vals_a.p,
                               h->sel.fb_vals_b.p, tr.U, 64, st);
            launch_fallback_write(u, nt.kcap, nt.kcap, h->sel.fb_vals_b.p, h->sel.row_exact.p, nt.idx.p, nt.sim.p,
                                  nt.cnt.p, st);
            h->tm.fallback_rows += 1;
        }
    }
    {
        unsigned long long two[2] = {0, 0};
        KN_HIP(hipMemcpyAsync(two, h->sel.stats.p, sizeof(two), hipMemcpyDeviceToHost, st));
        KN_HIP(hipStreamSynchronize(st));
        take_stats(two);
    }
}

void ensure_test_scratch(knncf_handle* h, int64_t n) {
    h->t_du.ensure(n); h->t_di.ensure(n); h->t_pred.ensure(n); h->t_err.ensure(n); h->t_owned.ensure(n);
    h->t_partial.ensure(1024); h->t_counts.ensure(1024);
}

// neighbourhoods needed by the test rows, in the order the reference's lazy closures would build
// them: a user's neighbourhood is built at its first test row whose item has raters
void ensure_neighbors_for_rows(knncf_handle* h, int64_t n) {
    Train& tr = h->tr;
    if (tr.U < 2 || h->nt.kcap <= 0) return;
    KN_REQUIRE(n < (int64_t)0xffffffffll, KNNCF_E_UNSUPPORTED, "more than 2^32-1 test rows");
    hipStream_t st = h->stream;
    h->first_row.ensure(tr.U);
    h->build_list.ensure(tr.U);
    h->build_count.ensure(1);
    KN_HIP(hipMemsetAsync(h->first_row.p, 0xff, tr.U * sizeof(uint32_t), st));
    KN_HIP(hipMemsetAsync(h->build_count.p, 0, sizeof(int32_t), st));
    // (every user's first row, whoever owns it: a shard needs the build sequence numbers of the other shards' users too)
    launch_first_rows(n, h->t_du.p, h->t_di.p, tr.user_avg.p, 0, tr.U, h->first_row.p, st);
    launch_collect_new(tr.U, h->first_row.p, h->nt.seq.p, h->epoch, tr.own_lo, tr.own_hi, h->build_list.p, h->build_count.p, st);
    h->epoch += 1;
    int32_t count = fetch(h, h->build_count.p, 0);
    build_neighbors(h, count);
}

// predictor(train, weightedSumDeviation(train, sim)) with sim = adjustedCosineSimilarityFunction(train) or
// jaccardCoefficient(train) (predict/Personalized.scala:61-72).  U <= 2048: the table of every non-zero similarity, built once
// per fit, through the kNN prediction kernels with k = U.  Beyond (or with KNNCF_DEBUG_PERSONALIZED_STREAM, a test hook that
// takes this path at any U): exact similarity rows built per block of test users and folded in file order (personalized.hip).
bool personalized_streams(const knncf_handle* h) { return h->tr.U > 2048 || getenv("KNNCF_DEBUG_PERSONALIZED_STREAM"); }

// the refusals of both forms
void require_personalized(knncf_handle* h) {
    Train& tr = h->tr;
    KN_REQUIRE(h->cfg.shard_count == 1, KNNCF_E_UNSUPPORTED, "PERSONALIZED is not sharded");
    if (h->cfg.similarity == KNNCF_SIM_COSINE) {
        std::vector<int64_t> ptr((size_t)tr.U + 1);
        KN_HIP(hipMemcpyAsync(ptr.data(), tr.u_ptr.p, ptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        KN_HIP(hipStreamSynchronize(h->stream));
        for (int32_t u = 0; u < tr.U; ++u)
            KN_REQUIRE(ptr[u + 1] - ptr[u] > 4, KNNCF_E_UNSUPPORTED,
                       "PERSONALIZED with the adjusted cosine: a user with <= 4 ratings makes the reference's summation order depend on its memo history pair by pair (SURVEY N6); not modelled");
    }
}

void ensure_personalized_table(knncf_handle* h) {
    if (h->pt_ready) return;
    Train& tr = h->tr;
    require_personalized(h);
    NeighborTable& pt = h->pt;
    pt.k = pt.kcap = tr.U;
    const size_t cells = (size_t)tr.U * (size_t)tr.U;
    pt.uidx.ensure(cells);
    pt.usim.ensure(cells);
    pt.cnt.ensure(tr.U);
    launch_full_rows(tr, h->cfg.similarity == KNNCF_SIM_JACCARD, pt.uidx.p, pt.usim.p, pt.cnt.p, h->stream);
    pt.by_id_valid = true;
    h->pt_ready = true;
}

// the item-major fp64 pre values, the raters in file order and the tile table: built on the first streamed call, charged to
// prep_ms (knncf_fit does not build them: the kNN step never reads them)
// (fitted = false: the Personalized QUERIES — fresh closures owned by the query user — take the copies without the fitted
// path's refusal of users with <= 4 ratings; the fitted path still checks on its own first use)
void ensure_personal_rows(knncf_handle* h, bool fitted = true) {
    if (fitted && !h->prow_checked) {
        require_personalized(h);
        h->prow_checked = true;
    }
    if (h->prow_ready) return;
    Stage s(h, &h->tm.prep_ms);
    h->prep.join_commit(h->stream);
    personalized_prepare(h->tr, h->prep, h->prow, h->stream);
    h->prow_ready = true;
}

// The plan of the streamed form over the rows whose dense ids are in t_du / t_di: rows sorted by (user, item) — the order is left
// in prep.v32_b — and the distinct users that have a row on a train item cut into equal blocks of R (their ids in prow.users,
// each one's row of its block in prow.slot, prow.S sized for a block).  Block b is users [b R, (b + 1) R) and the sorted rows
// from its first user's first row (block 0: from row 0) to the next block's (the last block: to n).
struct PersonalPlan {
    std::vector<int64_t> first_row;  // sorted row where each such user's rows begin
    int64_t nu = 0, R = 1, n_blocks = 1;
    int64_t row_begin(int64_t b) const { return b == 0 ? 0 : first_row[b * R]; }
    int64_t row_end(int64_t b, int64_t n) const { return b + 1 < n_blocks ? first_row[(b + 1) * R] : n; }
};
PersonalPlan plan_personal_rows(knncf_handle* h, int64_t n) {
    Train& tr = h->tr;
    PersonalRows& pr = h->prow;
    PrepScratch& sc = h->prep;
    hipStream_t st = h->stream;
    KN_REQUIRE(n < (int64_t)0xffffffffll, KNNCF_E_UNSUPPORTED, "more than 2^32-1 test rows");
    sc.k64_a.ensure(n); sc.k64_b.ensure(n); sc.v32_a.ensure(n); sc.v32_b.ensure(n);
    const int ibits = bits_for((uint64_t)tr.I);
    std::vector<uint64_t> keys((size_t)n);
    {
        Stage s(h, &h->tm.predict_ms);
        launch_personal_row_keys(tr, n, h->t_du.p, h->t_di.p, sc.k64_a.p, sc.v32_a.p, st);
        sort_pairs_u64_u32(sc.sort, sc.k64_a.p, sc.k64_b.p, sc.v32_a.p, sc.v32_b.p, n, ibits + bits_for((uint64_t)tr.U), st);
        KN_HIP(hipMemcpyAsync(keys.data(), sc.k64_b.p, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        KN_HIP(hipStreamSynchronize(st));
    }
    // the users whose rows are built: a known user with a row on a train item (its rows sort by item, absent item last)
    PersonalPlan plan;
    std::vector<int32_t> users;
    for (int64_t r = 0; r < n; ++r) {
        const uint64_t u = keys[r] >> ibits, i = keys[r] & ((1ull << ibits) - 1ull);
        if (u < (uint64_t)tr.U && i < (uint64_t)tr.I && (users.empty() || users.back() != (int32_t)u)) {
            users.push_back((int32_t)u);
            plan.first_row.push_back(r);
        }
    }
    const int64_t nu = plan.nu = (int64_t)users.size();
    if (nu > 0) {
        size_t free_b = 0, total_b = 0;
        KN_HIP(hipMemGetInfo(&free_b, &total_b));
        const int64_t row_bytes = (int64_t)tr.U * 8;
        const int64_t budget = h->cfg.workspace_bytes > 0 ? h->cfg.workspace_bytes / 2
                                                          : (int64_t)std::min<size_t>((size_t)48 << 30, (free_b + pr.S.bytes()) / 4);
        int64_t R = std::min<int64_t>(std::max<int64_t>(1, budget / row_bytes), nu);
        R = plan.R = ceil_div(nu, ceil_div(nu, R));  // equal blocks
        pr.S.ensure((size_t)R * tr.U);
        std::vector<int32_t> slot((size_t)tr.U, -1);
        for (int64_t k = 0; k < nu; ++k) slot[users[k]] = (int32_t)(k % R);
        pr.users.ensure(nu);
        pr.slot.ensure(tr.U);
        KN_HIP(hipMemcpyAsync(pr.users.p, users.data(), (size_t)nu * sizeof(int32_t), hipMemcpyHostToDevice, st));
        KN_HIP(hipMemcpyAsync(pr.slot.p, slot.data(), (size_t)tr.U * sizeof(int32_t), hipMemcpyHostToDevice, st));
        KN_HIP(hipStreamSynchronize(st));  // (the host vectors go out of scope)
    }
    plan.n_blocks = std::max<int64_t>(1, ceil_div(nu, plan.R));
    return plan;
}

// The streamed form over the test rows whose dense ids are in t_du / t_di: per block of the plan the users' exact rows
// (rerank_ms), then the folds of the block's rows (predict_ms).  Read-only on the kNN state.
void predict_personal_rows(knncf_handle* h, const double* d_ratings, int64_t n, double* d_pred) {
    Train& tr = h->tr;
    PersonalRows& pr = h->prow;
    hipStream_t st = h->stream;
    const PersonalPlan plan = plan_personal_rows(h, n);
    for (int64_t b = 0; b < plan.n_blocks; ++b) {
        const int64_t u0 = b * plan.R, u1 = std::min<int64_t>(plan.nu, u0 + plan.R);
        const int64_t r0 = plan.row_begin(b), r1 = plan.row_end(b, n);
        if (u1 > u0) {
            Stage s(h, &h->tm.rerank_ms);
            launch_sim_rows(tr, pr, pr.users.p + u0, (int32_t)(u1 - u0), pr.S.p, st);
        }
        Stage s(h, &h->tm.predict_ms);
        launch_fold_rows(tr, pr, r1 - r0, h->prep.v32_b.p + r0, h->t_du.p, h->t_di.p, d_ratings, pr.slot.p, pr.S.p, d_pred, h->t_err.p,
                         h->t_owned.p, st);
    }
}

// K4 on first use: computeItemAvg :141, computeItemAvgDev :193 and the Spark forms build their item maps when the predictor is
// constructed; the kNN predictor (:489-585) never does, so knncf_fit leaves them out (prep.hip: prep_item_stats)
void ensure_item_stats(knncf_handle* h) {
    if (h->tr.item_stats_ready) return;
    Stage s(h, &h->tm.prep_ms);
    h->prep.join_commit(h->stream);
    prep_item_stats(h->tr, h->prep, h->stream);
}

// The kNN kernels' row order over the test rows whose dense ids are in t_du / t_di: sorted by item (by_item) or by user,
// the rows the train set cannot place last; the order is left in prep.v32_b.  On a shard handle the test set is replicated on
// every shard and the work is not: this shard's rows sort first and only they are predicted; the other rows' error cells
// (cols columns of n in t_err) and ownership cells are cleared here instead of by the kernel.  Returns the rows to predict.
int64_t order_test_rows(knncf_handle* h, int64_t n, bool by_item, int32_t cols) {
    Train& tr = h->tr;
    hipStream_t st = h->stream;
    PrepScratch& sc = h->prep;
    sc.k64_a.ensure(n); sc.k64_b.ensure(n); sc.v32_a.ensure(n); sc.v32_b.ensure(n);
    const uint32_t key_limit = (uint32_t)(by_item ? tr.I : tr.U);  // the key of a row whose item / user the train set lacks
    if (h->cfg.shard_count > 1) {
        h->scalar_u64.ensure(1);
        KN_HIP(hipMemsetAsync(h->scalar_u64.p, 0, sizeof(unsigned long long), st));
        KN_HIP(hipMemsetAsync(h->t_err.p, 0, (size_t)cols * (size_t)n * sizeof(double), st));
        KN_HIP(hipMemsetAsync(h->t_owned.p, 0, (size_t)n, st));
        launch_owned_keys(n, by_item ? h->t_di.p : h->t_du.p, h->t_du.p, tr.own_lo, tr.own_hi, h->cfg.shard_rank == 0, key_limit,
                          sc.k64_a.p, sc.v32_a.p, h->scalar_u64.p, st);
        sort_pairs_u64_u32(sc.sort, sc.k64_a.p, sc.k64_b.p, sc.v32_a.p, sc.v32_b.p, n, bits_for((uint64_t)key_limit + 1), st);
        return (int64_t)fetch(h, h->scalar_u64.p, 0);
    }
    launch_user_keys(n, by_item ? h->t_di.p : h->t_du.p, key_limit, sc.k64_a.p, sc.v32_a.p, st);
    sort_pairs_u64_u32(sc.sort, sc.k64_a.p, sc.k64_b.p, sc.v32_a.p, sc.v32_b.p, n, bits_for((uint64_t)key_limit), st);
    return n;
}

// sum |r - p| of each of the cols columns of n cells in t_err (the deterministic fixed-shape reduction, one launch per column)
// and the count of t_owned; sums[c] per column (either pointer may be null)
void reduce_errors(knncf_handle* h, int64_t n, int32_t cols, double* sums, int64_t* count) {
    hipStream_t st = h->stream;
    const int32_t nb = 1024;
    h->t_partial.ensure((size_t)nb * cols);
    h->t_counts.ensure((size_t)nb * cols);
    for (int32_t c = 0; c < cols; ++c)
        launch_reduce_err(h->t_err.p + (size_t)c * n, h->t_owned.p, n, h->t_partial.p + (size_t)c * nb, h->t_counts.p + (size_t)c * nb, nb, st);
    std::vector<double> hp((size_t)nb * cols);
    std::vector<int64_t> hc((size_t)nb * cols);
    KN_HIP(hipMemcpyAsync(hp.data(), h->t_partial.p, hp.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    KN_HIP(hipMemcpyAsync(hc.data(), h->t_counts.p, hc.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    KN_HIP(hipStreamSynchronize(st));
    for (int32_t c = 0; c < cols; ++c) {
        double s_ = 0.0;
        int64_t c_ = 0;
        for (int32_t b = 0; b < nb; ++b) { s_ += hp[(size_t)c * nb + b]; c_ += hc[(size_t)c * nb + b]; }
        if (sums) sums[c] = s_;
        if (count && c == 0) *count = c_;
    }
}

void run_predict(knncf_handle* h, int predictor, const int32_t* d_users, const int32_t* d_items,
                 const double* d_ratings, int64_t n, double* sum_abs_err, int64_t* count, double* d_pred_out) {
    require_fitted(h);
    Train& tr = h->tr;
    hipStream_t st = h->stream;
    KN_REQUIRE(n >= 0, KNNCF_E_INVALID, "negative row count");
    if (sum_abs_err) *sum_abs_err = 0.0;
    if (count) *count = 0;
    if (n == 0) return;
    KN_REQUIRE(d_users && d_items, KNNCF_E_INVALID, "null test arrays");
    int kind = predictor;
    NeighborTable* table = &h->nt;
    bool stream = false;  // PERSONALIZED by streamed similarity rows
    if (predictor == KNNCF_PRED_PERSONALIZED) {
        if (h->cfg.similarity == KNNCF_SIM_ONE) {
            kind = KNNCF_PRED_BASELINE_RDD;  // num/den = file-order mean of the item's deviations (see predict.hip)
        } else if (personalized_streams(h)) {
            ensure_personal_rows(h);
            stream = true;
        } else {  // the adjusted cosine / the Jaccard coefficient themselves: every user is a "neighbour"
            ensure_personalized_table(h);
            kind = KNNCF_PRED_KNN;
            table = &h->pt;
        }
    }
    KN_REQUIRE(stream || (kind >= KNNCF_PRED_GLOBAL_AVG && kind <= KNNCF_PRED_KNN), KNNCF_E_INVALID, "unknown predictor");
    if (kind == KNNCF_PRED_ITEM_AVG || kind == KNNCF_PRED_BASELINE || kind == KNNCF_PRED_BASELINE_RDD) ensure_item_stats(h);
    ensure_test_scratch(h, n);
    {
        Stage s(h, &h->tm.predict_ms);
        launch_dense_ids(tr, d_users, d_items, n, h->t_du.p, h->t_di.p, st);
    }
    if (kind == KNNCF_PRED_KNN && table == &h->nt) ensure_neighbors_for_rows(h, n);
    h->prep.join_commit(st);  // the item-major copies and the rater bitmaps (second part of prep_commit)
    double* pred = d_pred_out ? d_pred_out : h->t_pred.p;
    if (stream) predict_personal_rows(h, d_ratings, n, pred);
    {
        Stage s(h, &h->tm.predict_ms);
        const uint32_t* d_order = nullptr;
        const bool by_item = tr.ib_words > 0 && lds_bitmap_fits(tr.ib_words);
        int64_t n_rows = n;  // rows the prediction kernel walks
        if (kind == KNNCF_PRED_KNN) {  // rows sorted by item (the item's rater bitmap lives in LDS) or else by user
            n_rows = order_test_rows(h, n, by_item, 1);
            d_order = h->prep.v32_b.p;
        }
        if (n_rows > 0 && !stream)
            launch_predict(tr, table, kind, n_rows, h->t_du.p, h->t_di.p, d_ratings, d_order, by_item, pred, h->t_err.p, h->t_owned.p,
                           h->cfg.shard_rank == 0, st);
        if (sum_abs_err || count) reduce_errors(h, n, 1, sum_abs_err, count);
    }
}

// ks of knncf_mae_sweep*: 1 .. 64 values, strictly ascending, each in [1, 2048]
void check_sweep_ks(const int32_t* ks, int32_t n_k) {
    KN_REQUIRE(ks && n_k >= 1 && n_k <= 64, KNNCF_E_INVALID, "sweep: 1 .. 64 values of k");
    for (int32_t q = 0; q < n_k; ++q)
        KN_REQUIRE(ks[q] >= 1 && ks[q] <= 2048 && (q == 0 || ks[q] > ks[q - 1]), KNNCF_E_INVALID,
                   "sweep: k must be strictly ascending in [1, 2048]");
}

// predict/kNN.scala:73 — the MAE at every k of ks[0 .. n_k) with fresh closures for each k, from ONE neighbour build: the lists
// at kmax = ks[n_k - 1] are built in the order ensure_neighbors_for_rows builds them (a user's list at its first test row on an
// item with raters: the same order, hence the same memo history, for every k) and k_predict_knn_sweep folds each k over the
// first k entries of them.  Whatever lists the handle held are ignored; on every return path the memo is dropped (as
// knncf_reset_neighbors) and the handle's k is the caller's.  sums[q] / *count: as run_predict; d_pred (may be null):
// [n_k * n] (row q: the predictions at ks[q]).
void run_mae_sweep(knncf_handle* h, const int32_t* ks, int32_t n_k, const int32_t* d_users, const int32_t* d_items,
                   const double* d_ratings, int64_t n, double* sums, int64_t* count, double* d_pred) {
    check_sweep_ks(ks, n_k);
    require_fitted(h);
    KN_REQUIRE(h->cfg.similarity != KNNCF_SIM_ONE, KNNCF_E_UNSUPPORTED,
               "kNN neighbourhoods with similarityOne: every similarity is 1.0, the neighbourhood is the first k users in Set order — not built");
    KN_REQUIRE(n >= 0, KNNCF_E_INVALID, "negative row count");
    for (int32_t q = 0; q < n_k; ++q) sums[q] = 0.0;
    *count = 0;
    if (n == 0) return;
    KN_REQUIRE(d_users && d_items && d_ratings, KNNCF_E_INVALID, "null test arrays");
    Train& tr = h->tr;
    hipStream_t st = h->stream;
    struct Restore {  // the caller's k and a dropped memo, whichever way the call ends
        knncf_handle* h;
        int32_t k;
        ~Restore() {
            h->cfg.k = k;
            try { reset_neighbors(h); } catch (const Error&) {}
        }
    } restore{h, h->cfg.k};
    h->cfg.k = ks[n_k - 1];
    reset_neighbors(h);  // fresh closures at kcap = min(kmax, U - 1)
    ensure_test_scratch(h, n);
    h->t_err.ensure((size_t)n_k * n);
    {
        Stage s(h, &h->tm.predict_ms);
        launch_dense_ids(tr, d_users, d_items, n, h->t_du.p, h->t_di.p, st);
    }
    ensure_neighbors_for_rows(h, n);
    h->prep.join_commit(st);  // the item-major copies and the rater bitmaps (second part of prep_commit)
    std::vector<int32_t> hk(ks, ks + n_k);
    h->sweep_ks.ensure(64);
    KN_HIP(hipMemcpyAsync(h->sweep_ks.p, hk.data(), (size_t)n_k * sizeof(int32_t), hipMemcpyHostToDevice, st));
    {
        Stage s(h, &h->tm.predict_ms);
        const int64_t n_rows = order_test_rows(h, n, /*by_item=*/true, n_k);
        if (n_rows > 0)  // (one train user: kcap = 0, every row is predicted without neighbours, as run_predict does)
            launch_predict_sweep(tr, h->nt, h->sweep_ks.p, n_k, n_rows, n, h->t_du.p, h->t_di.p, d_ratings, h->prep.v32_b.p, d_pred,
                                 h->t_err.p, h->t_owned.p, h->cfg.shard_rank == 0, st);
        reduce_errors(h, n, n_k, sums, count);
    }
}

// what the handle derives from a Train and a new one invalidates: the operand panel, the Personalized table and rater copies,
// the host id caches (a fit and knncf_append's swap)
void drop_fit_caches(knncf_handle* h) {
    h->short_rows = -1;
    h->b_ready = false;
    h->pt_ready = false;
    h->prow_ready = false;
    h->prow_checked = false;
    h->h_ukeys.clear(); h->h_ikeys.clear(); h->h_uid.clear(); h->h_uptr.clear(); h->h_uavg.clear(); h->h_utable.clear();
}

void do_fit_device(knncf_handle* h, const int32_t* d_users, const int32_t* d_items, const double* d_ratings, int64_t n) {
    KN_REQUIRE(n > 0 && d_users && d_items && d_ratings, KNNCF_E_INVALID, "fit: null or empty input");
    Train& tr = h->tr;
    hipStream_t st = h->stream;
    h->fitted = h->committed = false;
    drop_fit_caches(h);
    tr.n = n;
    tr.jaccard = h->cfg.similarity == KNNCF_SIM_JACCARD;
    {
        Stage s(h, &h->tm.prep_ms);
        if (tr.user_raw.p != d_users) {
            tr.user_raw.alloc(n); tr.item_raw.alloc(n); tr.rating.alloc(n);
            KN_HIP(hipMemcpyAsync(tr.user_raw.p, d_users, n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
            KN_HIP(hipMemcpyAsync(tr.item_raw.p, d_items, n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
            KN_HIP(hipMemcpyAsync(tr.rating.p, d_ratings, n * sizeof(double), hipMemcpyDeviceToDevice, st));
        }
        prep_fit(tr, h->prep, h->cfg.shard_rank, h->cfg.shard_count, st);
    }
    h->fitted = true;
    reset_neighbors(h);
    if (h->cfg.shard_count == 1) {
        Stage s(h, &h->tm.prep_ms);
        prep_commit(tr, h->prep, st);
        h->committed = true;
    }
}

// ---- fold-in queries: users outside the fit, answered chunk by chunk (foldin.hip) ------------------------------------------
// Every answer is the reference's on aug = train ++ the query rows with fresh closures whose first evaluation is the
// query user's.  Read-only on the handle: the neighbour table, its sequence numbers and epoch are not touched.
// knncf_query_*_batch take B independent queries; a single call is a chunk of one.
// Update queries (knncf_update_*) are the same calls for a user that may be in the fit: the rows given are then ADDITIONAL to
// the user's train rows, which foldin.hip seeds on the device, and the user is left out of its own candidates.
// Revise queries (knncf_revise_*) are update queries that also name train items of the user to REMOVE from aug: the seeding
// leaves their rows out.  A chunk without removals is an update chunk.
constexpr int64_t QUERY_MAX_RATINGS = 65536;
// QB_EXPLAIN_ALL: the explanations of KNNCF_PRED_PERSONALIZED predictions (knncf_*_explain_personalized*), a mode of its own so
// that QB_EXPLAIN keeps refusing that predictor
// QB_RECOMMEND_EXPLAIN: QB_RECOMMEND, then the explain kernel of the predictor over the rows the selection produced
// (knncf_*_recommend_explain*): no requested rows, so neither explains() nor wants_rows()
// QB_BY_NEIGHBORS / QB_BY_PREDICT: bystander queries (knncf_*_bystander_*) — a query's rows name fitted users; run_bystander_chunks
// QB_ENTERED: entered queries (knncf_query_entered*) — no rows; an answer step of run_query_chunks (answer_entered); under
// QF_UPDATE / QF_REVISE the entered queries of update and revise queries (knncf_update_entered*, knncf_revise_entered*;
// answer_entered_update)
enum QueryBatchMode { QB_NEIGHBORS, QB_PREDICT, QB_RECOMMEND, QB_EXPLAIN, QB_EXPLAIN_ALL, QB_RECOMMEND_EXPLAIN, QB_BY_NEIGHBORS, QB_BY_PREDICT, QB_ENTERED };
bool bystanders(QueryBatchMode mode) { return mode == QB_BY_NEIGHBORS || mode == QB_BY_PREDICT; }
bool explains(QueryBatchMode mode) { return mode == QB_EXPLAIN || mode == QB_EXPLAIN_ALL; }
bool recommends(QueryBatchMode mode) { return mode == QB_RECOMMEND || mode == QB_RECOMMEND_EXPLAIN; }
enum QueryFamily { QF_FOLD_IN, QF_UPDATE, QF_REVISE };

// what the handle must be for any fold-in query, single or batched
void require_query_support(knncf_handle* h, int predictor, QueryBatchMode mode) {
    KN_REQUIRE(!bystanders(mode) || predictor == KNNCF_PRED_KNN, KNNCF_E_UNSUPPORTED, "query bystander: only KNNCF_PRED_KNN");
    KN_REQUIRE(mode != QB_EXPLAIN_ALL || predictor == KNNCF_PRED_PERSONALIZED, KNNCF_E_UNSUPPORTED, "query explain: only KNNCF_PRED_PERSONALIZED");
    KN_REQUIRE(predictor == KNNCF_PRED_KNN || (predictor == KNNCF_PRED_PERSONALIZED && mode != QB_EXPLAIN), KNNCF_E_UNSUPPORTED,
               mode == QB_EXPLAIN ? "query explain: only KNNCF_PRED_KNN" : "query: only KNNCF_PRED_KNN and KNNCF_PRED_PERSONALIZED");
    KN_REQUIRE(h->cfg.similarity != KNNCF_SIM_ONE, KNNCF_E_UNSUPPORTED, "query: adjusted cosine or Jaccard");
    KN_REQUIRE(h->cfg.shard_count == 1, KNNCF_E_UNSUPPORTED, "query: single-shard handles only");
    KN_REQUIRE(h->tr.U >= 5, KNNCF_E_UNSUPPORTED, "query: fewer than 5 train users (the user set changes iteration class)");
}

// what the chunk rules of knncf.h divide: workspace_bytes / 2, else min(48 GiB, free device memory / 4)
int64_t batch_budget(knncf_handle* h) {
    if (h->cfg.workspace_bytes > 0) return h->cfg.workspace_bytes / 2;
    size_t free_b = 0, total_b = 0;
    KN_HIP(hipMemGetInfo(&free_b, &total_b));
    return (int64_t)std::min<size_t>((size_t)48 << 30, free_b / 4);
}

// queries per chunk: the rule of knncf.h ("Batched fold-in queries")
int64_t query_batch_chunk(knncf_handle* h, int64_t budget) {
    const Train& tr = h->tr;
    int64_t C = std::min<int64_t>(QB_MAX_CHUNK, budget / query_batch_bytes(tr.U, tr.I));
    C = std::min<int64_t>(C, (int64_t)0x7fffffff / std::max(tr.U, tr.I));  // slot * U + user and slot * I + item are 31-bit cells
    return std::max<int64_t>(C, 1);
}

// rows per chunk of knncf_explain_batch, and per launch of the query explanations: the rule of knncf.h ("Explanations")
size_t explain_row_bytes(int32_t cap) { return 20 * (size_t)cap + 28; }
int64_t explain_rows(int64_t budget, int32_t cap) { return std::max<int64_t>(budget / (int64_t)explain_row_bytes(cap), 1); }
int64_t explain_batch_chunk(knncf_handle* h, int32_t cap) { return explain_rows(batch_budget(h), cap); }
// rows per launch of a query explain mode: QB_EXPLAIN_ALL stages as many bytes again (explain_all_row_bytes)
int64_t query_explain_rows(int64_t budget, int32_t cap, bool all) {
    return all ? std::max<int64_t>(budget / (int64_t)explain_all_row_bytes(cap), 1) : explain_rows(budget, cap);
}

// the first query that was refused (-1: none) and why
struct QueryFailure {
    int64_t query = -1;
    const char* reason = "";
};

// ---- the explain outputs of a launch as one block (QB_EXPLAIN) -----------------------------------------------------------------
// The rows of a launch lie in one device block, so that one copy brings them back: sims, devs [nr * cap], sums [2 nr],
// predictions [nr] as doubles, then raters [nr * cap] and counts [nr] as int32 — the 20 * cap + 28 bytes per row that both chunk
// rules of knncf.h ("Explanations") divide by (explain_row_bytes).
// `like`'s order and cap over the block of nr rows at base (a device or a host address)
ExplainCells explain_pack(double* base, int64_t nr, const ExplainCells& like) {
    const size_t cells = (size_t)nr * (size_t)like.cap;
    ExplainCells o = like;
    o.sims = base; o.devs = base + cells; o.sums = base + 2 * cells; o.pred = o.sums + 2 * nr;
    o.raters = reinterpret_cast<int32_t*>(o.pred + nr); o.counts = o.raters + cells;
    return o;
}
// rows [0, nr) of a block on the host into the caller's arrays: row r goes to row rows[r].  The cells of a row beyond its
// terms stay as the caller left them
void explain_scatter(const ExplainCells& from, int64_t nr, const ExplainCells& to, const int64_t* rows) {
    for (int64_t r = 0, cap = to.cap; r < nr; ++r) {
        const int64_t j = rows[r];
        to.counts[j] = from.counts[r];
        if (to.sums) { to.sums[2 * j] = from.sums[2 * r]; to.sums[2 * j + 1] = from.sums[2 * r + 1]; }
        if (to.pred) to.pred[j] = from.pred[r];
        const size_t at = (size_t)r * cap, dst = (size_t)j * cap;
        const int64_t t = std::min<int64_t>(from.counts[r], cap);
        std::copy(from.raters + at, from.raters + at + t, to.raters + dst);
        std::copy(from.sims + at, from.sims + at + t, to.sims + dst);
        std::copy(from.devs + at, from.devs + at + t, to.devs + dst);
    }
}

// ---- one request type for every family, mode and form ---------------------------------------------------------------------
// A batch form fills users, B and the offsets arrays and leaves the last four fields 0.  A single form fills user, n_ratings,
// n_removed and m instead and leaves users, B and the three offsets arrays 0: BatchOfOne makes them (a chunk of one); its
// counts is the caller's *count.
// The bystander modes read their rows from pred_offsets (the calls' row_offsets; single: m) and others, QB_BY_PREDICT also from
// pred_items, and answer per ROW: QB_BY_NEIGHBORS into out_i / out_d / row_counts with width = cap, QB_BY_PREDICT into out_d; counts
// stays null.  QB_ENTERED has no rows and answers per QUERY into out_i / out_d / out_pos / out_displaced (width = cap) and counts.
struct QueryCall {
    QueryFamily family;
    QueryBatchMode mode;
    int predictor;
    const int32_t* users;            // [B]
    int64_t B;
    const int64_t* offsets;          // [B + 1] query b's rows are items / ratings [offsets[b], offsets[b + 1])
    const int32_t* items;
    const double* ratings;
    const int64_t* removed_offsets;  // QF_REVISE (null otherwise): [B + 1] into removed_items
    const int32_t* removed_items;    // QF_REVISE: the train items each query's user drops
    const int64_t* pred_offsets;     // QB_PREDICT, explain modes: [B + 1] into pred_items; row j of the call is pred_items[j]
    const int32_t* pred_items;       // QB_PREDICT, explain modes: the requested items
    const int32_t* others;           // bystander modes: the fitted user of each row (rows: pred_offsets; QB_BY_PREDICT: with pred_items)
    int32_t* row_counts;             // QB_BY_NEIGHBORS: [pred_offsets[B]] (counts stays null: the answers are per row)
    int32_t width;                   // QB_NEIGHBORS: cap; QB_RECOMMEND, QB_RECOMMEND_EXPLAIN: n
    int32_t* out_i;                  // QB_NEIGHBORS: ids [B * cap]; QB_RECOMMEND*: items [B * n]; unused otherwise
    double* out_d;                   // QB_NEIGHBORS: sims [B * cap]; QB_RECOMMEND*: predictions [B * n]; QB_PREDICT: [pred_offsets[B]]
    int32_t* counts;                 // QB_NEIGHBORS, QB_RECOMMEND*: [B]
    int32_t* statuses;               // [B]
    ExplainCells ex;                 // explain modes: pred_offsets[B] rows; QB_RECOMMEND_EXPLAIN: B * n rows, row b * n + j (pred null)
    int32_t* out_pos;                // QB_ENTERED: [B * cap] beside out_i (users) and out_d (sims), width = cap
    int32_t* out_displaced;          // QB_ENTERED: [B * cap]
    int32_t* out_prev;               // QB_ENTERED under QF_UPDATE / QF_REVISE (knncf_update_entered*, knncf_revise_entered*): [B * cap]; null otherwise
    int32_t user;                    // single forms only, from here on
    int64_t n_ratings, n_removed, m;
};

// One builder per mode: `rows` names the family and the queries (either form), the rest is what the mode answers into
QueryCall neighbors_call(QueryCall rows, int32_t cap, int32_t* ids, double* sims, int32_t* counts) {
    rows.mode = QB_NEIGHBORS; rows.predictor = KNNCF_PRED_KNN; rows.width = cap;
    rows.out_i = ids; rows.out_d = sims; rows.counts = counts;
    return rows;
}
QueryCall predict_call(QueryCall rows, int predictor, double* out) {
    rows.mode = QB_PREDICT; rows.predictor = predictor; rows.out_d = out;
    return rows;
}
QueryCall recommend_call(QueryCall rows, int predictor, int32_t n, int32_t* out_items, double* out_preds, int32_t* counts) {
    rows.mode = QB_RECOMMEND; rows.predictor = predictor; rows.width = n;
    rows.out_i = out_items; rows.out_d = out_preds; rows.counts = counts;
    return rows;
}
QueryCall explain_call(QueryCall rows, int predictor, const ExplainCells& ex) {
    rows.mode = QB_EXPLAIN; rows.predictor = predictor; rows.ex = ex;
    return rows;
}
QueryCall explain_all_call(QueryCall rows, const ExplainCells& ex) {
    rows.mode = QB_EXPLAIN_ALL; rows.predictor = KNNCF_PRED_PERSONALIZED; rows.ex = ex;
    return rows;
}
// (reco: a recommend_call)
QueryCall recommend_explain_call(QueryCall reco, const ExplainCells& ex) {
    reco.mode = QB_RECOMMEND_EXPLAIN; reco.ex = ex;
    return reco;
}
// (rows: with pred_offsets = the call's row_offsets, or m)
QueryCall bystander_neighbors_call(QueryCall rows, const int32_t* others, int32_t cap, int32_t* ids, double* sims, int32_t* row_counts) {
    rows.mode = QB_BY_NEIGHBORS; rows.predictor = KNNCF_PRED_KNN; rows.others = others; rows.width = cap;
    rows.out_i = ids; rows.out_d = sims; rows.row_counts = row_counts;
    return rows;
}
QueryCall bystander_predict_call(QueryCall rows, int predictor, const int32_t* others, double* out) {
    rows.mode = QB_BY_PREDICT; rows.predictor = predictor; rows.others = others; rows.out_d = out;
    return rows;
}
// (rows: with out_pos and out_displaced, which only this mode has)
QueryCall entered_call(QueryCall rows, int32_t cap, int32_t* out_users, double* out_sims, int32_t* counts) {
    rows.mode = QB_ENTERED; rows.predictor = KNNCF_PRED_KNN; rows.width = cap;
    rows.out_i = out_users; rows.out_d = out_sims; rows.counts = counts;
    return rows;
}
bool wants_rows(QueryBatchMode mode) { return mode == QB_PREDICT || explains(mode); }
// the modes that answer one count per query (the bystander modes count per row, the others have nothing to count)
bool counts_queries(QueryBatchMode mode) { return !wants_rows(mode) && !bystanders(mode); }
// whether the mode reads its slots' top-k lists (the Personalized fold has no cut, entered reads the similarity rows themselves)
bool needs_topk(const QueryCall& q) { return q.predictor != KNNCF_PRED_PERSONALIZED && q.mode != QB_ENTERED; }
// the modes that launch an explain kernel, and whether it is the Personalized one; their rows per launch (0: none)
bool runs_explain(const QueryCall& q) { return explains(q.mode) || q.mode == QB_RECOMMEND_EXPLAIN; }
bool explains_all(const QueryCall& q) {
    return q.mode == QB_EXPLAIN_ALL || (q.mode == QB_RECOMMEND_EXPLAIN && q.predictor == KNNCF_PRED_PERSONALIZED);
}
int64_t launch_rows(const QueryCall& q, int64_t budget) { return runs_explain(q) ? query_explain_rows(budget, q.ex.cap, explains_all(q)) : 0; }

// ---- the chunk loop ---------------------------------------------------------------------------------------------------------
// one slot as admit() or the bystander loop describes it: the query of the call, the raw user and its dense index in the fit (-1
// outside), its given rows q.items / q.ratings [a0, a1), the train items it drops q.removed_items [r0, r1), its rows in aug
struct Slot {
    int64_t query;
    int32_t user, self;
    int64_t a0, a1, r0, r1, rows;
};
// what one call's chunks share: the host vectors are reused from chunk to chunk
struct ChunkState {
    QueryFailure first;
    int32_t take = 0, C = 0;  // min(k, U); the chunk's C slots
    std::vector<int64_t> slot_query, qo, ao, ro;
    std::vector<int32_t> s_users, s_items, s_self, s_removed;
    std::vector<double> s_ratings;
    void reset() {  // an empty chunk (first and take stay)
        slot_query.clear(); s_users.clear(); s_items.clear(); s_ratings.clear(); s_self.clear(); s_removed.clear();
        qo.assign(1, 0); ao.assign(1, 0); ro.assign(1, 0);
        C = 0;
    }
    int32_t append(const QueryCall& q, const Slot& s) {  // one more slot; returns its index
        if (s.r1 > s.r0) s_removed.insert(s_removed.end(), q.removed_items + s.r0, q.removed_items + s.r1);
        ro.push_back((int64_t)s_removed.size());
        slot_query.push_back(s.query);
        s_users.push_back(s.user);
        s_self.push_back(s.self);
        if (s.a1 > s.a0) s_items.insert(s_items.end(), q.items + s.a0, q.items + s.a1);
        if (s.a1 > s.a0) s_ratings.insert(s_ratings.end(), q.ratings + s.a0, q.ratings + s.a1);
        ao.push_back((int64_t)s_items.size());
        qo.push_back(qo.back() + s.rows);
        return C++;
    }
    // as foldin_batch_neighbors takes it (a bystander chunk is an update chunk whatever the family: its bystander slots are)
    QueryChunk chunk(const QueryCall& q, const ByChunk* by) const {
        const bool update = q.family != QF_FOLD_IN || by, revise = q.family == QF_REVISE;
        return {.C = C, .users = s_users.data(), .qo = qo.data(), .items = s_items.data(), .ratings = s_ratings.data(),
                .self = update ? s_self.data() : nullptr, .ao = update ? ao.data() : nullptr, .ro = revise ? ro.data() : nullptr,
                .removed = revise ? s_removed.data() : nullptr, .topk = needs_topk(q), .by = by};
    }
    std::vector<long long> info;  // [4 C] of foldin_batch_neighbors
    std::vector<int32_t> good;    // settle_statuses: the slots whose query is KNNCF_OK
    std::vector<int64_t> ebase;   // [C + 1] of foldin_batch_predictions
    std::vector<int32_t> qrank;   // [C] of entered_chunk
    // the answers on their way back
    std::vector<int32_t> h_idx, h_items, pick_slot, pick_items;
    std::vector<int64_t> pick_row, reco_rb;  // reco_rb: [C + 1] of foldin_batch_reco_rows
    std::vector<double> h_vals, h_top;  // h_top: the recommend modes' predictions (h_vals is an explain launch's block)
};

void fail(const QueryCall& q, ChunkState& cs, int64_t b, int status, const char* why) {
    q.statuses[b] = status;
    if (q.counts) q.counts[b] = 0;
    if (explains(q.mode)) std::fill(q.ex.counts + q.pred_offsets[b], q.ex.counts + q.pred_offsets[b + 1], 0);
    if (cs.first.query < 0 || b < cs.first.query) cs.first = {b, why};
}

// the per-query admission checks of query b: its slot, or false with the refusal recorded (fail)
bool admit(knncf_handle* h, const QueryCall& q, ChunkState& cs, int64_t b, Slot& slot) {
    const bool update = q.family != QF_FOLD_IN, revise = q.family == QF_REVISE;
    const int64_t nb = q.offsets[b + 1] - q.offsets[b];
    const int64_t nr = revise ? q.removed_offsets[b + 1] - q.removed_offsets[b] : 0;
    const int32_t du = dense_user(h, q.users[b]);
    // rows of the user in aug: its train rows (update queries) without the removed ones (revise queries), and the
    // given ones; every train row is seeded, so all of them count against the cap
    const int64_t seeded = nb + (update && du >= 0 ? train_row_length(h, du) : 0);
    const int64_t rows = seeded - nr;
    int status = KNNCF_E_INVALID; const char* why = nullptr;
    if (nr > 0 && du < 0) why = "a removed item for a user that is not in the training set";
    else if (nr > seeded - nb) why = "more removed items than the user has train rows (one is not rated in train or listed twice)";
    else if (rows <= 0) why = nr > 0 ? "the removals leave the user without a row" : "null ratings or n_ratings <= 0";
    else if (seeded > QUERY_MAX_RATINGS) { status = KNNCF_E_UNSUPPORTED; why = "more than 65536 ratings"; }
    else if (!update && du >= 0) why = "the user occurs in the training set";
    if (why) { fail(q, cs, b, status, why); return false; }
    slot = {.query = b, .user = q.users[b], .self = du, .a0 = q.offsets[b], .a1 = q.offsets[b + 1],
            .r0 = nr > 0 ? q.removed_offsets[b] : 0, .r1 = nr > 0 ? q.removed_offsets[b + 1] : 0, .rows = rows};
    return true;
}

// queries [c0, c1): the slots of those that admit() passes; returns their number
int32_t pack_chunk(knncf_handle* h, const QueryCall& q, ChunkState& cs, int64_t c0, int64_t c1) {
    cs.reset();
    Slot slot;
    for (int64_t b = c0; b < c1; ++b)
        if (admit(h, q, cs, b, slot)) cs.append(q, slot);
    return cs.C;
}

// the device's status bits of every slot as the query's status, in this order of precedence; cs.good = the slots left to
// answer, returns their number
size_t settle_statuses(const QueryCall& q, ChunkState& cs) {
    cs.good.clear();
    for (int32_t s = 0; s < cs.C; ++s) {
        const uint64_t bits = (uint64_t)cs.info[4 * s];
        const int64_t b = cs.slot_query[s];
        if (bits & QUERY_ST_RM_UNRATED) fail(q, cs, b, KNNCF_E_INVALID, "a removed item that the user did not rate in train");
        else if (bits & QUERY_ST_RM_TWICE) fail(q, cs, b, KNNCF_E_INVALID, "a removed item listed twice");
        else if (bits & ST_DUPLICATE) fail(q, cs, b, KNNCF_E_DUPLICATE, "the ratings repeat an item");
        else if (bits & ST_NONFINITE) fail(q, cs, b, KNNCF_E_NONFINITE, "scale() == 0 gives a non-finite deviation");
        else if (bits & QUERY_ST_NEG_MEAN) fail(q, cs, b, KNNCF_E_UNSUPPORTED, "a negative mean rating (the predictor would answer aug's global average)");
        else { q.statuses[b] = KNNCF_OK; cs.good.push_back(s); }
    }
    return cs.good.size();
}

// what a bystander chunk has beside its slots (run_bystander_chunks packs it and answers its rows)
constexpr int32_t BY_NO_SLOT = -1;
struct ByRow {
    int64_t row;   // of the call
    int32_t slot;  // the bystander's slot in the chunk, or BY_NO_SLOT
    int32_t own;   // the newcomer's slot in the chunk
};
struct ByChunkState {
    std::vector<int32_t> qslot, qrank, qidx;  // qidx: the changer's index in a list, U for a newcomer (ByChunk)
    std::vector<ByRow> rows;
    int32_t fitted = 0, merged = 0;
    int32_t refolds = 0;  // revise queries whose average(aug) took a sequential fold over the file (answer_bystander_predict)
    void clear() { qslot.clear(); qrank.clear(); qidx.clear(); rows.clear(); fitted = merged = refolds = 0; }
};

// between packing and answering: the chunk (C > 0; bc: its bystander side, else null) through the neighbour pass and settle_statuses
size_t settle_chunk(knncf_handle* h, const QueryCall& q, ChunkState& cs, const ByChunkState* bc) {
    cs.info.assign((size_t)4 * cs.C, 0);
    const ByChunk by = bc ? ByChunk{bc->qslot.data(), bc->qrank.data(), bc->qidx.data(), bc->fitted, bc->merged} : ByChunk{};
    foldin_batch_neighbors(h->tr, h->query_batch, h->prep.sort, cs.chunk(q, bc ? &by : nullptr), h->cfg.k, cs.info.data(), h->stream);
    // a bystander slot stands or falls with its newcomer: the slot's own bits (a negative mean of the bystander, which
    // getNeighbors does not look at) are no status of the query
    for (int32_t s = 0; bc && s < cs.C; ++s)
        if (bc->qslot[s] != s) cs.info[4 * s] = cs.info[4 * bc->qslot[s]];
    return settle_statuses(q, cs);
}

// bs.nbr_idx / bs.nbr_sim [C][take] into cs.h_idx / cs.h_vals (synchronised)
void fetch_neighbor_lists(knncf_handle* h, ChunkState& cs) {
    cs.h_idx.resize((size_t)cs.C * cs.take); cs.h_vals.resize((size_t)cs.C * cs.take);
    KN_HIP(hipMemcpyAsync(cs.h_idx.data(), h->query_batch.nbr_idx.p, cs.h_idx.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    KN_HIP(hipMemcpyAsync(cs.h_vals.data(), h->query_batch.nbr_sim.p, cs.h_vals.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KN_HIP(hipStreamSynchronize(h->stream));
}

void answer_neighbors(knncf_handle* h, const QueryCall& q, ChunkState& cs) {
    const int32_t take = cs.take, width = q.width, c = std::min(take, width);
    if (c > 0) {
        fetch_neighbor_lists(h, cs);
        load_host_ids(h);
    }
    for (const int32_t s : cs.good) {
        const int64_t b = cs.slot_query[s];
        // neighbours of slot s: (allUsers - u) :608 drops a user of the fit
        const int32_t mine = q.family != QF_FOLD_IN && cs.s_self[s] >= 0 ? std::min(take, h->tr.U - 1) : take;
        for (int32_t j = 0; j < std::min(c, mine); ++j) {
            q.out_i[b * width + j] = h->h_uid[cs.h_idx[(size_t)s * take + j]];
            q.out_d[b * width + j] = cs.h_vals[(size_t)s * take + j];
        }
        q.counts[b] = mine;
    }
}

// bs.pred / bs.rated of the chunk: launched only when the chunk has something to answer
void fold_chunk(knncf_handle* h, const QueryCall& q, ChunkState& cs) {
    if (q.predictor == KNNCF_PRED_PERSONALIZED) {  // every rater of every item is a term: no neighbour list, no gather (predict_ms)
        Stage s(h, &h->tm.predict_ms);
        foldin_batch_fold_all(h->tr, h->prow, h->query_batch, h->prep.sort, cs.C, cs.qo[cs.C], q.family != QF_FOLD_IN, h->stream);
        return;
    }
    cs.ebase.assign((size_t)cs.C + 1, 0);
    for (int32_t s = 0; s < cs.C; ++s) cs.ebase[s + 1] = cs.ebase[s] + cs.info[4 * s + 2];
    foldin_batch_predictions(h->tr, h->query_batch, h->prep.sort, cs.C, cs.take, cs.ebase.data(), h->stream);
}

// the fold, then cs.pick_items / cs.pick_slot (m > 0 rows) uploaded to bs.pick_items / bs.pick_slot and, unless an explain kernel
// answers them, through the mode's pick kernel into cs.h_vals [m] (synchronised)
void answer_picks(knncf_handle* h, const QueryCall& q, ChunkState& cs) {
    fold_chunk(h, q, cs);
    QueryBatchScratch& bs = h->query_batch;
    hipStream_t st = h->stream;
    const int64_t m = (int64_t)cs.pick_items.size();
    bs.pick_items.ensure(m); bs.pick_slot.ensure(m);
    if (!explains(q.mode)) bs.pick_out.ensure(m);
    KN_HIP(hipMemcpyAsync(bs.pick_items.p, cs.pick_items.data(), (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, st));
    KN_HIP(hipMemcpyAsync(bs.pick_slot.p, cs.pick_slot.data(), (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (explains(q.mode)) return;
    if (bystanders(q.mode)) bystander_pick(h->tr, bs, bs.pick_items.p, bs.pick_slot.p, m, bs.pick_out.p, st);
    else if (q.predictor == KNNCF_PRED_PERSONALIZED) foldin_batch_pick_all(h->tr, bs, bs.pick_items.p, bs.pick_slot.p, m, bs.pick_out.p, st);
    else foldin_batch_pick(h->tr, bs, bs.pick_items.p, bs.pick_slot.p, m, bs.pick_out.p, st);
    cs.h_vals.resize((size_t)m);
    KN_HIP(hipMemcpyAsync(cs.h_vals.data(), bs.pick_out.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
    KN_HIP(hipStreamSynchronize(st));
}

// QB_PREDICT and the explain modes: the requested rows of the chunk's good queries, (item, slot) each, through answer_picks;
// explain modes: cs.pick_row = the row of the call behind each.  Returns their number m (0: nothing was launched)
int64_t pick_requested_rows(knncf_handle* h, const QueryCall& q, ChunkState& cs) {
    cs.pick_slot.clear(); cs.pick_items.clear(); cs.pick_row.clear();
    for (const int32_t s : cs.good) {
        const int64_t b = cs.slot_query[s];
        cs.pick_items.insert(cs.pick_items.end(), q.pred_items + q.pred_offsets[b], q.pred_items + q.pred_offsets[b + 1]);
        cs.pick_slot.insert(cs.pick_slot.end(), (size_t)(q.pred_offsets[b + 1] - q.pred_offsets[b]), s);
        if (explains(q.mode))
            for (int64_t j = q.pred_offsets[b]; j < q.pred_offsets[b + 1]; ++j) cs.pick_row.push_back(j);
    }
    const int64_t m = (int64_t)cs.pick_items.size();
    if (m > 0) answer_picks(h, q, cs);
    return m;
}

void answer_predict(knncf_handle* h, const QueryCall& q, ChunkState& cs) {
    if (pick_requested_rows(h, q, cs) == 0) return;
    int64_t at = 0;
    for (const int32_t s : cs.good) {
        const int64_t b = cs.slot_query[s];
        const int64_t mb = q.pred_offsets[b + 1] - q.pred_offsets[b];
        std::copy(cs.h_vals.begin() + at, cs.h_vals.begin() + at + mb, q.out_d + q.pred_offsets[b]);
        at += mb;
    }
}

// sub-ranges of at most ex_rows rows: the chunk's fold results stay where they are between the launches, and every launch's
// block comes back in one copy
void explain_picks(knncf_handle* h, const QueryCall& q, ChunkState& cs, int64_t m, int64_t ex_rows) {
    QueryBatchScratch& bs = h->query_batch;
    hipStream_t st = h->stream;
    const int64_t R = std::min(ex_rows, m);
    const size_t pack = ((size_t)R * explain_row_bytes(q.ex.cap) + 7) / 8;  // doubles
    h->ex_pack.ensure(pack);
    cs.h_vals.resize(pack);
    const bool all = explains_all(q);  // (the terms of the Personalized fold; BY_WEIGHT stages the selected ones)
    if (all && q.ex.order == KNNCF_EXPLAIN_BY_WEIGHT) h->ex_stage.ensure(((size_t)R * q.ex.cap * 20 + 7) / 8);
    for (int64_t r0 = 0; r0 < m; r0 += R) {
        const int64_t nr = std::min(R, m - r0);
        if (all) {
            Stage s(h, &h->tm.predict_ms);
            const QbExplainRows rows{0, 0, bs.pick_items.p, bs.pick_slot.p, r0, nr};
            foldin_batch_explain_all(h->tr, h->prow, bs, rows, q.family != QF_FOLD_IN, explain_pack(h->ex_pack.p, nr, q.ex),
                                     h->ex_stage.p, st);
        } else {
            const QbExplainRows rows{cs.take, cs.ebase[cs.C], bs.pick_items.p, bs.pick_slot.p, r0, nr};
            foldin_batch_explain(h->tr, bs, rows, explain_pack(h->ex_pack.p, nr, q.ex), st);
        }
        KN_HIP(hipMemcpyAsync(cs.h_vals.data(), h->ex_pack.p, (size_t)nr * explain_row_bytes(q.ex.cap), hipMemcpyDeviceToHost, st));
        KN_HIP(hipStreamSynchronize(st));
        explain_scatter(explain_pack(cs.h_vals.data(), nr, q.ex), nr, q.ex, cs.pick_row.data() + r0);
    }
}

void answer_explain(knncf_handle* h, const QueryCall& q, ChunkState& cs, int64_t ex_rows) {
    const int64_t m = pick_requested_rows(h, q, cs);
    if (m > 0) explain_picks(h, q, cs, m, ex_rows);
}

// the recommend modes: counts[b] of the chunk's good queries and, when their widest is > 0, the fold and the selection into
// bs.out_items / bs.out_preds [C][widest], on their way to cs.h_items / cs.h_top (not synchronised).  Returns widest
int32_t select_recommendations(knncf_handle* h, const QueryCall& q, ChunkState& cs) {
    QueryBatchScratch& bs = h->query_batch;
    hipStream_t st = h->stream;
    int32_t widest = 0;
    for (const int32_t s : cs.good) {
        const int64_t b = cs.slot_query[s];
        q.counts[b] = (int32_t)std::max<int64_t>(0, std::min<int64_t>(q.width, (int64_t)h->tr.I - cs.info[4 * s + 1]));
        widest = std::max(widest, q.counts[b]);
    }
    if (widest == 0) return 0;
    fold_chunk(h, q, cs);
    const size_t cells = (size_t)cs.C * widest;
    bs.out_items.ensure(cells); bs.out_preds.ensure(cells);
    foldin_batch_recommend(h->tr, bs, h->prep.sort, cs.C, widest, bs.out_items.p, bs.out_preds.p, st);
    cs.h_items.resize(cells); cs.h_top.resize(cells);
    KN_HIP(hipMemcpyAsync(cs.h_items.data(), bs.out_items.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    KN_HIP(hipMemcpyAsync(cs.h_top.data(), bs.out_preds.p, cells * sizeof(double), hipMemcpyDeviceToHost, st));
    return widest;
}
// after the stream was synchronised: the first counts[b] cells of every good slot into row b of the caller's arrays
void write_recommendations(const QueryCall& q, const ChunkState& cs, int32_t widest) {
    for (const int32_t s : cs.good) {
        const int64_t b = cs.slot_query[s];
        std::copy(cs.h_items.begin() + (size_t)s * widest, cs.h_items.begin() + (size_t)s * widest + q.counts[b], q.out_i + b * q.width);
        std::copy(cs.h_top.begin() + (size_t)s * widest, cs.h_top.begin() + (size_t)s * widest + q.counts[b], q.out_d + b * q.width);
    }
}

void answer_recommend(knncf_handle* h, const QueryCall& q, ChunkState& cs) {
    const int32_t widest = select_recommendations(h, q, cs);
    if (widest == 0) return;
    KN_HIP(hipStreamSynchronize(h->stream));
    write_recommendations(q, cs, widest);
}

// QB_RECOMMEND_EXPLAIN: the selection's cells become explain rows on the device, slot after slot and j ascending, so the first
// explain launch follows the selection without a round trip; its synchronisation is also the one of the top-n copies.  The
// host knows every count (select_recommendations) and with them the row of the call behind each device row: b * n + j.
void answer_recommend_explain(knncf_handle* h, const QueryCall& q, ChunkState& cs, int64_t ex_rows) {
    const int32_t widest = select_recommendations(h, q, cs);
    if (widest == 0) return;
    cs.reco_rb.assign((size_t)cs.C + 1, 0);
    cs.pick_row.clear();
    for (const int32_t s : cs.good) {
        const int64_t b = cs.slot_query[s];
        cs.reco_rb[s + 1] = q.counts[b];
        for (int32_t j = 0; j < q.counts[b]; ++j) cs.pick_row.push_back(b * q.width + j);
    }
    for (int32_t s = 0; s < cs.C; ++s) cs.reco_rb[s + 1] += cs.reco_rb[s];
    foldin_batch_reco_rows(h->query_batch, cs.C, widest, cs.reco_rb.data(), h->query_batch.out_items.p, h->stream);
    explain_picks(h, q, cs, cs.reco_rb[cs.C], ex_rows);
    write_recommendations(q, cs, widest);
}

// QB_ENTERED (entered.hip; knncf.h "Entered queries"): counts[b] and the first min(counts[b], cap) entered users of every good
// query in row b of the four output arrays.  One copy back per chunk.
void answer_entered(knncf_handle* h, const QueryCall& q, ChunkState& cs) {
    if (cs.take == 0) {  // (k <= 0: no list has a cell)
        for (const int32_t s : cs.good) q.counts[cs.slot_query[s]] = 0;
        return;
    }
    QueryBatchScratch& bs = h->query_batch;
    hipStream_t st = h->stream;
    const int32_t width = std::min(q.width, h->tr.U);
    load_host_ids(h);
    cs.qrank.resize((size_t)cs.C);
    for (int32_t s = 0; s < cs.C; ++s) {
        const uint32_t qkey = int_trie_key(cs.s_users[s]);
        cs.qrank[s] = (int32_t)(std::lower_bound(h->h_ukeys.begin(), h->h_ukeys.end(), qkey) - h->h_ukeys.begin());
    }
    entered_chunk(h->tr, h->nt, bs, cs.C, cs.take, width, cs.qo.data(), cs.qrank.data(), st);
    const size_t bytes = entered_pack_bytes(cs.C, width);
    cs.h_vals.resize((bytes + 7) / 8);
    KN_HIP(hipMemcpyAsync(cs.h_vals.data(), bs.en_pack.p, bytes, hipMemcpyDeviceToHost, st));
    KN_HIP(hipStreamSynchronize(st));
    const EnteredPack got = entered_pack(cs.h_vals.data(), cs.C, width);
    for (const int32_t s : cs.good) {
        const int64_t b = cs.slot_query[s];
        const size_t at = (size_t)s * width, dst = (size_t)b * q.width;
        const int64_t t = std::min<int64_t>(got.counts[s], width);
        q.counts[b] = got.counts[s];
        std::copy(got.users + at, got.users + at + t, q.out_i + dst);
        std::copy(got.sims + at, got.sims + at + t, q.out_d + dst);
        std::copy(got.pos + at, got.pos + at + t, q.out_pos + dst);
        std::copy(got.displaced + at, got.displaced + at + t, q.out_displaced + dst);
    }
}

QueryFailure run_bystander_chunks(knncf_handle* h, const QueryCall& q, int64_t chunk);
int64_t bystander_chunk(knncf_handle* h, int64_t budget);

// QB_ENTERED under QF_UPDATE (entered.hip; knncf.h "Entered queries of update queries"): phase 1 is answer_entered's with the
// chunk's update slots — counts[b] and the first min(counts[b], cap) reported users of every good query on the host.  Phase 2
// resolves the tail rows among them (pos == EN_TAIL: the changer sorts behind every other stored entry of a full list, and the
// best candidate outside the list decides) through the bystander path: one internal knncf_update_bystander_neighbors_batch over
// the chunk's queries that have some, rows = their tail users, cap = take.  A query's rows are written once all of them are
// resolved; a query whose tail user the bystander path refuses takes that status and keeps its rows untouched.
// Under QF_REVISE (knncf.h "Entered queries of revise queries") the chunk's slots are revise slots, and the internal call is
// knncf_revise_bystander_neighbors_batch with each query's removed items.
void answer_entered_update(knncf_handle* h, const QueryCall& q, ChunkState& cs) {
    if (cs.take == 0) {  // (k <= 0: no list has a cell)
        for (const int32_t s : cs.good) q.counts[cs.slot_query[s]] = 0;
        return;
    }
    QueryBatchScratch& bs = h->query_batch;
    hipStream_t st = h->stream;
    const int32_t width = std::min(q.width, h->tr.U), take = cs.take;
    load_host_ids(h);
    cs.qrank.resize((size_t)cs.C);
    for (int32_t s = 0; s < cs.C; ++s) {
        const uint32_t qkey = int_trie_key(cs.s_users[s]);
        cs.qrank[s] = (int32_t)(std::lower_bound(h->h_ukeys.begin(), h->h_ukeys.end(), qkey) - h->h_ukeys.begin());
    }
    entered_update_chunk(h->tr, h->nt, bs, cs.C, take, width, cs.qo.data(), cs.s_self.data(), cs.ro.data(), cs.qrank.data(), st);
    const size_t bytes = entered_update_pack_bytes(cs.C, width);
    cs.h_vals.resize((bytes + 7) / 8);
    KN_HIP(hipMemcpyAsync(cs.h_vals.data(), bs.en_pack.p, bytes, hipMemcpyDeviceToHost, st));
    KN_HIP(hipStreamSynchronize(st));
    const EnteredPack got = entered_pack(cs.h_vals.data(), cs.C, width);
    int32_t* prev = entered_pack_prev(got, cs.C);
    // phase 2: the tail rows within the written cells, query after query
    std::vector<int32_t> t_users, t_items, t_others, t_cell, t_status;
    std::vector<int32_t> t_removed;
    std::vector<int64_t> t_off(1, 0), t_rows(1, 0), t_roff(1, 0);
    std::vector<double> t_ratings;
    const bool revise = q.family == QF_REVISE;
    std::vector<int32_t> t_of((size_t)cs.C, -1);  // the slot's query of the internal call
    for (const int32_t s : cs.good) {
        const size_t at = (size_t)s * width;
        const int64_t t = std::min<int64_t>(got.counts[s], width), b = cs.slot_query[s];
        for (int64_t j = 0; j < t; ++j) {
            if (got.pos[at + j] != EN_TAIL) continue;
            t_others.push_back(got.users[at + j]);
            t_cell.push_back((int32_t)j);
        }
        if ((int64_t)t_others.size() == t_rows.back()) continue;
        t_of[s] = (int32_t)t_users.size();
        t_users.push_back(q.users[b]);
        t_items.insert(t_items.end(), q.items + q.offsets[b], q.items + q.offsets[b + 1]);
        t_ratings.insert(t_ratings.end(), q.ratings + q.offsets[b], q.ratings + q.offsets[b + 1]);
        t_off.push_back((int64_t)t_items.size());
        if (revise) t_removed.insert(t_removed.end(), q.removed_items + q.removed_offsets[b], q.removed_items + q.removed_offsets[b + 1]);
        t_roff.push_back((int64_t)t_removed.size());
        t_rows.push_back((int64_t)t_others.size());
    }
    std::vector<int32_t> l_ids((size_t)t_others.size() * take), l_counts(t_others.size(), 0);
    std::vector<double> l_sims((size_t)t_others.size() * take);
    if (!t_users.empty()) {
        t_status.assign(t_users.size(), KNNCF_OK);
        const QueryCall inner = bystander_neighbors_call({.family = q.family, .users = t_users.data(), .B = (int64_t)t_users.size(),
                                                          .offsets = t_off.data(), .items = t_items.data(), .ratings = t_ratings.data(),
                                                          .removed_offsets = revise ? t_roff.data() : nullptr,
                                                          .removed_items = revise ? t_removed.data() : nullptr,
                                                          .pred_offsets = t_rows.data(), .statuses = t_status.data()},
                                                         t_others.data(), take, l_ids.data(), l_sims.data(), l_counts.data());
        const auto t0 = std::chrono::steady_clock::now();  // (the hook also says what phase 2 took: it ends synchronised)
        run_bystander_chunks(h, inner, bystander_chunk(h, batch_budget(h)));  // (reuses the chunk's device scratch: its answers are on the host)
        KN_TRACE_DISPATCH("entered_update tails queries=%d rows=%d ms=%.3f", (int)t_users.size(), (int)t_others.size(),
                          std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    for (const int32_t s : cs.good) {
        const int64_t b = cs.slot_query[s];
        const size_t at = (size_t)s * width, dst = (size_t)b * q.width;
        const int64_t t = std::min<int64_t>(got.counts[s], width);
        if (t_of[s] >= 0) {
            const int32_t tq = t_of[s];
            if (t_status[tq] != KNNCF_OK) {
                fail(q, cs, b, t_status[tq], "a tail row's user that the bystander path refuses (more than 65536 ratings)");
                continue;
            }
            for (int64_t r = t_rows[tq]; r < t_rows[tq + 1]; ++r) {
                const size_t cell = at + (size_t)t_cell[r];
                const int32_t* ids = l_ids.data() + (size_t)r * take;
                const int32_t n = std::min(l_counts[r], take);
                const int32_t p = (int32_t)(std::find(ids, ids + n, q.users[b]) - ids);
                if (p < n) {  // the changer kept the last cell: the cell's own bits
                    got.pos[cell] = p; got.displaced[cell] = -1; got.sims[cell] = l_sims[(size_t)r * take + p];
                } else {      // it left: the user that came into the last cell
                    got.pos[cell] = -1; got.displaced[cell] = n > 0 ? ids[n - 1] : -1;
                }
            }
        }
        q.counts[b] = got.counts[s];
        std::copy(got.users + at, got.users + at + t, q.out_i + dst);
        std::copy(got.sims + at, got.sims + at + t, q.out_d + dst);
        std::copy(got.pos + at, got.pos + at + t, q.out_pos + dst);
        std::copy(got.displaced + at, got.displaced + at + t, q.out_displaced + dst);
        std::copy(prev + at, prev + at + t, q.out_prev + dst);
    }
}

// The validated queries of q in chunks of `chunk`, one slot per query: statuses[b] and, where it is KNNCF_OK, query b's answer
// in q's outputs.  A refused query gets ex.counts = 0 on its rows (the explain modes, answered ex_rows rows per launch)
QueryFailure run_query_chunks(knncf_handle* h, const QueryCall& q, int64_t chunk, int64_t ex_rows) {
    h->prep.join_commit(h->stream);
    if (q.predictor == KNNCF_PRED_PERSONALIZED) ensure_personal_rows(h, false);
    ChunkState cs;
    cs.take = std::max(0, std::min(h->cfg.k, h->tr.U));
    for (int64_t c0 = 0; c0 < q.B; c0 += chunk) {
        if (pack_chunk(h, q, cs, c0, std::min(q.B, c0 + chunk)) == 0) continue;
        if (settle_chunk(h, q, cs, nullptr) == 0) continue;
        switch (q.mode) {
            case QB_NEIGHBORS: answer_neighbors(h, q, cs); break;
            case QB_PREDICT: answer_predict(h, q, cs); break;
            case QB_EXPLAIN:
            case QB_EXPLAIN_ALL: answer_explain(h, q, cs, ex_rows); break;
            case QB_RECOMMEND: answer_recommend(h, q, cs); break;
            case QB_RECOMMEND_EXPLAIN: answer_recommend_explain(h, q, cs, ex_rows); break;
            case QB_ENTERED: q.family != QF_FOLD_IN ? answer_entered_update(h, q, cs) : answer_entered(h, q, cs); break;
            case QB_BY_NEIGHBORS:
            case QB_BY_PREDICT: throw Error(KNNCF_E_INVALID, "query: a bystander mode in run_query_chunks (run_bystander_chunks answers them)");
        }
    }
    return cs.first;
}

// ---- bystander queries: fitted users' answers on aug = train ++ a newcomer's rows (bystander.hip) ----------------------------
// A query is a fold-in query (admit admits it, settle_statuses gives it its status); its rows name bystanders.  The unit
// of a chunk is a slot: the newcomer's own, then one per distinct bystander that needs the device — a user of the fit, in
// QB_BY_PREDICT with a mean >= 0.  The rows of the other bystanders are answered on the host once the query's status is known.
// knncf_update_bystander_* run the same loop with family QF_UPDATE: the query is an update query, and where its user is of the
// fit (a fitted CHANGER) its own slot is an update slot and no list takes a newcomer in (bystander.hip).
// knncf_revise_bystander_* run it with family QF_REVISE: a fitted changer's own slot leaves out the train rows it removes (a
// revise slot; the chunk carries the removed CSR), and average(aug) of such a query is folded anew (revised_average).

// slots per chunk: the rule of knncf.h ("Bystander queries")
int64_t bystander_chunk(knncf_handle* h, int64_t budget) { return std::max<int64_t>(2, query_batch_chunk(h, budget)); }

// average(aug) :18: the fit's left fold of the train ratings, continued over query b's ratings in the given order
double aug_average(knncf_handle* h, const QueryCall& q, int64_t b) {
    double t = h->tr.total;
    for (int64_t j = q.offsets[b]; j < q.offsets[b + 1]; ++j) t = t + q.ratings[j];
    return t / (double)(h->tr.n + (q.offsets[b + 1] - q.offsets[b]));
}
// the removals of query b (revise queries)
int64_t removals(const QueryCall& q, int64_t b) { return q.family == QF_REVISE ? q.removed_offsets[b + 1] - q.removed_offsets[b] : 0; }
// average(aug) of a revise query with removals: `survivors` = the fold of the surviving train ratings in file order
// (bystander_survivor_totals), continued over query b's ratings in the given order, over n - n_removed + n_ratings
double revised_average(knncf_handle* h, const QueryCall& q, int64_t b, double survivors) {
    double t = survivors;
    for (int64_t j = q.offsets[b]; j < q.offsets[b + 1]; ++j) t = t + q.ratings[j];
    return t / (double)(h->tr.n - removals(q, b) + (q.offsets[b + 1] - q.offsets[b]));
}

// QB_BY_NEIGHBORS: the lists of the rows whose query is good
void answer_bystander_neighbors(knncf_handle* h, const QueryCall& q, ChunkState& cs, const ByChunkState& bc) {
    const int32_t U = h->tr.U, take = cs.take, width = q.width, c = std::min(take, width);
    if (c > 0) fetch_neighbor_lists(h, cs);
    for (const ByRow& r : bc.rows) {
        if (q.statuses[cs.slot_query[r.own]] != KNNCF_OK) continue;
        const bool fitted = cs.s_self[r.own] >= 0;  // the changer is a user of the fit: aug has the fit's users
        const int32_t newcomer = cs.s_users[r.own], at = fitted ? U : bc.qrank[r.own];
        int32_t* ids = q.out_i + r.row * width;
        double* sims = q.out_d + r.row * width;
        if (r.slot == BY_NO_SLOT) {  // unknown to aug: every similarity is 0.0, ties keep the set order of aug's users
            const int32_t n = (int32_t)std::min<int64_t>(h->cfg.k, (int64_t)U + (fitted ? 0 : 1));
            for (int32_t j = 0; j < std::min(n, width); ++j) {
                ids[j] = j < at ? h->h_uid[j] : j == at ? newcomer : h->h_uid[j - 1];
                sims[j] = 0.0;
            }
            q.row_counts[r.row] = std::max(n, 0);
            continue;
        }
        const int32_t mine = fitted ? std::min(take, U - 1) : take;  // (a fitted changer is one of the U - 1 candidates)
        for (int32_t j = 0; j < std::min(c, mine); ++j) {
            const int32_t v = cs.h_idx[(size_t)r.slot * take + j];
            ids[j] = v == U ? newcomer : h->h_uid[v];
            sims[j] = cs.h_vals[(size_t)r.slot * take + j];
        }
        q.row_counts[r.row] = mine;
    }
}

// QB_BY_PREDICT: the rows whose query is good — on the host where the bystander has no slot, else through answer_picks
// A revise query with removals and a row answered with average(aug) has its surviving train ratings folded on the device, once
// per query (the slot-less rows of a query all stand in the chunk of its first slot); bc.refolds counts the sequential folds
void answer_bystander_predict(knncf_handle* h, const QueryCall& q, ChunkState& cs, ByChunkState& bc) {
    cs.pick_slot.clear(); cs.pick_items.clear(); cs.pick_row.clear();
    std::vector<int32_t> fold_slots;  // the changer slots whose average is not the running total's continuation
    for (const ByRow& r : bc.rows) {
        if (q.statuses[cs.slot_query[r.own]] != KNNCF_OK) continue;
        if (r.slot == BY_NO_SLOT) {
            if (removals(q, cs.slot_query[r.own]) == 0) q.out_d[r.row] = aug_average(h, q, cs.slot_query[r.own]);
            else if (fold_slots.empty() || fold_slots.back() != r.own) fold_slots.push_back(r.own);  // (rows come query after query)
            continue;
        }
        cs.pick_items.push_back(q.pred_items[r.row]);
        cs.pick_slot.push_back(r.slot);
        cs.pick_row.push_back(r.row);
    }
    if (!fold_slots.empty()) {
        std::vector<double> survivors(fold_slots.size());
        bystander_survivor_totals(h->tr, h->query_batch, fold_slots.data(), (int32_t)fold_slots.size(), survivors.data(), h->stream);
        if (!h->tr.exact_total) bc.refolds += (int32_t)fold_slots.size();
        size_t x = 0;
        for (const ByRow& r : bc.rows) {
            if (r.slot != BY_NO_SLOT || q.statuses[cs.slot_query[r.own]] != KNNCF_OK || removals(q, cs.slot_query[r.own]) == 0) continue;
            while (fold_slots[x] != r.own) ++x;
            q.out_d[r.row] = revised_average(h, q, cs.slot_query[r.own], survivors[x]);
        }
    }
    if (cs.pick_items.empty()) return;
    answer_picks(h, q, cs);
    for (size_t j = 0; j < cs.pick_row.size(); ++j) q.out_d[cs.pick_row[j]] = cs.h_vals[j];
}

// The validated queries of q in chunks of `chunk` >= 2 slots: statuses[b] and, where it is KNNCF_OK, the answers of query b's
// rows.  (q.counts is null: fail() writes no per-query count; the rows' counts were zeroed by the caller.)  The packing is this
// loop's own: a query takes a varying number of slots and may span chunks
QueryFailure run_bystander_chunks(knncf_handle* h, const QueryCall& q, int64_t chunk) {
    h->prep.join_commit(h->stream);
    load_host_ids(h);
    KN_REQUIRE(h->tr.n + QUERY_MAX_RATINGS < ((int64_t)1 << 32), KNNCF_E_UNSUPPORTED, "query bystander: the newcomer's file rows pass 2^32");
    const bool predict = q.mode == QB_BY_PREDICT;
    ChunkState cs;
    ByChunkState bc;
    std::vector<int32_t> dist, row_at;  // query b's distinct slot bystanders (dense) in order of appearance; per row its index or -1
    std::vector<std::pair<int32_t, int32_t>> seen, firsts;  // (dense user, row) grouped by user; (first row, dense user)
    cs.take = std::max(0, std::min(h->cfg.k, h->tr.U));
    cs.reset();
    auto flush = [&] {  // the chunk in cs / bc through the device, then the answers of its rows
        if (cs.C > 0 && settle_chunk(h, q, cs, &bc) > 0)
            q.mode == QB_BY_NEIGHBORS ? answer_bystander_neighbors(h, q, cs, bc) : answer_bystander_predict(h, q, cs, bc);
        if (cs.C > 0 && cs.ro[cs.C] > 0) {  // (a chunk that holds a changer with removals)
            int32_t revise_slots = 0;
            for (int32_t s = 0; s < cs.C; ++s) revise_slots += cs.ro[s + 1] > cs.ro[s];
            KN_TRACE_DISPATCH("bystander-revise slots=%d removed=%lld refold=%d", (int)revise_slots, (long long)cs.ro[cs.C], (int)bc.refolds);
        }
        cs.reset(); bc.clear();
    };
    // one more slot of changer `own`'s (its own included): what the device reads beside the slot
    auto append = [&](const Slot& slot, int32_t own, int32_t at, int32_t ci) {
        bc.qslot.push_back(own); bc.qrank.push_back(at); bc.qidx.push_back(ci);
        return cs.append(q, slot);
    };
    for (int64_t b = 0; b < q.B; ++b) {
        const int64_t r0 = q.pred_offsets[b], r1 = q.pred_offsets[b + 1];
        Slot mine;
        if (!admit(h, q, cs, b, mine)) continue;
        bool self_row = false, long_row = false;
        dist.clear(); row_at.assign((size_t)(r1 - r0), -1); seen.clear(); firsts.clear();
        for (int64_t r = r0; r < r1; ++r) {
            if (q.others[r] == q.users[b]) { self_row = true; break; }
            const int32_t dv = dense_user(h, q.others[r]);
            if (dv < 0 || (predict && train_user_avg(h, dv) < 0.0)) continue;
            if (train_row_length(h, dv) > QUERY_MAX_RATINGS) { long_row = true; break; }
            seen.push_back({dv, (int32_t)(r - r0)});
        }
        if (self_row) { fail(q, cs, b, KNNCF_E_INVALID, "a row names the query's own user (ask the query's own predict call)"); continue; }
        if (long_row) { fail(q, cs, b, KNNCF_E_UNSUPPORTED, "a bystander with more than 65536 ratings"); continue; }
        std::stable_sort(seen.begin(), seen.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
        // distinct bystanders, numbered in order of first appearance
        for (size_t x = 0; x < seen.size(); ++x)
            if (x == 0 || seen[x].first != seen[x - 1].first) firsts.push_back({seen[x].second, seen[x].first});
        std::sort(firsts.begin(), firsts.end());
        for (const auto& f : firsts) dist.push_back(f.second);
        // (seen is grouped by user: one search per distinct bystander)
        for (size_t x = 0, d = 0; x < seen.size(); ++x) {
            if (x == 0 || seen[x].first != seen[x - 1].first) d = (size_t)(std::find(dist.begin(), dist.end(), seen[x].first) - dist.begin());
            row_at[(size_t)seen[x].second] = (int32_t)d;
        }
        const uint32_t qkey = int_trie_key(q.users[b]);
        const int32_t at = (int32_t)(std::lower_bound(h->h_ukeys.begin(), h->h_ukeys.end(), qkey) - h->h_ukeys.begin());
        // the changer: a newcomer (index U in a list), or with knncf_update_bystander_* a user of the fit whose own slot is an
        // update slot — its train rows seeded in front of the given ones.  (admit leaves no fold-in query with a user of the fit)
        const int32_t dc = mine.self, ci = dc >= 0 ? dc : h->tr.U;
        size_t pos = 0;
        do {
            if (chunk - cs.C < (dist.empty() ? 1 : 2)) flush();
            const int32_t own = append(mine, cs.C, at, ci);
            if (dc >= 0) ++bc.fitted;
            const size_t cnt = std::min<size_t>(dist.size() - pos, (size_t)(chunk - cs.C));
            for (size_t d = pos; d < pos + cnt; ++d) {
                const int32_t dv = dist[d];  // (a fitted user without rows of the call)
                append({.query = b, .user = h->h_uid[dv], .self = dv, .rows = train_row_length(h, dv)}, own, at, ci);
                if (dc < 0) ++bc.merged;
            }
            for (int64_t r = r0; r < r1; ++r) {
                const int32_t d = row_at[(size_t)(r - r0)];
                if (d < 0) { if (pos == 0) bc.rows.push_back({r, BY_NO_SLOT, own}); }
                else if ((size_t)d >= pos && (size_t)d < pos + cnt) bc.rows.push_back({r, own + 1 + (int32_t)((size_t)d - pos), own});
            }
            pos += cnt;
        } while (pos < dist.size());
    }
    flush();
    return cs.first;
}

// the refusals the explain forms add to those of the predict forms (knncf.h "Explanations of query predictions")
void require_explain_order(const ExplainCells& ex) {
    KN_REQUIRE(ex.cap >= 0, KNNCF_E_INVALID, "query explain: cap < 0");
    KN_REQUIRE(ex.order == KNNCF_EXPLAIN_SUM_ORDER || ex.order == KNNCF_EXPLAIN_BY_WEIGHT, KNNCF_E_INVALID,
               "query explain: unknown order");
}
void require_explain_outputs(const ExplainCells& ex, int64_t m) {
    KN_REQUIRE(m == 0 || (ex.counts && (ex.cap == 0 || (ex.raters && ex.sims && ex.devs))), KNNCF_E_INVALID,
               "query explain: null output");
}

// a CSR's offsets as the batch forms take them: B + 1 of them, from 0, never decreasing; the two refusals' texts
void require_offsets(const int64_t* o, int64_t B, const char* no_start, const char* decrease) {
    KN_REQUIRE(o && o[0] == 0, KNNCF_E_INVALID, no_start);
    for (int64_t b = 0; b < B; ++b) KN_REQUIRE(o[b] <= o[b + 1], KNNCF_E_INVALID, decrease);
}

// the first refused query as the call's error: thrown with the query's status by a single form (a batch of one), left in
// knncf_last_error by a batch form, whose return value stays KNNCF_OK
void report_failure(knncf_handle* h, const QueryCall& q, const QueryFailure& f, bool single) {
    if (f.query < 0) return;
    if (single) throw Error(q.statuses[0], std::string("query: ") + f.reason);
    h->err = "query batch: query " + std::to_string(f.query) + ": " + f.reason;
}

// Every batch form, and the bystander and entered single forms as a batch of one (single: the texts say "query", and the
// query's status is thrown as the call's).  The checks come in the order the call-level record pins
void do_query_batch(knncf_handle* h, const QueryCall& q, bool single) {
    const int64_t B = q.B;
    auto text = [&](const char* t) { return std::string(single ? "query: " : "query batch: ") + t; };
    require_fitted(h, false);
    KN_REQUIRE(B >= 0, KNNCF_E_INVALID, text("n_queries < 0"));
    KN_REQUIRE(wants_rows(q.mode) || q.mode == QB_BY_PREDICT || q.width >= 0, KNNCF_E_INVALID,
               text(bystanders(q.mode) || q.mode == QB_ENTERED ? "cap < 0" : "cap or n < 0"));
    if (runs_explain(q)) require_explain_order(q.ex);
    require_query_support(h, q.predictor, q.mode);
    KN_REQUIRE(q.mode != QB_ENTERED || h->cfg.similarity != KNNCF_SIM_COSINE || !has_short_rows(h), KNNCF_E_UNSUPPORTED,
               "query entered with the adjusted cosine: a user with <= 4 ratings makes the reference's summation order depend on its memo history pair by pair (SURVEY N6); the stored lists are not the fresh-closure lists");
    if (B == 0) return;
    KN_REQUIRE(q.users && q.offsets && q.statuses && (!counts_queries(q.mode) || q.counts), KNNCF_E_INVALID, text("null argument"));
    require_offsets(q.offsets, B, "query batch: offsets[0] != 0", "query batch: offsets decrease");
    KN_REQUIRE(q.offsets[B] < ((int64_t)1 << 31), KNNCF_E_INVALID, text("2^31 or more ratings in one call"));
    KN_REQUIRE(q.offsets[B] == 0 || (q.items && q.ratings), KNNCF_E_INVALID, text("null ratings"));
    if (q.family == QF_REVISE) {
        require_offsets(q.removed_offsets, B, "query batch: removed_offsets null or not starting at 0", "query batch: removed_offsets decrease");
        KN_REQUIRE(q.removed_offsets[B] < ((int64_t)1 << 31), KNNCF_E_INVALID, "query batch: 2^31 or more removed items in one call");
        KN_REQUIRE(q.removed_offsets[B] == 0 || q.removed_items, KNNCF_E_INVALID, "query batch: null removed items");
    }
    if (bystanders(q.mode)) {
        require_offsets(q.pred_offsets, B, "query batch: row_offsets null or not starting at 0", "query batch: row_offsets decrease");
        const int64_t rows = q.pred_offsets[B];
        KN_REQUIRE(rows < ((int64_t)1 << 31), KNNCF_E_INVALID, text("2^31 or more rows in one call"));
        const bool outputs = q.mode == QB_BY_PREDICT ? q.pred_items && q.out_d : q.row_counts && (q.width == 0 || (q.out_i && q.out_d));
        KN_REQUIRE(rows == 0 || (q.others && outputs), KNNCF_E_INVALID, text("null row arguments"));
        if (q.mode == QB_BY_NEIGHBORS) std::fill(q.row_counts, q.row_counts + rows, 0);
    } else if (wants_rows(q.mode)) {
        require_offsets(q.pred_offsets, B, "query batch: pred_offsets null or not starting at 0", "query batch: pred_offsets decrease");
        KN_REQUIRE(q.pred_offsets[B] == 0 || (q.pred_items && (explains(q.mode) || q.out_d)), KNNCF_E_INVALID,
                   "query batch: null prediction arguments");
        if (explains(q.mode)) require_explain_outputs(q.ex, q.pred_offsets[B]);
    } else {
        KN_REQUIRE(q.width == 0 || (q.out_i && q.out_d && (q.mode != QB_ENTERED || (q.out_pos && q.out_displaced && (q.family == QF_FOLD_IN || q.out_prev)))), KNNCF_E_INVALID,
                   text("null output"));
        if (q.mode == QB_RECOMMEND_EXPLAIN) require_explain_outputs(q.ex, q.width);
    }
    if (q.mode == QB_ENTERED) build_unbuilt_neighbors(h);  // (the place rule reads the handle's stored lists)
    const int64_t budget = batch_budget(h);  // (one hipMemGetInfo for both rules)
    report_failure(h, q, bystanders(q.mode) ? run_bystander_chunks(h, q, bystander_chunk(h, budget))
                                           : run_query_chunks(h, q, query_batch_chunk(h, budget), launch_rows(q, budget)), single);
}

// the rows a single form brings: a fold-in query needs some; an update query may come without (whether the user is in the fit
// is the chunk loop's to say)
void require_single_ratings(const QueryCall& call) {
    if (call.family != QF_FOLD_IN) {
        KN_REQUIRE(call.n_ratings >= 0 && (call.n_ratings == 0 || (call.items && call.ratings)), KNNCF_E_INVALID,
                   "query: null ratings or n_ratings < 0");
    } else {
        KN_REQUIRE(call.items && call.ratings && call.n_ratings > 0, KNNCF_E_INVALID, "query: null ratings or n_ratings <= 0");
    }
}

// a single form's call as a batch of one: q = the call with users, B, statuses and the offsets arrays made from its last four fields
struct BatchOfOne {
    int64_t offsets[2], pred_offsets[2], removed_offsets[2];
    int32_t status = KNNCF_OK;
    QueryCall q;
    explicit BatchOfOne(const QueryCall& call)
        : offsets{0, call.n_ratings}, pred_offsets{0, call.m}, removed_offsets{0, call.n_removed}, q(call) {
        q.users = &q.user; q.B = 1; q.statuses = &status;
        q.offsets = offsets; q.pred_offsets = pred_offsets; q.removed_offsets = removed_offsets;
    }
    BatchOfOne(const BatchOfOne&) = delete;  // (q points into this object)
};

// the single forms' own output arguments, checked in front of everything else (the explain forms check theirs after
// require_fitted, in do_query_single); a recommend form's *count is 0 whatever fails later
void require_single_outputs(const QueryCall& q) {
    if (q.mode == QB_PREDICT) KN_REQUIRE(q.m >= 0 && (q.m == 0 || (q.pred_items && q.out_d)), KNNCF_E_INVALID, "bad prediction arguments");
    if (q.mode == QB_NEIGHBORS || recommends(q.mode))
        KN_REQUIRE(q.counts && q.width >= 0 && (q.width == 0 || (q.out_i && q.out_d)), KNNCF_E_INVALID,
                   q.mode == QB_NEIGHBORS ? "bad output arguments" : "bad arguments");
    if (recommends(q.mode)) *q.counts = 0;
}

// One query as a chunk of one: the query's status is the call's.  *count (neighbours: min(k, U), min(k, U - 1) for a user of
// the fit; recommendations: min(n, I - known items)) is written on success.
void do_query_single(knncf_handle* h, const QueryCall& call) {
    require_single_outputs(call);
    require_fitted(h, false);
    if (explains(call.mode)) {
        require_explain_order(call.ex);
        KN_REQUIRE(call.m >= 0 && (call.m == 0 || call.pred_items), KNNCF_E_INVALID, "bad prediction arguments");
        require_explain_outputs(call.ex, call.m);
    }
    if (call.mode == QB_RECOMMEND_EXPLAIN) {
        require_explain_order(call.ex);
        require_explain_outputs(call.ex, call.width);
    }
    if (call.family == QF_REVISE)
        KN_REQUIRE(call.n_removed >= 0 && (call.n_removed == 0 || call.removed_items), KNNCF_E_INVALID, "query: null removed items or n_removed < 0");
    require_single_ratings(call);
    require_query_support(h, call.predictor, call.mode);
    BatchOfOne one(call);
    int32_t c = 0; one.q.counts = &c;  // (the caller's *count is written on success only)
    const int64_t ex_rows = runs_explain(call) ? launch_rows(call, batch_budget(h)) : 0;  // (no hipMemGetInfo otherwise)
    report_failure(h, one.q, run_query_chunks(h, one.q, 1, ex_rows), true);
    if (call.counts) *call.counts = c;
}

int query_batch(knncf_handle* h, const QueryCall& q) { return guarded(h, [&] { do_query_batch(h, q, false); }); }
int query_single(knncf_handle* h, const QueryCall& q) { return guarded(h, [&] { do_query_single(h, q); }); }
// the bystander and entered single forms: their own arguments' checks (an entered call's *count is 0 once they pass), then the batch of one
int rows_single(knncf_handle* h, const QueryCall& call) {
    return guarded(h, [&] {
        require_fitted(h, false);
        if (call.mode == QB_ENTERED)
            KN_REQUIRE(call.counts && call.width >= 0 && (call.width == 0 || (call.out_i && call.out_d && call.out_pos && call.out_displaced && (call.family == QF_FOLD_IN || call.out_prev))),
                       KNNCF_E_INVALID, "bad output arguments");
        if (call.family == QF_REVISE)
            KN_REQUIRE(call.n_removed >= 0 && (call.n_removed == 0 || call.removed_items), KNNCF_E_INVALID, "query: null removed items or n_removed < 0");
        require_single_ratings(call);
        KN_REQUIRE(call.m >= 0, KNNCF_E_INVALID, "query: m < 0");
        if (call.mode == QB_ENTERED) *call.counts = 0;
        BatchOfOne one(call);
        do_query_batch(h, one.q, true);
    });
}

// ---- checkpoint / resume of the neighbour table ------------------------------------------------------
struct NbrFileHeader {
    char magic[8];  // "KNNCFNB2" (NB1: the fingerprint without the ratings; refused)
    int32_t U, kcap, k, similarity;
    int64_t n;
    uint64_t fingerprint;
    int64_t epoch;
};

// FNV-1a over what identifies "the same fit": raw user ids in dense order, row extents, user means, and what decides the
// similarities — every rating's raw item id and value in row order (user-major, items ascending).  (Without the last two a fit
// that moved a rating to another item of the same user, or swapped two of a user's ratings, passed for the same.)
uint64_t fit_fingerprint(knncf_handle* h) {
    Train& tr = h->tr;
    std::vector<int32_t> uid(tr.U), iid(tr.I), col((size_t)tr.n);
    std::vector<int64_t> ptr((size_t)tr.U + 1);
    std::vector<double> avg(tr.U), rating((size_t)tr.n);
    KN_HIP(hipMemcpyAsync(uid.data(), tr.uid.p, (size_t)tr.U * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    KN_HIP(hipMemcpyAsync(ptr.data(), tr.u_ptr.p, ((size_t)tr.U + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    KN_HIP(hipMemcpyAsync(avg.data(), tr.user_avg.p, (size_t)tr.U * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KN_HIP(hipMemcpyAsync(iid.data(), tr.iid.p, (size_t)tr.I * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    KN_HIP(hipMemcpyAsync(col.data(), tr.s_col.p, (size_t)tr.n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    KN_HIP(hipMemcpyAsync(rating.data(), tr.s_rating.p, (size_t)tr.n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KN_HIP(hipStreamSynchronize(h->stream));
    uint64_t x = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t bytes) {
        const unsigned char* c = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < bytes; ++i) { x ^= c[i]; x *= 1099511628211ull; }
    };
    mix(uid.data(), uid.size() * sizeof(int32_t));
    mix(ptr.data(), ptr.size() * sizeof(int64_t));
    mix(avg.data(), avg.size() * sizeof(double));
    for (size_t p = 0; p < col.size(); ++p) {
        const int32_t item = iid[col[p]];
        mix(&item, sizeof item);
        mix(&rating[p], sizeof(double));
    }
    return x;
}

void do_neighbors_save(knncf_handle* h, const char* path) {
    require_fitted(h);
    KN_REQUIRE(path, KNNCF_E_INVALID, "null path");
    KN_REQUIRE(h->cfg.shard_count == 1, KNNCF_E_UNSUPPORTED, "neighbour checkpoints are written by unsharded handles");
    Train& tr = h->tr;
    NeighborTable& nt = h->nt;
    NbrFileHeader hd{};
    memcpy(hd.magic, "KNNCFNB2", 8);
    hd.U = tr.U; hd.kcap = nt.kcap; hd.k = nt.k; hd.similarity = h->cfg.similarity; hd.n = tr.n;
    hd.fingerprint = fit_fingerprint(h);
    hd.epoch = h->epoch;
    const size_t cells = (size_t)tr.U * (size_t)std::max(nt.kcap, 1);
    std::vector<int32_t> cnt(tr.U), idx(cells);
    std::vector<int64_t> seq(tr.U);
    std::vector<double> sim(cells);
    KN_HIP(hipMemcpyAsync(cnt.data(), nt.cnt.p, cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    KN_HIP(hipMemcpyAsync(seq.data(), nt.seq.p, seq.size() * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    KN_HIP(hipMemcpyAsync(idx.data(), nt.idx.p, idx.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    KN_HIP(hipMemcpyAsync(sim.data(), nt.sim.p, sim.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KN_HIP(hipStreamSynchronize(h->stream));
    FILE* f = fopen(path, "wb");
    KN_REQUIRE(f, KNNCF_E_INVALID, std::string("cannot create ") + path);
    bool ok = fwrite(&hd, sizeof hd, 1, f) == 1 && fwrite(cnt.data(), sizeof(int32_t), cnt.size(), f) == cnt.size() &&
              fwrite(seq.data(), sizeof(int64_t), seq.size(), f) == seq.size() &&
              fwrite(idx.data(), sizeof(int32_t), idx.size(), f) == idx.size() &&
              fwrite(sim.data(), sizeof(double), sim.size(), f) == sim.size();
    ok = (fclose(f) == 0) && ok;
    KN_REQUIRE(ok, KNNCF_E_INVALID, std::string("short write to ") + path);
}

void do_neighbors_load(knncf_handle* h, const char* path) {
    require_fitted(h);
    KN_REQUIRE(path, KNNCF_E_INVALID, "null path");
    KN_REQUIRE(h->cfg.shard_count == 1, KNNCF_E_UNSUPPORTED, "neighbour checkpoints are read by unsharded handles");
    Train& tr = h->tr;
    NeighborTable& nt = h->nt;
    FILE* f = fopen(path, "rb");
    KN_REQUIRE(f, KNNCF_E_INVALID, std::string("cannot open ") + path);
    NbrFileHeader hd{};
    bool ok = fread(&hd, sizeof hd, 1, f) == 1 && memcmp(hd.magic, "KNNCFNB2", 8) == 0;
    if (!ok) {
        const bool v1 = memcmp(hd.magic, "KNNCFNB1", 8) == 0;
        fclose(f);
        throw Error(KNNCF_E_INVALID, std::string(path) + (v1 ? ": neighbour checkpoint of the older format (its fingerprint does not cover the ratings): rebuild it"
                                                               : ": not a neighbour checkpoint"));
    }
    if (hd.U != tr.U || hd.kcap != nt.kcap || hd.k != nt.k || hd.similarity != h->cfg.similarity || hd.n != tr.n ||
        hd.fingerprint != fit_fingerprint(h)) {
        fclose(f);
        throw Error(KNNCF_E_STATE, std::string(path) + ": checkpoint of a different fit (users, ratings, k or similarity differ)");
    }
    const size_t cells = (size_t)tr.U * (size_t)std::max(nt.kcap, 1);
    std::vector<int32_t> cnt(tr.U), idx(cells);
    std::vector<int64_t> seq(tr.U);
    std::vector<double> sim(cells);
    ok = fread(cnt.data(), sizeof(int32_t), cnt.size(), f) == cnt.size() && fread(seq.data(), sizeof(int64_t), seq.size(), f) == seq.size() &&
         fread(idx.data(), sizeof(int32_t), idx.size(), f) == idx.size() && fread(sim.data(), sizeof(double), sim.size(), f) == sim.size();
    fclose(f);
    KN_REQUIRE(ok, KNNCF_E_INVALID, std::string(path) + ": truncated checkpoint");
    hipStream_t st = h->stream;
    KN_HIP(hipMemcpyAsync(nt.cnt.p, cnt.data(), cnt.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    KN_HIP(hipMemcpyAsync(nt.seq.p, seq.data(), seq.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    KN_HIP(hipMemcpyAsync(nt.idx.p, idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    KN_HIP(hipMemcpyAsync(nt.sim.p, sim.data(), sim.size() * sizeof(double), hipMemcpyHostToDevice, st));
    nt.by_id_valid = false;
    KN_HIP(hipStreamSynchronize(st));
    h->epoch = std::max<int64_t>(hd.epoch, 1);
}

// ---- knncf_append: new ratings into the fit, the neighbour lists they cannot change kept (append.hip; DESIGN.md "Append") ----
// The rows are grouped per user in file order: a changer's rows are one update query.  Marking: the changers run through update
// chunks on the OLD fit, each chunk's report bitmaps (entered_update_flags: the users knncf_update_entered_batch would report,
// tail rows included) and its fitted changers are ORed into one stale mask on the device.  Then the new Train is built beside
// the old one from the concatenated rows; the lists of K = built and not stale are carried into the new numbering; the swap
// comes last, so a refusal on the way leaves the handle as it was.
// knncf_amend (DESIGN.md "Amend") is the same call with removals in front: the changers are the users of the removals too and run
// through REVISE chunks, and the new Train's first part is the old file order without the removed rows (amend_flag, which also
// decides whether every removal is a train row, and amend_compact).  knncf_append is the call without removals.
// knncf_remove_users (DESIGN.md "Remove users") is the call whose changers are users that leave.  Three things differ: the removal
// source is the list of users (amend_flag_users: no (user, item) table), the marking is one pass over the stored lists
// (append_holders: the lists that hold a leaver) and a user that leaves is no reason for a plain refit — the map gives it -1.
struct AppendRows {
    std::vector<int32_t> changers, items;
    std::vector<int64_t> offsets;
    std::vector<double> ratings;
    // the removals (knncf_amend; all empty without any): per changer beside its rows, and as the table amend_flag searches
    std::vector<int64_t> removed_offsets;  // [changers + 1] into removed
    std::vector<int32_t> removed;          // the removed items of each changer, in the given order
    std::vector<uint64_t> keys;            // [n_removed] (user << 32 | item, both as uint32), ascending
    std::vector<int64_t> given;            // keys[j] is removal given[j] of the call
    std::vector<uint32_t> removers;        // the distinct users of keys, ascending
    std::vector<int64_t> roff;             // [removers + 1] into keys
};
AppendRows group_append_rows(const int32_t* users, const int32_t* items, const double* ratings, int64_t n) {
    AppendRows g;
    std::vector<int32_t> slot_of((size_t)n);
    std::vector<std::pair<int32_t, int64_t>> by_user((size_t)n);  // (raw user, row): a stable order finds each user's rows
    for (int64_t j = 0; j < n; ++j) by_user[j] = {users[j], j};
    std::sort(by_user.begin(), by_user.end());
    // changers in the order of their first row
    std::vector<int64_t> first;  // first row of every distinct user, then sorted
    for (int64_t j = 0; j < n; ++j)
        if (j == 0 || by_user[j].first != by_user[j - 1].first) first.push_back(by_user[j].second);
    std::sort(first.begin(), first.end());
    std::vector<int64_t> count(first.size(), 0);
    for (int64_t j = 0, s = -1; j < n; ++j) {
        if (j == 0 || by_user[j].first != by_user[j - 1].first)
            s = std::lower_bound(first.begin(), first.end(), by_user[j].second) - first.begin();
        slot_of[by_user[j].second] = (int32_t)s;
        count[s] += 1;
    }
    g.offsets.assign(first.size() + 1, 0);
    for (size_t s = 0; s < first.size(); ++s) {
        g.changers.push_back(users[first[s]]);
        g.offsets[s + 1] = g.offsets[s] + count[s];
    }
    g.items.resize((size_t)n); g.ratings.resize((size_t)n);
    std::vector<int64_t> at(g.offsets.begin(), g.offsets.end() - 1);
    for (int64_t j = 0; j < n; ++j) {
        const int64_t p = at[slot_of[j]]++;
        g.items[p] = items[j];
        g.ratings[p] = ratings[j];
    }
    return g;
}

// the removals into g: users that only remove become changers behind those of the rows, in the order of their first removal.
// Throws a removal listed twice.
void group_removals(AppendRows& g, const int32_t* users, const int32_t* items, int64_t n) {
    std::vector<std::pair<uint64_t, int64_t>> table((size_t)n);
    for (int64_t j = 0; j < n; ++j) table[j] = {((uint64_t)(uint32_t)users[j] << 32) | (uint32_t)items[j], j};
    std::sort(table.begin(), table.end());
    g.roff.assign(1, 0);
    for (int64_t j = 0; j < n; ++j) {
        if (j > 0 && table[j].first == table[j - 1].first)
            throw Error(KNNCF_E_INVALID, "amend: removal " + std::to_string(table[j].second) + " (user " + std::to_string(users[table[j].second]) +
                                             ", item " + std::to_string(items[table[j].second]) + ") is listed twice");
        g.keys.push_back(table[j].first);
        g.given.push_back(table[j].second);
        const uint32_t user = (uint32_t)(table[j].first >> 32);
        if (g.removers.empty() || g.removers.back() != user) {
            g.removers.push_back(user);
            g.roff.push_back(j);
        }
        g.roff.back() = j + 1;
    }
    std::map<int32_t, int32_t> slot_of;  // a changer's slot by its raw id
    for (size_t s = 0; s < g.changers.size(); ++s) slot_of[g.changers[s]] = (int32_t)s;
    std::vector<int32_t> slot((size_t)n);
    for (int64_t j = 0; j < n; ++j) {
        const auto [at, fresh] = slot_of.try_emplace(users[j], (int32_t)g.changers.size());
        if (fresh) {
            g.changers.push_back(users[j]);
            g.offsets.push_back(g.offsets.back());  // (no rows)
        }
        slot[j] = at->second;
    }
    g.removed_offsets.assign(g.changers.size() + 1, 0);
    for (int64_t j = 0; j < n; ++j) g.removed_offsets[slot[j] + 1] += 1;
    for (size_t s = 0; s < g.changers.size(); ++s) g.removed_offsets[s + 1] += g.removed_offsets[s];
    g.removed.resize((size_t)n);
    std::vector<int64_t> at(g.removed_offsets.begin(), g.removed_offsets.end() - 1);
    for (int64_t j = 0; j < n; ++j) g.removed[at[slot[j]]++] = items[j];
}

// the marking; false: a changer's update query — its revise query when the call has removals — is KNNCF_E_UNSUPPORTED (the plain
// refit).  Throws a duplicate or a non-finite deviation as the call's status.
bool mark_stale_lists(knncf_handle* h, const AppendRows& g) {
    const int64_t B = (int64_t)g.changers.size();
    std::vector<int32_t> statuses((size_t)B, KNNCF_OK);
    QueryCall q{};
    q.family = g.removed.empty() ? QF_UPDATE : QF_REVISE; q.mode = QB_ENTERED; q.predictor = KNNCF_PRED_KNN;
    q.users = g.changers.data(); q.B = B; q.offsets = g.offsets.data(); q.items = g.items.data(); q.ratings = g.ratings.data();
    if (q.family == QF_REVISE) { q.removed_offsets = g.removed_offsets.data(); q.removed_items = g.removed.data(); }
    q.statuses = statuses.data();
    ChunkState cs;
    cs.take = std::max(0, std::min(h->cfg.k, h->tr.U));
    const int64_t chunk = query_batch_chunk(h, batch_budget(h));
    load_host_ids(h);
    for (int64_t c0 = 0; c0 < B; c0 += chunk) {
        const int64_t c1 = std::min(B, c0 + chunk);
        const bool all = pack_chunk(h, q, cs, c0, c1) == c1 - c0 && settle_chunk(h, q, cs, nullptr) == (size_t)cs.C;
        if (!all) {
            for (const int status : {KNNCF_E_DUPLICATE, KNNCF_E_NONFINITE})  // (the fit's order of precedence)
                for (int64_t b = c0; b < c1; ++b)
                    if (statuses[b] == status)
                        throw Error(status, "append: user " + std::to_string(g.changers[b]) +
                                                (status == KNNCF_E_DUPLICATE ? ": a row repeats a (user, item) of train or of the rows"
                                                                             : ": scale() == 0 gives a non-finite deviation"));
            return false;
        }
        cs.qrank.resize((size_t)cs.C);
        for (int32_t s = 0; s < cs.C; ++s) {
            const uint32_t qkey = int_trie_key(cs.s_users[s]);
            cs.qrank[s] = (int32_t)(std::lower_bound(h->h_ukeys.begin(), h->h_ukeys.end(), qkey) - h->h_ukeys.begin());
        }
        const unsigned long long* bits = entered_update_flags(h->tr, h->nt, h->query_batch, cs.C, cs.take, cs.qo.data(), cs.s_self.data(),
                                                              cs.qrank.data(), h->stream);
        append_mark(h->append, h->tr.U, cs.C, bits, h->query_batch.self.p, h->stream);
    }
    return true;
}

// the leavers of knncf_remove_users as the stages want them: raw ids as uint32 ascending (amend_flag_users), their dense users on
// the old fit, the train rows they take with them.  Throws an id that is no user of train and an id listed twice.
struct Leavers {
    std::vector<uint32_t> raw;
    std::vector<int32_t> dense;
    int64_t rows = 0;
};
Leavers look_up_leavers(knncf_handle* h, const int32_t* users, int64_t n_users) {
    Leavers lv;
    load_host_ids(h);
    std::vector<std::pair<uint32_t, int64_t>> by_id((size_t)n_users);
    for (int64_t j = 0; j < n_users; ++j) by_id[j] = {(uint32_t)users[j], j};
    std::sort(by_id.begin(), by_id.end());
    for (int64_t j = 0; j < n_users; ++j) {
        const int32_t raw = users[by_id[j].second];
        const int32_t du = dense_lookup(h->h_ukeys.data(), h->tr.U, raw);
        KN_REQUIRE(du >= 0, KNNCF_E_INVALID, "remove_users: user " + std::to_string(raw) + " is no user of the training set");
        KN_REQUIRE(j == 0 || by_id[j].first != by_id[j - 1].first, KNNCF_E_INVALID,
                   "remove_users: user " + std::to_string(raw) + " is listed twice");
        lv.raw.push_back(by_id[j].first);
        lv.dense.push_back(du);
        lv.rows += train_row_length(h, du);
    }
    return lv;
}

// leavers / n_leavers: knncf_remove_users (then the call has neither removals nor rows)
void do_amend(knncf_handle* h, const int32_t* removed_users, const int32_t* removed_items, int64_t n_removed, const int32_t* users,
              const int32_t* items, const double* ratings, int64_t n, int64_t* n_carried, int64_t* n_dropped, int32_t* dropped,
              int64_t dropped_cap, const int32_t* leavers = nullptr, int64_t n_leavers = 0) {
    require_fitted(h, false);
    KN_REQUIRE(h->cfg.shard_count == 1, KNNCF_E_UNSUPPORTED, "append: single-shard handles only");
    KN_REQUIRE(n >= 0 && n_removed >= 0 && n_carried && n_dropped && dropped_cap >= 0 && (dropped_cap == 0 || dropped) &&
                   (n == 0 || (users && items && ratings)) && (n_removed == 0 || (removed_users && removed_items)),
               KNNCF_E_INVALID, "append: null argument, n < 0, n_removed < 0 or dropped_cap < 0");
    KN_REQUIRE(n_leavers >= 0 && (n_leavers == 0 || leavers), KNNCF_E_INVALID, "remove_users: null users or n_users < 0");
    const bool whole_users = n_leavers > 0;
    Train& tr = h->tr;
    NeighborTable& nt = h->nt;
    AppendScratch& as = h->append;
    hipStream_t st = h->stream;
    const int32_t U = tr.U;
    h->prep.join_commit(st);
    append_begin(as, U, st);
    int64_t totals[5] = {0, 0, 0, 0, 0};  // (|K|, |B ∩ S|; [4], fetched for knncf_remove_users only: the leavers in B ∩ S)
    auto fetch_totals = [&] {
        KN_HIP(hipMemcpyAsync(totals, as.totals.p, (whole_users ? 5 : 2) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        KN_HIP(hipStreamSynchronize(st));
    };
    if (n == 0 && n_removed == 0 && !whole_users) {  // touches nothing: |B| from the build numbers
        append_sets(as, tr, nt, false, 0, st);
        fetch_totals();
        *n_carried = totals[0];
        *n_dropped = 0;
        return;
    }
    AppendRows g = group_append_rows(users, items, ratings, n);
    // ---- the removals: which file rows go, and whether every removal is a train row
    int64_t kept_rows = tr.n;
    if (n_removed > 0) {
        group_removals(g, removed_users, removed_items, n_removed);
        int64_t verdict[2] = {0, 0};
        {
            Stage s(h, &h->tm.prep_ms);
            amend_flag(as, tr, g.keys.data(), n_removed, g.removers.data(), g.roff.data(), (int32_t)g.removers.size(), st);
        }
        KN_HIP(hipMemcpyAsync(verdict, as.totals.p + 2, sizeof verdict, hipMemcpyDeviceToHost, st));
        KN_HIP(hipStreamSynchronize(st));
        if (verdict[1] >= 0) {
            const int64_t j = g.given[(size_t)verdict[1]];
            throw Error(KNNCF_E_INVALID, "amend: removal " + std::to_string(j) + " (user " + std::to_string(removed_users[j]) + ", item " +
                                             std::to_string(removed_items[j]) + ") is not a row of the training set");
        }
        kept_rows = verdict[0];
        KN_REQUIRE(kept_rows == tr.n - n_removed, KNNCF_E_STATE, "amend: the surviving rows are not the train rows without the removals");
        KN_REQUIRE(kept_rows + n > 0, KNNCF_E_INVALID, "amend: the removals leave the training set without a row");
    }
    // ---- the users that leave: which file rows go; the host knows their number from the row lengths
    Leavers lv;
    if (whole_users) {
        lv = look_up_leavers(h, leavers, n_leavers);
        KN_REQUIRE(lv.rows < tr.n, KNNCF_E_INVALID, "remove_users: the users leave the training set without a row");
        int64_t verdict[2] = {0, 0};
        {
            Stage s(h, &h->tm.prep_ms);
            amend_flag_users(as, tr, lv.raw.data(), (int32_t)n_leavers, st);
        }
        KN_HIP(hipMemcpyAsync(verdict, as.totals.p + 2, sizeof verdict, hipMemcpyDeviceToHost, st));
        KN_HIP(hipStreamSynchronize(st));
        kept_rows = verdict[0];
        KN_REQUIRE(kept_rows == tr.n - lv.rows, KNNCF_E_STATE, "remove_users: the surviving rows are not the train rows without the users' rows");
    }
    KN_REQUIRE(kept_rows + n < ((int64_t)1 << 29), KNNCF_E_UNSUPPORTED, "append: more than 2^29-1 ratings");
    const int64_t n_changers = whole_users ? n_leavers : (int64_t)g.changers.size();
    // ---- the plain refits that the rows alone decide
    load_host_ids(h);
    int32_t joined = 0, left = (int32_t)n_leavers;
    int64_t removers = 0;
    bool short_changer = false;  // a newcomer of <= 4 rows, or a fitted changer that its removals leave that few
    for (int64_t b = 0; b < (int64_t)g.changers.size(); ++b) {  // (none for leavers: they are no rows of g)
        const int32_t du = dense_lookup(h->h_ukeys.data(), U, g.changers[b]);
        const int64_t nr = n_removed > 0 ? g.removed_offsets[b + 1] - g.removed_offsets[b] : 0;
        // (its rows on aug; a fitted changer without removals keeps its train rows, which nothing below asks for)
        const int64_t rows = g.offsets[b + 1] - g.offsets[b] - nr + (du >= 0 && nr > 0 ? train_row_length(h, du) : 0);
        removers += nr > 0;
        joined += du < 0;
        left += du >= 0 && nr > 0 && rows == 0;
        short_changer |= (du < 0 || nr > 0) && rows <= 4;
    }
    // (KNNCF_DEBUG_APPEND_MAX_CHANGERS: measurement hook of scripts/append_latency.py, which locates the crossover behind the
    // constant — another limit, 0 = every append is a plain refit)
    const char* limit = getenv("KNNCF_DEBUG_APPEND_MAX_CHANGERS");
    const int64_t max_changers = limit ? atoll(limit) : KNNCF_APPEND_MAX_CHANGERS;
    const int32_t new_kcap = std::max(0, std::min(h->cfg.k, U + joined - left - 1));
    const bool no_lists = h->cfg.similarity == KNNCF_SIM_ONE || nt.kcap <= 0 || h->epoch == 1;  // (no call has built one since the fit)
    bool plain = h->cfg.similarity == KNNCF_SIM_ONE || new_kcap != nt.kcap || nt.k != h->cfg.k ||
                 n_changers > max_changers ||
                 (left > 0 && !whole_users) ||  // (a leaver among other changers: its holders are not marked)
                 (whole_users && U - left < 5) ||
                 // (the update queries refuse such a fit: the id sets change their iteration class below five members)
                 U < 5 || tr.I < 5 ||
                 (h->cfg.similarity == KNNCF_SIM_COSINE && (short_changer || has_short_rows(h)));
    // ---- marking, on the old fit
    const bool lds_bitmap = lds_bitmap_fits(ceil_div(U, 64));  // (of append_holders)
    if (whole_users) append_leavers(as, U, lv.dense.data(), (int32_t)n_leavers, st);
    if (!plain && !no_lists) {
        if (whole_users) append_holders(as, tr, nt, lds_bitmap, st);
        else plain = !mark_stale_lists(h, g);
    }
    // ---- the new Train beside the old one
    Train next;
    next.n = kept_rows + n;
    next.jaccard = tr.jaccard;
    {
        Stage s(h, &h->tm.prep_ms);
        next.user_raw.alloc(next.n); next.item_raw.alloc(next.n); next.rating.alloc(next.n);
        if (n_removed > 0 || whole_users) {
            amend_compact(as, tr, next.user_raw.p, next.item_raw.p, next.rating.p, st);
        } else {
            KN_HIP(hipMemcpyAsync(next.user_raw.p, tr.user_raw.p, tr.n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
            KN_HIP(hipMemcpyAsync(next.item_raw.p, tr.item_raw.p, tr.n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
            KN_HIP(hipMemcpyAsync(next.rating.p, tr.rating.p, tr.n * sizeof(double), hipMemcpyDeviceToDevice, st));
        }
        if (n > 0) {
            KN_HIP(hipMemcpyAsync(next.user_raw.p + kept_rows, users, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
            KN_HIP(hipMemcpyAsync(next.item_raw.p + kept_rows, items, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
            KN_HIP(hipMemcpyAsync(next.rating.p + kept_rows, ratings, n * sizeof(double), hipMemcpyHostToDevice, st));
        }
        prep_fit(next, h->prep, h->cfg.shard_rank, h->cfg.shard_count, st);  // (throws a duplicate or a non-finite deviation)
        prep_commit(next, h->prep, st);
    }
    KN_REQUIRE(next.U == U + joined - left, KNNCF_E_STATE, "append: the new fit's users are not the old ones, the newcomers and the leavers");
    // ---- K, B ∩ S, the dropped ids (old dense order = new set order: the map is monotone)
    // (the user set changed its iteration class, upwards or — users left — downwards: every id is fetched and ordered on the host)
    const bool tiny = (U < 5) != (next.U < 5);
    if (whole_users && next.I < 5) plain = true;  // (the leavers took items with them: the item set changed its iteration class)
    append_sets(as, tr, nt, plain, tiny ? U : dropped_cap, st);
    if (whole_users) append_leavers_gone(as, (int32_t)n_leavers, st);
    const bool moved = !plain && next.U != U;
    NeighborTable table;
    if (!plain) {
        Stage s(h, &h->tm.prep_ms);
        if (moved) {
            const size_t cells = (size_t)next.U * (size_t)std::max(nt.kcap, 1);
            table.idx.alloc(cells); table.sim.alloc(cells); table.cnt.alloc(next.U); table.seq.alloc(next.U);
            KN_HIP(hipMemsetAsync(table.cnt.p, 0, next.U * sizeof(int32_t), st));
            KN_HIP(hipMemsetAsync(table.seq.p, 0xff, next.U * sizeof(int64_t), st));  // -1
            append_remap(as, tr, next.ukeys.p, next.U, st);
            append_number(as, h->prep.sort, tr, as.map.p, table.seq.p, st);
            append_carry(as, U, nt, table, st);
        } else {
            append_clear(as, U, nt.cnt.p, nt.seq.p, st);
            append_number(as, h->prep.sort, tr, nullptr, nt.seq.p, st);
        }
    }
    fetch_totals();
    const int64_t built = totals[0] + totals[1];
    std::vector<int32_t> ids((size_t)std::min<int64_t>(totals[1], tiny ? U : dropped_cap));
    if (!ids.empty()) {
        KN_HIP(hipMemcpyAsync(ids.data(), as.dropped.p, ids.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        KN_HIP(hipStreamSynchronize(st));
        if (tiny && next.U >= 5) {
            std::sort(ids.begin(), ids.end(), [](int32_t a, int32_t b) { return int_trie_key(a) < int_trie_key(b); });
        } else if (tiny) {  // the new fit's few users in their order, then the users that left
            std::vector<int32_t> order((size_t)next.U);
            KN_HIP(hipMemcpyAsync(order.data(), next.uid.p, order.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            KN_HIP(hipStreamSynchronize(st));
            auto place = [&](int32_t id) { return std::find(order.begin(), order.end(), id) - order.begin(); };
            std::stable_sort(ids.begin(), ids.end(), [&](int32_t a, int32_t b) { return place(a) < place(b); });
        }
        if (tiny) ids.resize((size_t)std::min<int64_t>((int64_t)ids.size(), dropped_cap));
        std::copy(ids.begin(), ids.end(), dropped);
    }
    // ---- the swap
    h->tr = std::move(next);
    drop_fit_caches(h);
    if (plain) {
        reset_neighbors(h);
    } else {
        if (moved) {
            nt.idx = std::move(table.idx); nt.sim = std::move(table.sim); nt.cnt = std::move(table.cnt); nt.seq = std::move(table.seq);
        }
        nt.by_id_valid = false;
        h->epoch = totals[0] > 0 ? 2 : 1;
    }
    *n_carried = totals[0];
    *n_dropped = totals[1];
    KN_TRACE_DISPATCH("append changers=%lld built=%lld carried=%lld dropped=%lld moved=%d plain=%d", (long long)n_changers,
                      (long long)built, (long long)totals[0], (long long)totals[1], (int)moved, (int)plain);
    if (n_removed > 0)
        KN_TRACE_DISPATCH("amend removers=%lld removed=%lld kept_rows=%lld", (long long)removers, (long long)n_removed, (long long)kept_rows);
    if (whole_users)
        KN_TRACE_DISPATCH("remove users=%lld removed=%lld kept_rows=%lld holders=%lld bitmap=%s", (long long)n_leavers, (long long)lv.rows,
                          (long long)kept_rows, (long long)(totals[1] - totals[4]), lds_bitmap ? "lds" : "global");
}

}  // namespace

extern "C" {

const char* knncf_version(void) { return "knncf 0.1 (gfx950)"; }

const char* knncf_status_string(int st) {
    switch (st) {
        case KNNCF_OK: return "ok";
        case KNNCF_E_INVALID: return "invalid argument";
        case KNNCF_E_NONFINITE: return "non-finite normalized deviation";
        case KNNCF_E_DUPLICATE: return "duplicate (user,item) rating";
        case KNNCF_E_NOMEM: return "out of memory";
        case KNNCF_E_HIP: return "HIP runtime error";
        case KNNCF_E_STATE: return "invalid call order";
        case KNNCF_E_UNSUPPORTED: return "unsupported configuration";
        case KNNCF_E_NODEVICE: return "no usable gfx950 device";
        case KNNCF_E_RCCL: return "RCCL error";
        default: return "unknown status";
    }
}

int knncf_create(const knncf_config* cfg, knncf_handle** out) {
    if (!cfg || !out || cfg->struct_size != sizeof(knncf_config)) return KNNCF_E_INVALID;
    if (cfg->shard_count < 1 || cfg->shard_rank < 0 || cfg->shard_rank >= cfg->shard_count || cfg->k < 0)
        return KNNCF_E_INVALID;
    if (cfg->similarity < KNNCF_SIM_COSINE || cfg->similarity > KNNCF_SIM_JACCARD) return KNNCF_E_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) {
        (void)hipGetLastError();
        return KNNCF_E_NODEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return KNNCF_E_NODEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return KNNCF_E_NODEVICE;  // CDNA4 code objects only
    knncf_handle* h = new (std::nothrow) knncf_handle();
    if (!h) return KNNCF_E_NOMEM;
    h->cfg = *cfg;
    if (hipSetDevice(cfg->device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return KNNCF_E_HIP;
    }
    bool ok = hipEventCreateWithFlags(&h->ev_ready, hipEventDisableTiming) == hipSuccess;
    for (int s = 0; s < 2; ++s) {
        ok = ok && hipEventCreateWithFlags(&h->ev_produced[s], hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&h->ev_consumed[s], hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) {
        knncf_destroy(h);
        return KNNCF_E_HIP;
    }
    *out = h;
    return KNNCF_OK;
}

void knncf_destroy(knncf_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    (void)hipStreamSynchronize(h->stream);
    for (auto& t : h->pending) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
    for (auto e : h->event_pool) (void)hipEventDestroy(e);
    if (h->stream2) (void)hipStreamSynchronize(h->stream2);
    if (h->ev_ready) (void)hipEventDestroy(h->ev_ready);
    for (int s = 0; s < 2; ++s) {
        if (h->ev_produced[s]) (void)hipEventDestroy(h->ev_produced[s]);
        if (h->ev_consumed[s]) (void)hipEventDestroy(h->ev_consumed[s]);
    }
    if (h->pinned_cnt) (void)hipHostFree(h->pinned_cnt);
    if (h->stream2) (void)hipStreamDestroy(h->stream2);
    (void)hipStreamDestroy(h->stream);
    delete h;
}

const char* knncf_last_error(const knncf_handle* h) { return h ? h->err.c_str() : "null handle"; }

int knncf_fit_device(knncf_handle* h, const int32_t* d_users, const int32_t* d_items, const double* d_ratings, int64_t n) {
    return guarded(h, [&] { do_fit_device(h, d_users, d_items, d_ratings, n); });
}

int knncf_fit(knncf_handle* h, const int32_t* users, const int32_t* items, const double* ratings, int64_t n) {
    return guarded(h, [&] {
        KN_REQUIRE(n > 0 && users && items && ratings, KNNCF_E_INVALID, "fit: null or empty input");
        Train& tr = h->tr;
        tr.user_raw.alloc(n); tr.item_raw.alloc(n); tr.rating.alloc(n);
        KN_HIP(hipMemcpyAsync(tr.user_raw.p, users, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        KN_HIP(hipMemcpyAsync(tr.item_raw.p, items, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        KN_HIP(hipMemcpyAsync(tr.rating.p, ratings, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
        do_fit_device(h, tr.user_raw.p, tr.item_raw.p, tr.rating.p, n);
    });
}

int knncf_num_users(const knncf_handle* h, int32_t* out) {
    if (!h || !out || !h->fitted) return KNNCF_E_STATE;
    *out = h->tr.U;
    return KNNCF_OK;
}
int knncf_num_items(const knncf_handle* h, int32_t* out) {
    if (!h || !out || !h->fitted) return KNNCF_E_STATE;
    *out = h->tr.I;
    return KNNCF_OK;
}

int knncf_global_avg(knncf_handle* h, double* out) {
    return guarded(h, [&] {
        require_fitted(h, false);
        KN_REQUIRE(out, KNNCF_E_INVALID, "null out");
        *out = h->tr.global_avg;
    });
}

int knncf_user_avg(knncf_handle* h, int32_t user, double* out) {
    return guarded(h, [&] {
        require_fitted(h);
        KN_REQUIRE(out, KNNCF_E_INVALID, "null out");
        int32_t d = dense_user(h, user);
        *out = d >= 0 ? fetch(h, h->tr.user_avg.p, d) : h->tr.global_avg;
    });
}

int knncf_item_avg(knncf_handle* h, int32_t item, double* out) {
    return guarded(h, [&] {
        require_fitted(h);
        KN_REQUIRE(out, KNNCF_E_INVALID, "null out");
        ensure_item_stats(h);
        int32_t d = dense_item(h, item);
        *out = d >= 0 ? fetch(h, h->tr.item_avg.p, d) : h->tr.global_avg;
    });
}

int knncf_item_avg_dev(knncf_handle* h, int32_t item, double* out) {
    return guarded(h, [&] {
        require_fitted(h);
        KN_REQUIRE(out, KNNCF_E_INVALID, "null out");
        ensure_item_stats(h);
        int32_t d = dense_item(h, item);
        *out = d >= 0 ? fetch(h, h->tr.item_dev_hash.p, d) : 0.0;
    });
}

int knncf_item_avg_dev_rdd(knncf_handle* h, int32_t item, double* out) {
    return guarded(h, [&] {
        require_fitted(h);
        KN_REQUIRE(out, KNNCF_E_INVALID, "null out");
        ensure_item_stats(h);
        int32_t d = dense_item(h, item);
        *out = d >= 0 ? fetch(h, h->tr.item_dev_file.p, d) : 0.0;
    });
}

int knncf_similarity(knncf_handle* h, int32_t u, int32_t v, double* out) {
    return guarded(h, [&] {
        require_fitted(h);
        KN_REQUIRE(out, KNNCF_E_INVALID, "null out");
        if (h->cfg.similarity == KNNCF_SIM_ONE) { *out = 1.0; return; }
        int32_t du = dense_user(h, u), dv = dense_user(h, v);
        h->scalar_out.ensure(1);
        if (h->cfg.similarity == KNNCF_SIM_JACCARD) {
            launch_jaccard_pair(h->tr, du, dv, h->scalar_out.p, h->stream);
        } else {
            if (du < 0 || dv < 0) { *out = 0.0; return; }
            launch_exact_pair(h->tr, du, dv, h->scalar_out.p, h->stream);
        }
        *out = fetch(h, h->scalar_out.p, 0);
    });
}

static void neighbors_of(knncf_handle* h, int32_t du, std::vector<int32_t>& ids, std::vector<double>& sims) {
    NeighborTable& nt = h->nt;
    Train& tr = h->tr;
    ids.clear(); sims.clear();
    if (tr.U < 2 || nt.kcap <= 0) return;
    int64_t seq = fetch(h, nt.seq.p, du);
    if (seq < 0) {
        require_shard_numbering(h);
        h->build_list.ensure(tr.U);
        int64_t new_seq = h->epoch << 32;
        h->epoch += 1;
        KN_HIP(hipMemcpyAsync(nt.seq.p + du, &new_seq, sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
        KN_HIP(hipMemcpyAsync(h->build_list.p, &du, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        KN_HIP(hipStreamSynchronize(h->stream));
        build_neighbors(h, 1);
    }
    int32_t cnt = fetch(h, nt.cnt.p, du);
    ids.resize(cnt); sims.resize(cnt);
    if (cnt > 0) {
        KN_HIP(hipMemcpyAsync(ids.data(), nt.idx.p + (int64_t)du * nt.kcap, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        KN_HIP(hipMemcpyAsync(sims.data(), nt.sim.p + (int64_t)du * nt.kcap, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        KN_HIP(hipStreamSynchronize(h->stream));
    }
}

int knncf_neighbors(knncf_handle* h, int32_t u, int32_t cap, int32_t* ids, double* sims, int32_t* count) {
    return guarded(h, [&] {
        require_fitted(h);
        KN_REQUIRE(count && cap >= 0 && (cap == 0 || (ids && sims)), KNNCF_E_INVALID, "bad output arguments");
        KN_REQUIRE(h->cfg.similarity != KNNCF_SIM_ONE, KNNCF_E_UNSUPPORTED, "neighbourhoods: adjusted cosine or Jaccard");
        int32_t du = dense_user(h, u);
        load_host_ids(h);
        if (du < 0) {  // user absent from train: every similarity is 0.0, ties keep Set order (N3)
            int32_t c = std::min(h->nt.k, h->tr.U);
            for (int32_t j = 0; j < c && j < cap; ++j) { ids[j] = h->h_uid[j]; sims[j] = 0.0; }
            *count = c;
            return;
        }
        KN_REQUIRE(du >= h->tr.own_lo && du < h->tr.own_hi, KNNCF_E_INVALID, "user belongs to another shard");
        std::vector<int32_t> di;
        std::vector<double> ds;
        neighbors_of(h, du, di, ds);
        for (size_t j = 0; j < di.size() && (int32_t)j < cap; ++j) { ids[j] = h->h_uid[di[j]]; sims[j] = ds[j]; }
        *count = (int32_t)di.size();
    });
}

// the neighbourhoods of the dense users du[0 .. n) (-1: absent from train) that do not exist yet, built in ONE batch and
// numbered (call epoch, position in du): the memo history of calls for du[0], du[1], ... in this order
static void build_missing_neighbors(knncf_handle* h, const std::vector<int32_t>& du) {
    Train& tr = h->tr;
    NeighborTable& nt = h->nt;
    hipStream_t st = h->stream;
    if (tr.U < 2 || nt.kcap <= 0) return;
    const int64_t n = (int64_t)du.size();
    std::vector<int64_t> seq((size_t)tr.U);
    KN_HIP(hipMemcpyAsync(seq.data(), nt.seq.p, seq.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    KN_HIP(hipStreamSynchronize(st));
    std::vector<int32_t> fresh;
    for (int64_t j = 0; j < n; ++j)
        if (du[j] >= 0 && seq[du[j]] < 0) {
            seq[du[j]] = (h->epoch << 32) | (int64_t)std::min<int64_t>(j, 0xffffffffll);
            fresh.push_back(du[j]);
        }
    if (fresh.empty()) return;
    require_shard_numbering(h);
    h->epoch += 1;
    h->build_list.ensure(tr.U);
    KN_HIP(hipMemcpyAsync(nt.seq.p, seq.data(), seq.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    KN_HIP(hipMemcpyAsync(h->build_list.p, fresh.data(), fresh.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    KN_HIP(hipStreamSynchronize(st));
    build_neighbors(h, (int32_t)fresh.size());
}

// getNeighbors(train, k, sim) for many users: the missing neighbourhoods are built in ONE batch (memo history: as if the
// closure had been called for users[0], users[1], ... in this order), then the lists are copied out
static void do_neighbors_batch(knncf_handle* h, const int32_t* users, int64_t n, int32_t cap, int32_t* ids, double* sims, int32_t* counts) {
    require_fitted(h);
    KN_REQUIRE(n >= 0 && cap >= 0 && (n == 0 || (users && counts)) && (n == 0 || cap == 0 || (ids && sims)), KNNCF_E_INVALID, "bad arguments");
    KN_REQUIRE(h->cfg.similarity != KNNCF_SIM_ONE, KNNCF_E_UNSUPPORTED, "neighbourhoods: adjusted cosine or Jaccard");
    if (n == 0) return;
    Train& tr = h->tr;
    NeighborTable& nt = h->nt;
    hipStream_t st = h->stream;
    load_host_ids(h);
    std::vector<int32_t> du((size_t)n);
    for (int64_t j = 0; j < n; ++j) {
        du[j] = dense_lookup(h->h_ukeys.data(), tr.U, users[j]);
        KN_REQUIRE(du[j] < 0 || (du[j] >= tr.own_lo && du[j] < tr.own_hi), KNNCF_E_INVALID, "user belongs to another shard");
    }
    const bool have_lists = tr.U >= 2 && nt.kcap > 0;
    build_missing_neighbors(h, du);
    const size_t kc = (size_t)std::max(nt.kcap, 1);
    std::vector<int32_t> h_cnt, h_idx;
    std::vector<double> h_sim;
    const bool whole = have_lists && n > 1024;  // one big copy instead of 2 n small ones
    if (have_lists) {
        h_cnt.resize(tr.U);
        KN_HIP(hipMemcpyAsync(h_cnt.data(), nt.cnt.p, h_cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (whole) {
            h_idx.resize((size_t)tr.U * kc);
            h_sim.resize((size_t)tr.U * kc);
            KN_HIP(hipMemcpyAsync(h_idx.data(), nt.idx.p, h_idx.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            KN_HIP(hipMemcpyAsync(h_sim.data(), nt.sim.p, h_sim.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        KN_HIP(hipStreamSynchronize(st));
    }
    std::vector<int32_t> row_idx(kc);
    std::vector<double> row_sim(kc);
    for (int64_t j = 0; j < n; ++j) {
        int32_t* oi = ids + (size_t)j * cap;
        double* os = sims + (size_t)j * cap;
        if (du[j] < 0) {  // user absent from train: every similarity is 0.0, ties keep Set order (N3)
            const int32_t c = std::min(nt.k, tr.U);
            for (int32_t q = 0; q < c && q < cap; ++q) { oi[q] = h->h_uid[q]; os[q] = 0.0; }
            counts[j] = c;
            continue;
        }
        const int32_t c = have_lists ? h_cnt[du[j]] : 0;
        const int32_t* src_i = nullptr;
        const double* src_s = nullptr;
        if (whole) {
            src_i = h_idx.data() + (size_t)du[j] * kc;
            src_s = h_sim.data() + (size_t)du[j] * kc;
        } else if (c > 0) {
            KN_HIP(hipMemcpyAsync(row_idx.data(), nt.idx.p + (size_t)du[j] * kc, c * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            KN_HIP(hipMemcpyAsync(row_sim.data(), nt.sim.p + (size_t)du[j] * kc, c * sizeof(double), hipMemcpyDeviceToHost, st));
            KN_HIP(hipStreamSynchronize(st));
            src_i = row_idx.data();
            src_s = row_sim.data();
        }
        for (int32_t q = 0; q < c && q < cap; ++q) { oi[q] = h->h_uid[src_i[q]]; os[q] = src_s[q]; }
        counts[j] = c;
    }
}

int knncf_neighbors_batch(knncf_handle* h, const int32_t* users, int64_t n, int32_t cap, int32_t* ids, double* sims, int32_t* counts) {
    return guarded(h, [&] { do_neighbors_batch(h, users, n, cap, ids, sims, counts); });
}

// entered queries (knncf.h "Entered queries"): the place rule reads the handle's stored lists, so the call first builds the lists
// that are missing: M = the train users without one in ascending raw id, in ONE batch numbered (call, position in M) — the state
// knncf_neighbors_batch over M leaves.
static void build_unbuilt_neighbors(knncf_handle* h) {
    Train& tr = h->tr;
    if (tr.U < 2 || h->nt.kcap <= 0) return;
    load_host_ids(h);
    std::vector<int64_t> seq((size_t)tr.U);
    KN_HIP(hipMemcpyAsync(seq.data(), h->nt.seq.p, seq.size() * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    KN_HIP(hipStreamSynchronize(h->stream));
    std::vector<int32_t> M;
    for (int32_t u = 0; u < tr.U; ++u)
        if (seq[u] < 0) M.push_back(u);
    if (M.empty()) return;
    std::sort(M.begin(), M.end(), [&](int32_t a, int32_t b) { return h->h_uid[a] < h->h_uid[b]; });
    build_missing_neighbors(h, M);
}

// users per chunk of knncf_recommend_batch: the rule of knncf.h ("Batched recommendations")
static int64_t recommend_batch_chunk(knncf_handle* h) {
    int64_t C = std::min<int64_t>(RB_MAX_CHUNK, batch_budget(h) / reco_batch_bytes(h->tr.I));
    C = std::min<int64_t>(C, (int64_t)0x7fffffff / h->tr.I);  // slot * I + item is a 31-bit cell
    return std::max<int64_t>(C, 1);
}

// recommendations(train, predictor)(users[b], n) shared/predictions.scala:651-674 for b = 0 .. n_users-1, as if asked in this
// order; knncf_recommend is the call over one user.  The missing neighbourhoods are built in one batch (build_missing_neighbors,
// as knncf_neighbors_batch numbers them), then chunks of users go through reco_batch.hip
static void do_recommend_batch(knncf_handle* h, int predictor, const int32_t* users, int64_t B, int32_t n, int32_t* out_items,
                               double* out_preds, int32_t* counts) {
    require_fitted(h);
    KN_REQUIRE(B >= 0 && n >= 0, KNNCF_E_INVALID, "recommend batch: n_users or n < 0");
    if (B == 0) return;
    KN_REQUIRE(users && counts && (n == 0 || (out_items && out_preds)), KNNCF_E_INVALID, "recommend batch: null argument");
    if (n == 0) {
        std::fill(counts, counts + B, 0);
        return;
    }
    KN_REQUIRE(predictor >= KNNCF_PRED_GLOBAL_AVG && predictor <= KNNCF_PRED_PERSONALIZED, KNNCF_E_INVALID, "unknown predictor");
    Train& tr = h->tr;
    NeighborTable& nt = h->nt;
    hipStream_t st = h->stream;
    const int32_t I = tr.I;
    load_host_ids(h);
    std::vector<int32_t> du((size_t)B);
    for (int64_t b = 0; b < B; ++b) {
        du[b] = dense_lookup(h->h_ukeys.data(), tr.U, users[b]);
        KN_REQUIRE(du[b] < 0 ? h->cfg.shard_rank == 0 : (du[b] >= tr.own_lo && du[b] < tr.own_hi), KNNCF_E_STATE,
                   "recommend batch: a user belongs to another shard");
    }
    const bool knn = predictor == KNNCF_PRED_KNN;
    if (knn && tr.U >= 2 && nt.kcap > 0) {
        // the reference evaluates weightedSumDeviation, hence getNeighbors, only for a train user whose mean is not negative
        // (:573 answers the global average otherwise): nobody else's list is built or numbered here
        std::vector<int32_t> wanted(du);
        bool any = false;
        for (int32_t& u : wanted) {
            if (u >= 0 && train_user_avg(h, u) < 0.0) u = -1;
            any = any || u >= 0;
        }
        if (any) {
            KN_REQUIRE(h->cfg.similarity != KNNCF_SIM_ONE, KNNCF_E_UNSUPPORTED,
                       "kNN neighbourhoods with similarityOne: every similarity is 1.0, the neighbourhood is the first k users in Set order — not built");
            build_missing_neighbors(h, wanted);
        }
    }
    const bool fast_select = n <= RB_FAST_N;
    const int32_t width = (int32_t)std::min<int64_t>(n, I);  // cells of a row that can be filled
    QueryBatchScratch& bs = h->query_batch;
    RecoBatchScratch& rb = h->reco_batch;
    h->prep.join_commit(st);
    const int64_t chunk = recommend_batch_chunk(h);
    if (fast_select) {
        Stage s(h, &h->tm.predict_ms);
        reco_batch_id_rank(tr, bs, rb, h->prep.sort, st);
    }
    std::vector<int32_t> h_items, h_counts;
    std::vector<double> h_preds;
    for (int64_t c0 = 0; c0 < B; c0 += chunk) {
        const int32_t C = (int32_t)std::min<int64_t>(chunk, B - c0);
        const size_t cells = (size_t)C * (size_t)I;
        rb.slot_user.ensure(C); rb.slot_raw.ensure(C); rb.counts.ensure(C);
        bs.pred.ensure(cells); bs.rated.ensure(cells); bs.info.ensure((size_t)4 * C);
        bs.out_items.ensure((size_t)C * width); bs.out_preds.ensure((size_t)C * width);
        KN_HIP(hipMemcpyAsync(rb.slot_user.p, du.data() + c0, (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice, st));
        KN_HIP(hipMemcpyAsync(rb.slot_raw.p, users + c0, (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice, st));
        rb.row_users.ensure(cells); rb.row_items.ensure(cells);
        reco_batch_rows(tr, rb, C, rb.row_users.p, rb.row_items.p, st);
        // one prediction batch over the chunk's C x I rows (every list the rows need exists: the batch numbers nothing, and its
        // call epoch is given back)
        const int64_t epoch = h->epoch;
        run_predict(h, predictor, rb.row_users.p, rb.row_items.p, nullptr, (int64_t)cells, nullptr, nullptr, bs.pred.p);
        if (knn) h->epoch = epoch;
        {
            Stage s(h, &h->tm.predict_ms);
            reco_batch_mark(tr, rb, C, n, bs.rated.p, (long long*)bs.info.p, st);
            if (fast_select) {
                reco_batch_select(tr, rb, C, width, bs.pred.p, bs.rated.p, bs.out_items.p, bs.out_preds.p, st);
            } else {
                bs.k64_a.ensure(cells); bs.k64_b.ensure(cells); bs.v32_a.ensure(cells); bs.v32_b.ensure(cells);
                bs.s32_a.ensure(cells); bs.s32_b.ensure(cells);
                foldin_batch_recommend(tr, bs, h->prep.sort, C, width, bs.out_items.p, bs.out_preds.p, st);
            }
        }
        h_items.resize((size_t)C * width); h_preds.resize((size_t)C * width); h_counts.resize(C);
        KN_HIP(hipMemcpyAsync(h_items.data(), bs.out_items.p, h_items.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        KN_HIP(hipMemcpyAsync(h_preds.data(), bs.out_preds.p, h_preds.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        KN_HIP(hipMemcpyAsync(h_counts.data(), rb.counts.p, (size_t)C * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        KN_HIP(hipStreamSynchronize(st));
        for (int32_t s = 0; s < C; ++s) {
            const int64_t b = c0 + s;
            const int32_t m = h_counts[s];
            std::copy(h_items.begin() + (size_t)s * width, h_items.begin() + (size_t)s * width + m, out_items + b * n);
            std::copy(h_preds.begin() + (size_t)s * width, h_preds.begin() + (size_t)s * width + m, out_preds + b * n);
            counts[b] = m;
        }
    }
}

int knncf_recommend_batch(knncf_handle* h, int predictor, const int32_t* users, int64_t n_users, int32_t n, int32_t* out_items,
                          double* out_preds, int32_t* counts) {
    return guarded(h, [&] { do_recommend_batch(h, predictor, users, n_users, n, out_items, out_preds, counts); });
}

int knncf_knn_similarity(knncf_handle* h, int32_t u, int32_t v, double* out) {
    return guarded(h, [&] {
        require_fitted(h);
        KN_REQUIRE(out, KNNCF_E_INVALID, "null out");
        KN_REQUIRE(h->cfg.similarity != KNNCF_SIM_ONE, KNNCF_E_UNSUPPORTED, "neighbourhoods: adjusted cosine or Jaccard");
        int32_t du = dense_user(h, u), dv = dense_user(h, v);
        *out = 0.0;
        if (du < 0 || dv < 0) return;  // all of an unseen user's similarities are 0.0
        KN_REQUIRE(du >= h->tr.own_lo && du < h->tr.own_hi, KNNCF_E_INVALID, "user belongs to another shard");
        std::vector<int32_t> di;
        std::vector<double> ds;
        neighbors_of(h, du, di, ds);
        for (size_t j = 0; j < di.size(); ++j)
            if (di[j] == dv) { *out = 0.0 + ds[j]; break; }
    });
}

// ---- bulk similarities (similarity_batch.hip; include/knncf.h "Bulk similarities") ---------------------------------------
// pairs per chunk of the host forms: the rule of knncf.h
static int64_t pair_batch_chunk(knncf_handle* h) { return std::max<int64_t>(1, batch_budget(h) / PAIR_BYTES); }

// consecutive chunks of the pairs through the handle's scratch: upload, launch(d_us, d_vs, C, d_out) under `acc`, download
typedef std::function<void(const int32_t*, const int32_t*, int64_t, double*)> PairLaunch;
static void run_pair_chunks(knncf_handle* h, const int32_t* us, const int32_t* vs, int64_t n, double* out, double* acc, const PairLaunch& launch) {
    hipStream_t st = h->stream;
    const int64_t chunk = std::min<int64_t>(pair_batch_chunk(h), n);
    h->pair_us.ensure(chunk); h->pair_vs.ensure(chunk); h->pair_out.ensure(chunk);
    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
        const int64_t C = std::min<int64_t>(chunk, n - c0);
        KN_HIP(hipMemcpyAsync(h->pair_us.p, us + c0, (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice, st));
        KN_HIP(hipMemcpyAsync(h->pair_vs.p, vs + c0, (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice, st));
        {
            Stage s(h, acc);
            launch(h->pair_us.p, h->pair_vs.p, C, h->pair_out.p);
        }
        KN_HIP(hipMemcpyAsync(out + c0, h->pair_out.p, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, st));
        KN_HIP(hipStreamSynchronize(st));
    }
}

int knncf_similarity_batch(knncf_handle* h, const int32_t* us, const int32_t* vs, int64_t n, double* out) {
    return guarded(h, [&] {
        require_fitted(h);
        KN_REQUIRE(n >= 0 && (n == 0 || (us && vs && out)), KNNCF_E_INVALID, "similarity batch: n < 0 or a null argument");
        if (n == 0) return;
        if (h->cfg.similarity == KNNCF_SIM_ONE) { std::fill(out, out + n, 1.0); return; }
        const bool jaccard = h->cfg.similarity == KNNCF_SIM_JACCARD;
        run_pair_chunks(h, us, vs, n, out, &h->tm.rerank_ms, [&](const int32_t* d_us, const int32_t* d_vs, int64_t C, double* d_out) {
            launch_pair_similarity(h->tr, jaccard, d_us, d_vs, C, d_out, h->stream);
        });
    });
}

int knncf_similarity_batch_device(knncf_handle* h, const int32_t* d_us, const int32_t* d_vs, int64_t n, double* d_out) {
    return guarded(h, [&] {
        require_fitted(h);
        KN_REQUIRE(n >= 0 && (n == 0 || (d_us && d_vs && d_out)), KNNCF_E_INVALID, "similarity batch: n < 0 or a null argument");
        if (n == 0) return;
        if (h->cfg.similarity == KNNCF_SIM_ONE) {
            const std::vector<double> ones((size_t)n, 1.0);
            KN_HIP(hipMemcpyAsync(d_out, ones.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
            KN_HIP(hipStreamSynchronize(h->stream));
            return;
        }
        Stage s(h, &h->tm.rerank_ms);
        launch_pair_similarity(h->tr, h->cfg.similarity == KNNCF_SIM_JACCARD, d_us, d_vs, n, d_out, h->stream);
    });
}

// getSimilarity(train, k, sim)(us[j], vs[j]) :634-648 for j = 0 .. n-1, as if asked in this order: u's neighbourhood is evaluated
// only when both ids are in train, so the missing lists are those of knncf_neighbors_batch over us with every other position taken
// out — built in one batch (build_missing_neighbors), then the lookup runs on the device and only `out` comes back
int knncf_knn_similarity_batch(knncf_handle* h, const int32_t* us, const int32_t* vs, int64_t n, double* out) {
    return guarded(h, [&] {
        require_fitted(h);
        KN_REQUIRE(n >= 0 && (n == 0 || (us && vs && out)), KNNCF_E_INVALID, "kNN similarity batch: n < 0 or a null argument");
        KN_REQUIRE(h->cfg.similarity != KNNCF_SIM_ONE, KNNCF_E_UNSUPPORTED, "neighbourhoods: adjusted cosine or Jaccard");
        if (n == 0) return;
        Train& tr = h->tr;
        load_host_ids(h);
        // two lookups per pair on the host: through a mirror of the fit's direct id table where it has one (a gather instead of a
        // hash and a binary search: 142 -> 2.1 ns per pair at the ml-25m shape)
        if (tr.u_table_n > 0 && h->h_utable.empty()) {
            h->h_utable.resize((size_t)tr.u_table_n);
            KN_HIP(hipMemcpyAsync(h->h_utable.data(), tr.u_table.p, h->h_utable.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
            KN_HIP(hipStreamSynchronize(h->stream));
        }
        const int32_t* table = tr.u_table_n > 0 ? h->h_utable.data() : nullptr;
        const int32_t table_n = tr.u_table_n;
        auto dense = [&](int32_t raw) {
            if (table) return raw >= 0 && raw < table_n ? table[raw] : -1;
            return dense_lookup(h->h_ukeys.data(), tr.U, raw);
        };
        std::vector<int32_t> wanted((size_t)n);
        for (int64_t j = 0; j < n; ++j) {
            const int32_t du = dense(us[j]);
            wanted[j] = du >= 0 && dense(vs[j]) >= 0 ? du : -1;
            KN_REQUIRE(wanted[j] < 0 || (du >= tr.own_lo && du < tr.own_hi), KNNCF_E_INVALID, "user belongs to another shard");
        }
        build_missing_neighbors(h, wanted);
        run_pair_chunks(h, us, vs, n, out, &h->tm.predict_ms, [&](const int32_t* d_us, const int32_t* d_vs, int64_t C, double* d_out) {
            launch_pair_knn_lookup(tr, h->nt, d_us, d_vs, C, d_out, h->stream);
        });
    });
}

int knncf_predict_batch_device(knncf_handle* h, int predictor, const int32_t* d_users, const int32_t* d_items,
                               int64_t n, double* d_out) {
    return guarded(h, [&] {
        KN_REQUIRE(d_out || n == 0, KNNCF_E_INVALID, "null output");
        run_predict(h, predictor, d_users, d_items, nullptr, n, nullptr, nullptr, d_out);
    });
}

int knncf_predict_batch(knncf_handle* h, int predictor, const int32_t* users, const int32_t* items, int64_t n, double* out) {
    return guarded(h, [&] {
        KN_REQUIRE(n >= 0 && (n == 0 || (users && items && out)), KNNCF_E_INVALID, "bad arguments");
        if (n == 0) return;
        h->t_users.ensure(n); h->t_items.ensure(n); h->t_pred.ensure(n);
        KN_HIP(hipMemcpyAsync(h->t_users.p, users, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        KN_HIP(hipMemcpyAsync(h->t_items.p, items, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        run_predict(h, predictor, h->t_users.p, h->t_items.p, nullptr, n, nullptr, nullptr, nullptr);
        KN_HIP(hipMemcpyAsync(out, h->t_pred.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        KN_HIP(hipStreamSynchronize(h->stream));
    });
}

int knncf_predict(knncf_handle* h, int predictor, int32_t user, int32_t item, double* out) {
    return knncf_predict_batch(h, predictor, &user, &item, 1, out);
}

// ---- explanations (explain.hip; include/knncf.h "Explanations") ---------------------------------------------------------
// the refusals of every form, before anything is built or written
static void explain_require(knncf_handle* h, const void* users, const void* items, int64_t n, int32_t order, int32_t cap,
                            const void* raters, const void* sims, const void* devs, const void* counts) {
    require_fitted(h, false);  // (a shard handle is refused below, committed or not)
    KN_REQUIRE(n >= 0 && cap >= 0, KNNCF_E_INVALID, "explain: n or cap < 0");
    KN_REQUIRE(order == KNNCF_EXPLAIN_SUM_ORDER || order == KNNCF_EXPLAIN_BY_WEIGHT, KNNCF_E_INVALID, "explain: unknown order");
    KN_REQUIRE(n < (int64_t)0xffffffffll, KNNCF_E_INVALID, "explain: 2^32-1 rows or more");
    KN_REQUIRE(h->cfg.similarity != KNNCF_SIM_ONE, KNNCF_E_UNSUPPORTED,
               "kNN neighbourhoods with similarityOne: every similarity is 1.0, the neighbourhood is the first k users in Set order — not built");
    KN_REQUIRE(h->cfg.shard_count == 1, KNNCF_E_UNSUPPORTED, "explain: single-shard handles only");
    KN_REQUIRE(n == 0 || (users && items && counts && (cap == 0 || (raters && sims && devs))), KNNCF_E_INVALID, "explain: null argument");
}

// what run_predict does in front of its kNN kernel, once for the whole call: the rows' dense ids in t_du / t_di and the
// neighbourhoods they need, built and numbered by ensure_neighbors_for_rows
static void explain_prepare(knncf_handle* h, const int32_t* d_users, const int32_t* d_items, int64_t n) {
    ensure_test_scratch(h, n);
    {
        Stage s(h, &h->tm.predict_ms);
        launch_dense_ids(h->tr, d_users, d_items, n, h->t_du.p, h->t_di.p, h->stream);
    }
    ensure_neighbors_for_rows(h, n);
    h->prep.join_commit(h->stream);  // the item-major copies and the rater bitmaps (second part of prep_commit)
}

int knncf_explain_batch_device(knncf_handle* h, const int32_t* d_users, const int32_t* d_items, int64_t n, int32_t order,
                               int32_t cap, int32_t* d_raters, double* d_sims, double* d_devs, int32_t* d_counts,
                               double* d_sums, double* d_predictions) {
    return guarded(h, [&] {
        explain_require(h, d_users, d_items, n, order, cap, d_raters, d_sims, d_devs, d_counts);
        if (n == 0) return;
        explain_prepare(h, d_users, d_items, n);
        Stage s(h, &h->tm.predict_ms);
        launch_explain(h->tr, h->nt, n, h->t_du.p, h->t_di.p, {order, cap, d_raters, d_sims, d_devs, d_counts, d_sums, d_predictions},
                       h->stream);
    });
}

int knncf_explain_batch(knncf_handle* h, const int32_t* users, const int32_t* items, int64_t n, int32_t order, int32_t cap,
                        int32_t* raters, double* sims, double* devs, int32_t* counts, double* sums, double* predictions) {
    return guarded(h, [&] {
        explain_require(h, users, items, n, order, cap, raters, sims, devs, counts);
        if (n == 0) return;
        hipStream_t st = h->stream;
        h->t_users.ensure(n); h->t_items.ensure(n);
        KN_HIP(hipMemcpyAsync(h->t_users.p, users, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        KN_HIP(hipMemcpyAsync(h->t_items.p, items, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        explain_prepare(h, h->t_users.p, h->t_items.p, n);
        const int64_t chunk = std::min<int64_t>(explain_batch_chunk(h, cap), n);
        const size_t cells = (size_t)chunk * (size_t)cap;
        h->ex_raters.ensure(cells); h->ex_sims.ensure(cells); h->ex_devs.ensure(cells);
        h->ex_counts.ensure(chunk); h->ex_sums.ensure((size_t)2 * chunk); h->ex_pred.ensure(chunk);
        const ExplainCells d_out{order, cap, h->ex_raters.p, h->ex_sims.p, h->ex_devs.p, h->ex_counts.p, h->ex_sums.p, h->ex_pred.p};
        std::vector<int32_t> h_raters(cells);
        std::vector<double> h_sims(cells), h_devs(cells);
        for (int64_t c0 = 0; c0 < n; c0 += chunk) {
            const int64_t C = std::min<int64_t>(chunk, n - c0);
            {
                Stage s(h, &h->tm.predict_ms);
                launch_explain(h->tr, h->nt, C, h->t_du.p + c0, h->t_di.p + c0, d_out, st);
            }
            KN_HIP(hipMemcpyAsync(counts + c0, h->ex_counts.p, (size_t)C * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            if (sums) KN_HIP(hipMemcpyAsync(sums + 2 * c0, h->ex_sums.p, (size_t)2 * C * sizeof(double), hipMemcpyDeviceToHost, st));
            if (predictions) KN_HIP(hipMemcpyAsync(predictions + c0, h->ex_pred.p, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, st));
            if (cap > 0) {
                KN_HIP(hipMemcpyAsync(h_raters.data(), h->ex_raters.p, (size_t)C * cap * sizeof(int32_t), hipMemcpyDeviceToHost, st));
                KN_HIP(hipMemcpyAsync(h_sims.data(), h->ex_sims.p, (size_t)C * cap * sizeof(double), hipMemcpyDeviceToHost, st));
                KN_HIP(hipMemcpyAsync(h_devs.data(), h->ex_devs.p, (size_t)C * cap * sizeof(double), hipMemcpyDeviceToHost, st));
            }
            KN_HIP(hipStreamSynchronize(st));
            for (int64_t r = 0; r < C && cap > 0; ++r) {  // (the cells of a row beyond its terms stay as the caller left them)
                const size_t from = (size_t)r * cap, to = (size_t)(c0 + r) * cap;
                const int32_t m = std::min(counts[c0 + r], cap);
                std::copy(h_raters.begin() + from, h_raters.begin() + from + m, raters + to);
                std::copy(h_sims.begin() + from, h_sims.begin() + from + m, sims + to);
                std::copy(h_devs.begin() + from, h_devs.begin() + from + m, devs + to);
            }
        }
    });
}

int knncf_explain(knncf_handle* h, int32_t user, int32_t item, int32_t order, int32_t cap, int32_t* raters, double* sims,
                  double* devs, int32_t* count, double* sums, double* prediction) {
    return knncf_explain_batch(h, &user, &item, 1, order, cap, raters, sims, devs, count, sums, prediction);
}

// ---- explanations of Personalized predictions (explain_all.hip; include/knncf.h "Explanations of Personalized predictions") ----
// The streamed form of predict_personal_rows at every number of users: per block of the plan the users' exact rows (rerank_ms),
// then the explain kernel over consecutive sub-ranges of the block's sorted rows (predict_ms), each one's block of outputs
// brought back with one copy and scattered to the caller's rows.  Read-only on the kNN state.
static void explain_personal_rows(knncf_handle* h, int64_t n, const ExplainCells& to) {
    Train& tr = h->tr;
    PersonalRows& pr = h->prow;
    hipStream_t st = h->stream;
    const PersonalPlan plan = plan_personal_rows(h, n);
    std::vector<uint32_t> order((size_t)n);
    KN_HIP(hipMemcpyAsync(order.data(), h->prep.v32_b.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    KN_HIP(hipStreamSynchronize(st));
    const std::vector<int64_t> rows(order.begin(), order.end());  // sorted row -> the caller's row
    const int64_t sub = std::min<int64_t>(n, std::max<int64_t>(1, batch_budget(h) / (int64_t)explain_all_row_bytes(to.cap)));
    const size_t pack = ((size_t)sub * explain_row_bytes(to.cap) + 7) / 8;  // doubles
    h->ex_pack.ensure(pack);
    if (to.order == KNNCF_EXPLAIN_BY_WEIGHT) h->ex_stage.ensure(((size_t)sub * to.cap * 20 + 7) / 8);
    std::vector<double> h_vals(pack);
    for (int64_t b = 0; b < plan.n_blocks; ++b) {
        const int64_t u0 = b * plan.R, u1 = std::min<int64_t>(plan.nu, u0 + plan.R);
        if (u1 > u0) {
            Stage s(h, &h->tm.rerank_ms);
            launch_sim_rows(tr, pr, pr.users.p + u0, (int32_t)(u1 - u0), pr.S.p, st);
        }
        for (int64_t r0 = plan.row_begin(b), r1 = plan.row_end(b, n); r0 < r1; r0 += sub) {
            const int64_t nr = std::min(sub, r1 - r0);
            {
                Stage s(h, &h->tm.predict_ms);
                launch_explain_all(tr, pr, nr, h->prep.v32_b.p + r0, h->t_du.p, h->t_di.p, pr.slot.p, pr.S.p,
                                   explain_pack(h->ex_pack.p, nr, to), h->ex_stage.p, st);
            }
            KN_HIP(hipMemcpyAsync(h_vals.data(), h->ex_pack.p, (size_t)nr * explain_row_bytes(to.cap), hipMemcpyDeviceToHost, st));
            KN_HIP(hipStreamSynchronize(st));
            explain_scatter(explain_pack(h_vals.data(), nr, to), nr, to, rows.data() + r0);
        }
    }
}

int knncf_explain_personalized_batch(knncf_handle* h, const int32_t* users, const int32_t* items, int64_t n, int32_t order, int32_t cap,
                                     int32_t* raters, double* sims, double* devs, int32_t* counts, double* sums, double* predictions) {
    return guarded(h, [&] {
        require_fitted(h, false);  // (a shard handle is refused below, committed or not)
        KN_REQUIRE(n >= 0 && cap >= 0, KNNCF_E_INVALID, "explain: n or cap < 0");
        KN_REQUIRE(order == KNNCF_EXPLAIN_SUM_ORDER || order == KNNCF_EXPLAIN_BY_WEIGHT, KNNCF_E_INVALID, "explain: unknown order");
        KN_REQUIRE(n < (int64_t)0xffffffffll, KNNCF_E_INVALID, "explain: 2^32-1 rows or more");
        KN_REQUIRE(n == 0 || (users && items && counts && (cap == 0 || (raters && sims && devs))), KNNCF_E_INVALID, "explain: null argument");
        KN_REQUIRE(h->cfg.similarity != KNNCF_SIM_ONE, KNNCF_E_UNSUPPORTED,
                   "PERSONALIZED explanations with similarityOne: every weight is 1.0, there is nothing to explain");
        KN_REQUIRE(h->cfg.shard_count == 1, KNNCF_E_UNSUPPORTED, "explain: single-shard handles only");
        if (n == 0) return;
        ensure_personal_rows(h);  // (and the fitted Personalized predictor's refusals)
        hipStream_t st = h->stream;
        h->t_users.ensure(n); h->t_items.ensure(n);
        KN_HIP(hipMemcpyAsync(h->t_users.p, users, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        KN_HIP(hipMemcpyAsync(h->t_items.p, items, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        ensure_test_scratch(h, n);
        {
            Stage s(h, &h->tm.predict_ms);
            launch_dense_ids(h->tr, h->t_users.p, h->t_items.p, n, h->t_du.p, h->t_di.p, st);
        }
        explain_personal_rows(h, n, {order, cap, raters, sims, devs, counts, sums, predictions});
    });
}

int knncf_explain_personalized(knncf_handle* h, int32_t user, int32_t item, int32_t order, int32_t cap, int32_t* raters, double* sims,
                               double* devs, int32_t* count, double* sums, double* prediction) {
    return knncf_explain_personalized_batch(h, &user, &item, 1, order, cap, raters, sims, devs, count, sums, prediction);
}

int knncf_recommend(knncf_handle* h, int predictor, int32_t user, int32_t n, int32_t* items, double* predictions, int32_t* count) {
    return guarded(h, [&] {
        require_fitted(h);
        KN_REQUIRE(count && n >= 0 && (n == 0 || (items && predictions)), KNNCF_E_INVALID, "bad arguments");
        *count = 0;
        do_recommend_batch(h, predictor, &user, 1, n, items, predictions, count);
    });
}

// ---- the 46 query entry points: the rows of the call by name, then the mode's builder (api.cpp "one request type") ----------
// fold-in queries: a user outside the fit
int knncf_query_neighbors(knncf_handle* h, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings,
                          int32_t cap, int32_t* ids, double* sims, int32_t* count) {
    return query_single(h, neighbors_call({.family = QF_FOLD_IN, .items = items, .ratings = ratings, .user = user, .n_ratings = n_ratings},
                                          cap, ids, sims, count));
}

int knncf_query_predict(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings,
                        int64_t n_ratings, const int32_t* pred_items, int64_t m, double* out) {
    return query_single(h, predict_call({.family = QF_FOLD_IN, .items = items, .ratings = ratings, .pred_items = pred_items, .user = user,
                                        .n_ratings = n_ratings, .m = m}, predictor, out));
}

int knncf_query_neighbors_batch(knncf_handle* h, const int32_t* users, const int64_t* offsets, const int32_t* items,
                                const double* ratings, int64_t n_queries, int32_t cap, int32_t* ids, double* sims, int32_t* counts,
                                int32_t* statuses) {
    return query_batch(h, neighbors_call({.family = QF_FOLD_IN, .users = users, .B = n_queries, .offsets = offsets, .items = items,
                                         .ratings = ratings, .statuses = statuses}, cap, ids, sims, counts));
}

int knncf_query_predict_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets, const int32_t* items,
                              const double* ratings, int64_t n_queries, const int64_t* pred_offsets, const int32_t* pred_items,
                              double* out, int32_t* statuses) {
    return query_batch(h, predict_call({.family = QF_FOLD_IN, .users = users, .B = n_queries, .offsets = offsets, .items = items,
                                       .ratings = ratings, .pred_offsets = pred_offsets, .pred_items = pred_items, .statuses = statuses},
                                       predictor, out));
}

int knncf_query_recommend_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets, const int32_t* items,
                                const double* ratings, int64_t n_queries, int32_t n, int32_t* out_items, double* out_preds,
                                int32_t* counts, int32_t* statuses) {
    return query_batch(h, recommend_call({.family = QF_FOLD_IN, .users = users, .B = n_queries, .offsets = offsets, .items = items,
                                         .ratings = ratings, .statuses = statuses}, predictor, n, out_items, out_preds, counts));
}

int knncf_query_recommend(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings,
                          int64_t n_ratings, int32_t n, int32_t* out_items, double* out_preds, int32_t* count) {
    return query_single(h, recommend_call({.family = QF_FOLD_IN, .items = items, .ratings = ratings, .user = user, .n_ratings = n_ratings},
                                          predictor, n, out_items, out_preds, count));
}

// update queries: the same calls for a user that may be in the fit (the rows are additional to its train rows)
int knncf_update_neighbors(knncf_handle* h, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings,
                           int32_t cap, int32_t* ids, double* sims, int32_t* count) {
    return query_single(h, neighbors_call({.family = QF_UPDATE, .items = items, .ratings = ratings, .user = user, .n_ratings = n_ratings},
                                          cap, ids, sims, count));
}

int knncf_update_predict(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings,
                         int64_t n_ratings, const int32_t* pred_items, int64_t m, double* out) {
    return query_single(h, predict_call({.family = QF_UPDATE, .items = items, .ratings = ratings, .pred_items = pred_items, .user = user,
                                        .n_ratings = n_ratings, .m = m}, predictor, out));
}

int knncf_update_neighbors_batch(knncf_handle* h, const int32_t* users, const int64_t* offsets, const int32_t* items,
                                 const double* ratings, int64_t n_queries, int32_t cap, int32_t* ids, double* sims, int32_t* counts,
                                 int32_t* statuses) {
    return query_batch(h, neighbors_call({.family = QF_UPDATE, .users = users, .B = n_queries, .offsets = offsets, .items = items,
                                         .ratings = ratings, .statuses = statuses}, cap, ids, sims, counts));
}

int knncf_update_predict_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets, const int32_t* items,
                               const double* ratings, int64_t n_queries, const int64_t* pred_offsets, const int32_t* pred_items,
                               double* out, int32_t* statuses) {
    return query_batch(h, predict_call({.family = QF_UPDATE, .users = users, .B = n_queries, .offsets = offsets, .items = items,
                                       .ratings = ratings, .pred_offsets = pred_offsets, .pred_items = pred_items, .statuses = statuses},
                                       predictor, out));
}

int knncf_update_recommend_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets, const int32_t* items,
                                 const double* ratings, int64_t n_queries, int32_t n, int32_t* out_items, double* out_preds,
                                 int32_t* counts, int32_t* statuses) {
    return query_batch(h, recommend_call({.family = QF_UPDATE, .users = users, .B = n_queries, .offsets = offsets, .items = items,
                                         .ratings = ratings, .statuses = statuses}, predictor, n, out_items, out_preds, counts));
}

int knncf_update_recommend(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings,
                           int64_t n_ratings, int32_t n, int32_t* out_items, double* out_preds, int32_t* count) {
    return query_single(h, recommend_call({.family = QF_UPDATE, .items = items, .ratings = ratings, .user = user, .n_ratings = n_ratings},
                                          predictor, n, out_items, out_preds, count));
}

// revise queries: update queries that also remove train rows of the user (removed_items) from aug
int knncf_revise_neighbors(knncf_handle* h, int32_t user, const int32_t* removed_items, int64_t n_removed, const int32_t* items,
                           const double* ratings, int64_t n_ratings, int32_t cap, int32_t* ids, double* sims, int32_t* count) {
    return query_single(h, neighbors_call({.family = QF_REVISE, .items = items, .ratings = ratings, .removed_items = removed_items,
                                          .user = user, .n_ratings = n_ratings, .n_removed = n_removed}, cap, ids, sims, count));
}

int knncf_revise_predict(knncf_handle* h, int predictor, int32_t user, const int32_t* removed_items, int64_t n_removed,
                         const int32_t* items, const double* ratings, int64_t n_ratings, const int32_t* pred_items, int64_t m, double* out) {
    return query_single(h, predict_call({.family = QF_REVISE, .items = items, .ratings = ratings, .removed_items = removed_items,
                                        .pred_items = pred_items, .user = user, .n_ratings = n_ratings, .n_removed = n_removed, .m = m},
                                        predictor, out));
}

int knncf_revise_recommend(knncf_handle* h, int predictor, int32_t user, const int32_t* removed_items, int64_t n_removed,
                           const int32_t* items, const double* ratings, int64_t n_ratings, int32_t n, int32_t* out_items,
                           double* out_preds, int32_t* count) {
    return query_single(h, recommend_call({.family = QF_REVISE, .items = items, .ratings = ratings, .removed_items = removed_items,
                                          .user = user, .n_ratings = n_ratings, .n_removed = n_removed}, predictor, n, out_items, out_preds,
                                          count));
}

int knncf_revise_neighbors_batch(knncf_handle* h, const int32_t* users, const int64_t* removed_offsets, const int32_t* removed_items,
                                 const int64_t* offsets, const int32_t* items, const double* ratings, int64_t n_queries, int32_t cap,
                                 int32_t* ids, double* sims, int32_t* counts, int32_t* statuses) {
    return query_batch(h, neighbors_call({.family = QF_REVISE, .users = users, .B = n_queries, .offsets = offsets, .items = items,
                                         .ratings = ratings, .removed_offsets = removed_offsets, .removed_items = removed_items,
                                         .statuses = statuses}, cap, ids, sims, counts));
}

int knncf_revise_predict_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* removed_offsets,
                               const int32_t* removed_items, const int64_t* offsets, const int32_t* items, const double* ratings,
                               int64_t n_queries, const int64_t* pred_offsets, const int32_t* pred_items, double* out, int32_t* statuses) {
    return query_batch(h, predict_call({.family = QF_REVISE, .users = users, .B = n_queries, .offsets = offsets, .items = items,
                                       .ratings = ratings, .removed_offsets = removed_offsets, .removed_items = removed_items,
                                       .pred_offsets = pred_offsets, .pred_items = pred_items, .statuses = statuses}, predictor, out));
}

int knncf_revise_recommend_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* removed_offsets,
                                 const int32_t* removed_items, const int64_t* offsets, const int32_t* items, const double* ratings,
                                 int64_t n_queries, int32_t n, int32_t* out_items, double* out_preds, int32_t* counts, int32_t* statuses) {
    return query_batch(h, recommend_call({.family = QF_REVISE, .users = users, .B = n_queries, .offsets = offsets, .items = items,
                                         .ratings = ratings, .removed_offsets = removed_offsets, .removed_items = removed_items,
                                         .statuses = statuses}, predictor, n, out_items, out_preds, counts));
}

// explanations of query predictions: the *_predict calls' arguments, the terms behind every requested row
int knncf_query_explain(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings,
                        const int32_t* pred_items, int64_t m, int32_t order, int32_t cap, int32_t* raters, double* sims, double* devs,
                        int32_t* counts, double* sums, double* predictions) {
    return query_single(h, explain_call({.family = QF_FOLD_IN, .items = items, .ratings = ratings, .pred_items = pred_items, .user = user,
                                        .n_ratings = n_ratings, .m = m},
                                        predictor, {order, cap, raters, sims, devs, counts, sums, predictions}));
}

int knncf_update_explain(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings,
                         const int32_t* pred_items, int64_t m, int32_t order, int32_t cap, int32_t* raters, double* sims, double* devs,
                         int32_t* counts, double* sums, double* predictions) {
    return query_single(h, explain_call({.family = QF_UPDATE, .items = items, .ratings = ratings, .pred_items = pred_items, .user = user,
                                        .n_ratings = n_ratings, .m = m},
                                        predictor, {order, cap, raters, sims, devs, counts, sums, predictions}));
}

int knncf_revise_explain(knncf_handle* h, int predictor, int32_t user, const int32_t* removed_items, int64_t n_removed,
                         const int32_t* items, const double* ratings, int64_t n_ratings, const int32_t* pred_items, int64_t m,
                         int32_t order, int32_t cap, int32_t* raters, double* sims, double* devs, int32_t* counts, double* sums,
                         double* predictions) {
    return query_single(h, explain_call({.family = QF_REVISE, .items = items, .ratings = ratings, .removed_items = removed_items,
                                        .pred_items = pred_items, .user = user, .n_ratings = n_ratings, .n_removed = n_removed, .m = m},
                                        predictor, {order, cap, raters, sims, devs, counts, sums, predictions}));
}

int knncf_query_explain_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets, const int32_t* items,
                              const double* ratings, int64_t n_queries, const int64_t* pred_offsets, const int32_t* pred_items,
                              int32_t order, int32_t cap, int32_t* raters, double* sims, double* devs, int32_t* counts, double* sums,
                              double* predictions, int32_t* statuses) {
    return query_batch(h, explain_call({.family = QF_FOLD_IN, .users = users, .B = n_queries, .offsets = offsets, .items = items,
                                       .ratings = ratings, .pred_offsets = pred_offsets, .pred_items = pred_items, .statuses = statuses},
                                       predictor, {order, cap, raters, sims, devs, counts, sums, predictions}));
}

int knncf_update_explain_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets, const int32_t* items,
                               const double* ratings, int64_t n_queries, const int64_t* pred_offsets, const int32_t* pred_items,
                               int32_t order, int32_t cap, int32_t* raters, double* sims, double* devs, int32_t* counts, double* sums,
                               double* predictions, int32_t* statuses) {
    return query_batch(h, explain_call({.family = QF_UPDATE, .users = users, .B = n_queries, .offsets = offsets, .items = items,
                                       .ratings = ratings, .pred_offsets = pred_offsets, .pred_items = pred_items, .statuses = statuses},
                                       predictor, {order, cap, raters, sims, devs, counts, sums, predictions}));
}

int knncf_revise_explain_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* removed_offsets,
                               const int32_t* removed_items, const int64_t* offsets, const int32_t* items, const double* ratings,
                               int64_t n_queries, const int64_t* pred_offsets, const int32_t* pred_items, int32_t order, int32_t cap,
                               int32_t* raters, double* sims, double* devs, int32_t* counts, double* sums, double* predictions,
                               int32_t* statuses) {
    return query_batch(h, explain_call({.family = QF_REVISE, .users = users, .B = n_queries, .offsets = offsets, .items = items,
                                       .ratings = ratings, .removed_offsets = removed_offsets, .removed_items = removed_items,
                                       .pred_offsets = pred_offsets, .pred_items = pred_items, .statuses = statuses}, predictor, {order,
                                       cap, raters, sims, devs, counts, sums, predictions}));
}

// explanations of Personalized query predictions: the explain calls' arguments without the predictor (QB_EXPLAIN_ALL)
int knncf_query_explain_personalized(knncf_handle* h, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings,
                                     const int32_t* pred_items, int64_t m, int32_t order, int32_t cap, int32_t* raters, double* sims,
                                     double* devs, int32_t* counts, double* sums, double* predictions) {
    return query_single(h, explain_all_call({.family = QF_FOLD_IN, .items = items, .ratings = ratings, .pred_items = pred_items,
                                            .user = user, .n_ratings = n_ratings, .m = m},
                                            {order, cap, raters, sims, devs, counts, sums, predictions}));
}

int knncf_update_explain_personalized(knncf_handle* h, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings,
                                      const int32_t* pred_items, int64_t m, int32_t order, int32_t cap, int32_t* raters, double* sims,
                                      double* devs, int32_t* counts, double* sums, double* predictions) {
    return query_single(h, explain_all_call({.family = QF_UPDATE, .items = items, .ratings = ratings, .pred_items = pred_items,
                                            .user = user, .n_ratings = n_ratings, .m = m},
                                            {order, cap, raters, sims, devs, counts, sums, predictions}));
}

int knncf_revise_explain_personalized(knncf_handle* h, int32_t user, const int32_t* removed_items, int64_t n_removed,
                                      const int32_t* items, const double* ratings, int64_t n_ratings, const int32_t* pred_items,
                                      int64_t m, int32_t order, int32_t cap, int32_t* raters, double* sims, double* devs,
                                      int32_t* counts, double* sums, double* predictions) {
    return query_single(h, explain_all_call({.family = QF_REVISE, .items = items, .ratings = ratings, .removed_items = removed_items,
                                            .pred_items = pred_items, .user = user, .n_ratings = n_ratings, .n_removed = n_removed,
                                            .m = m},
                                            {order, cap, raters, sims, devs, counts, sums, predictions}));
}

int knncf_query_explain_personalized_batch(knncf_handle* h, const int32_t* users, const int64_t* offsets, const int32_t* items,
                                           const double* ratings, int64_t n_queries, const int64_t* pred_offsets,
                                           const int32_t* pred_items, int32_t order, int32_t cap, int32_t* raters, double* sims,
                                           double* devs, int32_t* counts, double* sums, double* predictions, int32_t* statuses) {
    return query_batch(h, explain_all_call({.family = QF_FOLD_IN, .users = users, .B = n_queries, .offsets = offsets, .items = items,
                                           .ratings = ratings, .pred_offsets = pred_offsets, .pred_items = pred_items,
                                           .statuses = statuses},
                                           {order, cap, raters, sims, devs, counts, sums, predictions}));
}

int knncf_update_explain_personalized_batch(knncf_handle* h, const int32_t* users, const int64_t* offsets, const int32_t* items,
                                            const double* ratings, int64_t n_queries, const int64_t* pred_offsets,
                                            const int32_t* pred_items, int32_t order, int32_t cap, int32_t* raters, double* sims,
                                            double* devs, int32_t* counts, double* sums, double* predictions, int32_t* statuses) {
    return query_batch(h, explain_all_call({.family = QF_UPDATE, .users = users, .B = n_queries, .offsets = offsets, .items = items,
                                           .ratings = ratings, .pred_offsets = pred_offsets, .pred_items = pred_items,
                                           .statuses = statuses},
                                           {order, cap, raters, sims, devs, counts, sums, predictions}));
}

int knncf_revise_explain_personalized_batch(knncf_handle* h, const int32_t* users, const int64_t* removed_offsets,
                                            const int32_t* removed_items, const int64_t* offsets, const int32_t* items,
                                            const double* ratings, int64_t n_queries, const int64_t* pred_offsets,
                                            const int32_t* pred_items, int32_t order, int32_t cap, int32_t* raters, double* sims,
                                            double* devs, int32_t* counts, double* sums, double* predictions, int32_t* statuses) {
    return query_batch(h, explain_all_call({.family = QF_REVISE, .users = users, .B = n_queries, .offsets = offsets, .items = items,
                                           .ratings = ratings, .removed_offsets = removed_offsets, .removed_items = removed_items,
                                           .pred_offsets = pred_offsets, .pred_items = pred_items, .statuses = statuses},
                                           {order, cap, raters, sims, devs, counts, sums, predictions}));
}

// recommendations with the terms behind them in one pass (QB_RECOMMEND_EXPLAIN): the *_recommend calls' arguments, then order,
// cap and the explain outputs of row b * n + j (no predictions array: out_preds holds them)
int knncf_query_recommend_explain(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings,
                                  int64_t n_ratings, int32_t n, int32_t order, int32_t cap, int32_t* out_items, double* out_preds,
                                  int32_t* count, int32_t* raters, double* sims, double* devs, int32_t* term_counts, double* sums) {
    return query_single(h, recommend_explain_call(recommend_call({.family = QF_FOLD_IN, .items = items, .ratings = ratings, .user = user,
                                                  .n_ratings = n_ratings},
                                                  predictor, n, out_items, out_preds, count),
                                                  {order, cap, raters, sims, devs, term_counts, sums, nullptr}));
}

int knncf_update_recommend_explain(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings,
                                   int64_t n_ratings, int32_t n, int32_t order, int32_t cap, int32_t* out_items, double* out_preds,
                                   int32_t* count, int32_t* raters, double* sims, double* devs, int32_t* term_counts, double* sums) {
    return query_single(h, recommend_explain_call(recommend_call({.family = QF_UPDATE, .items = items, .ratings = ratings, .user = user,
                                                  .n_ratings = n_ratings},
                                                  predictor, n, out_items, out_preds, count),
                                                  {order, cap, raters, sims, devs, term_counts, sums, nullptr}));
}

int knncf_revise_recommend_explain(knncf_handle* h, int predictor, int32_t user, const int32_t* removed_items, int64_t n_removed,
                                   const int32_t* items, const double* ratings, int64_t n_ratings, int32_t n, int32_t order,
                                   int32_t cap, int32_t* out_items, double* out_preds, int32_t* count, int32_t* raters, double* sims,
                                   double* devs, int32_t* term_counts, double* sums) {
    return query_single(h, recommend_explain_call(recommend_call({.family = QF_REVISE, .items = items, .ratings = ratings,
                                                  .removed_items = removed_items, .user = user, .n_ratings = n_ratings,
                                                  .n_removed = n_removed},
                                                  predictor, n, out_items, out_preds, count),
                                                  {order, cap, raters, sims, devs, term_counts, sums, nullptr}));
}

int knncf_query_recommend_explain_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets,
                                        const int32_t* items, const double* ratings, int64_t n_queries, int32_t n, int32_t order,
                                        int32_t cap, int32_t* out_items, double* out_preds, int32_t* counts, int32_t* raters,
                                        double* sims, double* devs, int32_t* term_counts, double* sums, int32_t* statuses) {
    return query_batch(h, recommend_explain_call(recommend_call({.family = QF_FOLD_IN, .users = users, .B = n_queries, .offsets = offsets,
                                                 .items = items, .ratings = ratings, .statuses = statuses},
                                                 predictor, n, out_items, out_preds, counts),
                                                 {order, cap, raters, sims, devs, term_counts, sums, nullptr}));
}

int knncf_update_recommend_explain_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets,
                                         const int32_t* items, const double* ratings, int64_t n_queries, int32_t n, int32_t order,
                                         int32_t cap, int32_t* out_items, double* out_preds, int32_t* counts, int32_t* raters,
                                         double* sims, double* devs, int32_t* term_counts, double* sums, int32_t* statuses) {
    return query_batch(h, recommend_explain_call(recommend_call({.family = QF_UPDATE, .users = users, .B = n_queries, .offsets = offsets,
                                                 .items = items, .ratings = ratings, .statuses = statuses},
                                                 predictor, n, out_items, out_preds, counts),
                                                 {order, cap, raters, sims, devs, term_counts, sums, nullptr}));
}

int knncf_revise_recommend_explain_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* removed_offsets,
                                         const int32_t* removed_items, const int64_t* offsets, const int32_t* items,
                                         const double* ratings, int64_t n_queries, int32_t n, int32_t order, int32_t cap,
                                         int32_t* out_items, double* out_preds, int32_t* counts, int32_t* raters, double* sims,
                                         double* devs, int32_t* term_counts, double* sums, int32_t* statuses) {
    return query_batch(h, recommend_explain_call(recommend_call({.family = QF_REVISE, .users = users, .B = n_queries, .offsets = offsets,
                                                 .items = items, .ratings = ratings, .removed_offsets = removed_offsets,
                                                 .removed_items = removed_items, .statuses = statuses},
                                                 predictor, n, out_items, out_preds, counts),
                                                 {order, cap, raters, sims, devs, term_counts, sums, nullptr}));
}

// bystander queries: fitted users' answers once the fold-in query's user has joined (knncf.h "Bystander queries")
int knncf_query_bystander_neighbors(knncf_handle* h, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings,
                                    const int32_t* others, int64_t m, int32_t cap, int32_t* ids, double* sims, int32_t* counts) {
    return rows_single(h, bystander_neighbors_call({.family = QF_FOLD_IN, .items = items, .ratings = ratings, .user = user,
                                                         .n_ratings = n_ratings, .m = m}, others, cap, ids, sims, counts));
}

int knncf_query_bystander_predict(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings,
                                  int64_t n_ratings, const int32_t* others, const int32_t* pred_items, int64_t m, double* out) {
    return rows_single(h, bystander_predict_call({.family = QF_FOLD_IN, .items = items, .ratings = ratings, .pred_items = pred_items,
                                                       .user = user, .n_ratings = n_ratings, .m = m}, predictor, others, out));
}

int knncf_query_bystander_neighbors_batch(knncf_handle* h, const int32_t* users, const int64_t* offsets, const int32_t* items,
                                          const double* ratings, int64_t n_queries, const int64_t* row_offsets, const int32_t* others,
                                          int32_t cap, int32_t* ids, double* sims, int32_t* counts, int32_t* statuses) {
    return query_batch(h, bystander_neighbors_call({.family = QF_FOLD_IN, .users = users, .B = n_queries, .offsets = offsets,
                                                        .items = items, .ratings = ratings, .pred_offsets = row_offsets,
                                                        .statuses = statuses}, others, cap, ids, sims, counts));
}

int knncf_query_bystander_predict_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets,
                                        const int32_t* items, const double* ratings, int64_t n_queries, const int64_t* row_offsets,
                                        const int32_t* others, const int32_t* pred_items, double* out, int32_t* statuses) {
    return query_batch(h, bystander_predict_call({.family = QF_FOLD_IN, .users = users, .B = n_queries, .offsets = offsets,
                                                      .items = items, .ratings = ratings, .pred_offsets = row_offsets,
                                                      .pred_items = pred_items, .statuses = statuses}, predictor, others, out));
}

// bystanders of update queries: the same four calls for a user that may be in the fit, whose given rows are then additional to
// its train rows (knncf.h "Bystanders of update queries")
int knncf_update_bystander_neighbors(knncf_handle* h, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings,
                                    const int32_t* others, int64_t m, int32_t cap, int32_t* ids, double* sims, int32_t* counts) {
    return rows_single(h, bystander_neighbors_call({.family = QF_UPDATE, .items = items, .ratings = ratings, .user = user,
                                                         .n_ratings = n_ratings, .m = m}, others, cap, ids, sims, counts));
}

int knncf_update_bystander_predict(knncf_handle* h, int predictor, int32_t user, const int32_t* items, const double* ratings,
                                  int64_t n_ratings, const int32_t* others, const int32_t* pred_items, int64_t m, double* out) {
    return rows_single(h, bystander_predict_call({.family = QF_UPDATE, .items = items, .ratings = ratings, .pred_items = pred_items,
                                                       .user = user, .n_ratings = n_ratings, .m = m}, predictor, others, out));
}

int knncf_update_bystander_neighbors_batch(knncf_handle* h, const int32_t* users, const int64_t* offsets, const int32_t* items,
                                          const double* ratings, int64_t n_queries, const int64_t* row_offsets, const int32_t* others,
                                          int32_t cap, int32_t* ids, double* sims, int32_t* counts, int32_t* statuses) {
    return query_batch(h, bystander_neighbors_call({.family = QF_UPDATE, .users = users, .B = n_queries, .offsets = offsets,
                                                        .items = items, .ratings = ratings, .pred_offsets = row_offsets,
                                                        .statuses = statuses}, others, cap, ids, sims, counts));
}

int knncf_update_bystander_predict_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* offsets,
                                        const int32_t* items, const double* ratings, int64_t n_queries, const int64_t* row_offsets,
                                        const int32_t* others, const int32_t* pred_items, double* out, int32_t* statuses) {
    return query_batch(h, bystander_predict_call({.family = QF_UPDATE, .users = users, .B = n_queries, .offsets = offsets,
                                                      .items = items, .ratings = ratings, .pred_offsets = row_offsets,
                                                      .pred_items = pred_items, .statuses = statuses}, predictor, others, out));
}

// bystanders of revise queries: the same four calls for a user that also removes train rows (knncf.h "Bystanders of revise
// queries")
int knncf_revise_bystander_neighbors(knncf_handle* h, int32_t user, const int32_t* removed_items, int64_t n_removed,
                                     const int32_t* items, const double* ratings, int64_t n_ratings, const int32_t* others, int64_t m,
                                     int32_t cap, int32_t* ids, double* sims, int32_t* counts) {
    return rows_single(h, bystander_neighbors_call({.family = QF_REVISE, .items = items, .ratings = ratings, .removed_items = removed_items,
                                                    .user = user, .n_ratings = n_ratings, .n_removed = n_removed, .m = m},
                                                   others, cap, ids, sims, counts));
}

int knncf_revise_bystander_predict(knncf_handle* h, int predictor, int32_t user, const int32_t* removed_items, int64_t n_removed,
                                   const int32_t* items, const double* ratings, int64_t n_ratings, const int32_t* others,
                                   const int32_t* pred_items, int64_t m, double* out) {
    return rows_single(h, bystander_predict_call({.family = QF_REVISE, .items = items, .ratings = ratings, .removed_items = removed_items,
                                                  .pred_items = pred_items, .user = user, .n_ratings = n_ratings,
                                                  .n_removed = n_removed, .m = m}, predictor, others, out));
}

int knncf_revise_bystander_neighbors_batch(knncf_handle* h, const int32_t* users, const int64_t* removed_offsets,
                                           const int32_t* removed_items, const int64_t* offsets, const int32_t* items,
                                           const double* ratings, int64_t n_queries, const int64_t* row_offsets, const int32_t* others,
                                           int32_t cap, int32_t* ids, double* sims, int32_t* counts, int32_t* statuses) {
    return query_batch(h, bystander_neighbors_call({.family = QF_REVISE, .users = users, .B = n_queries, .offsets = offsets,
                                                    .items = items, .ratings = ratings, .removed_offsets = removed_offsets,
                                                    .removed_items = removed_items, .pred_offsets = row_offsets,
                                                    .statuses = statuses}, others, cap, ids, sims, counts));
}

int knncf_revise_bystander_predict_batch(knncf_handle* h, int predictor, const int32_t* users, const int64_t* removed_offsets,
                                         const int32_t* removed_items, const int64_t* offsets, const int32_t* items,
                                         const double* ratings, int64_t n_queries, const int64_t* row_offsets, const int32_t* others,
                                         const int32_t* pred_items, double* out, int32_t* statuses) {
    return query_batch(h, bystander_predict_call({.family = QF_REVISE, .users = users, .B = n_queries, .offsets = offsets,
                                                  .items = items, .ratings = ratings, .removed_offsets = removed_offsets,
                                                  .removed_items = removed_items, .pred_offsets = row_offsets,
                                                  .pred_items = pred_items, .statuses = statuses}, predictor, others, out));
}

// entered queries: the fitted users whose lists the fold-in query's user joins (knncf.h "Entered queries")
int knncf_query_entered(knncf_handle* h, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings, int32_t cap,
                        int32_t* out_users, double* out_sims, int32_t* out_pos, int32_t* out_displaced, int32_t* count) {
    return rows_single(h, entered_call({.family = QF_FOLD_IN, .items = items, .ratings = ratings, .out_pos = out_pos,
                                        .out_displaced = out_displaced, .user = user, .n_ratings = n_ratings}, cap, out_users, out_sims, count));
}

int knncf_query_entered_batch(knncf_handle* h, const int32_t* users, const int64_t* offsets, const int32_t* items,
                              const double* ratings, int64_t n_queries, int32_t cap, int32_t* out_users, double* out_sims,
                              int32_t* out_pos, int32_t* out_displaced, int32_t* counts, int32_t* statuses) {
    return query_batch(h, entered_call({.family = QF_FOLD_IN, .users = users, .B = n_queries, .offsets = offsets, .items = items,
                                        .ratings = ratings, .statuses = statuses, .out_pos = out_pos, .out_displaced = out_displaced},
                                       cap, out_users, out_sims, counts));
}

// the same question for an update query's user, which may be of the fit (knncf.h "Entered queries of update queries")
int knncf_update_entered(knncf_handle* h, int32_t user, const int32_t* items, const double* ratings, int64_t n_ratings, int32_t cap,
                         int32_t* out_users, double* out_sims, int32_t* out_pos, int32_t* out_prev, int32_t* out_other, int32_t* count) {
    return rows_single(h, entered_call({.family = QF_UPDATE, .items = items, .ratings = ratings, .out_pos = out_pos,
                                        .out_displaced = out_other, .out_prev = out_prev, .user = user, .n_ratings = n_ratings},
                                       cap, out_users, out_sims, count));
}

int knncf_update_entered_batch(knncf_handle* h, const int32_t* users, const int64_t* offsets, const int32_t* items,
                               const double* ratings, int64_t n_queries, int32_t cap, int32_t* out_users, double* out_sims,
                               int32_t* out_pos, int32_t* out_prev, int32_t* out_other, int32_t* counts, int32_t* statuses) {
    return query_batch(h, entered_call({.family = QF_UPDATE, .users = users, .B = n_queries, .offsets = offsets, .items = items,
                                        .ratings = ratings, .statuses = statuses, .out_pos = out_pos, .out_displaced = out_other,
                                        .out_prev = out_prev}, cap, out_users, out_sims, counts));
}

// the same question for a revise query's user, which may also remove train rows (knncf.h "Entered queries of revise queries")
int knncf_revise_entered(knncf_handle* h, int32_t user, const int32_t* removed_items, int64_t n_removed, const int32_t* items,
                         const double* ratings, int64_t n_ratings, int32_t cap, int32_t* out_users, double* out_sims, int32_t* out_pos,
                         int32_t* out_prev, int32_t* out_other, int32_t* count) {
    return rows_single(h, entered_call({.family = QF_REVISE, .items = items, .ratings = ratings, .removed_items = removed_items,
                                        .out_pos = out_pos, .out_displaced = out_other, .out_prev = out_prev, .user = user,
                                        .n_ratings = n_ratings, .n_removed = n_removed}, cap, out_users, out_sims, count));
}

int knncf_revise_entered_batch(knncf_handle* h, const int32_t* users, const int64_t* removed_offsets, const int32_t* removed_items,
                               const int64_t* offsets, const int32_t* items, const double* ratings, int64_t n_queries, int32_t cap,
                               int32_t* out_users, double* out_sims, int32_t* out_pos, int32_t* out_prev, int32_t* out_other,
                               int32_t* counts, int32_t* statuses) {
    return query_batch(h, entered_call({.family = QF_REVISE, .users = users, .B = n_queries, .offsets = offsets, .items = items,
                                        .ratings = ratings, .removed_offsets = removed_offsets, .removed_items = removed_items,
                                        .statuses = statuses, .out_pos = out_pos, .out_displaced = out_other, .out_prev = out_prev},
                                       cap, out_users, out_sims, counts));
}

int knncf_append(knncf_handle* h, const int32_t* users, const int32_t* items, const double* ratings, int64_t n, int64_t* n_carried,
                 int64_t* n_dropped, int32_t* dropped, int64_t dropped_cap) {
    return guarded(h, [&] { do_amend(h, nullptr, nullptr, 0, users, items, ratings, n, n_carried, n_dropped, dropped, dropped_cap); });
}

int knncf_remove_users(knncf_handle* h, const int32_t* users, int64_t n_users, int64_t* n_carried, int64_t* n_dropped, int32_t* dropped,
                       int64_t dropped_cap) {
    return guarded(h, [&] { do_amend(h, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, n_carried, n_dropped, dropped, dropped_cap, users, n_users); });
}

int knncf_amend(knncf_handle* h, const int32_t* removed_users, const int32_t* removed_items, int64_t n_removed, const int32_t* users,
                const int32_t* items, const double* ratings, int64_t n, int64_t* n_carried, int64_t* n_dropped, int32_t* dropped,
                int64_t dropped_cap) {
    return guarded(h, [&] {
        do_amend(h, removed_users, removed_items, n_removed, users, items, ratings, n, n_carried, n_dropped, dropped, dropped_cap);
    });
}

int knncf_neighbors_save(knncf_handle* h, const char* path) {
    return guarded(h, [&] { do_neighbors_save(h, path); });
}

int knncf_neighbors_load(knncf_handle* h, const char* path) {
    return guarded(h, [&] { do_neighbors_load(h, path); });
}

int knncf_mae_device(knncf_handle* h, int predictor, const int32_t* d_users, const int32_t* d_items,
                     const double* d_ratings, int64_t n, double* sum_abs_err, int64_t* count, double* d_pred) {
    return guarded(h, [&] {
        KN_REQUIRE(sum_abs_err && count && (n == 0 || d_ratings), KNNCF_E_INVALID, "bad arguments");
        run_predict(h, predictor, d_users, d_items, d_ratings, n, sum_abs_err, count, d_pred);
    });
}

int knncf_mae(knncf_handle* h, int predictor, const int32_t* users, const int32_t* items, const double* ratings,
              int64_t n, double* mae) {
    return guarded(h, [&] {
        KN_REQUIRE(mae && n >= 0 && (n == 0 || (users && items && ratings)), KNNCF_E_INVALID, "bad arguments");
        KN_REQUIRE(h->cfg.shard_count == 1, KNNCF_E_STATE, "sharded handle: use knncf_mae_device and all-reduce the partial sums");
        if (n == 0) { *mae = NAN; return; }  // 0.0 / 0 in applyAndMean :85
        h->t_users.ensure(n); h->t_items.ensure(n); h->t_ratings.ensure(n);
        KN_HIP(hipMemcpyAsync(h->t_users.p, users, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        KN_HIP(hipMemcpyAsync(h->t_items.p, items, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        KN_HIP(hipMemcpyAsync(h->t_ratings.p, ratings, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
        double s = 0.0;
        int64_t c = 0;
        run_predict(h, predictor, h->t_users.p, h->t_items.p, h->t_ratings.p, n, &s, &c, nullptr);
        *mae = s / (double)n;
    });
}

int knncf_mae_sweep_device(knncf_handle* h, const int32_t* ks, int32_t n_k, const int32_t* d_users, const int32_t* d_items,
                           const double* d_ratings, int64_t n, double* sum_abs_err, int64_t* count, double* d_pred) {
    return guarded(h, [&] {
        KN_REQUIRE(sum_abs_err && count, KNNCF_E_INVALID, "bad arguments");
        run_mae_sweep(h, ks, n_k, d_users, d_items, d_ratings, n, sum_abs_err, count, d_pred);
    });
}

int knncf_mae_sweep(knncf_handle* h, const int32_t* ks, int32_t n_k, const int32_t* users, const int32_t* items,
                    const double* ratings, int64_t n, double* maes, double* predictions) {
    return guarded(h, [&] {
        check_sweep_ks(ks, n_k);
        KN_REQUIRE(maes && n >= 0 && (n == 0 || (users && items && ratings)), KNNCF_E_INVALID, "bad arguments");
        KN_REQUIRE(h->cfg.shard_count == 1, KNNCF_E_STATE, "sharded handle: use knncf_mae_sweep_device and all-reduce the partial sums");
        require_fitted(h);
        KN_REQUIRE(h->cfg.similarity != KNNCF_SIM_ONE, KNNCF_E_UNSUPPORTED, "kNN predictor with similarityOne");
        if (n == 0) {  // 0.0 / 0 in applyAndMean :85
            for (int32_t q = 0; q < n_k; ++q) maes[q] = NAN;
            return;
        }
        h->t_users.ensure(n); h->t_items.ensure(n); h->t_ratings.ensure(n);
        KN_HIP(hipMemcpyAsync(h->t_users.p, users, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        KN_HIP(hipMemcpyAsync(h->t_items.p, items, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        KN_HIP(hipMemcpyAsync(h->t_ratings.p, ratings, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
        if (predictions) h->t_pred.ensure((size_t)n_k * n);
        std::vector<double> s(n_k);
        int64_t c = 0;
        run_mae_sweep(h, ks, n_k, h->t_users.p, h->t_items.p, h->t_ratings.p, n, s.data(), &c, predictions ? h->t_pred.p : nullptr);
        for (int32_t q = 0; q < n_k; ++q) maes[q] = s[q] / (double)n;
        if (predictions) {
            KN_HIP(hipMemcpyAsync(predictions, h->t_pred.p, (size_t)n_k * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            KN_HIP(hipStreamSynchronize(h->stream));
        }
    });
}

int knncf_shard_view_get(knncf_handle* h, knncf_shard_view* out) {
    return guarded(h, [&] {
        require_fitted(h, false);
        KN_REQUIRE(out, KNNCF_E_INVALID, "null out");
        Train& tr = h->tr;
        out->user_begin = tr.own_lo;
        out->user_end = tr.own_hi;
        out->nnz_begin = tr.own_p0;  // (read back once by prep_fit: no device round trip per view)
        out->nnz_end = tr.own_p1;
        out->num_users = tr.U;
        out->num_ratings = tr.n;
        out->d_user_avg = tr.user_avg.p;
        out->d_user_norm = tr.user_norm.p;
        out->d_dev = tr.s_dev.p;
        out->d_pre = tr.s_pre.p;
    });
}

int knncf_shard_commit(knncf_handle* h) {
    return guarded(h, [&] {
        require_fitted(h, false);
        if (h->committed) return;
        Stage s(h, &h->tm.prep_ms);
        if (h->cfg.shard_count > 1) prep_complete_rows(h->tr, h->prep, h->stream);
        prep_commit(h->tr, h->prep, h->stream);
        h->committed = true;
        h->h_uavg.clear();  // (the exchange before the commit wrote the other shards' means)
    });
}

int knncf_get_timings(const knncf_handle* h, knncf_timings* out) {
    if (!h || !out) return KNNCF_E_INVALID;
    *out = h->tm;
    return KNNCF_OK;
}

int knncf_reset_timings(knncf_handle* h) {
    if (!h) return KNNCF_E_INVALID;
    h->tm = knncf_timings{};
    return KNNCF_OK;
}

int knncf_reset_neighbors(knncf_handle* h) {
    return guarded(h, [&] {
        require_fitted(h, false);
        reset_neighbors(h);
    });
}

int knncf_set_k(knncf_handle* h, int32_t k) {
    return guarded(h, [&] {
        KN_REQUIRE(k >= 0, KNNCF_E_INVALID, "negative k");
        h->cfg.k = k;
        if (h->fitted) reset_neighbors(h);
    });
}

}  // extern "C"
