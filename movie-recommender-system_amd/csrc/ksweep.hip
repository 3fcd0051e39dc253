// ksweep.hip — the kNN prediction of every test row at many neighbourhood sizes from ONE neighbour table
// (predict/kNN.scala:73: the MAE at k = 10, 30, ..., 943).
//
// getNeighbors :603-616 sorts every other user by similarity (stable) and takes k, so the list at k is the first k entries
// of the list at kmax, and getSimilarity(train, k, sim)(u, v) :634-648 is the kmax similarity of v when v's position in u's
// list is below k, else 0.  The prediction of row (u, i) at k is therefore the left fold, in file order, over the raters of
// i whose position in u's reference-order list is below k (terms of the other raters add +-0.0: identities).
//
// Rows are sorted by item and a workgroup keeps the item's rater bitmap + rank prefixes in LDS, as k_predict_knn_items
// does (or, without bitmaps, probes the item's rater list in global memory by binary search).  A wave takes one row: it
// streams u's reference-order list in 64-wide trips; every match is stored with its file row t and its list position j.
// The matches are ordered by t (rank by counting), then lane q folds them for k = ks[q], skipping j >= ks[q]: each k is
// its own serial fp64 fold in file order — the same additions in the same order as the one-k kernels.
#include <math.h>

#include "knn_terms.h"

namespace knncf {

static constexpr int SWEEP_CHUNK = 64;  // test rows per workgroup
static constexpr int SWEEP_SLOTS = 2048;  // match slots per workgroup (CAP x WAVES): 24 B each, 48 KiB

struct SweepArgs {
    const double* user_avg;
    double global_avg;
    int32_t own_lo, own_hi;
    ProbeArgs P;  // (the lists in reference order; ib_words = 0 when the bitmaps are not used)
    const int32_t* ks;  // [n_k] ascending
    int32_t n_k;
};

// CAP: match slots per wave (>= kcap), BITS: the item's rater bitmap sits in LDS (dynamic shared memory)
template <int CAP, int WAVES, bool BITS>
__global__ void __launch_bounds__(WAVES * 64) k_predict_knn_sweep(SweepArgs A, int64_t n, int64_t stride, const int32_t* __restrict__ du,
                                                              const int32_t* __restrict__ di, const double* __restrict__ ratings,
                                                              const uint32_t* __restrict__ order, double* __restrict__ pred,
                                                              double* __restrict__ abs_err, uint8_t* __restrict__ owned,
                                                              int unknown_owned) {
    static_assert(CAP * WAVES <= SWEEP_SLOTS && CAP % 64 == 0 && CAP <= 65536, "match slots");
    constexpr int CHUNK = SWEEP_CHUNK;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ __attribute__((aligned(16))) uint32_t m_t[WAVES][CAP];  // file row of each match (slot order)
    __shared__ double m_dev[WAVES][CAP];
    __shared__ double m_sim[WAVES][CAP];
    __shared__ uint16_t m_j[WAVES][CAP];     // its position in u's list
    __shared__ uint16_t m_perm[WAVES][CAP];  // slot of the match of file-order rank c
    __shared__ int64_t s_row[CHUNK];
    __shared__ int32_t s_u[CHUNK], s_i[CHUNK], s_cnt[CHUNK];
    __shared__ uint32_t s_rb[CHUNK], s_len[CHUNK];
    __shared__ double s_ua[CHUNK], s_p[CHUNK];
    __shared__ uint8_t s_mine[CHUNK], s_active[CHUNK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * CHUNK;
    if (r0 >= n) return;
    const int nr = (int)min((int64_t)CHUNK, n - r0);
    const int n_k = A.n_k;
    const int32_t my_k = lane < n_k ? A.ks[lane] : 0;  // lane q folds for k = ks[q]
    const int ibw = (int)A.P.ib_words;
    const int ibw2 = (ibw + 1) >> 1;
    // as in k_predict_knn_items: the rank prefix of every second bitmap word (the odd word adds its even neighbour's popcount)
    unsigned long long* bits = reinterpret_cast<unsigned long long*>(smem);  // [2 * ibw2]
    uint32_t* rnk = reinterpret_cast<uint32_t*>(bits + 2 * ibw2);             // [ibw2]
    if ((int)threadIdx.x < nr) {
        const int l = threadIdx.x;
        const int64_t row = order[r0 + l];
        const int32_t u = du[row], i = di[row];
        const bool mine = (u < 0) ? (unknown_owned != 0) : (u >= A.own_lo && u < A.own_hi);
        double ua = -1.0;  // usersAvgValue.getOrElse(u, -1.0) :572
        int32_t cnt = 0;
        uint32_t rb = 0, len = 0;
        if (u >= 0) { ua = A.user_avg[u]; cnt = A.P.nbr_cnt[u]; }
        if (i >= 0) { rb = (uint32_t)A.P.i_ptr[i]; len = (uint32_t)A.P.i_ptr[i + 1] - rb; }
        s_row[l] = row; s_u[l] = u; s_i[l] = i; s_cnt[l] = cnt; s_rb[l] = rb; s_len[l] = len; s_ua[l] = ua;
        s_p[l] = (ua < 0.0) ? A.global_avg : combine(ua, 0.0);  // unknown user / no rater: den = 0 -> 0.0 :527-529
        s_mine[l] = mine ? 1 : 0;
        s_active[l] = (mine && ua >= 0.0 && i >= 0 && cnt > 0 && len > 0) ? 1 : 0;
    }
    __syncthreads();
    uint32_t* mt = m_t[wave];
    double* md = m_dev[wave];
    double* ms = m_sim[wave];
    uint16_t* mj = m_j[wave];
    uint16_t* mp = m_perm[wave];
    int ra = 0;
    while (ra < nr) {  // runs of rows of one item (block-uniform)
        const int32_t item = s_i[ra];
        int rbn = ra + 1;
        bool any = s_active[ra] != 0;
        while (rbn < nr && s_i[rbn] == item) { any = any || s_active[rbn] != 0; ++rbn; }
        if (any) {
            if (BITS) {
                const unsigned long long* gb = A.P.item_bits + (int64_t)item * ibw;
                const uint32_t* gr = A.P.item_rank + (int64_t)item * ibw;
                for (int w = threadIdx.x; w < 2 * ibw2; w += WAVES * 64) bits[w] = w < ibw ? gb[w] : 0ull;
                for (int j = threadIdx.x; j < ibw2; j += WAVES * 64) rnk[j] = gr[2 * j];
                __syncthreads();
            }
            for (int r = ra + wave; r < rbn; r += WAVES) {  // one row per wave and trip
                if (!s_active[r]) continue;  // (wave-uniform)
                const int32_t u = s_u[r];
                const int32_t cnt = s_cnt[r];
                const uint32_t rb = s_rb[r], len = s_len[r];
                const int32_t* lid = A.P.nbr_idx + (int64_t)u * A.P.kcap;
                const double* lsim = A.P.nbr_sim + (int64_t)u * A.P.kcap;
                int32_t total = 0;
                for (int32_t j0 = 0; j0 < cnt; j0 += 64) {  // u's list in reference order: position j = rank in it
                    const int32_t j = j0 + lane;
                    const bool have = j < cnt;
                    const uint32_t x = have ? (uint32_t)lid[j] : 0u;
                    bool f;
                    uint32_t q;  // the match's entry in the item's rater list
                    if (BITS) {
                        f = lds_pair_probe(bits, rnk, x, 0u, q) && have;
                    } else {
                        uint32_t lo = 0, hi = have ? len : 0u;
                        while (lo < hi) {
                            const uint32_t mid = (lo + hi) >> 1;
                            if ((uint32_t)A.P.it_user[rb + mid] < x) lo = mid + 1;
                            else hi = mid;
                        }
                        f = have && lo < len && (uint32_t)A.P.it_user[rb + lo] == x;
                        q = lo;
                    }
                    const unsigned long long hit = __ballot(f);
                    if (f) {
                        const int32_t slot = total + lanes_below(hit);
                        mt[slot] = A.P.it_t[rb + q];
                        md[slot] = A.P.it_dev[rb + q];
                        ms[slot] = lsim[j];
                        mj[slot] = (uint16_t)j;
                    }
                    total += __popcll(hit);
                }
                if (total == 0) continue;  // no neighbour rated the item: every k predicts the user's mean (preset)
                // order the matches by training file row (the order of ratedI(i) :508-517): rank by counting (the file rows of
                // one item's ratings are distinct); LDS broadcast reads, 4 keys per read
                pad_file_rows(mt, total, lane);
                const uint4* keys4 = reinterpret_cast<const uint4*>(mt);
                const int32_t n4 = (total + 3) >> 2;
                for (int32_t s0 = 0; s0 < total; s0 += 64) {
                    const int32_t s = s0 + lane;
                    const uint32_t key = s < total ? mt[s] : 0u;
                    uint32_t rank = 0;
                    for (int32_t c = 0; c < n4; ++c) {
                        const uint4 kq = keys4[c];
                        rank += (uint32_t)(kq.x < key) + (uint32_t)(kq.y < key) + (uint32_t)(kq.z < key) + (uint32_t)(kq.w < key);
                    }
                    if (s < total) mp[rank] = (uint16_t)s;
                }
                wave_sync();
                // lane q: the fold at k = ks[q] over the matches of position < k, in file order
                double num = 0.0, den = 0.0;
                for (int32_t c = 0; c < total; ++c) {
                    const int32_t s = mp[c];
                    const double sc = ms[s];
                    const double dv = md[s];
                    if ((int32_t)mj[s] < my_k) {
                        num = num + dv * sc;
                        den = den + fabs(sc);
                    }
                }
                wave_sync();  // (the buffers are refilled by the wave's next row)
                if (lane < n_k) {
                    const double wsd = (den > 0) ? num / den : 0.0;
                    const double p = combine(s_ua[r], wsd);
                    const int64_t row = s_row[r];
                    const int64_t cell = (int64_t)lane * stride + row;
                    if (pred) pred[cell] = p;
                    abs_err[cell] = ratings ? fabs(ratings[row] - p) : 0.0;
                }
                if (lane == 0) s_active[r] = 2;  // written: the tail below leaves it alone
            }
            __syncthreads();  // the bitmap is overwritten by the next run; s_active of the run is final
        }
        ra = rbn;
    }
    __syncthreads();
    // every (row, k) not written by a fold: the preset prediction, or nothing for another shard's row
    for (int e = threadIdx.x; e < nr * n_k; e += WAVES * 64) {
        const int l = e / n_k, q = e - l * n_k;
        if (s_active[l] == 2) continue;
        const int64_t row = s_row[l];
        const int64_t cell = (int64_t)q * stride + row;
        if (s_mine[l]) {
            const double p = s_p[l];
            if (pred) pred[cell] = p;
            abs_err[cell] = ratings ? fabs(ratings[row] - p) : 0.0;
        } else {
            abs_err[cell] = 0.0;
        }
    }
    for (int l = threadIdx.x; l < nr; l += WAVES * 64) owned[s_row[l]] = s_mine[l];
}

static size_t sweep_bitmap_lds(int64_t ib_words) {
    const size_t ibw2 = (size_t)(ib_words + 1) / 2;
    return ibw2 * 16 + ibw2 * 4;
}

void launch_predict_sweep(const Train& tr, NeighborTable& nt, const int32_t* d_ks, int32_t n_k, int64_t n, int64_t n_total,
                          const int32_t* d_du, const int32_t* d_di, const double* d_ratings, const uint32_t* d_order,
                          double* d_pred, double* d_abs_err, uint8_t* d_owned, bool unknown_users_owned, hipStream_t st) {
    if (n <= 0) return;
    KN_REQUIRE(n_k >= 1 && n_k <= 64, KNNCF_E_INVALID, "sweep: 1 .. 64 values of k");
    KN_REQUIRE(nt.kcap <= SWEEP_SLOTS, KNNCF_E_UNSUPPORTED, "sweep: more than 2048 neighbours");
    SweepArgs A{};
    A.user_avg = tr.user_avg.p; A.global_avg = tr.global_avg;
    A.own_lo = tr.own_lo; A.own_hi = tr.own_hi;
    A.P = probe_args(tr, nt, /*by_id=*/false, st);
    A.ks = d_ks; A.n_k = n_k;
    // the item's bitmap in LDS when it is built and small enough (the bound of the item-grouped one-k kernel)
    const bool bits = tr.ib_words > 0 && lds_bitmap_fits(tr.ib_words);
    if (!bits) A.P.ib_words = 0;
    const unsigned blocks = (unsigned)ceil_div(n, SWEEP_CHUNK);
    const size_t smem = bits ? sweep_bitmap_lds(tr.ib_words) : 0;
    const int uo = unknown_users_owned ? 1 : 0;
#define KN_LAUNCH_SWEEP(CAPV, WV)                                                                                              \
    do {                                                                                                                       \
        KN_TRACE_DISPATCH("sweep CAP=%d bits=%d", CAPV, bits ? 1 : 0);                                                         \
        if (bits) {                                                                                                            \
            KN_HIP(hipFuncSetAttribute((const void*)k_predict_knn_sweep<CAPV, WV, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)); \
            k_predict_knn_sweep<CAPV, WV, true><<<blocks, WV * 64, smem, st>>>(A, n, n_total, d_du, d_di, d_ratings, d_order, d_pred, d_abs_err, d_owned, uo); \
        } else {                                                                                                               \
            k_predict_knn_sweep<CAPV, WV, false><<<blocks, WV * 64, 0, st>>>(A, n, n_total, d_du, d_di, d_ratings, d_order, d_pred, d_abs_err, d_owned, uo); \
        }                                                                                                                      \
    } while (0)
    if (nt.kcap <= 512) KN_LAUNCH_SWEEP(512, 4);
    else if (nt.kcap <= 1024) KN_LAUNCH_SWEEP(1024, 2);
    else KN_LAUNCH_SWEEP(2048, 1);
#undef KN_LAUNCH_SWEEP
    KN_HIP(hipGetLastError());
}

}  // namespace knncf
