// foldin.hip — fold-in kNN queries: the neighbourhood, predictions and recommendations of users that are not in the
// fitted training set, given their ratings, without a refit (DESIGN.md "Fold-in queries").
//
// The answers are those of the reference on aug = train ++ query rows (data.union(personal), recommend/Recommender.scala:68)
// with fresh closures whose first evaluation is the query user's: adding the user changes no existing user's mean,
// deviations or preprocessed ratings (usersAvg :113, preprocessedRating :470-481), and (allUsers - q).toSeq is the
// train user order.  So only the query's own quantities are computed here; everything else is read from the fit.
//
// There is one path.  A chunk of C <= QB_MAX_CHUNK independent queries goes through the stages below, every stage as ONE
// launch (or one sort) over the chunk; a single call is a chunk of one.  Rows of the chunk are concatenated in slot order:
// slot b owns rows [qo[b], qo[b + 1]).  Nothing of one slot enters another, and each slot's arithmetic and its order do not
// depend on C, so a query's answer is the same bit for bit in whatever chunk it travels.
//   k_qb_seed_keys / sort / k_qb_seed   (update queries only) the rows of a slot whose user is in the fit: the user's train
//                                       rows in file order, then the additional rows
//   k_qb_mark / k_qb_seed_keys_rv / sort / k_qb_seed_rv   (revise queries with removals, instead) the removed items are
//                                       found in the user's train row and marked; the marked rows sort behind the slot's
//                                       live rows, and the slot takes its declared number of rows from the front
//   k_qb_gone (after k_qb_prep) / k_qb_gone_rated (after k_qb_pred)   (revise) removed items that nobody else rates have
//                                       left aug: not candidates, counted with the slot's known items
//   k_qb_keys / sort (slot, trie key) / k_qb_prep / k_qb_rank / k_qb_scatter   query prep, one workgroup per slot: dense
//                                       items, mean, deviations, hash-ordered norm, preprocessed values, a dense-item
//                                       bitmap with rank prefixes
//   k_qb_transpose + k_query_sim_dual   (C >= QB_DUAL_MIN) every train row read once for the whole chunk, lane b = slot b
//   k_query_sim per slot                (C <  QB_DUAL_MIN) one exact fp64 similarity per train user (one streaming pass of s_col)
//   (bystander_place of bystander.hip)  (a bystander chunk with a changer of the fit) S(v, c) on aug over the train value
//   fallback keys over [C][U] / sort 64 bits / stable sort by slot / k_qb_write   top-k (similarity desc, dense user asc);
//                                       k_qb_mask_self keys a fitted user's own cell behind every other: (allUsers - u) :608
//   k_qb_offsets / k_qb_gather / sort (slot * I + item, file row) / k_q_fold      the neighbours' ratings grouped by (item,
//                                       file row): the left folds of weightedSumDeviation :504-548
//   k_qb_pred                           predictor :568-585 for every (slot, dense item)
//   k_qb_reco_keys / sort 64 bits / stable sort by slot / k_qb_take               recommendations
//   k_qb_explain                        (knncf_*_explain*) the elements of those folds for requested (slot, item) rows: one
//                                       wave per row reads the row's segment of the sorted list that k_q_fold folded
//   k_qb_self_keys / sort / k_qb_self_sim / k_qb_sim_transpose / k_qb_fold_all / k_qb_pred<false> / k_qb_pick_all
//                                       (KNNCF_PRED_PERSONALIZED, instead of everything from the top-k to k_qb_pred) S(u, u), the
//                                       similarities side by side, one fold per (slot, item) over ALL raters of the item
//   k_qb_explain_all                    (knncf_*_explain_personalized*) the terms of those folds for requested (slot, item) rows:
//                                       one wave per row walks the item's raters, the slot's own term among them, and picks the
//                                       cap heaviest with the steps of explain_select.h
#include <math.h>

#include <algorithm>

#include "explain_select.h"
#include "qb_helpers.h"

namespace knncf {

// neighbours.hip
void launch_fallback_keys(int32_t U, const double* d_exact, uint64_t* d_keys, uint32_t* d_vals, hipStream_t st);

static constexpr int TPB = 256;
// query bitmap + rank prefixes held in LDS by k_query_sim up to this many words (16 B each: 64 KB = 262 144 items);
// beyond that the waves probe them in global memory (L2-resident)
static constexpr int64_t SIM_LDS_WORDS = 4096;
// the predictor answers aug's global average for a user mean < 0 (:571-574): not served by a fold-in query
static constexpr uint32_t ST_NEG_MEAN = QUERY_ST_NEG_MEAN;
// revise queries: a removed item that is no train item of the user / that is listed twice
static constexpr uint32_t ST_RM_UNRATED = QUERY_ST_RM_UNRATED, ST_RM_TWICE = QUERY_ST_RM_TWICE;

// exact similarity of q (first argument, fresh closure: it owns every pair) against every train user, one wave per
// user: the wave reads the user's row 64 entries at a time (coalesced), probes the query bitmap, and folds the products of
// the matches left in row order = dense item order = q's trie order (q with > 4 ratings).  A query of <= 4 ratings
// iterates in its given order (Set1..Set4): the <= 4 products are kept by given position and folded at the end.
// Jaccard counts the matches: |I(q) & I(v)| / (|I(q)| + |I(v)| - |I(q) & I(v)|) :446-463.
template <bool IN_LDS>
__global__ void __launch_bounds__(TPB) k_query_sim(int32_t U, int32_t nq, bool jaccard, const int64_t* __restrict__ u_ptr,
                                                   const int32_t* __restrict__ s_col, const double* __restrict__ s_pre,
                                                   int64_t W, const unsigned long long* __restrict__ g_bits,
                                                   const int64_t* __restrict__ g_rank, const double* __restrict__ pre_d,
                                                   const int32_t* __restrict__ given_d, double* __restrict__ out) {
    extern __shared__ unsigned long long lds[];
    const unsigned long long* bits = g_bits;
    const int64_t* rank = g_rank;
    if (IN_LDS) {
        unsigned long long* lb = lds;
        int64_t* lr = (int64_t*)(lds + W);
        for (int64_t w = threadIdx.x; w < W; w += blockDim.x) {
            lb[w] = g_bits[w];
            lr[w] = g_rank[w];
        }
        __syncthreads();
        bits = lb;
        rank = lr;
    }
    const bool small = nq <= 4;
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (TPB / 64);
    for (int64_t v = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); v < U; v += waves) {
        const int64_t b = u_ptr[v], e = u_ptr[v + 1];
        double s = 0.0, x0 = 0.0, x1 = 0.0, x2 = 0.0, x3 = 0.0;
        uint32_t found = 0;
        int64_t both = 0;
        for (int64_t base = b; base < e; base += 64) {
            const int64_t p = base + lane;
            int32_t c = 0;
            bool hit = false;
            if (p < e) {
                c = s_col[p];
                hit = (bits[c >> 6] >> (c & 63)) & 1ull;
            }
            unsigned long long mask = __ballot(hit);
            if (jaccard) {
                both += __popcll(mask);
                continue;
            }
            double prod = 0.0;
            int32_t g = 0;
            if (hit) {
                const int32_t r = bit_rank(bits, rank, c);
                prod = pre_d[r] * s_pre[p];
                if (small) g = given_d[r];
            }
            while (mask) {
                const int l = __ffsll((long long)mask) - 1;
                const double xv = __shfl(prod, l);
                if (small) {
                    const int gg = __shfl(g, l);
                    if (gg == 0) x0 = xv;
                    else if (gg == 1) x1 = xv;
                    else if (gg == 2) x2 = xv;
                    else x3 = xv;
                    found |= 1u << gg;
                } else {
                    s = s + xv;
                }
                mask &= mask - 1ull;
            }
        }
        if (jaccard) {
            s = (double)both / (double)((int64_t)nq + (e - b) - both);
        } else if (small) {
            if (found & 1u) s = s + x0;
            if (found & 2u) s = s + x1;
            if (found & 4u) s = s + x2;
            if (found & 8u) s = s + x3;
        }
        if (lane == 0) out[v] = s;
    }
}

// weightedSumDeviation :517-545 per item: num += dev * s, den += |s| over the item's neighbour ratings in file order
// (the other raters add dev * 0.0 and 0.0, which change neither sum: num starts at +0.0 and never becomes -0.0)
__global__ void k_q_fold(int64_t E, const uint64_t* __restrict__ key, const uint32_t* __restrict__ val,
                         const double* __restrict__ edev, const double* __restrict__ esim, double* __restrict__ num,
                         double* __restrict__ den) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= E) return;
    const uint32_t item = (uint32_t)(key[p] >> 32);
    if (p > 0 && (uint32_t)(key[p - 1] >> 32) == item) return;
    double a = 0.0, d = 0.0;
    for (int64_t x = p; x < E && (uint32_t)(key[x] >> 32) == item; ++x) {
        const uint32_t t = val[x];
        a = a + edev[t] * esim[t];
        d = d + fabs(esim[t]);
    }
    num[item] = a;
    den[item] = d;
}

static PerDeviceState g_sim_lds;

static int32_t table_cells(const Train& tr) { return (tr.u_table_n > 0 && tr.i_table_n > 0) ? tr.i_table_n : 0; }

// ---- update queries (knncf_update_*): the query user may be in the fit.  self[b] = its dense index, -1 when it is not.
// (qb_take of qb_helpers.h: the neighbours a slot returns.)
// Chunk row j of slot b is row r = j - qo[b] of the slot: r < (train row length of self[b]) is the user's train entry at
// position u_ptr[self] + r, the others are the additional rows in their given order.  The key orders a slot's rows as aug
// holds them: train rows by file row (s_t), then the additional ones.
__global__ void k_qb_seed_keys(int64_t n, int32_t C, const int64_t* __restrict__ qo, const int32_t* __restrict__ self,
                               const int64_t* __restrict__ u_ptr, const uint32_t* __restrict__ s_t, uint64_t* __restrict__ key,
                               uint32_t* __restrict__ val) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t b = qb_slot(qo, C, j), sd = self[b];
    const int64_t r = j - qo[b], p0 = sd >= 0 ? u_ptr[sd] : 0, tl = sd >= 0 ? u_ptr[sd + 1] - p0 : 0;
    const uint64_t in_slot = r < tl ? (uint64_t)s_t[p0 + r] : ((1ull << 32) | (uint64_t)(r - tl));
    key[j] = ((uint64_t)(uint32_t)b << 33) | in_slot;
    val[j] = (uint32_t)j;
}

// items / ratings of the chunk in that order: raw item iid[s_col], rating s_rating of a train entry; the additional rows
// (add_* rows [ao[b], ao[b + 1]) of slot b) behind them
__global__ void k_qb_seed(int64_t n, int32_t C, const int64_t* __restrict__ qo, const int64_t* __restrict__ ao,
                          const int32_t* __restrict__ self, const int64_t* __restrict__ u_ptr, const int32_t* __restrict__ s_col,
                          const double* __restrict__ s_rating, const int32_t* __restrict__ iid, const int32_t* __restrict__ add_items,
                          const double* __restrict__ add_ratings, const uint32_t* __restrict__ sval, int32_t* __restrict__ items,
                          double* __restrict__ ratings) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t b = qb_slot(qo, C, j), sd = self[b];
    const int64_t r = (int64_t)sval[j] - qo[b], p0 = sd >= 0 ? u_ptr[sd] : 0, tl = sd >= 0 ? u_ptr[sd + 1] - p0 : 0;
    if (r < tl) {
        items[j] = iid[s_col[p0 + r]];
        ratings[j] = s_rating[p0 + r];
    } else {
        items[j] = add_items[ao[b] + (r - tl)];
        ratings[j] = add_ratings[ao[b] + (r - tl)];
    }
}

// ---- revise queries (knncf_revise_*): an update query that also REMOVES train rows of the user.  rm_items rows [ro[b],
// ro[b + 1]) are the raw items slot b drops.  The slot's SOURCE rows [so[b], so[b + 1]) are all its train rows followed by
// its additional rows; the host declares qo[b + 1] - qo[b] = source rows - removed items, which is right when every removal
// names a different train row of the user.
// One thread per removed item: raw -> dense item through the fit's tables (as k_qb_keys), binary search in the user's s_col
// row (sorted by dense item), mark[source row] = 1.  Not found: ST_RM_UNRATED; marked before: ST_RM_TWICE.  gone[j] = the
// dense item when the user was its only train rater (it may leave aug: k_qb_gone), else -1.
__global__ void k_qb_mark(int64_t m, int32_t C, const int64_t* __restrict__ ro, const int64_t* __restrict__ so,
                          const int32_t* __restrict__ self, const int32_t* __restrict__ rm_items,
                          const int32_t* __restrict__ i_table, int32_t i_cells, const uint32_t* __restrict__ ikeys, int32_t I,
                          const int64_t* __restrict__ u_ptr, const int32_t* __restrict__ s_col, const int64_t* __restrict__ i_ptr,
                          uint32_t* __restrict__ mark, int32_t* __restrict__ rm_slot, int32_t* __restrict__ gone,
                          long long* __restrict__ info) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const int32_t b = qb_slot(ro, C, j), sd = self[b], it = rm_items[j];
    rm_slot[j] = b;
    gone[j] = -1;
    int32_t d;
    if (i_cells > 0) d = (it >= 0 && it < i_cells) ? i_table[it] : -1;
    else d = dense_lookup(ikeys, I, it);
    int64_t at = -1;
    if (sd >= 0 && d >= 0) {
        const int64_t p0 = u_ptr[sd];
        int64_t lo = p0, hi = u_ptr[sd + 1];
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (s_col[mid] < d) lo = mid + 1;
            else hi = mid;
        }
        if (lo < u_ptr[sd + 1] && s_col[lo] == d) at = lo - p0;
    }
    unsigned long long* st = (unsigned long long*)(info + 4 * b);
    if (at < 0) {
        atomicOr(st, (unsigned long long)ST_RM_UNRATED);
    } else if (atomicExch(mark + so[b] + at, 1u) != 0u) {
        atomicOr(st, (unsigned long long)ST_RM_TWICE);
    } else if (i_ptr[d + 1] - i_ptr[d] == 1) {
        gone[j] = d;
    }
}

// k_qb_seed_keys over the SOURCE rows: a marked train row gets the bit above the in-slot order, so a slot's rows sort as
// [live train rows by file row, additional rows, dropped train rows]
__global__ void k_qb_seed_keys_rv(int64_t ns, int32_t C, const int64_t* __restrict__ so, const int32_t* __restrict__ self,
                                  const int64_t* __restrict__ u_ptr, const uint32_t* __restrict__ s_t,
                                  const uint32_t* __restrict__ mark, uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ns) return;
    const int32_t b = qb_slot(so, C, j), sd = self[b];
    const int64_t r = j - so[b], p0 = sd >= 0 ? u_ptr[sd] : 0, tl = sd >= 0 ? u_ptr[sd + 1] - p0 : 0;
    const uint64_t in_slot = r < tl ? (uint64_t)s_t[p0 + r] : ((1ull << 32) | (uint64_t)(r - tl));
    const uint64_t dropped = (r < tl && mark[j] != 0u) ? 1ull : 0ull;
    key[j] = ((uint64_t)(uint32_t)b << 34) | (dropped << 33) | in_slot;
    val[j] = (uint32_t)j;
}

// k_qb_seed for chunk row j of slot b: the (j - qo[b])-th of the slot's sorted source rows.  At most (removed items) rows
// of a slot are marked, so the slot's first qo[b + 1] - qo[b] sorted rows are live ones whatever the removals were, and
// they lie inside [so[b], so[b + 1]): a slot with a bad removal (its status bit is set) reads its own rows and writes its
// own extent only.
__global__ void k_qb_seed_rv(int64_t n, int32_t C, const int64_t* __restrict__ qo, const int64_t* __restrict__ so,
                             const int64_t* __restrict__ ao, const int32_t* __restrict__ self, const int64_t* __restrict__ u_ptr,
                             const int32_t* __restrict__ s_col, const double* __restrict__ s_rating, const int32_t* __restrict__ iid,
                             const int32_t* __restrict__ add_items, const double* __restrict__ add_ratings,
                             const uint32_t* __restrict__ sval, int32_t* __restrict__ items, double* __restrict__ ratings) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t b = qb_slot(qo, C, j), sd = self[b];
    const int64_t r = (int64_t)sval[so[b] + (j - qo[b])] - so[b], p0 = sd >= 0 ? u_ptr[sd] : 0, tl = sd >= 0 ? u_ptr[sd + 1] - p0 : 0;
    if (r < tl) {
        items[j] = iid[s_col[p0 + r]];
        ratings[j] = s_rating[p0 + r];
    } else {
        items[j] = add_items[ao[b] + (r - tl)];
        ratings[j] = add_ratings[ao[b] + (r - tl)];
    }
}

// after k_qb_prep: a removed item whose only train rater was the user has left aug unless an additional row gives it again
// (its bit of the slot's bitmap).  Such an item is no member of ratings.map(_.item).toSet :667: info[4 b + 1] counts it
// with the slot's known items (k_qb_take and the host take I - info[4 b + 1] candidates), gone[j] keeps it for k_qb_gone_rated
__global__ void k_qb_gone(int64_t m, int64_t W, const int32_t* __restrict__ rm_slot, int32_t* __restrict__ gone,
                          const unsigned long long* __restrict__ bits, long long* __restrict__ info) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const int32_t d = gone[j];
    if (d < 0) return;
    const int32_t b = rm_slot[j];
    if ((bits[(int64_t)b * W + (d >> 6)] >> (d & 63)) & 1ull) gone[j] = -1;
    else atomicAdd((unsigned long long*)(info + 4 * b + 1), 1ull);
}

// after k_qb_pred: the items that left aug sort with the rated ones, behind every candidate
__global__ void k_qb_gone_rated(int64_t m, int32_t I, const int32_t* __restrict__ rm_slot, const int32_t* __restrict__ gone,
                                uint8_t* __restrict__ rated) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const int32_t d = gone[j];
    if (d >= 0) rated[(int64_t)rm_slot[j] * I + d] = 1;
}

// the user's own cell of [C][U] gets the last key of all (the bit pattern no similarity has), so it sorts behind every other
// user of its slot whatever s(u, u) is, and the first min(k, U - 1) of the slot are getNeighbors' (allUsers - u) :608
__global__ void k_qb_mask_self(int32_t C, int32_t U, const int32_t* __restrict__ self, uint64_t* __restrict__ key) {
    const int32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < C && self[b] >= 0) key[(int64_t)b * U + self[b]] = ~0ull;
}

// raw -> dense item through the fit's tables (dense_lookup beyond them); key of the norm's fold order: the slot, then the
// trie order of the (q, item) tuple hash (usersWeights :474, N4).  tuple_trie_key(q, .) is a bijection of the item id, so two
// rows of a slot have equal keys only when they repeat an item: after the sort, equal neighbours are the duplicates.
__global__ void k_qb_keys(int64_t n, int32_t C, const int64_t* __restrict__ qo, const int32_t* __restrict__ users,
                          const int32_t* __restrict__ items, const int32_t* __restrict__ i_table, int32_t i_cells,
                          const uint32_t* __restrict__ ikeys, int32_t I, int32_t* __restrict__ slot, int32_t* __restrict__ di,
                          uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t b = qb_slot(qo, C, j);
    const int32_t it = items[j];
    int32_t d;
    if (i_cells > 0) d = (it >= 0 && it < i_cells) ? i_table[it] : -1;
    else d = dense_lookup(ikeys, I, it);
    slot[j] = b;
    di[j] = d;
    key[j] = ((uint64_t)(uint32_t)b << 32) | (uint64_t)tuple_trie_key(users[b], it);
    val[j] = (uint32_t)j;
}

// one workgroup per slot b: mean (left fold in the given order, usersAvg :113), deviations (computeNormalizeDeviation
// :155-169), norm (sqrt of the left fold of dev^2 in tuple-hash order), preprocessed ratings, the bitmap of the known items.
// info[4 b] |= status bits, info[4 b + 1] = known items; scal[2 b] = mean, scal[2 b + 1] = norm
__global__ void k_qb_prep(const int64_t* __restrict__ qo, const double* __restrict__ r, const uint64_t* __restrict__ skey,
                          const uint32_t* __restrict__ sval, const int32_t* __restrict__ di, int64_t W, double* __restrict__ dev,
                          double* __restrict__ pre, unsigned long long* __restrict__ bits, long long* __restrict__ info,
                          double* __restrict__ scal) {
    __shared__ double s_avg, s_norm;
    __shared__ int32_t s_known;
    const int32_t b = blockIdx.x;
    const int64_t o = qo[b];
    const int32_t n = (int32_t)(qo[b + 1] - o);
    bits += (int64_t)b * W;
    info += 4 * b;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int32_t j = 0; j < n; ++j) s = s + r[o + j];
        const double avg = s / (double)n;
        double w = 0.0;
        for (int32_t p = 0; p < n; ++p) {
            const double x = r[sval[o + p]];
            const double d = (x - avg) / scale_fn(x, avg);
            w = w + d * d;
        }
        s_avg = avg;
        s_norm = sqrt(w);
        s_known = 0;
    }
    __syncthreads();
    const double avg = s_avg, norm = s_norm;
    unsigned long long st = 0;
    int32_t known = 0;
    for (int32_t j = threadIdx.x; j < n; j += blockDim.x) {
        const double x = r[o + j];
        const double d = (x - avg) / scale_fn(x, avg);
        if (!isfinite(d)) st |= ST_NONFINITE;
        dev[o + j] = d;
        pre[o + j] = (norm != 0) ? d / norm : 0.0;
        const int32_t c = di[o + j];
        if (c >= 0) {
            atomicOr(bits + (c >> 6), 1ull << (c & 63));
            ++known;
        }
        if (j > 0 && skey[o + j] == skey[o + j - 1]) st |= ST_DUPLICATE;
    }
    if (st) atomicOr((unsigned long long*)info, st);
    if (known) atomicAdd(&s_known, known);
    __syncthreads();
    if (threadIdx.x == 0) {
        info[1] = s_known;
        scal[2 * b] = avg;
        scal[2 * b + 1] = norm;
        if (avg < 0.0) atomicOr((unsigned long long*)info, (unsigned long long)ST_NEG_MEAN);
    }
}

__global__ void __launch_bounds__(ONE_BLOCK) k_qb_rank(int64_t W, const unsigned long long* __restrict__ bits,
                                                       int64_t* __restrict__ rank) {
    const unsigned long long* mine = bits + (int64_t)blockIdx.x * W;
    block_exclusive_scan(W, [&](int64_t w) { return (int64_t)__popcll(mine[w]); }, rank + (int64_t)blockIdx.x * (W + 1));
}

// the known items of every slot in dense order: preprocessed value, deviation, position in the given order
__global__ void k_qb_scatter(int64_t n, const int64_t* __restrict__ qo, const int32_t* __restrict__ slot,
                             const int32_t* __restrict__ di, const double* __restrict__ pre, const double* __restrict__ dev,
                             int64_t W, const unsigned long long* __restrict__ bits, const int64_t* __restrict__ rank,
                             double* __restrict__ pre_d, double* __restrict__ dev_d, int32_t* __restrict__ given_d) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t c = di[j];
    if (c < 0) return;
    const int32_t b = slot[j];
    const int64_t o = qo[b];
    const int32_t r = bit_rank(bits + (int64_t)b * W, rank + (int64_t)b * (W + 1), c);
    pre_d[o + r] = pre[j];
    dev_d[o + r] = dev[j];
    given_d[o + r] = (int32_t)(j - o);
}

// the chunk's bitmaps side by side for k_query_sim_dual: word x of 32 items, lane b -> tb[x * 64 + b] (the bits of slot b)
// and tr[x * 64 + b] (the number of slot b's known items below item 32 x); lanes >= C hold zeros
__global__ void k_qb_transpose(int64_t W, int32_t C, const unsigned long long* __restrict__ bits,
                               const int64_t* __restrict__ rank, uint32_t* __restrict__ tb, uint32_t* __restrict__ tr) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= 2 * W * QB_MAX_CHUNK) return;
    const int32_t b = (int32_t)(g % QB_MAX_CHUNK);
    const int64_t x = g / QB_MAX_CHUNK, w = x >> 1;
    uint32_t word = 0, below = 0;
    if (b < C) {
        const unsigned long long full = bits[(int64_t)b * W + w];
        below = (uint32_t)rank[(int64_t)b * (W + 1) + w];
        if (x & 1) {
            word = (uint32_t)(full >> 32);
            below += __popc((uint32_t)full);
        } else {
            word = (uint32_t)full;
        }
    }
    tb[g] = word;
    tr[g] = below;
}

// The similarity pass of a chunk: a wave owns a train row and walks its entries in row order; LANE b OWNS SLOT b.  The row
// is fetched once for the whole chunk (64 entries per coalesced load, then one wave-uniform entry at a time); every lane
// probes its own slot's bitmap word (one coalesced 256-byte read of tb per entry) and folds its own fp64 accumulator, so the
// left fold in row order = dense item order is exact by construction.  A slot of <= 4 ratings keeps its <= 4 products by given
// position and folds them at the end, as k_query_sim does; Jaccard counts.  out[b * U + v].
__global__ void __launch_bounds__(TPB) k_query_sim_dual(int32_t U, int32_t C, bool jaccard, const int64_t* __restrict__ u_ptr,
                                                        const int32_t* __restrict__ s_col, const double* __restrict__ s_pre,
                                                        const uint32_t* __restrict__ tb, const uint32_t* __restrict__ tr,
                                                        const int64_t* __restrict__ qo, const double* __restrict__ pre_d,
                                                        const int32_t* __restrict__ given_d, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const bool live = lane < C;
    const int64_t o = live ? qo[lane] : 0;
    const int32_t nq = live ? (int32_t)(qo[lane + 1] - o) : 0;
    const bool small = nq <= 4;
    const int64_t waves = (int64_t)gridDim.x * (TPB / 64);
    for (int64_t v = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); v < U; v += waves) {
        const int64_t b = u_ptr[v], e = u_ptr[v + 1];
        double s = 0.0, x0 = 0.0, x1 = 0.0, x2 = 0.0, x3 = 0.0;
        uint32_t found = 0;
        int64_t both = 0;
        for (int64_t base = b; base < e; base += 64) {
            const int cnt = (int)min((int64_t)64, e - base);
            const int32_t mine = lane < cnt ? s_col[base + lane] : 0;
#pragma unroll 4
            for (int l = 0; l < cnt; ++l) {
                const int32_t c = __builtin_amdgcn_readlane(mine, l);
                const int64_t cell = (int64_t)(c >> 5) * QB_MAX_CHUNK + lane;
                const uint32_t word = tb[cell];
                const uint32_t bit = 1u << (c & 31);
                if (word & bit) {
                    if (jaccard) {
                        ++both;
                    } else {
                        const int32_t r = (int32_t)(tr[cell] + __popc(word & (bit - 1u)));
                        const double xv = pre_d[o + r] * s_pre[base + l];
                        if (small) {
                            const int gg = given_d[o + r];
                            if (gg == 0) x0 = xv;
                            else if (gg == 1) x1 = xv;
                            else if (gg == 2) x2 = xv;
                            else x3 = xv;
                            found |= 1u << gg;
                        } else {
                            s = s + xv;
                        }
                    }
                }
            }
        }
        if (jaccard) {
            s = (double)both / (double)((int64_t)nq + (e - b) - both);
        } else if (small) {
            if (found & 1u) s = s + x0;
            if (found & 2u) s = s + x1;
            if (found & 4u) s = s + x2;
            if (found & 8u) s = s + x3;
        }
        if (live) out[(int64_t)lane * U + v] = s;
    }
}

// key of the stable second sort that groups a (value-ordered) list by slot: val = slot * stride + index
__global__ void k_qb_slot_keys(int64_t n, uint32_t stride, const uint32_t* __restrict__ val, uint32_t* __restrict__ key) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x < n) key[x] = val[x] / stride;
}

// the first qb_take of slot b's sorted list -> nbr_idx / nbr_sim [b][take]
__global__ void k_qb_write(int32_t C, int32_t take, int32_t U, const int32_t* __restrict__ self,
                           const uint32_t* __restrict__ sorted_val, const double* __restrict__ sim, int32_t* __restrict__ nbr_idx,
                           double* __restrict__ nbr_sim) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (int64_t)C * take) return;
    const int32_t b = (int32_t)(g / take), j = (int32_t)(g - (int64_t)b * take);
    if (j >= qb_take(self, b, take, U)) return;
    const uint32_t x = sorted_val[(int64_t)b * U + j];
    nbr_idx[g] = (int32_t)(x - (uint32_t)b * (uint32_t)U);
    nbr_sim[g] = sim[x];
}

// off[b][0 .. take]: first entry of each neighbour's ratings inside slot b's part of the gathered list; info[4 b + 2] = their
// number.  A slot whose status is already set takes no part in the prediction pass (0 entries), nor do the cells of a slot
// beyond its qb_take.
__global__ void __launch_bounds__(ONE_BLOCK) k_qb_offsets(int32_t take, int32_t U, const int32_t* __restrict__ self,
                                                          const int32_t* __restrict__ nbr, const int64_t* __restrict__ u_ptr,
                                                          int64_t* __restrict__ off, long long* __restrict__ info) {
    const int32_t b = blockIdx.x;
    const int32_t* mine = nbr + (int64_t)b * take;
    const int64_t live = info[4 * b] != 0 ? 0 : qb_take(self, b, take, U);
    const int64_t total = block_exclusive_scan(
        take, [&](int64_t j) { return j >= live ? (int64_t)0 : u_ptr[mine[j] + 1] - u_ptr[mine[j]]; }, off + (int64_t)b * (take + 1));
    if (threadIdx.x == 0) info[4 * b + 2] = total;
}

// the neighbours' ratings, one wave per (slot, neighbour); key = (slot * I + item, train file row): ratedI(i) :508-517 is in
// file order
__global__ void __launch_bounds__(TPB) k_qb_gather(int32_t C, int32_t take, int32_t I, const int32_t* __restrict__ nbr,
                                                   const double* __restrict__ nsim, const int64_t* __restrict__ off,
                                                   const int64_t* __restrict__ ebase, const int64_t* __restrict__ u_ptr,
                                                   const int32_t* __restrict__ s_col, const uint32_t* __restrict__ s_t,
                                                   const double* __restrict__ s_dev, uint64_t* __restrict__ key,
                                                   uint32_t* __restrict__ val, double* __restrict__ edev, double* __restrict__ esim) {
    const int64_t g = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (g >= (int64_t)C * take) return;
    const int32_t sb = (int32_t)(g / take), j = (int32_t)(g - (int64_t)sb * take);
    const int64_t lo = off[(int64_t)sb * (take + 1) + j], hi = off[(int64_t)sb * (take + 1) + j + 1];
    if (hi == lo) return;  // (a failed slot, a cell beyond the slot's qb_take, or a neighbour without ratings)
    const int32_t v = nbr[g];
    const int64_t b = u_ptr[v], e = u_ptr[v + 1], o = ebase[sb] + lo;
    const double sj = nsim[g];
    for (int64_t p = b + (threadIdx.x & 63); p < e; p += 64) {
        const int64_t x = o + (p - b);
        key[x] = ((uint64_t)((uint32_t)sb * (uint32_t)I + (uint32_t)s_col[p]) << 32) | (uint64_t)s_t[p];
        val[x] = (uint32_t)x;
        edev[x] = s_dev[p];
        esim[x] = sj;
    }
}

// predictor :568-585 over [C][I]; q's own row of the item comes last in aug with s(q, q) = 0 (q is not in its own
// neighbour list).  SELF_ZERO = false (the Personalized mode): k_qb_fold_all has folded q's own term at its place already
template <bool SELF_ZERO>
__global__ void k_qb_pred(int32_t C, int32_t I, int64_t W, const double* __restrict__ num, const double* __restrict__ den,
                          const unsigned long long* __restrict__ bits, const int64_t* __restrict__ rank,
                          const int64_t* __restrict__ qo, const double* __restrict__ dev_d, const double* __restrict__ scal,
                          double* __restrict__ pred, uint8_t* __restrict__ rated) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (int64_t)C * I) return;
    const int32_t b = (int32_t)(g / I), i = (int32_t)(g - (int64_t)b * I);
    const unsigned long long* mb = bits + (int64_t)b * W;
    double a = num[g], d = den[g];
    const bool mine = (mb[i >> 6] >> (i & 63)) & 1ull;
    if (SELF_ZERO && mine) {
        const double s = 0.0;
        a = a + dev_d[qo[b] + bit_rank(mb, rank + (int64_t)b * (W + 1), i)] * s;
        d = d + fabs(s);
    }
    const double avg = scal[2 * b];
    const double w = d > 0 ? a / d : 0.0;
    pred[g] = avg + w * scale_fn(avg + w, avg);
    rated[g] = mine ? 1 : 0;
}

// requested raw items with their slot: the dense item's prediction; an item without a train rater has den = 0 (avg exactly)
__global__ void k_qb_pick(int64_t m, const int32_t* __restrict__ items, const int32_t* __restrict__ slot,
                          const int32_t* __restrict__ i_table, int32_t i_cells, const uint32_t* __restrict__ ikeys, int32_t I,
                          const double* __restrict__ pred, const double* __restrict__ scal, double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const int32_t it = items[j], b = slot[j];
    int32_t c;
    if (i_cells > 0) c = (it >= 0 && it < i_cells) ? i_table[it] : -1;
    else c = dense_lookup(ikeys, I, it);
    if (c >= 0) {
        out[j] = pred[(int64_t)b * I + c];
    } else {
        const double avg = scal[2 * b], w = 0.0;
        out[j] = avg + w * scale_fn(avg + w, avg);
    }
}

// ---- explanations of query predictions (knncf_query_explain* / knncf_update_explain* / knncf_revise_explain*) ------------
// After foldin_batch_predictions the chunk's gathered neighbour ratings lie sorted by (slot * I + item, train file row) in
// key / val, with edev / esim behind the permutation val.  The entries whose key's high word is slot * I + item are, one for
// one and in summation order, simVal :513-517 of that (query user, item) on aug restricted to the slot's neighbours — the
// other raters' elements have similarity 0.0, as do the listed neighbours whose similarity is exactly 0.0: neither is a term.
// k_q_fold folded exactly this segment into num / den (the zero elements add +-0.0: identities), k_qb_pred combined them.
struct QbExplainArgs {
    const int32_t* items;  // [rows of the chunk] requested raw item and slot, as k_qb_pick takes them
    const int32_t* slot;
    const int32_t* i_table;
    int32_t i_cells;
    const uint32_t* ikeys;
    int32_t I, take, order, cap;
    int64_t E;             // entries of the chunk's sorted list (0: key .. ebase are not read)
    const uint64_t* key;
    const uint32_t* val;
    const double* edev;
    const double* esim;
    const int64_t* ebase;  // [C + 1]
    const int64_t* off;    // [C][take + 1]
    const int32_t* nbr;    // [C][take] dense neighbours
    const int32_t* uid;    // raw id of a dense user
    const double* num;     // [C][I]
    const double* den;
    const double* pred;
    const double* scal;    // [C][2]
    // outputs of the launch's rows [r0, r0 + n): cell 0 is row r0.  Terms [n * cap] (unused with cap == 0), counts [n],
    // sums [2 n], pred [n]
    int32_t* raters;
    double* sims;
    double* devs;
    int32_t* counts;
    double* sums;
    double* out_pred;
};

// the raw id of the neighbour whose ratings k_qb_gather wrote at position t of the gathered list: slot b's part starts at
// ebase[b], neighbour j's extent inside it is [off[b][j], off[b][j + 1])
__device__ __forceinline__ int32_t qb_rater(const QbExplainArgs& A, int32_t b, uint32_t t) {
    const int64_t* mine = A.off + (int64_t)b * (A.take + 1);
    const int64_t r = (int64_t)t - A.ebase[b];
    int32_t lo = 0, hi = A.take;  // first j with mine[j] > r: mine[take] = the slot's entries > r, so 1 <= j <= take
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (mine[mid] > r) hi = mid;
        else lo = mid + 1;
    }
    return A.uid[A.nbr[(int64_t)b * A.take + (lo - 1)]];
}

// One wave per requested row.  No LDS and no tile: a segment of any length is walked 64 entries per trip, and BY_WEIGHT
// ranks each term by counting against the whole segment, which the wave re-reads 64 entries at a time and broadcasts lane by
// lane (v_readlane), QBX_OWN terms per lane and pass.
// Bounds.  rows: the host uploads items / slot for every row of [r0, r0 + n) and sizes the outputs for n rows of cap cells; a
// term is stored only at a place < cap.  slot < C.  c is a dense item of [0, I) or -1.  Segment positions x lie in [lo, hi)
// within [0, E); val is a permutation of [0, E).  The slot is the major part of the key, so every entry of the segment was
// gathered for slot b: ebase[b] <= t < ebase[b + 1], hence 0 <= r < off[b][take] in qb_rater, whose answer j has a non-empty
// extent — a cell k_qb_write filled with a dense user of [0, U).
static constexpr int QBX_WAVES = 4;  // waves (rows) per workgroup
static constexpr int QBX_OWN = 4;    // BY_WEIGHT: terms a lane ranks per pass over the segment
__global__ void __launch_bounds__(QBX_WAVES * 64) k_qb_explain(QbExplainArgs A, int64_t r0, int64_t n) {
    const int lane = threadIdx.x & 63;
    const int64_t jj = (int64_t)blockIdx.x * QBX_WAVES + (threadIdx.x >> 6);
    if (jj >= n) return;
    const int64_t j = r0 + jj;
    const int32_t it = A.items[j], b = A.slot[j];
    int32_t c;
    if (A.i_cells > 0) c = (it >= 0 && it < A.i_cells) ? A.i_table[it] : -1;
    else c = dense_lookup(A.ikeys, A.I, it);
    if (c < 0) {  // unknown to train: no rater (k_qb_pick's expression)
        if (lane == 0) {
            A.counts[jj] = 0;
            if (A.sums) A.sums[2 * jj] = A.sums[2 * jj + 1] = 0.0;
            if (A.out_pred) {
                const double avg = A.scal[2 * b], w = 0.0;
                A.out_pred[jj] = avg + w * scale_fn(avg + w, avg);
            }
        }
        return;
    }
    // the segment [lo, hi) of key high word slot * I + item (every lane runs the same search; E < 2^32 - 1)
    const uint32_t want = (uint32_t)b * (uint32_t)A.I + (uint32_t)c;
    uint32_t lo = 0, hi = 0;
    if (A.E > 0) {
        int64_t a = 0, z = A.E;
        while (a < z) {
            const int64_t mid = (a + z) >> 1;
            if ((uint32_t)(A.key[mid] >> 32) < want) a = mid + 1;
            else z = mid;
        }
        lo = (uint32_t)a;
        z = A.E;
        while (a < z) {
            const int64_t mid = (a + z) >> 1;
            if ((uint32_t)(A.key[mid] >> 32) <= want) a = mid + 1;
            else z = mid;
        }
        hi = (uint32_t)a;
    }
    lo = __builtin_amdgcn_readfirstlane(lo);
    hi = __builtin_amdgcn_readfirstlane(hi);
    const int64_t ob = jj * (int64_t)A.cap;
    const bool by_weight = A.order == KNNCF_EXPLAIN_BY_WEIGHT;
    // walk and compact: the running place of a term is its place in the fold
    int32_t total = 0;
    for (uint32_t base = lo; base < hi; base += 64) {
        const uint32_t x = base + lane;
        uint32_t t = 0;
        double s = 0.0;
        if (x < hi) {
            t = A.val[x];
            s = A.esim[t];
        }
        const bool keep = s != 0.0;
        const unsigned long long hit = __ballot(keep);
        if (keep && !by_weight) {
            const int32_t place = total + lanes_below(hit);
            if (place < A.cap) {
                A.raters[ob + place] = qb_rater(A, b, t);
                A.sims[ob + place] = s;
                A.devs[ob + place] = A.edev[t];
            }
        }
        total += __popcll(hit);
    }
    if (by_weight && A.cap > 0 && total > 0) {
        // place = the number of terms that go first under (|similarity| descending, summation place ascending); segment
        // position orders the terms as the summation place does.  An entry with similarity 0.0, or past the segment,
        // broadcasts magnitude 0.0, which goes before no term (a term's magnitude is > 0) and is counted by none.
        for (uint32_t own = lo; own < hi; own += 64 * QBX_OWN) {
            uint32_t x[QBX_OWN], t[QBX_OWN], rank[QBX_OWN];
            double s[QBX_OWN], a[QBX_OWN];
#pragma unroll
            for (int q = 0; q < QBX_OWN; ++q) {
                x[q] = own + 64u * q + lane;
                t[q] = 0;
                s[q] = 0.0;
                rank[q] = 0;
                if (x[q] < hi) {
                    t[q] = A.val[x[q]];
                    s[q] = A.esim[t[q]];
                }
                a[q] = fabs(s[q]);
            }
            for (uint32_t yb = lo; yb < hi; yb += 64) {
                const uint32_t y = yb + lane;
                const double sy = y < hi ? fabs(A.esim[A.val[y]]) : 0.0;
                const int32_t sy_lo = __double2loint(sy), sy_hi = __double2hiint(sy);
                const int cnt = (int)min(64u, hi - yb);
                for (int l = 0; l < cnt; ++l) {
                    const double m = __hiloint2double(__builtin_amdgcn_readlane(sy_hi, l), __builtin_amdgcn_readlane(sy_lo, l));
                    const uint32_t yl = yb + (uint32_t)l;
#pragma unroll
                    for (int q = 0; q < QBX_OWN; ++q) rank[q] += (uint32_t)(m > a[q] || (m == a[q] && yl < x[q]));
                }
            }
#pragma unroll
            for (int q = 0; q < QBX_OWN; ++q) {
                if (s[q] != 0.0 && rank[q] < (uint32_t)A.cap) {
                    A.raters[ob + rank[q]] = qb_rater(A, b, t[q]);
                    A.sims[ob + rank[q]] = s[q];
                    A.devs[ob + rank[q]] = A.edev[t[q]];
                }
            }
        }
    }
    if (lane == 0) {
        // what k_q_fold and k_qb_pred wrote for the cell: the fold over all terms and the predict call's answer
        const int64_t cell = (int64_t)b * A.I + c;
        A.counts[jj] = total;
        if (A.sums) {
            A.sums[2 * jj] = A.num[cell];
            A.sums[2 * jj + 1] = A.den[cell];
        }
        if (A.out_pred) A.out_pred[jj] = A.pred[cell];
    }
}

// the order key of recommendations :651-674 over [C][I]: ascending key <=> descending prediction, rated items last; -0.0 and
// +0.0 compare equal in the reference's `x._2 == y._2`, so both map to the same key (k_rb_select_tile of reco_batch.hip
// computes the same key).  The input order inside a slot is ascending raw id (by_id), val = slot * I + dense item
__global__ void k_qb_reco_keys(int32_t C, int32_t I, const uint32_t* __restrict__ by_id, const double* __restrict__ pred,
                               const uint8_t* __restrict__ rated, uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (int64_t)C * I) return;
    const int32_t b = (int32_t)(g / I);
    const int64_t cell = (int64_t)b * I + by_id[g - (int64_t)b * I];
    double p = pred[cell];
    if (p == 0.0) p = 0.0;
    const uint64_t bits = (uint64_t)__double_as_longlong(p);
    const uint64_t asc = (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
    key[g] = rated[cell] ? ~0ull : ~asc;
    val[g] = (uint32_t)cell;
}

// slot b's first min(n, I - known) entries -> out_items / out_preds [b][n]
__global__ void k_qb_take(int32_t C, int32_t n, int32_t I, const long long* __restrict__ info,
                          const uint32_t* __restrict__ order, const int32_t* __restrict__ iid, const double* __restrict__ pred,
                          int32_t* __restrict__ out_items, double* __restrict__ out_preds) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (int64_t)C * n) return;
    const int32_t b = (int32_t)(g / n), j = (int32_t)(g - (int64_t)b * n);
    if (j >= (int64_t)I - info[4 * b + 1]) return;
    const uint32_t cell = order[(int64_t)b * I + j];
    out_items[g] = iid[cell - (uint32_t)b * (uint32_t)I];
    out_preds[g] = pred[cell];
}

// the recommended cells of a chunk as the rows the explain kernels take (knncf_*_recommend_explain*): cell j of slot b of the
// [C][n] raw items k_qb_take wrote becomes row rb[b] + j, (raw item, slot), for j < rb[b + 1] - rb[b] — slot after slot, j
// ascending.  rb is the host's exclusive prefix of the slots' counts: a refused slot, whose cells of `items` and of bs.pred
// hold nothing meaningful, has count 0 and gives no row; a slot with a count below n gives its count.
// Bounds.  One thread per cell g < C * n; b < C reads rb[b], rb[b + 1] of the [C + 1] uploaded.  A cell is read only with j <
// its slot's count <= min(n, I - known), which k_qb_take wrote.  The row rb[b] + j < rb[b + 1] <= rb[C] = the rows both
// outputs are sized for.
__global__ void k_qb_reco_rows(int32_t C, int32_t n, const int64_t* __restrict__ rb, const int32_t* __restrict__ items,
                               int32_t* __restrict__ row_items, int32_t* __restrict__ row_slot) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (int64_t)C * n) return;
    const int32_t b = (int32_t)(g / n), j = (int32_t)(g - (int64_t)b * n);
    const int64_t at = rb[b];
    if (j >= rb[b + 1] - at) return;
    row_items[at + j] = items[g];
    row_slot[at + j] = b;
}

// [C][stride] cells ordered by (slot, 64-bit key, input order): one stable sort by the key, then one by the slot; returns
// the ordered values (val = slot * stride + index)
static const uint32_t* qb_segmented_sort(QueryBatchScratch& bs, SortWorkspace& ws, int32_t C, int64_t stride, hipStream_t st) {
    const size_t m = (size_t)C * (size_t)stride;
    sort_pairs_u64_u32(ws, bs.k64_a.p, bs.k64_b.p, bs.v32_a.p, bs.v32_b.p, m, 64, st);
    if (C == 1) return bs.v32_b.p;
    k_qb_slot_keys<<<(unsigned)ceil_div((int64_t)m, TPB), TPB, 0, st>>>((int64_t)m, (uint32_t)stride, bs.v32_b.p, bs.s32_a.p);
    sort_pairs_u32_u32(ws, bs.s32_a.p, bs.s32_b.p, bs.v32_b.p, bs.v32_a.p, m, bits_for((uint64_t)(C - 1)), st);
    return bs.v32_a.p;
}

void foldin_batch_neighbors(const Train& tr, QueryBatchScratch& bs, SortWorkspace& ws, const QueryChunk& q, int32_t k, long long* h_info, hipStream_t st) {
    const int32_t C = q.C, *h_users = q.users, *h_items = q.items, *h_self = q.self, *h_removed = q.removed;
    const int64_t *h_qo = q.qo, *h_ao = q.ao, *h_ro = q.ro;
    const double* h_ratings = q.ratings;
    const ByChunk* by = q.by;
    const bool topk = q.topk;
    KN_REQUIRE(!h_self == !h_ao && (!h_ro || h_self) && (!by || (h_self && topk)), KNNCF_E_INVALID, "query chunk: fields that do not go together");
    bs.by_chunk = by != nullptr;
    const int32_t U = tr.U, I = tr.I;
    const int64_t W = ceil_div(I, 64), n = h_qo[C];
    const int64_t cells = (int64_t)C * std::max(U, I);
    const int32_t take = std::max(0, std::min(k, U));
    bs.users.ensure(C); bs.qo.ensure((size_t)C + 1);
    bs.items.ensure(n); bs.ratings.ensure(n); bs.slot.ensure(n); bs.di.ensure(n); bs.dev.ensure(n); bs.pre.ensure(n);
    bs.pre_d.ensure(n); bs.dev_d.ensure(n); bs.given_d.ensure(n);
    bs.bits.ensure((size_t)C * W); bs.rank.ensure((size_t)C * (W + 1));
    // revise queries: the removed items of the chunk; a chunk without any is an update chunk
    const int64_t nrm = (h_self && h_ro) ? h_ro[C] : 0;
    bs.n_removed = nrm;
    const int64_t keys = std::max<int64_t>(n + nrm, cells);
    bs.k64_a.ensure(keys); bs.k64_b.ensure(keys); bs.v32_a.ensure(keys); bs.v32_b.ensure(keys);
    bs.s32_a.ensure(cells); bs.s32_b.ensure(cells);
    bs.sim.ensure((size_t)C * U);
    bs.info.ensure((size_t)4 * C); bs.scal.ensure((size_t)2 * C);
    bs.nbr_idx.ensure(std::max<size_t>((size_t)C * take, 1)); bs.nbr_sim.ensure(std::max<size_t>((size_t)C * take, 1));
    bs.off.ensure((size_t)C * ((size_t)take + 1));

    // one upload of the chunk
    KN_HIP(hipMemcpyAsync(bs.users.p, h_users, (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice, st));
    KN_HIP(hipMemcpyAsync(bs.qo.p, h_qo, ((size_t)C + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    // (the status words are cleared before the seeding: k_qb_mark sets bits in them)
    KN_HIP(hipMemsetAsync(bs.info.p, 0, (size_t)4 * C * sizeof(int64_t), st));
    if (by) bystander_upload(bs, C, *by, st);
    long long* info = (long long*)bs.info.p;
    const int32_t* self = nullptr;
    if (!h_self) {
        KN_HIP(hipMemcpyAsync(bs.items.p, h_items, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        KN_HIP(hipMemcpyAsync(bs.ratings.p, h_ratings, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    } else {
        // update queries: only the additional rows travel; the train rows of the fitted users are seeded on the device
        const int64_t na = h_ao[C];
        bs.self.ensure(C); bs.ao.ensure((size_t)C + 1);
        bs.add_items.ensure(std::max<int64_t>(na, 1)); bs.add_ratings.ensure(std::max<int64_t>(na, 1));
        KN_HIP(hipMemcpyAsync(bs.self.p, h_self, (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice, st));
        KN_HIP(hipMemcpyAsync(bs.ao.p, h_ao, ((size_t)C + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        if (na > 0) {
            KN_HIP(hipMemcpyAsync(bs.add_items.p, h_items, (size_t)na * sizeof(int32_t), hipMemcpyHostToDevice, st));
            KN_HIP(hipMemcpyAsync(bs.add_ratings.p, h_ratings, (size_t)na * sizeof(double), hipMemcpyHostToDevice, st));
        }
        self = bs.self.p;
        const int slot_bits = C > 1 ? bits_for((uint64_t)(C - 1)) : 0;
        if (nrm == 0) {
            k_qb_seed_keys<<<(unsigned)ceil_div(n, TPB), TPB, 0, st>>>(n, C, bs.qo.p, self, tr.u_ptr.p, tr.s_t.p, bs.k64_a.p, bs.v32_a.p);
            sort_pairs_u64_u32(ws, bs.k64_a.p, bs.k64_b.p, bs.v32_a.p, bs.v32_b.p, (size_t)n, 33 + slot_bits, st);
            k_qb_seed<<<(unsigned)ceil_div(n, TPB), TPB, 0, st>>>(n, C, bs.qo.p, bs.ao.p, self, tr.u_ptr.p, tr.s_col.p, tr.s_rating.p,
                                                                  tr.iid.p, bs.add_items.p, bs.add_ratings.p, bs.v32_b.p, bs.items.p,
                                                                  bs.ratings.p);
        } else {
            // source rows of slot b: every train row of its user + its additional rows = its declared rows + its removed items
            std::vector<int64_t>& so = bs.h_so;  // (outlives the asynchronous upload)
            so.assign((size_t)C + 1, 0);
            for (int32_t b = 0; b < C; ++b) so[b + 1] = so[b] + (h_qo[b + 1] - h_qo[b]) + (h_ro[b + 1] - h_ro[b]);
            const int64_t ns = so[C];  // == n + nrm
            bs.ro.ensure((size_t)C + 1); bs.so.ensure((size_t)C + 1);
            bs.rm_items.ensure(nrm); bs.rm_slot.ensure(nrm); bs.rm_gone.ensure(nrm); bs.rm_mark.ensure(ns);
            KN_HIP(hipMemcpyAsync(bs.ro.p, h_ro, ((size_t)C + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
            KN_HIP(hipMemcpyAsync(bs.so.p, so.data(), ((size_t)C + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
            KN_HIP(hipMemcpyAsync(bs.rm_items.p, h_removed, (size_t)nrm * sizeof(int32_t), hipMemcpyHostToDevice, st));
            KN_HIP(hipMemsetAsync(bs.rm_mark.p, 0, (size_t)ns * sizeof(uint32_t), st));
            k_qb_mark<<<(unsigned)ceil_div(nrm, TPB), TPB, 0, st>>>(nrm, C, bs.ro.p, bs.so.p, self, bs.rm_items.p, tr.i_table.p,
                                                                    table_cells(tr), tr.ikeys.p, I, tr.u_ptr.p, tr.s_col.p, tr.i_ptr.p,
                                                                    bs.rm_mark.p, bs.rm_slot.p, bs.rm_gone.p, info);
            k_qb_seed_keys_rv<<<(unsigned)ceil_div(ns, TPB), TPB, 0, st>>>(ns, C, bs.so.p, self, tr.u_ptr.p, tr.s_t.p, bs.rm_mark.p,
                                                                           bs.k64_a.p, bs.v32_a.p);
            sort_pairs_u64_u32(ws, bs.k64_a.p, bs.k64_b.p, bs.v32_a.p, bs.v32_b.p, (size_t)ns, 34 + slot_bits, st);
            k_qb_seed_rv<<<(unsigned)ceil_div(n, TPB), TPB, 0, st>>>(n, C, bs.qo.p, bs.so.p, bs.ao.p, self, tr.u_ptr.p, tr.s_col.p,
                                                                     tr.s_rating.p, tr.iid.p, bs.add_items.p, bs.add_ratings.p,
                                                                     bs.v32_b.p, bs.items.p, bs.ratings.p);
        }
    }
    KN_HIP(hipMemsetAsync(bs.bits.p, 0, (size_t)C * W * sizeof(uint64_t), st));
    unsigned long long* bits = (unsigned long long*)bs.bits.p;
    // query prep
    k_qb_keys<<<(unsigned)ceil_div(n, TPB), TPB, 0, st>>>(n, C, bs.qo.p, bs.users.p, bs.items.p, tr.i_table.p, table_cells(tr),
                                                          tr.ikeys.p, I, bs.slot.p, bs.di.p, bs.k64_a.p, bs.v32_a.p);
    sort_pairs_u64_u32(ws, bs.k64_a.p, bs.k64_b.p, bs.v32_a.p, bs.v32_b.p, (size_t)n, 32 + (C > 1 ? bits_for((uint64_t)(C - 1)) : 0), st);
    k_qb_prep<<<C, ONE_BLOCK, 0, st>>>(bs.qo.p, bs.ratings.p, bs.k64_b.p, bs.v32_b.p, bs.di.p, W, bs.dev.p, bs.pre.p, bits, info,
                                       bs.scal.p);
    if (nrm > 0) k_qb_gone<<<(unsigned)ceil_div(nrm, TPB), TPB, 0, st>>>(nrm, W, bs.rm_slot.p, bs.rm_gone.p, bits, info);
    k_qb_rank<<<C, ONE_BLOCK, 0, st>>>(W, bits, bs.rank.p);
    k_qb_scatter<<<(unsigned)ceil_div(n, TPB), TPB, 0, st>>>(n, bs.qo.p, bs.slot.p, bs.di.p, bs.pre.p, bs.dev.p, W, bits, bs.rank.p,
                                                             bs.pre_d.p, bs.dev_d.p, bs.given_d.p);
    KN_HIP(hipGetLastError());
    // similarities [C][U]
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(U, TPB / 64), 2048);
    if (C >= QB_DUAL_MIN) {
        const int64_t cellsT = 2 * W * QB_MAX_CHUNK;
        bs.tbits.ensure(cellsT); bs.trank.ensure(cellsT);
        k_qb_transpose<<<(unsigned)ceil_div(cellsT, TPB), TPB, 0, st>>>(W, C, bits, bs.rank.p, bs.tbits.p, bs.trank.p);
        k_query_sim_dual<<<grid, TPB, 0, st>>>(U, C, tr.jaccard, tr.u_ptr.p, tr.s_col.p, tr.s_pre.p, bs.tbits.p, bs.trank.p,
                                               bs.qo.p, bs.pre_d.p, bs.given_d.p, bs.sim.p);
    } else {
        const size_t lds = (size_t)W * (sizeof(uint64_t) + sizeof(int64_t));
        if (W <= SIM_LDS_WORDS) ensure_dynamic_lds(g_sim_lds, (const void*)k_query_sim<true>, lds);
        for (int32_t b = 0; b < C; ++b) {
            const int32_t nq = (int32_t)(h_qo[b + 1] - h_qo[b]);
            const unsigned long long* bb = bits + (int64_t)b * W;
            const int64_t* rb = bs.rank.p + (int64_t)b * (W + 1);
            if (W <= SIM_LDS_WORDS) {
                k_query_sim<true><<<grid, TPB, lds, st>>>(U, nq, tr.jaccard, tr.u_ptr.p, tr.s_col.p, tr.s_pre.p, W, bb, rb,
                                                          bs.pre_d.p + h_qo[b], bs.given_d.p + h_qo[b], bs.sim.p + (int64_t)b * U);
            } else {
                k_query_sim<false><<<grid, TPB, 0, st>>>(U, nq, tr.jaccard, tr.u_ptr.p, tr.s_col.p, tr.s_pre.p, W, bb, rb,
                                                         bs.pre_d.p + h_qo[b], bs.given_d.p + h_qo[b], bs.sim.p + (int64_t)b * U);
            }
        }
    }
    KN_HIP(hipGetLastError());
    const bool placed = by && by->fitted > 0;
    if (placed) bystander_place(tr, bs, C, st);
    if (topk) {  // (the Personalized mode has no neighbourhood cut: foldin_batch_fold_all reads bs.sim as it is)
        // top-k of every slot: (similarity desc, dense user asc)
        launch_fallback_keys((int32_t)((int64_t)C * U), bs.sim.p, bs.k64_a.p, bs.v32_a.p, st);
        if (self) k_qb_mask_self<<<(unsigned)ceil_div(C, 64), 64, 0, st>>>(C, U, self, bs.k64_a.p);
        const uint32_t* order = qb_segmented_sort(bs, ws, C, U, st);
        if (take > 0) {
            k_qb_write<<<(unsigned)ceil_div((int64_t)C * take, TPB), TPB, 0, st>>>(C, take, U, self, order, bs.sim.p, bs.nbr_idx.p,
                                                                                   bs.nbr_sim.p);
        }
        if (by) bystander_merge(tr, bs, C, take, placed, st);
        else k_qb_offsets<<<C, ONE_BLOCK, 0, st>>>(take, U, self, bs.nbr_idx.p, tr.u_ptr.p, bs.off.p, info);
        KN_HIP(hipGetLastError());
    }
    // the chunk's one round trip: statuses, known items and the sizes of the prediction pass
    KN_HIP(hipMemcpyAsync(h_info, bs.info.p, (size_t)4 * C * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    KN_HIP(hipStreamSynchronize(st));
}

void foldin_batch_predictions(const Train& tr, QueryBatchScratch& bs, SortWorkspace& ws, int32_t C, int32_t take,
                              const int64_t* h_ebase, hipStream_t st) {
    const int32_t I = tr.I;
    const int64_t W = ceil_div(I, 64), E = h_ebase[C], cells = (int64_t)C * I;
    bs.num.ensure(cells); bs.den.ensure(cells); bs.pred.ensure(cells); bs.rated.ensure(cells);
    KN_HIP(hipMemsetAsync(bs.num.p, 0, (size_t)cells * sizeof(double), st));  // +0.0
    KN_HIP(hipMemsetAsync(bs.den.p, 0, (size_t)cells * sizeof(double), st));
    if (E > 0) {
        KN_REQUIRE(E < (int64_t)0xffffffffll, KNNCF_E_UNSUPPORTED, "query: more than 2^32-1 neighbour ratings in a chunk");
        bs.ebase.ensure((size_t)C + 1);
        bs.e_k64_a.ensure(E); bs.e_k64_b.ensure(E); bs.e_v32_a.ensure(E); bs.e_v32_b.ensure(E);
        bs.e_dev.ensure(E); bs.e_sim.ensure(E);
        KN_HIP(hipMemcpyAsync(bs.ebase.p, h_ebase, ((size_t)C + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        if (bs.by_chunk) bystander_gather(tr, bs, C, take, st);
        else k_qb_gather<<<(unsigned)ceil_div((int64_t)C * take, TPB / 64), TPB, 0, st>>>(
            C, take, I, bs.nbr_idx.p, bs.nbr_sim.p, bs.off.p, bs.ebase.p, tr.u_ptr.p, tr.s_col.p, tr.s_t.p, tr.s_dev.p, bs.e_k64_a.p,
            bs.e_v32_a.p, bs.e_dev.p, bs.e_sim.p);
        sort_pairs_u64_u32(ws, bs.e_k64_a.p, bs.e_k64_b.p, bs.e_v32_a.p, bs.e_v32_b.p, (size_t)E, 32 + bits_for((uint64_t)cells), st);
        k_q_fold<<<(unsigned)ceil_div(E, TPB), TPB, 0, st>>>(E, bs.e_k64_b.p, bs.e_v32_b.p, bs.e_dev.p, bs.e_sim.p, bs.num.p, bs.den.p);
    }
    k_qb_pred<true><<<(unsigned)ceil_div(cells, TPB), TPB, 0, st>>>(C, I, W, bs.num.p, bs.den.p, (const unsigned long long*)bs.bits.p,
                                                                    bs.rank.p, bs.qo.p, bs.dev_d.p, bs.scal.p, bs.pred.p, bs.rated.p);
    if (bs.n_removed > 0)
        k_qb_gone_rated<<<(unsigned)ceil_div(bs.n_removed, TPB), TPB, 0, st>>>(bs.n_removed, I, bs.rm_slot.p, bs.rm_gone.p, bs.rated.p);
    KN_HIP(hipGetLastError());
}

// ---- the Personalized predictor of a chunk (KNNCF_PRED_PERSONALIZED on the query families; DESIGN.md "Personalized queries")
// predictor(aug, weightedSumDeviation(aug, S)) with no neighbourhood cut: every rating of an item in aug is a term of its
// fold :508-524, the query user's own included, with S(u, u) != 0 as its weight.  bs.sim[C][U] holds S(u, v) for every train
// user v already (the query user owns every pair); what is added here is S(u, u), the transposed similarities and ONE fold
// per (slot, item) over the item's raters in file order.  No top-k, no gather, no sort of neighbour ratings.

// key of u's item-set order (ratedByUsers(u).map(_.item).toSet :418): the slot, then the trie order of the item id — every
// item of the slot's rows, the ones unknown to train included
__global__ void k_qb_self_keys(int64_t n, const int32_t* __restrict__ slot, const int32_t* __restrict__ items,
                               uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    key[j] = ((uint64_t)(uint32_t)slot[j] << 32) | (uint64_t)int_trie_key(items[j]);
    val[j] = (uint32_t)j;
}

// S(u, u) on aug, one wave per slot.  Cosine :424-426: ratedByBoth = u's item set, so the value is the left fold from 0.0 of
// pre(u, j) * pre(u, j) in the set's iteration order: the trie order (sval, sorted by k_qb_self_keys) for more than 4 rows,
// the given order (Set1..Set4) otherwise.  The products are formed 64 at a time, the additions run one by one in order.
// Jaccard :454-458: n / (n + n - n) = 1.0.  A fitted user's cell of [C][U] was computed against its OLD train row: replaced.
__global__ void __launch_bounds__(64) k_qb_self_sim(int32_t U, bool jaccard, const int64_t* __restrict__ qo,
                                                    const double* __restrict__ pre, const uint32_t* __restrict__ sval,
                                                    const int32_t* __restrict__ self, double* __restrict__ suu,
                                                    double* __restrict__ sim) {
    const int32_t b = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t o = qo[b];
    const int32_t n = (int32_t)(qo[b + 1] - o);
    const bool small = n <= 4;
    double s = 0.0;
    if (jaccard) {
        s = 1.0;
    } else {
        for (int32_t base = 0; base < n; base += 64) {
            const int cnt = min(64, n - base);
            double x = 0.0;
            if (lane < cnt) {
                const double v = small ? pre[o + base + lane] : pre[sval[o + base + lane]];
                x = v * v;
            }
            const int32_t x_lo = __double2loint(x), x_hi = __double2hiint(x);
            for (int l = 0; l < cnt; ++l)
                s = s + __hiloint2double(__builtin_amdgcn_readlane(x_hi, l), __builtin_amdgcn_readlane(x_lo, l));
        }
    }
    if (lane == 0) {
        suu[b] = s;
        if (self && self[b] >= 0) sim[(int64_t)b * U + self[b]] = s;
    }
}

// [C][U] -> [U][stride]: one train user's similarities to all slots of the chunk side by side (stride = a power of two >= C;
// the cells of slots >= C hold 0.0 and are never folded).  64 x 64 tiles through LDS: both sides coalesced.
__global__ void __launch_bounds__(TPB) k_qb_sim_transpose(int32_t U, int32_t C, int32_t stride, const double* __restrict__ sim,
                                                          double* __restrict__ simT) {
    __shared__ double tile[64][65];
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const int64_t v0 = (int64_t)blockIdx.x * 64;
    for (int b = y; b < 64; b += TPB / 64) tile[b][x] = (b < C && v0 + x < U) ? sim[(int64_t)b * U + v0 + x] : 0.0;
    __syncthreads();
    if (x >= stride) return;
    for (int vv = y; vv < 64 && v0 + vv < U; vv += TPB / 64) simT[(v0 + vv) * stride + x] = tile[x][vv];
}

// Slot b's own rating of dense item i as a term of aug (the Personalized mode; k_qb_fold_all folds it, k_qb_explain_all lists
// it).  The slot rates i in aug when i's bit of its bitmap is set; its deviation ON AUG is dev_d at the bit's rank.  The row is a
// SURVIVING TRAIN ROW when its given position is below the slot's number of surviving train rows (they come first: k_qb_seed /
// k_qb_seed_rv; ao == nullptr, a fold-in chunk, has none): the term (suu[b], dev) then stands at the file place of the rater
// self[b] (own_s / own_dev).  Otherwise it is an additional row — any row of a fold-in user, a re-rated item — and the term
// comes LAST, after every train row (last, last_s / last_dev).  With neither, the rater self[b] of the item, if there is one,
// is a removed or re-rated train row: own_s = own_dev = 0.0, no term.
// Bounds: bit_rank of a set bit of slot b is below the slot's number of known items <= its rows, so o + r is inside the slot's
// extent of dev_d / given_d.
struct QbOwnTerm {
    double own_s = 0.0, own_dev = 0.0, last_s = 0.0, last_dev = 0.0;
    bool last = false;
};
__device__ __forceinline__ QbOwnTerm qb_own_term(int32_t b, int32_t i, int64_t W, const unsigned long long* __restrict__ bits,
                                                 const int64_t* __restrict__ rank, const int64_t* __restrict__ qo,
                                                 const int64_t* __restrict__ ao, const double* __restrict__ dev_d,
                                                 const int32_t* __restrict__ given_d, const double* __restrict__ suu) {
    QbOwnTerm t;
    const unsigned long long* mb = bits + (int64_t)b * W;
    if ((mb[i >> 6] >> (i & 63)) & 1ull) {
        const int64_t o = qo[b];
        const int32_t r = bit_rank(mb, rank + (int64_t)b * (W + 1), i);
        const int64_t survivors = ao ? (qo[b + 1] - o) - (ao[b + 1] - ao[b]) : 0;
        if (given_d[o + r] < survivors) {
            t.own_s = suu[b];
            t.own_dev = dev_d[o + r];
        } else {
            t.last = true;
            t.last_s = suu[b];
            t.last_dev = dev_d[o + r];
        }
    }
    return t;
}

// The fold of a chunk: ONE WAVE PER TRAIN ITEM, LANE b OWNS SLOT b (the layout of k_query_sim_dual).  The wave walks the item's
// raters in file order (pf_user / pf_dev, 64 per coalesced load), one wave-uniform entry at a time; every lane reads its own
// similarity to that rater from the transposed row (one coalesced read per entry) and runs num = num + dev * s, den = den +
// |s| in its own registers: the left folds of :520-524, multiply and add separate.  The similarity loads do not depend on the
// add chains, so FA_AHEAD of them are issued before the adds that use them.
// The slot's own user as a rater (self[b]) is qb_own_term's: a surviving train row is folded at its file place with the slot's
// deviation ON AUG (the mean changed) and S(u, u); a removed or re-rated train row is no term: it adds dev 0.0 * s 0.0, an
// identity (the sums start at +0.0 and cannot become -0.0); a slot that rates the item through an additional row has that
// term last, after every train row.  Longest items first (pop_item).
// Bounds.  w < I, i = pop_item[w] is a dense item of [0, I); entries lie in [i_ptr[i], i_ptr[i + 1]) within [0, n); pf_user is
// a dense user of [0, U), col < stride, so the read cell is inside simT [U][stride].  Lanes >= C read column 0 and write
// nothing.
static constexpr int FA_WAVES = 4;  // waves (items) per workgroup
static constexpr int FA_AHEAD = 8;  // similarity loads in flight per lane
__global__ void __launch_bounds__(FA_WAVES * 64) k_qb_fold_all(int32_t I, int32_t C, int32_t stride, int64_t W,
                                                               const int32_t* __restrict__ pop_item, const int64_t* __restrict__ i_ptr,
                                                               const int32_t* __restrict__ pf_user, const double* __restrict__ pf_dev,
                                                               const double* __restrict__ simT,
                                                               const unsigned long long* __restrict__ bits,
                                                               const int64_t* __restrict__ rank, const int64_t* __restrict__ qo,
                                                               const int64_t* __restrict__ ao, const int32_t* __restrict__ self,
                                                               const double* __restrict__ dev_d, const int32_t* __restrict__ given_d,
                                                               const double* __restrict__ suu, double* __restrict__ num,
                                                               double* __restrict__ den) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * FA_WAVES + (threadIdx.x >> 6);
    if (w >= I) return;
    const int32_t i = __builtin_amdgcn_readfirstlane(pop_item[w]);  // (wave-uniform: the list bounds and the trip counts are scalars)
    const bool live = lane < C;
    const int col = live ? lane : 0;
    int32_t me = -1;
    QbOwnTerm own;
    if (live) {
        if (self) me = self[lane];
        own = qb_own_term(lane, i, W, bits, rank, qo, ao, dev_d, given_d, suu);
    }
    const double own_s = own.own_s, own_dev = own.own_dev, last_s = own.last_s, last_dev = own.last_dev;
    const bool last = own.last;
    double a = 0.0, d = 0.0;
    const int64_t rb = i_ptr[i], re = i_ptr[i + 1];
    for (int64_t base = rb; base < re; base += 64) {
        const int cnt = (int)min((int64_t)64, re - base);
        const int32_t mv = lane < cnt ? pf_user[base + lane] : 0;
        const double md = lane < cnt ? pf_dev[base + lane] : 0.0;
        const int32_t md_lo = __double2loint(md), md_hi = __double2hiint(md);
        // (wave-uniform l: the rater and its deviation come out of the lanes' registers, v_readlane)
        auto term = [&](int32_t v, double sl, int l) {
            const double dv = __hiloint2double(__builtin_amdgcn_readlane(md_hi, l), __builtin_amdgcn_readlane(md_lo, l));
            const bool mine = v == me;
            const double sv = mine ? own_s : sl;
            const double dd = mine ? own_dev : dv;
            a = a + dd * sv;
            d = d + fabs(sv);
        };
        int l0 = 0;
        for (; l0 + FA_AHEAD <= cnt; l0 += FA_AHEAD) {
            int32_t v[FA_AHEAD];
            double s[FA_AHEAD];
#pragma unroll
            for (int q = 0; q < FA_AHEAD; ++q) {
                v[q] = __builtin_amdgcn_readlane(mv, l0 + q);
                s[q] = simT[(int64_t)v[q] * stride + col];
            }
#pragma unroll
            for (int q = 0; q < FA_AHEAD; ++q) term(v[q], s[q], l0 + q);
        }
        for (; l0 < cnt; ++l0) {
            const int32_t v = __builtin_amdgcn_readlane(mv, l0);
            term(v, simT[(int64_t)v * stride + col], l0);
        }
    }
    if (last) {
        a = a + last_dev * last_s;
        d = d + fabs(last_s);
    }
    if (live) {
        num[(int64_t)lane * I + i] = a;
        den[(int64_t)lane * I + i] = d;
    }
}

// k_qb_pick of the Personalized mode: an item that has no dense id but is one of the slot's rows (an additional item unknown
// to train) has exactly one term in aug, the slot's own: num = 0.0 + dev(u, i) * S(u, u), den = 0.0 + |S(u, u)|.  Any other
// item without a dense id is unknown to aug: the mean exactly.
__global__ void k_qb_pick_all(int64_t m, const int32_t* __restrict__ items, const int32_t* __restrict__ slot,
                              const int32_t* __restrict__ i_table, int32_t i_cells, const uint32_t* __restrict__ ikeys, int32_t I,
                              const double* __restrict__ pred, const double* __restrict__ scal, const int64_t* __restrict__ qo,
                              const int32_t* __restrict__ q_items, const double* __restrict__ q_dev, const double* __restrict__ suu,
                              double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const int32_t it = items[j], b = slot[j];
    int32_t c;
    if (i_cells > 0) c = (it >= 0 && it < i_cells) ? i_table[it] : -1;
    else c = dense_lookup(ikeys, I, it);
    if (c >= 0) {
        out[j] = pred[(int64_t)b * I + c];
        return;
    }
    double a = 0.0, d = 0.0;
    for (int64_t x = qo[b]; x < qo[b + 1]; ++x) {
        if (q_items[x] == it) {
            const double s = suu[b];
            a = a + q_dev[x] * s;
            d = d + fabs(s);
            break;
        }
    }
    const double avg = scal[2 * b];
    const double w = d > 0 ? a / d : 0.0;
    out[j] = avg + w * scale_fn(avg + w, avg);
}

// ---- explanations of Personalized query predictions (knncf_*_explain_personalized*; DESIGN.md "Explanations of Personalized
// query predictions") --------------------------------------------------------------------------------------------------------
// After foldin_batch_fold_all the chunk holds everything a row (slot b, item) needs: bs.sim[b][v] = S(u, v) for every train
// user, suu[b] = S(u, u) on aug, the fold results num / den / pred [C][I].  ONE WAVE PER REQUESTED ROW.
//   sums, prediction   are not recomputed: a dense item's are the cell (b, c) of num / den / pred, as k_qb_fold_all and
//           k_qb_pred<false> wrote them, so the prediction is the predict call's by construction; an item without a dense id that
//           the slot rates has k_qb_pick_all's one-term fold, any other item without a dense id (0, 0) and the mean.
//   terms   QueryTerms below, a reader of explain_select.h: positions [rb, re) = [i_ptr[c], i_ptr[c + 1]) are the item's raters in
//           file order with s = sim[b * U + rater], EXCEPT the rater self[b], whose cell holds S(u, u) whether or not its train
//           row survives: it takes qb_own_term's (own_s, own_dev) — the term on aug at its file place, or (0.0, 0.0), no term, for
//           a removed or re-rated row.  When the slot rates the item through an additional row, position re is one more term:
//           (the query's raw user id users[b], suu[b], the slot's deviation).  An item without a dense id has rb = re = 0.
//   walk    classifies and counts (ballot / mbcnt: the running count of non-zero similarities is the term's place in the
//           fold); SUM_ORDER stores a term while its place is below cap, BY_WEIGHT counts the top byte of |s| into the LDS
//           histogram.  No serial add chain.  Then explain_by_weight: select (count > cap only), emit, rank.
// Bounds.  Row w < n of the launch is row r0 + w of items / slot (the host uploads every row of the chunk) and owns cells
// [w * cap, (w + 1) * cap) of the outputs and of the staging.  slot b < C; c is a dense item of [0, I) or -1.  Every pf_user /
// pf_dev read is at a position p with rb <= p < re, inside [i_ptr[c], i_ptr[c + 1]); every similarity read is at b * U + v with v
// a rater read there, a dense user of [0, U); uid[v] likewise.  o + r of qb_own_term is inside the slot's extent by bit_rank's
// bound.  The search of a raw item runs over the slot's rows [qo[b], qo[b + 1]) of q_items / q_dev.  A term is stored at a
// place < min(count, cap) inside row w's cap cells, checked at the store; lanes past the sequence contribute similarity 0.0.
static constexpr int QXA_WAVES = 4;  // rows per workgroup

struct QbExplainAllArgs {
    const int32_t* items;  // [rows of the chunk] requested raw item and slot, as k_qb_pick_all takes them
    const int32_t* slot;
    const int32_t* i_table;
    int32_t i_cells;
    const uint32_t* ikeys;
    int32_t I, U;
    int64_t W;
    const int64_t* i_ptr;
    const int32_t* pf_user;
    const double* pf_dev;
    const double* sim;      // [C][U]
    const unsigned long long* bits;
    const int64_t* rank;
    const int64_t* qo;
    const int64_t* ao;      // null: a fold-in chunk
    const int32_t* self;    // null: a fold-in chunk
    const double* dev_d;
    const int32_t* given_d;
    const double* suu;      // [C]
    const int32_t* users;   // [C] raw id of the slot's user (a fold-in user has no dense id)
    const int32_t* q_items; // [rows of the slots] raw items and deviations in the given order
    const double* q_dev;
    const int32_t* uid;     // raw id of a dense user
    const double* num;      // [C][I]
    const double* den;
    const double* pred;
    const double* scal;     // [C][2]
    ExplainCells out;       // rows [0, n) of the launch
    ExplainStage st;        // BY_WEIGHT staging
};

struct QueryTerms {
    int64_t lo, hi, re;      // train raters [lo, re), hi = re + (the slot's additional row on the item ? 1 : 0)
    const int32_t* pf_user;
    const double* pf_dev;
    const double* row;       // sim + b * U
    const int32_t* uid;
    int32_t me, quser;       // self[b] (-1: not in the fit), users[b]
    double own_s, own_dev, last_s, last_dev;
    __device__ __forceinline__ int32_t rater(int64_t p) const { return p < re ? pf_user[p] : 0; }
    __device__ __forceinline__ double sim(int64_t p, int32_t v) const { return p >= re ? last_s : (v == me ? own_s : row[v]); }
    __device__ __forceinline__ double dev(int64_t p, int32_t v) const { return p >= re ? last_dev : (v == me ? own_dev : pf_dev[p]); }
    __device__ __forceinline__ int32_t raw(int64_t p, int32_t v) const { return p >= re ? quser : uid[v]; }
};

__global__ void __launch_bounds__(QXA_WAVES * 64) k_qb_explain_all(QbExplainAllArgs A, int64_t r0, int64_t n) {
    __shared__ double s_abs[QXA_WAVES][64];
    __shared__ uint32_t s_hist[QXA_WAVES][256];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (wave-uniform: the row, its slot and its item are scalars)
    const int64_t w = (int64_t)blockIdx.x * QXA_WAVES + wave;
    if (w >= n) return;
    const int64_t j = r0 + w;
    const int32_t it = A.items[j], b = A.slot[j];
    const int32_t cap = A.out.cap;
    int32_t c;
    if (A.i_cells > 0) c = (it >= 0 && it < A.i_cells) ? A.i_table[it] : -1;
    else c = dense_lookup(A.ikeys, A.I, it);
    QueryTerms rd{};
    rd.row = A.sim + (int64_t)b * A.U;
    rd.uid = A.uid;
    rd.me = A.self ? A.self[b] : -1;
    rd.quser = A.users[b];
    double num, den, p;
    if (c >= 0) {
        const QbOwnTerm own = qb_own_term(b, c, A.W, A.bits, A.rank, A.qo, A.ao, A.dev_d, A.given_d, A.suu);
        const int64_t rb = A.i_ptr[c], re = A.i_ptr[c + 1];
        rd.lo = rb;
        rd.re = re;
        rd.hi = re + (own.last ? 1 : 0);
        rd.pf_user = A.pf_user;
        rd.pf_dev = A.pf_dev;
        rd.own_s = own.own_s; rd.own_dev = own.own_dev; rd.last_s = own.last_s; rd.last_dev = own.last_dev;
        const int64_t cell = (int64_t)b * A.I + c;
        num = A.num[cell];
        den = A.den[cell];
        p = A.pred[cell];
    } else {
        // no dense id: the slot's own row on the raw item, if it has one, is the only rating of the item in aug
        int64_t at = -1;
        for (int64_t x = A.qo[b] + lane; x < A.qo[b + 1]; x += 64)
            if (A.q_items[x] == it) at = x;
        const unsigned long long found = __ballot(at >= 0);
        num = 0.0;
        den = 0.0;
        if (found) {
            const double s = A.suu[b];
            const double dv = __shfl(at >= 0 ? A.q_dev[at] : 0.0, __ffsll((long long)found) - 1);
            rd.hi = 1;  // (lo = re = 0: position 0 is the slot's own row)
            rd.last_s = s;
            rd.last_dev = dv;
            num = num + dv * s;  // (k_qb_pick_all's one-term fold)
            den = den + fabs(s);
        }
        const double avg = A.scal[2 * b];
        const double wsd = den > 0 ? num / den : 0.0;
        p = avg + wsd * scale_fn(avg + wsd, avg);
    }
    const int64_t ob = w * (int64_t)cap;
    const bool by_weight = A.out.order == KNNCF_EXPLAIN_BY_WEIGHT && cap > 0;
    uint32_t* hist = s_hist[wave];
    if (by_weight) {
        for (int x = lane; x < 256; x += 64) hist[x] = 0;
        wave_sync();
    }
    int32_t total = 0;
    walk_terms(rd, lane, [&](int64_t p0, int32_t v, double s) {
        const bool nz = s != 0.0;
        const unsigned long long hit = __ballot(nz);
        if (nz) {
            if (by_weight) {
                atomicAdd(&hist[(uint32_t)(mag_key(s) >> 56)], 1u);
            } else {
                const int32_t place = total + lanes_below(hit);
                if (place < cap) {
                    A.out.raters[ob + place] = rd.raw(p0 + lane, v);
                    A.out.sims[ob + place] = s;
                    A.out.devs[ob + place] = rd.dev(p0 + lane, v);
                }
            }
        }
        total += __popcll(hit);
        return true;
    });
    if (by_weight && total > 0) explain_by_weight(rd, lane, total, A.out, A.st, ob, hist, s_abs[wave]);
    if (lane == 0) {
        A.out.counts[w] = total;
        A.out.sums[2 * w] = num;
        A.out.sums[2 * w + 1] = den;
        A.out.pred[w] = p;
    }
}

void foldin_batch_fold_all(const Train& tr, const PersonalRows& pr, QueryBatchScratch& bs, SortWorkspace& ws, int32_t C, int64_t n,
                           bool update, hipStream_t st) {
    const int32_t U = tr.U, I = tr.I;
    const int64_t W = ceil_div(I, 64), cells = (int64_t)C * I;
    int32_t stride = 1;
    while (stride < C) stride <<= 1;
    bs.suu.ensure(C); bs.simT.ensure((size_t)U * stride);
    bs.num.ensure(cells); bs.den.ensure(cells); bs.pred.ensure(cells); bs.rated.ensure(cells);
    const int32_t* self = update ? bs.self.p : nullptr;
    // S(u, u) of every slot (and the own cell of a fitted user), then the similarities side by side
    k_qb_self_keys<<<(unsigned)ceil_div(n, TPB), TPB, 0, st>>>(n, bs.slot.p, bs.items.p, bs.k64_a.p, bs.v32_a.p);
    sort_pairs_u64_u32(ws, bs.k64_a.p, bs.k64_b.p, bs.v32_a.p, bs.v32_b.p, (size_t)n, 32 + (C > 1 ? bits_for((uint64_t)(C - 1)) : 0), st);
    k_qb_self_sim<<<C, 64, 0, st>>>(U, tr.jaccard, bs.qo.p, bs.pre.p, bs.v32_b.p, self, bs.suu.p, bs.sim.p);
    k_qb_sim_transpose<<<(unsigned)ceil_div(U, 64), TPB, 0, st>>>(U, C, stride, bs.sim.p, bs.simT.p);
    KN_TRACE_DISPATCH("qb_fold_all stride=%d", (int)stride);
    k_qb_fold_all<<<(unsigned)ceil_div(I, FA_WAVES), FA_WAVES * 64, 0, st>>>(
        I, C, stride, W, tr.pop_item.p, tr.i_ptr.p, pr.pf_user.p, pr.pf_dev.p, bs.simT.p, (const unsigned long long*)bs.bits.p, bs.rank.p,
        bs.qo.p, update ? bs.ao.p : nullptr, self, bs.dev_d.p, bs.given_d.p, bs.suu.p, bs.num.p, bs.den.p);
    k_qb_pred<false><<<(unsigned)ceil_div(cells, TPB), TPB, 0, st>>>(C, I, W, bs.num.p, bs.den.p, (const unsigned long long*)bs.bits.p,
                                                                     bs.rank.p, bs.qo.p, bs.dev_d.p, bs.scal.p, bs.pred.p, bs.rated.p);
    if (bs.n_removed > 0)
        k_qb_gone_rated<<<(unsigned)ceil_div(bs.n_removed, TPB), TPB, 0, st>>>(bs.n_removed, I, bs.rm_slot.p, bs.rm_gone.p, bs.rated.p);
    KN_HIP(hipGetLastError());
}

void foldin_batch_pick_all(const Train& tr, QueryBatchScratch& bs, const int32_t* d_items, const int32_t* d_slot, int64_t m,
                           double* d_out, hipStream_t st) {
    if (m <= 0) return;
    k_qb_pick_all<<<(unsigned)ceil_div(m, TPB), TPB, 0, st>>>(m, d_items, d_slot, tr.i_table.p, table_cells(tr), tr.ikeys.p, tr.I,
                                                              bs.pred.p, bs.scal.p, bs.qo.p, bs.items.p, bs.dev.p, bs.suu.p, d_out);
    KN_HIP(hipGetLastError());
}

void foldin_batch_pick(const Train& tr, QueryBatchScratch& bs, const int32_t* d_items, const int32_t* d_slot, int64_t m,
                       double* d_out, hipStream_t st) {
    if (m <= 0) return;
    k_qb_pick<<<(unsigned)ceil_div(m, TPB), TPB, 0, st>>>(m, d_items, d_slot, tr.i_table.p, table_cells(tr), tr.ikeys.p, tr.I,
                                                          bs.pred.p, bs.scal.p, d_out);
    KN_HIP(hipGetLastError());
}

void foldin_batch_explain(const Train& tr, QueryBatchScratch& bs, const QbExplainRows& rows, const ExplainCells& out, hipStream_t st) {
    const int64_t n = rows.n;
    if (n <= 0) return;
    QbExplainArgs A{};
    A.items = rows.d_items; A.slot = rows.d_slot;
    A.i_table = tr.i_table.p; A.i_cells = table_cells(tr); A.ikeys = tr.ikeys.p;
    A.I = tr.I; A.take = rows.take; A.order = out.order; A.cap = out.cap;
    A.E = rows.E;
    A.key = bs.e_k64_b.p; A.val = bs.e_v32_b.p; A.edev = bs.e_dev.p; A.esim = bs.e_sim.p;
    A.ebase = bs.ebase.p; A.off = bs.off.p; A.nbr = bs.nbr_idx.p; A.uid = tr.uid.p;
    A.num = bs.num.p; A.den = bs.den.p; A.pred = bs.pred.p; A.scal = bs.scal.p;
    A.raters = out.raters; A.sims = out.sims; A.devs = out.devs; A.counts = out.counts; A.sums = out.sums; A.out_pred = out.pred;
    KN_TRACE_DISPATCH("qb_explain order=%d", (int)out.order);
    k_qb_explain<<<(unsigned)ceil_div(n, QBX_WAVES), QBX_WAVES * 64, 0, st>>>(A, rows.r0, n);
    KN_HIP(hipGetLastError());
}

void foldin_batch_explain_all(const Train& tr, const PersonalRows& pr, QueryBatchScratch& bs, const QbExplainRows& rows, bool update,
                              const ExplainCells& out, double* d_stage, hipStream_t st) {
    const int64_t n = rows.n;
    if (n <= 0) return;
    QbExplainAllArgs A{};
    A.items = rows.d_items; A.slot = rows.d_slot;
    A.i_table = tr.i_table.p; A.i_cells = table_cells(tr); A.ikeys = tr.ikeys.p;
    A.I = tr.I; A.U = tr.U; A.W = ceil_div(tr.I, 64);
    A.i_ptr = tr.i_ptr.p; A.pf_user = pr.pf_user.p; A.pf_dev = pr.pf_dev.p;
    A.sim = bs.sim.p; A.bits = (const unsigned long long*)bs.bits.p; A.rank = bs.rank.p; A.qo = bs.qo.p;
    A.ao = update ? bs.ao.p : nullptr; A.self = update ? bs.self.p : nullptr;
    A.dev_d = bs.dev_d.p; A.given_d = bs.given_d.p; A.suu = bs.suu.p; A.users = bs.users.p;
    A.q_items = bs.items.p; A.q_dev = bs.dev.p; A.uid = tr.uid.p;
    A.num = bs.num.p; A.den = bs.den.p; A.pred = bs.pred.p; A.scal = bs.scal.p;
    A.out = out;
    A.st = explain_stage(d_stage, n, out.cap);
    KN_TRACE_DISPATCH("qb_explain_all order=%d cap=%d rows=%lld", (int)out.order, (int)out.cap, (long long)n);
    k_qb_explain_all<<<(unsigned)ceil_div(n, QXA_WAVES), QXA_WAVES * 64, 0, st>>>(A, rows.r0, n);
    KN_HIP(hipGetLastError());
}

void foldin_batch_recommend(const Train& tr, QueryBatchScratch& bs, SortWorkspace& ws, int32_t C, int32_t n, int32_t* d_items,
                            double* d_preds, hipStream_t st) {
    const int32_t I = tr.I;
    const int64_t cells = (int64_t)C * I;
    // dense items by ascending raw id: the same for every slot
    bs.by_id.ensure(I);
    launch_reco_id_order(tr, ws, bs.k64_a.p, bs.k64_b.p, bs.v32_a.p, bs.by_id.p, st);
    k_qb_reco_keys<<<(unsigned)ceil_div(cells, TPB), TPB, 0, st>>>(C, I, bs.by_id.p, bs.pred.p, bs.rated.p, bs.k64_a.p, bs.v32_a.p);
    const uint32_t* order = qb_segmented_sort(bs, ws, C, I, st);
    k_qb_take<<<(unsigned)ceil_div((int64_t)C * n, TPB), TPB, 0, st>>>(C, n, I, (const long long*)bs.info.p, order, tr.iid.p,
                                                                       bs.pred.p, d_items, d_preds);
    KN_HIP(hipGetLastError());
}

void foldin_batch_reco_rows(QueryBatchScratch& bs, int32_t C, int32_t n, const int64_t* h_rb, const int32_t* d_items, hipStream_t st) {
    const int64_t rows = h_rb[C];
    if (rows <= 0) return;
    bs.reco_rb.ensure((size_t)C + 1); bs.pick_items.ensure((size_t)rows); bs.pick_slot.ensure((size_t)rows);
    KN_HIP(hipMemcpyAsync(bs.reco_rb.p, h_rb, ((size_t)C + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    KN_TRACE_DISPATCH("qb_reco_rows C=%d n=%d rows=%lld", (int)C, (int)n, (long long)rows);
    k_qb_reco_rows<<<(unsigned)ceil_div((int64_t)C * n, TPB), TPB, 0, st>>>(C, n, bs.reco_rb.p, d_items, bs.pick_items.p, bs.pick_slot.p);
    KN_HIP(hipGetLastError());
}

}  // namespace knncf
