// bystander.hip — bystander queries: the neighbours and kNN predictions of a FITTED user v once a newcomer q has joined the
// data, without a refit (DESIGN.md "Bystander queries"; knncf_query_bystander_*).
//
// The answers are those of the reference on aug = train ++ q's rows with fresh closures whose first evaluation is v's, so v
// owns every pair.  A chunk of foldin.hip carries both kinds of slot: the newcomer's own (a fold-in slot: its prepared row is
// what k_qb_prep makes) and one per bystander (an update slot with no additional row: v's train rows seeded on the device,
// S(v, x) for every train user x in bs.sim, v's top list without v itself in bs.nbr_idx / bs.nbr_sim).  What q adds to a
// bystander slot is computed here:
//   k_by_pair      S(v, q) from the two prepared rows, folded in v's item-set order
//   k_by_merge     (q, S(v, q)) into v's sorted list under (similarity descending, set order ascending); q is index U
//   k_by_offsets / k_by_gather   k_qb_offsets / k_qb_gather in which index U reads q's prepared row; its file rows are
//                  n_train + position, behind every train row: q's term is the last of an item's fold :520-524
//   k_by_pick      k_qb_pick in which an item that only q rates has that one term
// The sort of the gathered entries, k_q_fold and k_qb_pred of foldin.hip run between them unchanged.
//
// The changer may also be a user c of the fit that adds ratings (DESIGN.md "Bystanders of update queries";
// knncf_update_bystander_*).  Its own slot is then an update slot — train rows seeded, the additional rows behind them — and
// qidx[b], the changer's index of slot b, is dense(c) instead of U.  c is a train candidate of every bystander already:
//   k_by_pair      as above: c's side is its prepared row on aug
//   k_by_place     that value into cell [b][dense(c)] of bs.sim BEFORE the keys and the sorts: c keeps its place in set order,
//                  and when it leaves a full list the next candidate of the slot's row comes in.  No merge.
//   k_by_merge     for such a slot only looks c up in the written list (in_list for k_by_pick)
//   k_by_offsets / k_by_gather   index dense(c) reads c's prepared row: deviations on aug, a train row at its train file row,
//                  an additional row at n_train + its position among the additional rows
//
// A fitted changer may also REMOVE train rows (DESIGN.md "Bystanders of revise queries"; knncf_revise_bystander_*).  Its own slot
// is then a revise slot — k_qb_mark / k_qb_seed_rv leave the removed rows out — and everything above reads that prepared row:
//   k_by_gather    decides "train row or additional row" by the given position against the slot's LIVE train rows, so a removed
//                  row is no term and a re-rated item's term stands behind every train row
//   k_by_survivors average(aug) for the rows answered with it: the fold of the surviving train ratings in file order
// An item that only c rated and that c removed has no rater in aug: its cell of bs.pred folds nothing (den = 0: v's mean).
#include <math.h>

#include <algorithm>

#include "engine.h"
#include "qb_helpers.h"
#include "wave_helpers.h"

namespace knncf {

static constexpr int TPB = 256;

// One wave per bystander slot b (qslot[b] != b): S(v, q), v = the slot's fitted user and q = the newcomer of slot qslot[b].
// The wave walks q's known items in dense-item order 64 at a time (rank r of q's bitmap -> given position -> dense item),
// probes v's bitmap and folds pre_v * pre_q left in that order = v's trie order (v with > 4 ratings).  A v of <= 4 ratings
// iterates in its file order (Set1..Set4): the <= 4 products are kept by v's position and folded at the end, as k_query_sim
// does for the query side.  Jaccard counts the matches: |I(v) & I(q)| / (|I(v)| + |I(q)| - |I(v) & I(q)|) :446-463, |I(q)| with
// q's items unknown to train.
// Bounds.  b < C.  q's distinct known items number rank[qs][W] (the bitmap's population), and k_qb_scatter wrote given_d /
// pre_d of exactly those ranks; a given position is < the slot's rows, di of a known row is a dense item of [0, I).  A hit's
// rank in v's bitmap is < v's rows.  (info[4 qs + 1] is NOT used: it counts a repeated item twice.)
__global__ void __launch_bounds__(TPB) k_by_pair(int32_t C, int64_t W, bool jaccard, const int32_t* __restrict__ qslot,
                                                 const int64_t* __restrict__ qo, const int32_t* __restrict__ di,
                                                 const int32_t* __restrict__ given_d, const double* __restrict__ pre_d,
                                                 const unsigned long long* __restrict__ bits, const int64_t* __restrict__ rank,
                                                 double* __restrict__ pair) {
    const int lane = threadIdx.x & 63;
    const int32_t b = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (b >= C) return;
    const int32_t qs = qslot[b];
    if (qs == b) return;
    const int64_t oq = qo[qs], ov = qo[b];
    const int32_t nq = (int32_t)(qo[qs + 1] - oq), nv = (int32_t)(qo[b + 1] - ov);
    const int32_t kq = (int32_t)rank[(int64_t)qs * (W + 1) + W];
    const unsigned long long* vb = bits + (int64_t)b * W;
    const int64_t* vr = rank + (int64_t)b * (W + 1);
    const bool small = nv <= 4;
    double s = 0.0, x0 = 0.0, x1 = 0.0, x2 = 0.0, x3 = 0.0;
    uint32_t found = 0;
    int64_t both = 0;
    for (int32_t base = 0; base < kq; base += 64) {
        const int32_t r = base + lane;
        int32_t c = 0;
        bool hit = false;
        if (r < kq) {
            c = di[oq + given_d[oq + r]];
            hit = (vb[c >> 6] >> (c & 63)) & 1ull;
        }
        unsigned long long mask = __ballot(hit);
        if (jaccard) {
            both += __popcll(mask);
            continue;
        }
        double prod = 0.0;
        int32_t g = 0;
        if (hit) {
            const int32_t rv = bit_rank(vb, vr, c);
            prod = pre_d[ov + rv] * pre_d[oq + r];
            if (small) g = given_d[ov + rv];
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
        s = (double)both / (double)((int64_t)nv + (int64_t)nq - both);
    } else if (small) {
        if (found & 1u) s = s + x0;
        if (found & 2u) s = s + x1;
        if (found & 4u) s = s + x2;
        if (found & 8u) s = s + x3;
    }
    if (lane == 0) pair[b] = s;
}

// A fitted changer c of bystander slot b: S(v, c) on aug into the slot's similarity row, over the train value that the
// similarity kernel put there.  Runs after that kernel and before the keys, k_qb_mask_self and the sorts.
// Bounds.  b < C; qidx[b] < U is a dense user, so the cell is inside row b of sim [C][U].
__global__ void k_by_place(int32_t C, int32_t U, const int32_t* __restrict__ qslot, const int32_t* __restrict__ qidx,
                           const double* __restrict__ pair, double* __restrict__ sim) {
    const int32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= C || qslot[b] == b) return;
    const int32_t ci = qidx[b];
    if (ci >= 0 && ci < U) sim[(int64_t)b * U + ci] = pair[b];
}

// One wave per bystander slot b: (q, pair[b]) enters the slot's sorted list of L = min(take, U - 1) train users (k_qb_write;
// v itself is masked out).  (allUsers(aug) - v).toSeq is the train users in dense order with q in front of dense user
// qrank[b], and the stable sortWith keeps that order among equal similarities: an entry goes before q when its key is smaller,
// or equal with a dense index < qrank.  The list is sorted, so those entries are its first `pos`.  pos == take: q is not a
// neighbour (in_list[b] = +0.0).  Otherwise the entries from pos move one cell up — the last one drops out when the list was
// full (L == take), the list grows to L + 1 <= take when it was not (k >= U) — and q goes to cell pos as index U.
// The move runs from the top in blocks of 64 cells: every lane's store takes the value its own load returned, so a block's
// loads have all completed before its first store, and a block only writes cells that blocks above it have read already.
// Bounds.  Cells [0, L) are read, cells [pos, min(L + 1, take)) of the slot's `take` cells are written.
// A fitted changer (qidx[b] < U) sits in the list already where it belongs, or not at all: the wave only looks for it among
// the L written cells, in_list[b] = its similarity there (the list's, which is pair[b]) or +0.0.
__global__ void __launch_bounds__(TPB) k_by_merge(int32_t C, int32_t take, int32_t U, const int32_t* __restrict__ qslot,
                                                  const int32_t* __restrict__ qidx, const int32_t* __restrict__ qrank,
                                                  const double* __restrict__ pair, int32_t* __restrict__ nbr_idx,
                                                  double* __restrict__ nbr_sim, double* __restrict__ in_list) {
    const int lane = threadIdx.x & 63;
    const int32_t b = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (b >= C || qslot[b] == b) return;
    const int32_t L = min(take, U - 1), at = qrank[b];
    int32_t* idx = nbr_idx + (int64_t)b * take;
    double* sim = nbr_sim + (int64_t)b * take;
    const int32_t ci = qidx[b];
    if (ci != U) {
        for (int32_t base = 0; base < L; base += 64) {
            const int32_t j = base + lane;
            if (j < L && idx[j] == ci) in_list[b] = sim[j];  // (at most one cell holds c)
        }
        return;
    }
    const double s = pair[b];
    const uint64_t ks = by_sim_key(s);
    int32_t pos = 0;
    for (int32_t base = 0; base < L; base += 64) {
        const int32_t j = base + lane;
        bool first = false;
        if (j < L) {
            const uint64_t kj = by_sim_key(sim[j]);
            first = kj < ks || (kj == ks && idx[j] < at);
        }
        pos += __popcll(__ballot(first));
    }
    if (pos >= take) {
        if (lane == 0) in_list[b] = 0.0;
        return;
    }
    const int32_t last = min(L + 1, take) - 1;  // the top cell of the list afterwards
    for (int32_t top = last; top > pos; top -= 64) {
        const int32_t j = top - lane;
        if (j > pos) {
            const int32_t vi = idx[j - 1];
            const double vs = sim[j - 1];
            idx[j] = vi;
            sim[j] = vs;
        }
    }
    if (lane == 0) {
        idx[pos] = U;
        sim[pos] = s;
        in_list[b] = s;
    }
}

// k_qb_offsets for a chunk with bystander slots: off[b][0 .. take] and info[4 b + 2] of the slot's neighbours, where the
// changer's index qidx[b] stands for its distinct known items on aug.  The list of a newcomer's bystander has `take` cells,
// that of a fitted changer's min(take, U - 1).  A changer's own slot, a slot whose status is set and a bystander slot whose
// changer's status is set take no part in the prediction pass (0 entries).
__global__ void __launch_bounds__(ONE_BLOCK) k_by_offsets(int32_t take, int32_t U, int64_t W, const int32_t* __restrict__ qslot,
                                                          const int32_t* __restrict__ qidx, const int32_t* __restrict__ nbr,
                                                          const int64_t* __restrict__ u_ptr, const int64_t* __restrict__ rank,
                                                          int64_t* __restrict__ off, long long* __restrict__ info) {
    const int32_t b = blockIdx.x, qs = qslot[b], ci = qidx[b];
    const int32_t* mine = nbr + (int64_t)b * take;
    const int64_t live = (qs == b || info[4 * b] != 0 || info[4 * qs] != 0) ? 0 : (ci == U ? take : min(take, U - 1));
    const int64_t kq = rank[(int64_t)qs * (W + 1) + W];
    const int64_t total = block_exclusive_scan(
        take,
        [&](int64_t j) {
            if (j >= live) return (int64_t)0;
            const int32_t v = mine[j];
            return v == ci ? kq : u_ptr[v + 1] - u_ptr[v];
        },
        off + (int64_t)b * (take + 1));
    if (threadIdx.x == 0) info[4 * b + 2] = total;
}

// k_qb_gather in which neighbour index qidx[slot] is the changer: entry r of its extent is its r-th known item in dense order,
// with the deviation k_qb_scatter put there.  The given order of the changer's slot is its LIVE train rows in file order, then
// its additional rows (k_qb_seed / k_qb_seed_rv): live = the slot's rows - its additional rows, 0 for a newcomer, c's train
// rows for an update slot, fewer for a revise slot.  A given position g < live is a live train row: it stays at its train file
// row s_t, found in c's row of the fit (sorted by dense item) — removals keep the relative order of the other rows.  g >= live
// is an additional row, behind every train row: n_train + (g - live).  So a removed row is no term, and a re-rated item's term
// stands at its additional row, whatever c's row of the fit holds for the item.
// Bounds.  g < live only for a fitted c, whose live rows are rows of [u_ptr[c], u_ptr[c + 1]): the search finds the item there
// (tl >= live > 0; the index is clamped all the same).  g - live < the slot's additional rows <= 65536.
__global__ void __launch_bounds__(TPB) k_by_gather(int32_t C, int32_t take, int32_t U, int32_t I, uint32_t n_train,
                                                   const int32_t* __restrict__ qslot, const int32_t* __restrict__ qidx,
                                                   const int64_t* __restrict__ qo, const int64_t* __restrict__ ao,
                                                   const int32_t* __restrict__ di, const int32_t* __restrict__ given_d,
                                                   const double* __restrict__ dev_d, const int32_t* __restrict__ nbr,
                                                   const double* __restrict__ nsim, const int64_t* __restrict__ off,
                                                   const int64_t* __restrict__ ebase, const int64_t* __restrict__ u_ptr,
                                                   const int32_t* __restrict__ s_col, const uint32_t* __restrict__ s_t,
                                                   const double* __restrict__ s_dev, uint64_t* __restrict__ key,
                                                   uint32_t* __restrict__ val, double* __restrict__ edev, double* __restrict__ esim) {
    const int64_t g = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (g >= (int64_t)C * take) return;
    const int32_t sb = (int32_t)(g / take), j = (int32_t)(g - (int64_t)sb * take);
    const int64_t lo = off[(int64_t)sb * (take + 1) + j], hi = off[(int64_t)sb * (take + 1) + j + 1];
    if (hi == lo) return;  // (a slot that takes no part, or a neighbour without ratings)
    const int32_t v = nbr[g];
    const int64_t o = ebase[sb] + lo;
    const double sj = nsim[g];
    if (v == qidx[sb]) {
        const int32_t qs = qslot[sb];
        const int64_t oq = qo[qs], live = (qo[qs + 1] - oq) - (ao[qs + 1] - ao[qs]);
        const int64_t c0 = v == U ? 0 : u_ptr[v], tl = v == U ? 0 : u_ptr[v + 1] - c0;
        for (int64_t r = threadIdx.x & 63; r < hi - lo; r += 64) {
            const int32_t gv = given_d[oq + r], d = di[oq + gv];
            const int64_t x = o + r;
            uint32_t row = n_train + (uint32_t)(gv - live);
            if (gv < live && tl > 0) {
                int64_t a = 0, e = tl;
                while (a < e) {
                    const int64_t mid = (a + e) >> 1;
                    if (s_col[c0 + mid] < d) a = mid + 1;
                    else e = mid;
                }
                row = s_t[c0 + min(a, tl - 1)];
            }
            key[x] = ((uint64_t)((uint32_t)sb * (uint32_t)I + (uint32_t)d) << 32) | (uint64_t)row;
            val[x] = (uint32_t)x;
            edev[x] = dev_d[oq + r];
            esim[x] = sj;
        }
        return;
    }
    const int64_t b = u_ptr[v], e = u_ptr[v + 1];
    for (int64_t p = b + (threadIdx.x & 63); p < e; p += 64) {
        const int64_t x = o + (p - b);
        key[x] = ((uint64_t)((uint32_t)sb * (uint32_t)I + (uint32_t)s_col[p]) << 32) | (uint64_t)s_t[p];
        val[x] = (uint32_t)x;
        edev[x] = s_dev[p];
        esim[x] = sj;
    }
}

// requested raw items with their (bystander) slot: the dense item's prediction of k_qb_pred.  An item unknown to train has at
// most one rater in aug, the changer (a fitted one rates it in an additional row): its term dev_q(i) * S(v, q) when q is in
// v's list (in_list = S, else +0.0) is the whole fold :520-524, and without a non-zero S the answer is v's mean exactly
// (den = 0), as for an item unknown to aug
__global__ void k_by_pick(int64_t m, const int32_t* __restrict__ items, const int32_t* __restrict__ slot,
                          const int32_t* __restrict__ i_table, int32_t i_cells, const uint32_t* __restrict__ ikeys, int32_t I,
                          const int32_t* __restrict__ qslot, const int64_t* __restrict__ qo, const int32_t* __restrict__ q_items,
                          const double* __restrict__ q_dev, const double* __restrict__ in_list, const double* __restrict__ pred,
                          const double* __restrict__ scal, double* __restrict__ out) {
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
    const double avg = scal[2 * b], s = in_list[b];
    double a = 0.0, d = 0.0;
    const int32_t qs = qslot[b];
    for (int64_t x = qo[qs]; x < qo[qs + 1]; ++x) {
        if (q_items[x] == it) {
            a = a + q_dev[x] * s;
            d = d + fabs(s);
            break;
        }
    }
    const double w = d > 0 ? a / d : 0.0;
    out[j] = avg + w * scale_fn(avg + w, avg);
}

// average(aug) :18 of a revise query with removals divides the left fold from 0.0 of the SURVIVING train ratings in file order,
// continued over the additional ratings (the host continues it).  One workgroup per changer slot b = slots[blockIdx.x], a fitted
// user's revise slot whose status is clear: mark[so[b] + r] != 0 says that row r of its train row [u_ptr, u_ptr + tl) is removed
// (k_qb_mark), s_t its file row.
// EXACT (tr.exact_total: every rating is dyadic, the premise under which the fit itself sums with k_exact_sum): every partial
//   sum is exact, so the fold over the surviving rows is total - (the removed ratings summed in any order).
// otherwise: the removed file rows are collected into rows[so[b] ..) (any order), then k_sequential_sum's fold over the file in
//   which a removed rating is replaced by +0.0.  That is the fold without the row bit for bit: x + (+0.0) == x for every x but
//   -0.0, and a fold from +0.0 never holds -0.0 (a sum is -0.0 only when both operands are).
// Bounds.  r < tl <= so[b + 1] - so[b] (the slot's source rows are its train rows, then its additional rows), so the marks read
// and the cells of `rows` written — at most one per mark — lie inside the slot's extent of [so[C]].  A removed file row t is
// zeroed in buf only when c <= t < c + len.
static constexpr int AVG_CHUNK = 2048;
template <bool EXACT>
__global__ void __launch_bounds__(TPB) k_by_survivors(const int32_t* __restrict__ slots, const int64_t* __restrict__ so,
                                                      const int32_t* __restrict__ self, const int64_t* __restrict__ u_ptr,
                                                      const uint32_t* __restrict__ s_t, const double* __restrict__ s_rating,
                                                      const uint32_t* __restrict__ mark, int64_t n, const double* __restrict__ rating,
                                                      double total, uint32_t* __restrict__ rows, double* __restrict__ out) {
    __shared__ double buf[AVG_CHUNK];
    __shared__ int32_t gone;
    const int32_t b = slots[blockIdx.x], sd = self[b];
    const int64_t p0 = u_ptr[sd], tl = u_ptr[sd + 1] - p0, s0 = so[b];
    if (EXACT) {
        double acc = 0.0;
        for (int64_t r = threadIdx.x; r < tl; r += TPB)
            if (mark[s0 + r] != 0u) acc += s_rating[p0 + r];
        buf[threadIdx.x] = acc;
        __syncthreads();
        for (int o = TPB / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) buf[threadIdx.x] += buf[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[blockIdx.x] = total - buf[0];
        return;
    }
    if (threadIdx.x == 0) gone = 0;
    __syncthreads();
    for (int64_t r = threadIdx.x; r < tl; r += TPB)
        if (mark[s0 + r] != 0u) rows[s0 + atomicAdd(&gone, 1)] = s_t[p0 + r];
    __syncthreads();
    const int32_t m = gone;
    double acc = 0.0;
    for (int64_t c = 0; c < n; c += AVG_CHUNK) {
        const int32_t len = (int32_t)min((int64_t)AVG_CHUNK, n - c);
        for (int32_t j = threadIdx.x; j < len; j += TPB) buf[j] = rating[c + j];
        __syncthreads();
        for (int32_t x = threadIdx.x; x < m; x += TPB) {
            const int64_t t = (int64_t)rows[s0 + x] - c;
            if (t >= 0 && t < len) buf[t] = 0.0;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int32_t j = 0; j < len; ++j) acc = acc + buf[j];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

static int32_t table_cells(const Train& tr) { return (tr.u_table_n > 0 && tr.i_table_n > 0) ? tr.i_table_n : 0; }

void bystander_survivor_totals(const Train& tr, QueryBatchScratch& bs, const int32_t* h_slots, int32_t n_slots, double* h_out,
                               hipStream_t st) {
    KN_REQUIRE(n_slots > 0 && bs.by_chunk && bs.n_removed > 0, KNNCF_E_STATE, "bystander: survivor totals of a chunk without removals");
    bs.by_rf_slot.ensure(n_slots); bs.by_rf_out.ensure(n_slots); bs.by_rf_rows.ensure(bs.h_so.back());
    KN_HIP(hipMemcpyAsync(bs.by_rf_slot.p, h_slots, (size_t)n_slots * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (tr.exact_total)
        k_by_survivors<true><<<n_slots, TPB, 0, st>>>(bs.by_rf_slot.p, bs.so.p, bs.self.p, tr.u_ptr.p, tr.s_t.p, tr.s_rating.p,
                                                      bs.rm_mark.p, tr.n, tr.rating.p, tr.total, bs.by_rf_rows.p, bs.by_rf_out.p);
    else
        k_by_survivors<false><<<n_slots, TPB, 0, st>>>(bs.by_rf_slot.p, bs.so.p, bs.self.p, tr.u_ptr.p, tr.s_t.p, tr.s_rating.p,
                                                       bs.rm_mark.p, tr.n, tr.rating.p, tr.total, bs.by_rf_rows.p, bs.by_rf_out.p);
    KN_HIP(hipGetLastError());
    KN_HIP(hipMemcpyAsync(h_out, bs.by_rf_out.p, (size_t)n_slots * sizeof(double), hipMemcpyDeviceToHost, st));
    KN_HIP(hipStreamSynchronize(st));
}

void bystander_upload(QueryBatchScratch& bs, int32_t C, const ByChunk& by, hipStream_t st) {
    bs.by_qslot.ensure(C); bs.by_qidx.ensure(C); bs.by_qrank.ensure(C); bs.by_pair.ensure(C); bs.by_in.ensure(C);
    KN_TRACE_DISPATCH("bystander slots=%d fitted=%d merge=%d", (int)C, (int)by.fitted, (int)by.merged);
    KN_HIP(hipMemcpyAsync(bs.by_qslot.p, by.h_qslot, (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice, st));
    KN_HIP(hipMemcpyAsync(bs.by_qidx.p, by.h_qidx, (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice, st));
    KN_HIP(hipMemcpyAsync(bs.by_qrank.p, by.h_qrank, (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice, st));
    KN_HIP(hipMemsetAsync(bs.by_pair.p, 0, (size_t)C * sizeof(double), st));
    KN_HIP(hipMemsetAsync(bs.by_in.p, 0, (size_t)C * sizeof(double), st));
}

static void launch_pair(const Train& tr, QueryBatchScratch& bs, int32_t C, hipStream_t st) {
    k_by_pair<<<(unsigned)ceil_div(C, TPB / 64), TPB, 0, st>>>(C, ceil_div(tr.I, 64), tr.jaccard, bs.by_qslot.p, bs.qo.p, bs.di.p,
                                                               bs.given_d.p, bs.pre_d.p, (const unsigned long long*)bs.bits.p,
                                                               bs.rank.p, bs.by_pair.p);
}

void bystander_place(const Train& tr, QueryBatchScratch& bs, int32_t C, hipStream_t st) {
    launch_pair(tr, bs, C, st);
    k_by_place<<<(unsigned)ceil_div(C, TPB), TPB, 0, st>>>(C, tr.U, bs.by_qslot.p, bs.by_qidx.p, bs.by_pair.p, bs.sim.p);
    KN_HIP(hipGetLastError());
}

void bystander_merge(const Train& tr, QueryBatchScratch& bs, int32_t C, int32_t take, bool placed, hipStream_t st) {
    const int64_t W = ceil_div(tr.I, 64);
    const unsigned grid = (unsigned)ceil_div(C, TPB / 64);
    if (!placed) launch_pair(tr, bs, C, st);
    if (take > 0)
        k_by_merge<<<grid, TPB, 0, st>>>(C, take, tr.U, bs.by_qslot.p, bs.by_qidx.p, bs.by_qrank.p, bs.by_pair.p, bs.nbr_idx.p,
                                         bs.nbr_sim.p, bs.by_in.p);
    k_by_offsets<<<C, ONE_BLOCK, 0, st>>>(take, tr.U, W, bs.by_qslot.p, bs.by_qidx.p, bs.nbr_idx.p, tr.u_ptr.p, bs.rank.p, bs.off.p,
                                          (long long*)bs.info.p);
    KN_HIP(hipGetLastError());
}

void bystander_gather(const Train& tr, QueryBatchScratch& bs, int32_t C, int32_t take, hipStream_t st) {
    k_by_gather<<<(unsigned)ceil_div((int64_t)C * take, TPB / 64), TPB, 0, st>>>(
        C, take, tr.U, tr.I, (uint32_t)tr.n, bs.by_qslot.p, bs.by_qidx.p, bs.qo.p, bs.ao.p, bs.di.p, bs.given_d.p, bs.dev_d.p, bs.nbr_idx.p, bs.nbr_sim.p,
        bs.off.p, bs.ebase.p, tr.u_ptr.p, tr.s_col.p, tr.s_t.p, tr.s_dev.p, bs.e_k64_a.p, bs.e_v32_a.p, bs.e_dev.p, bs.e_sim.p);
}

void bystander_pick(const Train& tr, QueryBatchScratch& bs, const int32_t* d_items, const int32_t* d_slot, int64_t m, double* d_out,
                    hipStream_t st) {
    k_by_pick<<<(unsigned)ceil_div(m, TPB), TPB, 0, st>>>(m, d_items, d_slot, tr.i_table.p, table_cells(tr), tr.ikeys.p, tr.I,
                                                          bs.by_qslot.p, bs.qo.p, bs.items.p, bs.dev.p, bs.by_in.p, bs.pred.p,
                                                          bs.scal.p, d_out);
    KN_HIP(hipGetLastError());
}

}  // namespace knncf
