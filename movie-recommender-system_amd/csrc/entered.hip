// entered.hip — entered queries: which FITTED users' neighbour lists a newcomer q joins, without a refit (DESIGN.md "Entered
// queries"; knncf_query_entered*).
//
// Fitted user v is entered iff q occurs in getNeighbors(aug, k, sim)(v) :596-617 on closures of v's own, aug = train ++ q's rows.
// Adding q changes no fitted user's mean, deviations or preprocessed ratings, so v's list on aug is v's list on train with one
// more candidate, and the handle's neighbour table holds every v's list on train already (every list is built before a chunk
// runs; with no train user of <= 4 ratings a pair's fold order is the dense-item order from both sides, so the stored lists are
// the fresh-closure lists).  A chunk is a fold-in chunk of foldin.hip: k_qb_keys .. k_qb_scatter prepare each newcomer's row,
// k_query_sim / k_query_sim_dual leave S(q, v) for every train user in bs.sim [C][U].  Three stages follow, each a launch over the
// chunk (the second one a launch for the flags and one for their compaction):
//   k_en_pair    S(v, q) where it is not S(q, v) bit for bit: the adjusted cosine of a newcomer with <= 4 rows, which the
//                fold-in kernels fold in the newcomer's given order (Set1..Set4) and v folds in dense-item order
//   k_en_flag    one thread per (slot, v): the place rule against the last stored cell of v's list; a wave's ballot is one word
//                of the slot's bitmap of entered users
//   k_en_compact one workgroup per slot: the bitmap's rank prefixes (block_exclusive_scan), the entered users in dense order,
//                their number
//   k_en_place   one wave per reported (slot, v): q's position in v's list, the user it displaces, raw ids
#include <math.h>

#include <algorithm>

#include "engine.h"
#include "qb_helpers.h"
#include "wave_helpers.h"

namespace knncf {

static constexpr int TPB = 256;

// One thread per (slot b, dense user v) of a slot with <= 4 rows: S(v, q_b) as v's closure folds it — the left fold from 0.0
// of pre(v, i) * pre(q, i) over the common items in dense-item order (v has > 4 ratings: its item set iterates in trie order).
// q's <= 4 known items are walked in dense order (rank r -> given position -> dense item) and looked up in v's row, which is
// sorted by dense item.  A slot with more rows keeps bs.sim's cell: k_query_sim / k_query_sim_dual folded it in v's row order =
// dense-item order, the same products in the same order.
// The slot may be a newcomer's or a fitted changer's that its removals leave with <= 4 rows on aug (a revise slot): the fold-in
// kernels folded that cell in the slot's given order — live train rows in file order, then the additional rows — like a
// newcomer's, and pre_d holds c's preprocessed values ON AUG.  (Cell [b][self[b]] gets c's row on aug against its row of the
// fit: no stage reads it.)
// Bounds.  g < C * U, so b < C and v < U.  q's distinct known items number kq = rank[b][W] <= its rows <= 4, and k_qb_scatter
// wrote given_d / pre_d of exactly those ranks; a given position is < the slot's rows and di of a known row is in [0, I).  The
// search stays inside [u_ptr[v], u_ptr[v + 1]).
// A revise slot: the sorted SOURCE rows of the slot are [live train rows by file row, additional rows, dropped rows], of which
// k_qb_seed_rv copies the first qo[b + 1] - qo[b] into the chunk — the dropped rows never become chunk rows, whatever the
// removals were (a bad removal included: its slot keeps its declared extent).  So qo, di, given_d, pre_d and rank describe the
// live and additional rows only, exactly as for a newcomer: the bitmap's population counts distinct known items among those
// qo[b + 1] - qo[b] <= 4 rows, k_qb_scatter wrote ranks [0, kq) of the slot's extent, and every given position is < that extent.
__global__ void __launch_bounds__(TPB) k_en_pair(int32_t C, int32_t U, int64_t W, const int64_t* __restrict__ qo,
                                                 const int32_t* __restrict__ di, const int32_t* __restrict__ given_d,
                                                 const double* __restrict__ pre_d, const int64_t* __restrict__ rank,
                                                 const int64_t* __restrict__ u_ptr, const int32_t* __restrict__ s_col,
                                                 const double* __restrict__ s_pre, double* __restrict__ sim) {
    const int64_t g = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (g >= (int64_t)C * U) return;
    const int32_t b = (int32_t)(g / U), v = (int32_t)(g - (int64_t)b * U);
    const int64_t oq = qo[b];
    if (qo[b + 1] - oq > 4) return;
    const int32_t kq = (int32_t)rank[(int64_t)b * (W + 1) + W];
    const int64_t r0 = u_ptr[v], r1 = u_ptr[v + 1];
    double s = 0.0;
    for (int32_t r = 0; r < kq; ++r) {
        const int32_t c = di[oq + given_d[oq + r]];
        int64_t lo = r0, hi = r1;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (s_col[mid] < c) lo = mid + 1;
            else hi = mid;
        }
        if (lo < r1 && s_col[lo] == c) s = s + s_pre[lo] * pre_d[oq + r];
    }
    sim[g] = s;
}

// does the entry (x, sx) of a list go before the newcomer (set-order rank `at`, similarity key ks)?  k_by_merge's rule
__device__ __forceinline__ bool en_before(double sx, int32_t x, uint64_t ks, int32_t at) {
    const uint64_t kx = by_sim_key(sx);
    return kx < ks || (kx == ks && x < at);
}

// One thread per (slot b, dense user v), a wave per 64 consecutive users of one slot (rows padded to Upad = 64 ceil(U / 64)
// threads).  v's stored list is sorted by the place rule's order, so the entries that go before q are a prefix of it: q is
// entered iff the list is not full (cnt[v] < take: k >= U, every user is entered) or its last cell does not go before q.  The
// wave's ballot is word v / 64 of the slot's bitmap of entered users.
// Bounds.  g < C * Upad, so b < C; a lane with v >= U votes 0 and reads nothing.  A full list has cnt[v] == take == kcap >= 1
// cells (take > 0 is the launcher's), so its last cell is v * kcap + take - 1 < U * kcap.  Word v / 64 < Upad / 64 = Wu.
__global__ void __launch_bounds__(TPB) k_en_flag(int32_t C, int32_t U, int32_t take, int32_t kcap, const int32_t* __restrict__ qrank,
                                                 const double* __restrict__ sim, const int32_t* __restrict__ cnt,
                                                 const int32_t* __restrict__ idx, const double* __restrict__ nsim,
                                                 unsigned long long* __restrict__ bits) {
    const int64_t Wu = ((int64_t)U + 63) >> 6, Upad = Wu << 6;
    const int64_t g = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (g >= (int64_t)C * Upad) return;  // (whole waves: C * Upad is a multiple of 64)
    const int32_t b = (int32_t)(g / Upad), v = (int32_t)(g - (int64_t)b * Upad);
    bool f = false;
    if (v < U) {
        f = true;
        if (cnt[v] >= take) {
            const int64_t last = (int64_t)v * kcap + take - 1;
            f = !en_before(nsim[last], idx[last], by_sim_key(sim[(int64_t)b * U + v]), qrank[b]);
        }
    }
    const unsigned long long word = __ballot(f);
    if ((threadIdx.x & 63) == 0) bits[(int64_t)b * Wu + (v >> 6)] = word;
}

// One workgroup per slot b: the rank prefixes of the slot's bitmap (block_exclusive_scan over its Wu words, as k_qb_rank makes
// those of an item bitmap); entered user v is the bit_rank(v)-th entered user of the slot in dense order and goes to that cell
// of the slot's row when it is one of the `width` reported cells.  counts[b] = the bitmap's population.  The order comes from
// the scan alone: no atomics.
// Bounds.  v < U, word v / 64 < Wu.  pre holds Wu + 1 cells per slot; a written cell j < width lies in the slot's row of ent.
__global__ void __launch_bounds__(ONE_BLOCK) k_en_compact(int32_t U, int32_t width, const unsigned long long* __restrict__ bits,
                                                          int64_t* __restrict__ pre, int32_t* __restrict__ ent,
                                                          int32_t* __restrict__ counts) {
    const int64_t Wu = ((int64_t)U + 63) >> 6;
    const int32_t b = blockIdx.x;
    const unsigned long long* mine = bits + (int64_t)b * Wu;
    int64_t* p = pre + (int64_t)b * (Wu + 1);
    const int64_t total = block_exclusive_scan(Wu, [&](int64_t w) { return (int64_t)__popcll(mine[w]); }, p);
    __syncthreads();
    for (int32_t v = threadIdx.x; v < U; v += ONE_BLOCK) {
        if (!((mine[v >> 6] >> (v & 63)) & 1ull)) continue;
        const int32_t j = bit_rank(mine, p, v);
        if (j < width) ent[(int64_t)b * width + j] = v;
    }
    if (threadIdx.x == 0) counts[b] = (int32_t)total;
}

// One wave per reported cell (slot b, j): v = the slot's j-th entered user.  pos = the entries of v's list that go before q,
// counted 64 cells at a time as k_by_merge counts them; displaced = the last entry of a full list, which q pushes out, or -1
// when the list grows (k >= U).  The cell's dense user is replaced by its raw id.
// Bounds.  g < C * width; only cells j < counts[b] hold a user (k_en_compact), v < U.  Cells [0, cnt[v]) of v's kcap are read,
// cnt[v] <= kcap.
__global__ void __launch_bounds__(TPB) k_en_place(int32_t C, int32_t U, int32_t take, int32_t kcap, int32_t width,
                                                  const int32_t* __restrict__ qrank, const double* __restrict__ sim,
                                                  const int32_t* __restrict__ cnt, const int32_t* __restrict__ idx,
                                                  const double* __restrict__ nsim, const int32_t* __restrict__ uid,
                                                  const int32_t* __restrict__ counts, int32_t* __restrict__ ent,
                                                  double* __restrict__ osim, int32_t* __restrict__ opos, int32_t* __restrict__ odisp) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (g >= (int64_t)C * width) return;
    const int32_t b = (int32_t)(g / width), j = (int32_t)(g - (int64_t)b * width);
    if (j >= counts[b]) return;
    const int32_t v = __builtin_amdgcn_readfirstlane(ent[g]);
    const int32_t L = __builtin_amdgcn_readfirstlane(cnt[v]), at = qrank[b];
    const double s = sim[(int64_t)b * U + v];
    const uint64_t ks = by_sim_key(s);
    const int32_t* li = idx + (int64_t)v * kcap;
    const double* ls = nsim + (int64_t)v * kcap;
    int32_t pos = 0;
    for (int32_t base = 0; base < L; base += 64) {
        const int32_t c = base + lane;
        const bool first = c < L && en_before(ls[c], li[c], ks, at);
        pos += __popcll(__ballot(first));
    }
    if (lane == 0) {
        ent[g] = uid[v];
        osim[g] = s;
        opos[g] = pos;
        odisp[g] = (L == take && L > 0) ? uid[li[L - 1]] : -1;
    }
}

void entered_chunk(const Train& tr, const NeighborTable& nt, QueryBatchScratch& bs, int32_t C, int32_t take, int32_t width,
                   const int64_t* h_qo, const int32_t* h_qrank, hipStream_t st) {
    const int32_t U = tr.U;
    const int64_t W = ceil_div(tr.I, 64);
    bs.by_qrank.ensure(C);
    bs.en_pack.ensure((entered_pack_bytes(C, width) + 7) / 8);
    const EnteredPack out = entered_pack(bs.en_pack.p, C, width);
    KN_HIP(hipMemcpyAsync(bs.by_qrank.p, h_qrank, (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice, st));
    bool small = false;
    for (int32_t b = 0; b < C; ++b) small |= h_qo[b + 1] - h_qo[b] <= 4;
    if (small && !tr.jaccard)  // (a ratio of counts has no order: bs.sim's cell is S(v, q) whatever the rows)
        k_en_pair<<<(unsigned)ceil_div((int64_t)C * U, TPB), TPB, 0, st>>>(C, U, W, bs.qo.p, bs.di.p, bs.given_d.p, bs.pre_d.p, bs.rank.p,
                                                                           tr.u_ptr.p, tr.s_col.p, tr.s_pre.p, bs.sim.p);
    // the bitmaps [C][Wu] and their rank prefixes [C][Wu + 1] lie in the chunk's sort keys ([C * max(U, I)] cells each), which are
    // free once the similarities stand
    const int64_t Wu = ceil_div(U, 64);
    unsigned long long* ebits = (unsigned long long*)bs.k64_b.p;
    k_en_flag<<<(unsigned)ceil_div((int64_t)C * Wu * 64, TPB), TPB, 0, st>>>(C, U, take, nt.kcap, bs.by_qrank.p, bs.sim.p, nt.cnt.p, nt.idx.p,
                                                                             nt.sim.p, ebits);
    k_en_compact<<<C, ONE_BLOCK, 0, st>>>(U, width, ebits, (int64_t*)bs.k64_a.p, out.users, out.counts);
    if (width > 0)
        k_en_place<<<(unsigned)ceil_div((int64_t)C * width, TPB / 64), TPB, 0, st>>>(C, U, take, nt.kcap, width, bs.by_qrank.p, bs.sim.p,
                                                                                    nt.cnt.p, nt.idx.p, nt.sim.p, tr.uid.p, out.counts,
                                                                                    out.users, out.sims, out.pos, out.displaced);
    KN_HIP(hipGetLastError());
}

// ---- entered queries of update queries (DESIGN.md "Entered queries of update queries"; knncf_update_entered*) ----------------
// The changer c of a slot may be a user of the fit (self[b] = dense(c) >= 0): it stands in stored lists already, so it can move
// or leave as well as enter.  Adding rows to c changes c's mean and deviations only: S(v, x) of every other pair is the fit's,
// and v's list on aug is v's list on train with one candidate's key changed.  bs.sim [C][U] holds S(c, v) on aug (an update
// chunk of foldin.hip), which is S(v, c) bit for bit under the handles the call accepts.  The stages:
//   k_enu_locate  was[b][v] = the cell of v's stored list that holds dense(c_b), one pass over nt.idx for the whole chunk
//   k_enu_flag    one thread per (slot, v): the report rule; the ballots are the slot's bitmap (k_en_compact is reused)
//   k_enu_place   one wave per reported cell: the five outputs; a cell the stored list cannot decide is marked EN_TAIL
// A slot with self[b] < 0 is a newcomer's: was = -1 everywhere, and the three kernels do what k_en_flag / k_en_place do.
//
// ---- entered queries of revise queries (DESIGN.md "Entered queries of revise queries"; knncf_revise_entered*) ----------------
// A fitted changer may also REMOVE train rows: its slot is a revise slot of foldin.hip, and bs.sim holds S(c, v) on aug = train
// without those rows ++ the additional ones.  Removing rows of c changes c's mean, deviations and norm only, like adding some:
// every other pair, c's place in set order and the stored lists are the fit's, so the stages above answer it.  Two things differ:
//   k_en_pair   also runs for a fitted changer that falls to <= 4 rows on aug — its cell was folded in c's given order
//   k_enu_flag  is silent for a fitted slot only when it has neither additional rows nor removals (aug is train)

static constexpr int LOC_BITS = 32768;  // cells of k_enu_locate's filter: 4 KB of LDS whatever U is

// One wave per fitted user v (grid-stride), a workgroup's four waves share the chunk's changers: who[b] = self[b] and a filter
// of LOC_BITS bits over dense user mod LOC_BITS.  A cell of v's list probes the filter; a hit (a changer, or one of the C / 32768
// of the other users that share a changer's bit) is compared with the <= 64 changers themselves, and each slot whose changer it
// is gets the cell's position.  One raw id may be the changer of several slots.  was [C][U] is -1 beforehand (the launcher's).
// Bounds.  C <= QB_MAX_CHUNK = 64 <= TPB.  v < U; cells [0, min(cnt[v], kcap)) of v's kcap are read; a stored id is a dense
// user of [0, U), so the filter index is < LOC_BITS and the written cell b * U + v < C * U.
__global__ void __launch_bounds__(TPB) k_enu_locate(int32_t C, int32_t U, int32_t kcap, const int32_t* __restrict__ self,
                                                    const int32_t* __restrict__ cnt, const int32_t* __restrict__ idx,
                                                    int32_t* __restrict__ was) {
    __shared__ uint32_t filt[LOC_BITS / 32];
    __shared__ int32_t who[QB_MAX_CHUNK];
    for (int i = threadIdx.x; i < LOC_BITS / 32; i += TPB) filt[i] = 0u;
    __syncthreads();
    if ((int32_t)threadIdx.x < C) {
        const int32_t c = self[threadIdx.x];
        who[threadIdx.x] = c;
        if (c >= 0) atomicOr(&filt[((uint32_t)c & (LOC_BITS - 1)) >> 5], 1u << (c & 31));
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int64_t v = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); v < U; v += (int64_t)gridDim.x * (TPB / 64)) {
        const int32_t L = min(cnt[v], kcap);
        const int32_t* li = idx + v * kcap;
        for (int32_t j = lane; j < L; j += 64) {
            const int32_t x = li[j];
            if (!((filt[((uint32_t)x & (LOC_BITS - 1)) >> 5] >> (x & 31)) & 1u)) continue;
            for (int32_t b = 0; b < C; ++b)
                if (who[b] == x) was[(int64_t)b * U + v] = j;
        }
    }
}

// One thread per (slot b, dense user v), laid out as k_en_flag's.  v is reported iff c occurs in its list on train or on aug,
// but for a c that stays where it is with a similarity of +-0.0 of the same bits (no term of any fold), and for a fitted c
// without additional rows and without removals (aug is train; ao [C + 1] = the first additional row of each slot, as the
// update chunk uploaded it; ro [C + 1] = the first removed item of each slot, null for a chunk without removals).
//   was < 0   c is not in the stored list: it enters under k_en_flag's rule, `at` = dense(c) for a fitted c (its place in set
//             order), the number of train users in front of it for a newcomer
//   was >= 0  c is in the stored list, so v is reported unless the new similarity has the stored cell's bits (the same key, the
//             same place) and is +-0.0
// Bounds.  As k_en_flag; was[b * U + v] and sim[b * U + v] with b < C, v < U; the stored cell v * kcap + was < U * kcap; ao and
// ro hold C + 1 cells.
__global__ void __launch_bounds__(TPB) k_enu_flag(int32_t C, int32_t U, int32_t take, int32_t kcap, const int32_t* __restrict__ self,
                                                  const int32_t* __restrict__ qrank, const int64_t* __restrict__ ao,
                                                  const int64_t* __restrict__ ro, const double* __restrict__ sim,
                                                  const int32_t* __restrict__ was,
                                                  const int32_t* __restrict__ cnt, const int32_t* __restrict__ idx,
                                                  const double* __restrict__ nsim, unsigned long long* __restrict__ bits) {
    const int64_t Wu = ((int64_t)U + 63) >> 6, Upad = Wu << 6;
    const int64_t g = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (g >= (int64_t)C * Upad) return;  // (whole waves: C * Upad is a multiple of 64)
    const int32_t b = (int32_t)(g / Upad), v = (int32_t)(g - (int64_t)b * Upad);
    bool f = false;
    if (v < U && v != self[b] && (ao[b + 1] > ao[b] || (ro && ro[b + 1] > ro[b]))) {
        const double s = sim[(int64_t)b * U + v];
        const int32_t w = was[(int64_t)b * U + v];
        if (w >= 0) {
            f = __double_as_longlong(s) != __double_as_longlong(nsim[(int64_t)v * kcap + w]) || s != 0.0;
        } else {
            f = true;
            if (cnt[v] >= take) {
                const int64_t last = (int64_t)v * kcap + take - 1;
                f = !en_before(nsim[last], idx[last], by_sim_key(s), qrank[b]);
            }
        }
    }
    const unsigned long long word = __ballot(f);
    if ((threadIdx.x & 63) == 0) bits[(int64_t)b * Wu + (v >> 6)] = word;
}

// One wave per reported cell (slot b, j), as k_en_place.  p = the OTHER entries of v's stored list that go before c's new key
// (the list is sorted, c's own cell is skipped), counted 64 cells at a time.
//   was < 0   k_en_place's answer: pos = p, other = the last entry of a full list; prev = -1
//   was >= 0  prev = was.  The list is not full, or p < take - 1: c stands at p on aug.  Otherwise c sorts behind every other
//             stored entry of a full list.  It keeps the last cell when no user is outside the list (take >= U - 1), or when it
//             held the last cell on train and its key did not get worse: every user outside goes behind c's old place.
//             Else the best candidate outside decides, which the handle does not have: pos = EN_TAIL, for the host to resolve.
// Bounds.  As k_en_place.
__global__ void __launch_bounds__(TPB) k_enu_place(int32_t C, int32_t U, int32_t take, int32_t kcap, int32_t width,
                                                   const int32_t* __restrict__ qrank, const double* __restrict__ sim,
                                                   const int32_t* __restrict__ was, const int32_t* __restrict__ cnt,
                                                   const int32_t* __restrict__ idx, const double* __restrict__ nsim,
                                                   const int32_t* __restrict__ uid, const int32_t* __restrict__ counts,
                                                   int32_t* __restrict__ ent, double* __restrict__ osim, int32_t* __restrict__ opos,
                                                   int32_t* __restrict__ oother, int32_t* __restrict__ oprev) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (g >= (int64_t)C * width) return;
    const int32_t b = (int32_t)(g / width), j = (int32_t)(g - (int64_t)b * width);
    if (j >= counts[b]) return;
    const int32_t v = __builtin_amdgcn_readfirstlane(ent[g]);
    const int32_t L = __builtin_amdgcn_readfirstlane(min(cnt[v], kcap)), at = qrank[b];
    const int32_t w = __builtin_amdgcn_readfirstlane(was[(int64_t)b * U + v]);
    const double s = sim[(int64_t)b * U + v];
    const uint64_t ks = by_sim_key(s);
    const int32_t* li = idx + (int64_t)v * kcap;
    const double* ls = nsim + (int64_t)v * kcap;
    int32_t p = 0;
    for (int32_t base = 0; base < L; base += 64) {
        const int32_t c = base + lane;
        const bool first = c < L && c != w && en_before(ls[c], li[c], ks, at);
        p += __popcll(__ballot(first));
    }
    if (lane != 0) return;
    const bool full = L >= take && L > 0;
    int32_t pos = p, other = -1;
    if (w < 0) {
        if (full) other = uid[li[L - 1]];
    } else if (full && p >= take - 1) {
        const bool kept = take >= U - 1 || (w == take - 1 && ks <= by_sim_key(ls[w]));
        if (!kept) pos = EN_TAIL;
    }
    ent[g] = uid[v];
    osim[g] = s;
    opos[g] = pos;
    oother[g] = other;
    oprev[g] = w;
}

// phase 1 of an update or revise chunk: S(v, c) where it is not bs.sim's cell, the stored cell of every fitted changer (was
// [C][U]) and the report bitmaps [C][ceil(U / 64)], which are returned.  *was_out = was; *fitted_out / *pair_out / *small_out =
// the chunk's fitted changers, whether k_en_pair ran and the fitted changers of <= 4 rows on aug (the caller's trace lines).
static unsigned long long* enu_phase1(const Train& tr, const NeighborTable& nt, QueryBatchScratch& bs, int32_t C, int32_t take,
                                      const int64_t* h_qo, const int32_t* h_self, const int32_t* h_qrank, int32_t** was_out,
                                      int32_t* fitted_out, bool* pair_out, int32_t* small_out, hipStream_t st) {
    const int32_t U = tr.U;
    const int64_t W = ceil_div(tr.I, 64);
    bs.by_qrank.ensure(C);
    KN_HIP(hipMemcpyAsync(bs.by_qrank.p, h_qrank, (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice, st));
    // a slot of <= 4 rows on aug folds in its given order (k_en_pair): a newcomer, or a fitted changer whose removals leave it
    // that few (a fitted cosine changer has > 4 TRAIN rows on the accepted handles, so without removals there is none)
    bool small = false;
    int32_t fitted = 0, small_fitted = 0;
    for (int32_t b = 0; b < C; ++b) {
        const bool few = h_qo[b + 1] - h_qo[b] <= 4;
        small |= few;
        fitted += h_self[b] >= 0;
        small_fitted += h_self[b] >= 0 && few;
    }
    if (small && !tr.jaccard)  // (slots of > 4 rows return at once: their cell stays)
        k_en_pair<<<(unsigned)ceil_div((int64_t)C * U, TPB), TPB, 0, st>>>(C, U, W, bs.qo.p, bs.di.p, bs.given_d.p, bs.pre_d.p, bs.rank.p,
                                                                           tr.u_ptr.p, tr.s_col.p, tr.s_pre.p, bs.sim.p);
    // the bitmaps and their prefixes as entered_chunk keeps them; was [C][U] lies in the chunk's sort values ([C * max(U, I)]
    // 32-bit cells), free like the keys
    const int64_t Wu = ceil_div(U, 64);
    unsigned long long* ebits = (unsigned long long*)bs.k64_b.p;
    int32_t* was = (int32_t*)bs.v32_a.p;
    KN_HIP(hipMemsetAsync(was, 0xff, (size_t)C * U * sizeof(int32_t), st));  // -1
    if (fitted > 0)
        k_enu_locate<<<(unsigned)std::min<int64_t>(ceil_div(U, TPB / 64), 4096), TPB, 0, st>>>(C, U, nt.kcap, bs.self.p, nt.cnt.p,
                                                                                              nt.idx.p, was);
    // (bs.ro holds the chunk's removed CSR only when the chunk has removals: foldin_batch_neighbors uploads it then)
    const int64_t* ro = bs.n_removed > 0 ? bs.ro.p : nullptr;
    k_enu_flag<<<(unsigned)ceil_div((int64_t)C * Wu * 64, TPB), TPB, 0, st>>>(C, U, take, nt.kcap, bs.self.p, bs.by_qrank.p, bs.ao.p, ro,
                                                                              bs.sim.p, was, nt.cnt.p, nt.idx.p, nt.sim.p, ebits);
    KN_HIP(hipGetLastError());
    *was_out = was;
    *pair_out = small && !tr.jaccard;
    *fitted_out = fitted;
    *small_out = small_fitted;
    return ebits;
}

void entered_update_chunk(const Train& tr, const NeighborTable& nt, QueryBatchScratch& bs, int32_t C, int32_t take, int32_t width,
                          const int64_t* h_qo, const int32_t* h_self, const int64_t* h_ro, const int32_t* h_qrank, hipStream_t st) {
    const int32_t U = tr.U;
    bs.en_pack.ensure((entered_update_pack_bytes(C, width) + 7) / 8);
    const EnteredPack out = entered_pack(bs.en_pack.p, C, width);
    int32_t* prev = entered_pack_prev(out, C);
    int32_t* was = nullptr;
    int32_t fitted = 0, small = 0;
    bool pair = false;
    unsigned long long* ebits = enu_phase1(tr, nt, bs, C, take, h_qo, h_self, h_qrank, &was, &fitted, &pair, &small, st);
    KN_TRACE_DISPATCH("entered_update slots=%d fitted=%d pair=%d width=%d", (int)C, (int)fitted, (int)pair, (int)width);
    if (h_ro[C] > 0) {  // (a chunk that holds a changer with removals)
        int32_t revise_slots = 0;
        for (int32_t b = 0; b < C; ++b) revise_slots += h_ro[b + 1] > h_ro[b];
        KN_TRACE_DISPATCH("entered_revise slots=%d removed=%lld small=%d", (int)revise_slots, (long long)h_ro[C], (int)small);
    }
    k_en_compact<<<C, ONE_BLOCK, 0, st>>>(U, width, ebits, (int64_t*)bs.k64_a.p, out.users, out.counts);
    if (width > 0)
        k_enu_place<<<(unsigned)ceil_div((int64_t)C * width, TPB / 64), TPB, 0, st>>>(C, U, take, nt.kcap, width, bs.by_qrank.p, bs.sim.p,
                                                                                     was, nt.cnt.p, nt.idx.p, nt.sim.p, tr.uid.p, out.counts,
                                                                                     out.users, out.sims, out.pos, out.displaced, prev);
    KN_HIP(hipGetLastError());
}

const unsigned long long* entered_update_flags(const Train& tr, const NeighborTable& nt, QueryBatchScratch& bs, int32_t C, int32_t take,
                                               const int64_t* h_qo, const int32_t* h_self, const int32_t* h_qrank, hipStream_t st) {
    int32_t* was = nullptr;
    int32_t fitted = 0, small = 0;
    bool pair = false;
    return enu_phase1(tr, nt, bs, C, take, h_qo, h_self, h_qrank, &was, &fitted, &pair, &small, st);
}

}  // namespace knncf
