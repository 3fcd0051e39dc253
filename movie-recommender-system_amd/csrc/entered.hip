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
// Bounds.  g < C * U, so b < C and v < U.  q's distinct known items number kq = rank[b][W] <= its rows <= 4, and k_qb_scatter
// wrote given_d / pre_d of exactly those ranks; a given position is < the slot's rows and di of a known row is in [0, I).  The
// search stays inside [u_ptr[v], u_ptr[v + 1]).
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

}  // namespace knncf
