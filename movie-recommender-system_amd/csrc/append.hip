// append.hip — knncf_append: new ratings go into the fit and the neighbour lists they cannot change are kept (DESIGN.md
// "Append").
//
// api.cpp runs the changers through update chunks of foldin.hip and the first stage of entered.hip's update pass
// (entered_update_flags): per chunk a bitmap of the fitted users whose list holds the changer on train or on aug.  The kernels
// here do the rest, all over the OLD fit's dense users:
//   k_ap_mark     stale |= the OR of a chunk's bitmaps, and the chunk's fitted changers; the mask stays on the device
//   k_ap_sets     kept = built and not stale (K), gone = built and stale (B ∩ S), one ballot per 64 users
//   k_ap_report   one workgroup: |K|, |B ∩ S| and the raw ids of B ∩ S in dense order (block_exclusive_scan, no atomics)
//   k_ap_raw_keys / k_ap_number   the users by ascending raw id (one radix sort), the rank of every kept one among K: its build
//                 number, as knncf_neighbors_batch over K in ascending raw id gives it
//   k_ap_remap    old dense user -> new dense user: the lower bound of its trie key among the new fit's keys (monotone)
//   k_ap_carry    the table moves (a user joined): one wave per kept row, ids through the map, similarities verbatim
//   k_ap_clear    the table stays: the rows outside K lose their length and build number
// Stores are vector stores and atomicOr on global memory.
#include <algorithm>

#include "engine.h"
#include "qb_helpers.h"

namespace knncf {

static constexpr int TPB = 256;

__device__ __forceinline__ bool ap_bit(const unsigned long long* __restrict__ bits, int32_t v) { return (bits[v >> 6] >> (v & 63)) & 1ull; }

// One thread per word w of the mask: the OR of the chunk's C rows.  The first C threads of workgroup 0 add the fitted changers.
// Both go through atomicOr: a changer's word is some other thread's word.
// Bounds.  w < Wu, b < C: cell b * Wu + w of the [C][Wu] bitmaps.  C <= QB_MAX_CHUNK = 64 <= TPB; self[b] is -1 or a dense user
// of [0, U), whose word is < Wu.
__global__ void __launch_bounds__(TPB) k_ap_mark(int64_t Wu, int32_t C, const unsigned long long* __restrict__ bits,
                                                 const int32_t* __restrict__ self, unsigned long long* __restrict__ stale) {
    const int64_t w = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (w < Wu) {
        unsigned long long acc = 0ull;
        for (int32_t b = 0; b < C; ++b) acc |= bits[(int64_t)b * Wu + w];
        if (acc) atomicOr(&stale[w], acc);
    }
    if (blockIdx.x == 0 && (int32_t)threadIdx.x < C) {
        const int32_t c = self[threadIdx.x];
        if (c >= 0) atomicOr(&stale[c >> 6], 1ull << (c & 63));
    }
}

// One thread per dense user, padded to whole waves (k_en_flag's layout): a wave's two ballots are word v / 64 of kept and gone.
// Bounds.  g < Wu * 64; a lane with v >= U votes 0 and reads nothing; word v / 64 < Wu.
__global__ void __launch_bounds__(TPB) k_ap_sets(int32_t U, int32_t all, const int64_t* __restrict__ seq,
                                                 const unsigned long long* __restrict__ stale, unsigned long long* __restrict__ kept,
                                                 unsigned long long* __restrict__ gone) {
    const int64_t Wu = ((int64_t)U + 63) >> 6;
    const int64_t g = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (g >= Wu * 64) return;  // (whole waves)
    const int32_t v = (int32_t)g;
    const bool built = v < U && seq[v] >= 0;
    const bool st = built && (all || ap_bit(stale, v));
    const unsigned long long k = __ballot(built && !st), d = __ballot(st);
    if ((threadIdx.x & 63) == 0) {
        kept[v >> 6] = k;
        gone[v >> 6] = d;
    }
}

// One workgroup: totals[0] = |K|, totals[1] = |B ∩ S|; the j-th user of B ∩ S in dense order goes to cell j < cap as its raw id.
// Bounds.  pre holds Wu + 1 cells; v < U; a written cell j < cap.
__global__ void __launch_bounds__(ONE_BLOCK) k_ap_report(int32_t U, int64_t cap, const unsigned long long* __restrict__ kept,
                                                         const unsigned long long* __restrict__ gone, const int32_t* __restrict__ uid,
                                                         int64_t* __restrict__ pre, int32_t* __restrict__ dropped,
                                                         int64_t* __restrict__ totals) {
    const int64_t Wu = ((int64_t)U + 63) >> 6;
    const int64_t n_kept = block_exclusive_scan(Wu, [&](int64_t w) { return (int64_t)__popcll(kept[w]); }, pre);
    __syncthreads();
    const int64_t n_gone = block_exclusive_scan(Wu, [&](int64_t w) { return (int64_t)__popcll(gone[w]); }, pre);
    __syncthreads();
    for (int32_t v = threadIdx.x; v < U; v += ONE_BLOCK) {
        if (!ap_bit(gone, v)) continue;
        const int32_t j = bit_rank(gone, pre, v);
        if (j < cap) dropped[j] = uid[v];
    }
    if (threadIdx.x == 0) {
        totals[0] = n_kept;
        totals[1] = n_gone;
    }
}

// sort keys of the users by raw id: the sign bit flipped, so that the unsigned order is the signed one
__global__ void __launch_bounds__(TPB) k_ap_raw_keys(int32_t U, const int32_t* __restrict__ uid, uint32_t* __restrict__ key,
                                                     uint32_t* __restrict__ val) {
    const int32_t v = blockIdx.x * TPB + threadIdx.x;
    if (v >= U) return;
    key[v] = (uint32_t)uid[v] ^ 0x80000000u;
    val[v] = (uint32_t)v;
}

// One workgroup.  by_raw [U] = the dense users by ascending raw id; the exclusive count of kept users in front of place i is the
// rank among K of the user there.  A kept user v gets seq[map[v]] = 1 << 32 | rank: epoch 1, position in K.
// Bounds.  pre holds U + 1 cells; by_raw[i] < U; map[v] < the new fit's users (k_ap_remap), or v itself without a map.
__global__ void __launch_bounds__(ONE_BLOCK) k_ap_number(int32_t U, const uint32_t* __restrict__ by_raw,
                                                         const unsigned long long* __restrict__ kept, const int32_t* __restrict__ map,
                                                         int64_t* __restrict__ pre, int64_t* __restrict__ seq) {
    block_exclusive_scan(U, [&](int64_t i) { return (int64_t)ap_bit(kept, (int32_t)by_raw[i]); }, pre);
    __syncthreads();
    for (int32_t i = threadIdx.x; i < U; i += ONE_BLOCK) {
        const int32_t v = (int32_t)by_raw[i];
        if (ap_bit(kept, v)) seq[map ? map[v] : v] = ((int64_t)1 << 32) | pre[i];
    }
}

// One thread per old dense user: the lower bound of its trie key among the new keys, which hold it (no user leaves a fit).
// Bounds.  v < U; the search stays inside [0, new_U) and ends on the key itself.
__global__ void __launch_bounds__(TPB) k_ap_remap(int32_t U, const uint32_t* __restrict__ ukeys, const uint32_t* __restrict__ new_ukeys,
                                                  int32_t new_U, int32_t* __restrict__ map) {
    const int32_t v = blockIdx.x * TPB + threadIdx.x;
    if (v >= U) return;
    const uint32_t key = ukeys[v];
    int32_t lo = 0, hi = new_U;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (new_ukeys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    map[v] = min(lo, new_U - 1);
}

__global__ void __launch_bounds__(TPB) k_ap_clear(int32_t U, const unsigned long long* __restrict__ kept, int32_t* __restrict__ cnt,
                                                  int64_t* __restrict__ seq) {
    const int32_t v = blockIdx.x * TPB + threadIdx.x;
    if (v >= U || ap_bit(kept, v)) return;
    cnt[v] = 0;
    seq[v] = -1;
}

// One wave per old dense user (grid-stride); a kept row's filled cells go to row map[v] of the new table.
// Bounds.  v < U; cells [0, min(cnt[v], kcap)) of row v are read, a stored id is a dense user of [0, U); map[.] < the new fit's
// users, so the written cells lie in row map[v] of a table of as many rows with kcap cells each.
__global__ void __launch_bounds__(TPB) k_ap_carry(int32_t U, int32_t kcap, const unsigned long long* __restrict__ kept,
                                                  const int32_t* __restrict__ map, const int32_t* __restrict__ cnt,
                                                  const int32_t* __restrict__ idx, const double* __restrict__ sim,
                                                  int32_t* __restrict__ ncnt, int32_t* __restrict__ nidx, double* __restrict__ nsim) {
    const int lane = threadIdx.x & 63;
    for (int64_t v = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); v < U; v += (int64_t)gridDim.x * (TPB / 64)) {
        if (!ap_bit(kept, (int32_t)v)) continue;
        const int32_t L = min(cnt[v], kcap);
        const int64_t from = v * kcap, to = (int64_t)map[v] * kcap;
        for (int32_t j = lane; j < L; j += 64) {
            nidx[to + j] = map[idx[from + j]];
            nsim[to + j] = sim[from + j];
        }
        if (lane == 0) ncnt[map[v]] = cnt[v];
    }
}

static inline unsigned blocks_for(int64_t n, int per = TPB) { return (unsigned)std::max<int64_t>(1, ceil_div(n, per)); }

void append_begin(AppendScratch& as, int32_t U, hipStream_t st) {
    const int64_t Wu = ceil_div(U, 64);
    as.stale.ensure(Wu); as.kept.ensure(Wu); as.gone.ensure(Wu);
    as.pre.ensure((size_t)std::max<int64_t>(U, Wu) + 1);
    as.totals.ensure(2);
    KN_HIP(hipMemsetAsync(as.stale.p, 0, (size_t)Wu * sizeof(unsigned long long), st));
}

void append_mark(AppendScratch& as, int32_t U, int32_t C, const unsigned long long* d_bits, const int32_t* d_self, hipStream_t st) {
    const int64_t Wu = ceil_div(U, 64);
    k_ap_mark<<<blocks_for(Wu), TPB, 0, st>>>(Wu, C, d_bits, d_self, as.stale.p);
    KN_HIP(hipGetLastError());
}

void append_sets(AppendScratch& as, const Train& tr, const NeighborTable& nt, bool all, int64_t cap, hipStream_t st) {
    const int32_t U = tr.U;
    const int64_t Wu = ceil_div(U, 64);
    cap = std::min<int64_t>(cap, U);
    as.dropped.ensure((size_t)std::max<int64_t>(cap, 1));
    k_ap_sets<<<blocks_for(Wu * 64), TPB, 0, st>>>(U, all ? 1 : 0, nt.seq.p, as.stale.p, as.kept.p, as.gone.p);
    k_ap_report<<<1, ONE_BLOCK, 0, st>>>(U, cap, as.kept.p, as.gone.p, tr.uid.p, as.pre.p, as.dropped.p, as.totals.p);
    KN_HIP(hipGetLastError());
}

void append_remap(AppendScratch& as, const Train& tr, const uint32_t* new_ukeys, int32_t new_U, hipStream_t st) {
    as.map.ensure(tr.U);
    k_ap_remap<<<blocks_for(tr.U), TPB, 0, st>>>(tr.U, tr.ukeys.p, new_ukeys, new_U, as.map.p);
    KN_HIP(hipGetLastError());
}

void append_number(AppendScratch& as, SortWorkspace& ws, const Train& tr, const int32_t* d_map, int64_t* d_seq, hipStream_t st) {
    const int32_t U = tr.U;
    as.k_a.ensure(U); as.k_b.ensure(U); as.v_a.ensure(U); as.v_b.ensure(U);
    k_ap_raw_keys<<<blocks_for(U), TPB, 0, st>>>(U, tr.uid.p, as.k_a.p, as.v_a.p);
    KN_HIP(hipGetLastError());
    sort_pairs_u32_u32(ws, as.k_a.p, as.k_b.p, as.v_a.p, as.v_b.p, (size_t)U, 32, st);
    k_ap_number<<<1, ONE_BLOCK, 0, st>>>(U, as.v_b.p, as.kept.p, d_map, as.pre.p, d_seq);
    KN_HIP(hipGetLastError());
}

void append_clear(AppendScratch& as, int32_t U, int32_t* d_cnt, int64_t* d_seq, hipStream_t st) {
    k_ap_clear<<<blocks_for(U), TPB, 0, st>>>(U, as.kept.p, d_cnt, d_seq);
    KN_HIP(hipGetLastError());
}

void append_carry(AppendScratch& as, int32_t U, const NeighborTable& from, NeighborTable& to, hipStream_t st) {
    k_ap_carry<<<(unsigned)std::min<int64_t>(blocks_for(U, TPB / 64), 8192), TPB, 0, st>>>(U, from.kcap, as.kept.p, as.map.p, from.cnt.p,
                                                                                         from.idx.p, from.sim.p, to.cnt.p, to.idx.p,
                                                                                         to.sim.p);
    KN_HIP(hipGetLastError());
}

}  // namespace knncf
