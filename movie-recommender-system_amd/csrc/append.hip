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
// knncf_amend (DESIGN.md "Amend") is the same call with removals: its changers run through REVISE chunks, and the k_am_* kernels
// below take the removed rows out of the file-order arrays that the new fit is built from.
// knncf_remove_users (DESIGN.md "Remove users") is the call whose changers leave the fit: k_am_flag_users flags every file row of
// a leaver, and the marking is one pass over the stored lists:
//   k_ap_leaver_bits   the leavers as a bitmap over the old fit's dense users
//   k_ap_holders       stale |= every user whose stored list holds a leaver, and the leavers themselves
//   k_ap_leavers_gone  how many leavers are in B ∩ S (the trace line's holders = |B ∩ S| without them)
// k_ap_remap gives a user that left -1; the carry never reads that cell for a kept row.
// Stores are vector stores, atomicOr and atomicAdd on global memory.
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
// Bounds.  pre holds U + 1 cells; by_raw[i] < U; map[v] < the new fit's users (k_ap_remap), or v itself without a map.  map is
// read for kept users only, and a kept user is no leaver: map[v] >= 0.
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

// One thread per old dense user: the lower bound of its trie key among the new keys — its place where they hold the key, -1
// ("gone") where they do not: the user left the fit (knncf_remove_users; in knncf_append and knncf_amend no user leaves a carried
// fit, and every key is found).
// Bounds.  v < U; the search stays inside [0, new_U), and new_ukeys[lo] is read only with lo < new_U.
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
    map[v] = (lo < new_U && new_ukeys[lo] == key) ? lo : -1;
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
// users, so the written cells lie in row map[v] of a table of as many rows with kcap cells each.  map[v] >= 0: a kept user did
// not leave.  A stored id of a kept row did not leave either (k_ap_holders put every holder of a leaver into stale), so no
// written id is -1.
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

// ---- knncf_remove_users: the marking (DESIGN.md "Remove users") -----------------------------------------------------------------
// One thread per leaver: its bit in the leaver bitmap (zeroed beforehand).
// Bounds.  j < L; dense[j] is a dense user of [0, U) (the host looked it up), whose word is < Wu.
__global__ void __launch_bounds__(TPB) k_ap_leaver_bits(int32_t L, const int32_t* __restrict__ dense, unsigned long long* __restrict__ leaver) {
    const int32_t j = blockIdx.x * TPB + threadIdx.x;
    if (j >= L) return;
    const int32_t d = dense[j];
    atomicOr(&leaver[d >> 6], 1ull << (d & 63));
}

// One wave per fitted user v (grid-stride, as k_enu_locate walks the table): the lanes read the filled cells of v's stored row in
// strides of 64 and test each stored dense id against the leaver bitmap, whatever similarity stands beside it.  A wave with a
// hit, and the wave of a leaver, sets v's bit in the stale mask: one atomicOr per wave, as in k_ap_mark.  IN_LDS: every workgroup
// first copies the bitmap's Wu words into LDS (dynamic, Wu * 8 bytes); otherwise the tests read global memory.
// Bounds.  v < U; cells [0, min(cnt[v], kcap)) of row v are read, inside the table's U * kcap cells; a stored id is a dense user
// of [0, U), whose word is < Wu = the words of `leaver`, of the LDS copy and of `stale`.
template <bool IN_LDS>
__global__ void __launch_bounds__(TPB) k_ap_holders(int32_t U, int32_t kcap, const int32_t* __restrict__ cnt, const int32_t* __restrict__ idx,
                                                    const unsigned long long* __restrict__ leaver, unsigned long long* __restrict__ stale) {
    extern __shared__ unsigned long long s_leaver[];
    if (IN_LDS) {
        const int32_t Wu = (U + 63) >> 6;
        for (int32_t w = threadIdx.x; w < Wu; w += TPB) s_leaver[w] = leaver[w];
        __syncthreads();
    }
    auto left = [&](int32_t x) -> bool { return IN_LDS ? (s_leaver[x >> 6] >> (x & 63)) & 1ull : ap_bit(leaver, x); };
    const int lane = threadIdx.x & 63;
    for (int64_t v = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); v < U; v += (int64_t)gridDim.x * (TPB / 64)) {
        const int32_t L = min(cnt[v], kcap);
        const int64_t from = v * kcap;
        bool hit = lane == 0 && left((int32_t)v);
        for (int32_t j = lane; j < L; j += 64) hit |= left(idx[from + j]);
        if (__ballot(hit) != 0ull && lane == 0) atomicOr(&stale[v >> 6], 1ull << (v & 63));
    }
}

// One workgroup: out[0] = the leavers whose bit is set in gone (a leaver that had a list).
// Bounds.  j < L; dense[j] < U, whose word of gone is < Wu.
__global__ void __launch_bounds__(ONE_BLOCK) k_ap_leavers_gone(int32_t L, const int32_t* __restrict__ dense, const unsigned long long* __restrict__ gone,
                                                               int64_t* __restrict__ out) {
    __shared__ int32_t found;
    if (threadIdx.x == 0) found = 0;
    __syncthreads();
    int32_t mine = 0;
    for (int32_t j = threadIdx.x; j < L; j += ONE_BLOCK) mine += ap_bit(gone, dense[j]) ? 1 : 0;
    if (mine) atomicAdd(&found, mine);  // (an LDS cell)
    __syncthreads();
    if (threadIdx.x == 0) out[0] = found;
}

// ---- knncf_amend: the removed rows leave the file order (DESIGN.md "Amend") -----------------------------------------------------
// The removals are one table of keys (raw user as uint32) << 32 | (raw item as uint32), ascending, with a CSR over its distinct
// users (removers [R] ascending, roff [R + 1]).  The train rows go in tiles of AM_TILE file rows, one workgroup each:
//   k_am_flag     every row looks its (user, item) up: the removed-row bitmap, one hit per found removal, the tile's survivors
//   k_am_offsets  one workgroup: the exclusive scan of the tiles' survivors, and "every removal was hit exactly once"
//   k_am_compact  the surviving rows of the three file-order arrays to tile offset + rank within the tile: stable, no atomics
static constexpr int AM_TILE = KNNCF_AMEND_TILE;
static constexpr int AM_WORDS = AM_TILE / 64;  // bitmap words of a tile
static_assert(AM_TILE % TPB == 0 && AM_WORDS <= 64, "a tile is whole passes of the workgroup, and one wave scans its words");

// the place of (user, item) in the table, or -1: the user among the removers first, where almost every row ends
__device__ __forceinline__ int64_t am_find(uint32_t user, uint32_t item, int32_t R, const uint32_t* __restrict__ removers,
                                           const int64_t* __restrict__ roff, const uint64_t* __restrict__ keys) {
    int32_t lo = 0, hi = R;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (removers[mid] < user) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= R || removers[lo] != user) return -1;
    const uint64_t key = ((uint64_t)user << 32) | item;
    int64_t a = roff[lo];
    const int64_t end = roff[lo + 1];
    int64_t b = end;
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (keys[mid] < key) a = mid + 1;
        else b = mid;
    }
    return (a < end && keys[a] == key) ? a : -1;
}

// One workgroup per tile, AM_TILE / TPB passes; a wave's ballot of the hits is word i / 64 of the removed-row bitmap.
// Bounds.  Row i < n reads user_raw[i], item_raw[i]; am_find stays inside removers [R], roff [R + 1] and keys [roff[R]], so a
// hit's cell of hits is < roff[R] = the removals; lane 0 writes word i / 64 only with i < n, which is < ceil(n / 64); cell
// blockIdx.x < the tiles = ceil(n / AM_TILE).
__global__ void __launch_bounds__(TPB) k_am_flag(int64_t n, int32_t R, const uint32_t* __restrict__ removers,
                                                 const int64_t* __restrict__ roff, const uint64_t* __restrict__ keys,
                                                 const int32_t* __restrict__ user_raw, const int32_t* __restrict__ item_raw,
                                                 int32_t* __restrict__ hits, unsigned long long* __restrict__ bits,
                                                 int32_t* __restrict__ tile_cnt) {
    __shared__ int32_t part[TPB / 64];
    const int64_t base = (int64_t)blockIdx.x * AM_TILE;
    int32_t mine = 0;  // the survivors of this wave's rows (the same in every lane)
    for (int it = 0; it < AM_TILE / TPB; ++it) {
        const int64_t i = base + it * TPB + threadIdx.x;
        bool hit = false;
        if (i < n) {
            const int64_t at = am_find((uint32_t)user_raw[i], (uint32_t)item_raw[i], R, removers, roff, keys);
            if (at >= 0) {
                hit = true;
                atomicAdd(&hits[at], 1);
            }
        }
        const unsigned long long word = __ballot(hit), live = __ballot(i < n);
        if ((threadIdx.x & 63) == 0 && i < n) bits[i >> 6] = word;
        mine += __popcll(live & ~word);
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t c = 0;
        for (int w = 0; w < TPB / 64; ++w) c += part[w];
        tile_cnt[blockIdx.x] = c;
    }
}

// k_am_flag for whole users (knncf_remove_users): a row is removed when its user is one of the L leavers (ascending as uint32).
// The same tiles, the same removed-row bitmap and the same per-tile survivor counts; no table of (user, item), no hits.
// Bounds.  Row i < n reads user_raw[i]; the search stays inside leavers [L]; lane 0 writes word i / 64 only with i < n, which is
// < ceil(n / 64); cell blockIdx.x < the tiles = ceil(n / AM_TILE).
__global__ void __launch_bounds__(TPB) k_am_flag_users(int64_t n, int32_t L, const uint32_t* __restrict__ leavers,
                                                       const int32_t* __restrict__ user_raw, unsigned long long* __restrict__ bits,
                                                       int32_t* __restrict__ tile_cnt) {
    __shared__ int32_t part[TPB / 64];
    const int64_t base = (int64_t)blockIdx.x * AM_TILE;
    int32_t mine = 0;  // the survivors of this wave's rows (the same in every lane)
    for (int it = 0; it < AM_TILE / TPB; ++it) {
        const int64_t i = base + it * TPB + threadIdx.x;
        bool hit = false;
        if (i < n) {
            const uint32_t user = (uint32_t)user_raw[i];
            int32_t lo = 0, hi = L;
            while (lo < hi) {
                const int32_t mid = (lo + hi) >> 1;
                if (leavers[mid] < user) lo = mid + 1;
                else hi = mid;
            }
            hit = lo < L && leavers[lo] == user;
        }
        const unsigned long long word = __ballot(hit), live = __ballot(i < n);
        if ((threadIdx.x & 63) == 0 && i < n) bits[i >> 6] = word;
        mine += __popcll(live & ~word);
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t c = 0;
        for (int w = 0; w < TPB / 64; ++w) c += part[w];
        tile_cnt[blockIdx.x] = c;
    }
}

// One workgroup.  tile_off [tiles + 1] = the exclusive scan of tile_cnt; verdict[0] = the surviving rows, verdict[1] = the first
// cell of hits that is not 1 (a removal that is no train row), or -1.
// Bounds.  tile_cnt holds `tiles` cells and tile_off tiles + 1 (block_exclusive_scan writes cell `tiles`); j < n_removed.
__global__ void __launch_bounds__(ONE_BLOCK) k_am_offsets(int64_t tiles, const int32_t* __restrict__ tile_cnt,
                                                          int64_t* __restrict__ tile_off, int64_t n_removed,
                                                          const int32_t* __restrict__ hits, int64_t* __restrict__ verdict) {
    __shared__ unsigned long long first;
    if (threadIdx.x == 0) first = ~0ull;
    const int64_t total = block_exclusive_scan(tiles, [&](int64_t t) { return (int64_t)tile_cnt[t]; }, tile_off);
    __syncthreads();
    for (int64_t j = threadIdx.x; j < n_removed; j += ONE_BLOCK)
        if (hits[j] != 1) atomicMin(&first, (unsigned long long)j);  // (an LDS cell)
    __syncthreads();
    if (threadIdx.x == 0) {
        verdict[0] = total;
        verdict[1] = first == ~0ull ? -1 : (int64_t)first;
    }
}

// One workgroup per tile.  Wave 0 scans the survivors of the tile's AM_WORDS bitmap words into LDS; the rank of a surviving row
// within the tile is its word's prefix plus the survivors below its lane.  File order is kept: tile offsets, word prefixes and
// lanes all ascend with the row.
// Bounds.  Words w < ceil(n / 64) are read; row i < n reads the three arrays; its place is tile_off[tile] + rank < tile_off[tiles]
// = the surviving rows (k_am_flag counted the same bitmap), and the three outputs hold at least that many cells.
__global__ void __launch_bounds__(TPB) k_am_compact(int64_t n, const unsigned long long* __restrict__ bits,
                                                    const int64_t* __restrict__ tile_off, const int32_t* __restrict__ user_raw,
                                                    const int32_t* __restrict__ item_raw, const double* __restrict__ rating,
                                                    int32_t* __restrict__ out_user, int32_t* __restrict__ out_item,
                                                    double* __restrict__ out_rating) {
    __shared__ int32_t wpre[AM_WORDS];
    const int64_t base = (int64_t)blockIdx.x * AM_TILE, Wn = (n + 63) >> 6;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 64) {  // (a whole wave: the scan runs over all 64 lanes)
        const int64_t w = (base >> 6) + lane;
        uint32_t c = 0;
        if (lane < AM_WORDS && w < Wn) {
            const int64_t rows = std::min<int64_t>(64, n - w * 64);
            const unsigned long long valid = rows == 64 ? ~0ull : (1ull << rows) - 1ull;
            c = (uint32_t)__popcll(~bits[w] & valid);
        }
        const uint32_t upto = wave_incl_scan(c);
        if (lane < AM_WORDS) wpre[lane] = (int32_t)(upto - c);
    }
    __syncthreads();
    const int64_t off = tile_off[blockIdx.x];
    for (int it = 0; it < AM_TILE / TPB; ++it) {
        const int64_t i = base + it * TPB + threadIdx.x;
        if (i >= n) break;
        const unsigned long long word = bits[i >> 6];
        if ((word >> lane) & 1ull) continue;
        const int64_t to = off + wpre[(i - base) >> 6] + __popcll(~word & ((1ull << lane) - 1ull));
        out_user[to] = user_raw[i];
        out_item[to] = item_raw[i];
        out_rating[to] = rating[i];
    }
}

static inline unsigned blocks_for(int64_t n, int per = TPB) { return (unsigned)std::max<int64_t>(1, ceil_div(n, per)); }

void amend_flag(AppendScratch& as, const Train& tr, const uint64_t* h_keys, int64_t n_removed, const uint32_t* h_removers,
                const int64_t* h_roff, int32_t R, hipStream_t st) {
    const int64_t tiles = ceil_div(tr.n, AM_TILE);
    as.am_keys.ensure(n_removed); as.am_hits.ensure(n_removed);
    as.am_removers.ensure(R); as.am_roff.ensure((size_t)R + 1);
    as.am_bits.ensure(ceil_div(tr.n, 64)); as.am_tile_cnt.ensure(tiles); as.am_tile_off.ensure((size_t)tiles + 1);
    KN_HIP(hipMemcpyAsync(as.am_keys.p, h_keys, (size_t)n_removed * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    KN_HIP(hipMemcpyAsync(as.am_removers.p, h_removers, (size_t)R * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    KN_HIP(hipMemcpyAsync(as.am_roff.p, h_roff, ((size_t)R + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    KN_HIP(hipMemsetAsync(as.am_hits.p, 0, (size_t)n_removed * sizeof(int32_t), st));
    k_am_flag<<<(unsigned)tiles, TPB, 0, st>>>(tr.n, R, as.am_removers.p, as.am_roff.p, as.am_keys.p, tr.user_raw.p, tr.item_raw.p,
                                               as.am_hits.p, as.am_bits.p, as.am_tile_cnt.p);
    k_am_offsets<<<1, ONE_BLOCK, 0, st>>>(tiles, as.am_tile_cnt.p, as.am_tile_off.p, n_removed, as.am_hits.p, as.totals.p + 2);
    KN_HIP(hipGetLastError());
}

void amend_flag_users(AppendScratch& as, const Train& tr, const uint32_t* h_leavers, int32_t L, hipStream_t st) {
    const int64_t tiles = ceil_div(tr.n, AM_TILE);
    as.am_removers.ensure(L);
    as.am_bits.ensure(ceil_div(tr.n, 64)); as.am_tile_cnt.ensure(tiles); as.am_tile_off.ensure((size_t)tiles + 1);
    KN_HIP(hipMemcpyAsync(as.am_removers.p, h_leavers, (size_t)L * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    k_am_flag_users<<<(unsigned)tiles, TPB, 0, st>>>(tr.n, L, as.am_removers.p, tr.user_raw.p, as.am_bits.p, as.am_tile_cnt.p);
    k_am_offsets<<<1, ONE_BLOCK, 0, st>>>(tiles, as.am_tile_cnt.p, as.am_tile_off.p, 0, nullptr, as.totals.p + 2);
    KN_HIP(hipGetLastError());
}

void append_leavers(AppendScratch& as, int32_t U, const int32_t* h_dense, int32_t L, hipStream_t st) {
    const int64_t Wu = ceil_div(U, 64);
    as.leaver.ensure(Wu); as.leaver_dense.ensure(L);
    KN_HIP(hipMemsetAsync(as.leaver.p, 0, (size_t)Wu * sizeof(unsigned long long), st));
    KN_HIP(hipMemcpyAsync(as.leaver_dense.p, h_dense, (size_t)L * sizeof(int32_t), hipMemcpyHostToDevice, st));
    k_ap_leaver_bits<<<blocks_for(L), TPB, 0, st>>>(L, as.leaver_dense.p, as.leaver.p);
    KN_HIP(hipGetLastError());
}

void append_holders(AppendScratch& as, const Train& tr, const NeighborTable& nt, bool in_lds, hipStream_t st) {
    const int32_t U = tr.U;
    const unsigned grid = (unsigned)std::min<int64_t>(blocks_for(U, TPB / 64), 2048);
    if (in_lds)
        k_ap_holders<true><<<grid, TPB, (size_t)ceil_div(U, 64) * sizeof(unsigned long long), st>>>(U, nt.kcap, nt.cnt.p, nt.idx.p, as.leaver.p,
                                                                                                   as.stale.p);
    else
        k_ap_holders<false><<<grid, TPB, 0, st>>>(U, nt.kcap, nt.cnt.p, nt.idx.p, as.leaver.p, as.stale.p);
    KN_HIP(hipGetLastError());
}

void append_leavers_gone(AppendScratch& as, int32_t L, hipStream_t st) {
    k_ap_leavers_gone<<<1, ONE_BLOCK, 0, st>>>(L, as.leaver_dense.p, as.gone.p, as.totals.p + 4);
    KN_HIP(hipGetLastError());
}

void amend_compact(AppendScratch& as, const Train& tr, int32_t* d_user, int32_t* d_item, double* d_rating, hipStream_t st) {
    k_am_compact<<<(unsigned)ceil_div(tr.n, AM_TILE), TPB, 0, st>>>(tr.n, as.am_bits.p, as.am_tile_off.p, tr.user_raw.p, tr.item_raw.p,
                                                                    tr.rating.p, d_user, d_item, d_rating);
    KN_HIP(hipGetLastError());
}

void append_begin(AppendScratch& as, int32_t U, hipStream_t st) {
    const int64_t Wu = ceil_div(U, 64);
    as.stale.ensure(Wu); as.kept.ensure(Wu); as.gone.ensure(Wu);
    as.pre.ensure((size_t)std::max<int64_t>(U, Wu) + 1);
    as.totals.ensure(5);  // (|K|, |B ∩ S|; the removal stage's verdict; knncf_remove_users: the leavers in B ∩ S)
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
