// reco_batch.hip — recommendations :651-674 for MANY users of the fit in one pass (knncf_recommend_batch; DESIGN.md
// "Batched recommendations").  A chunk of C users ("slots") is answered by a few launches over the chunk:
//   k_rb_fold          kNN predictor (:489-585) of every (slot, item) from the slot's neighbour list, one workgroup per
//                      (slot, tile of RB_TILE items): the neighbours' rows are item-ascending, so the tile's part of each is
//                      found by one binary search; the entries are counted per item in LDS, prefixed, scattered into
//                      per-item LDS lists and folded per item in training-file order (fp64, left to right, no FMA) —
//                      bit for bit the fold of predict.hip
//   k_rb_rows          the other predictors: the chunk's C x I (user, item) rows for the general prediction batch
//   k_rb_mark / k_rb_info   the items each slot has rated; the slots' counts min(n, I - #rated)
//   k_rb_select_tile / k_rb_merge   n <= RB_FAST_N: the n best of every tile by repeated workgroup arg-min on the
//                      (order key, raw-id rank) pair, then the n best of a slot's tile winners.  Nothing is sorted.
//   larger n           the segmented full order of foldin.hip (foldin_batch_recommend)
#include <math.h>

#include <algorithm>

#include "engine.h"

namespace knncf {

static constexpr int TPB = RB_TPB;
static_assert(RB_MAX_K <= RB_CAP, "one item's list (at most one entry per neighbour) must fit the LDS entry store");
static_assert(RB_TILE % TPB == 0 && RB_TILE / TPB == 8, "k_rb_fold: 8 consecutive items per thread in the prefix");
static_assert(RB_TILE <= 65535, "seg_len is 16 bits");

// first position p in [b, e) with col[p] >= x (the row is item-ascending)
__device__ __forceinline__ int64_t rb_lower_bound(const int32_t* __restrict__ col, int64_t b, int64_t e, int32_t x) {
    while (b < e) {
        const int64_t mid = (b + e) >> 1;
        if (col[mid] < x) b = mid + 1;
        else e = mid;
    }
    return b;
}

// grid (tiles, C).  slot_user[s] = dense user of slot s, -1 for a raw id absent from train (every prediction is the
// global average :571-574, as for a user whose mean is negative).  LDS: 4 (RB_TILE + 1) + 6 RB_MAX_K + 16 RB_CAP + 16 B =
// 61 468 B, so two workgroups share a CU's 160 KB.
__global__ void __launch_bounds__(TPB) k_rb_fold(int32_t I, int32_t kcap, const int32_t* __restrict__ slot_user,
                                                 const int64_t* __restrict__ u_ptr, const int32_t* __restrict__ s_col,
                                                 const uint32_t* __restrict__ s_t, const double* __restrict__ s_dev,
                                                 const double* __restrict__ user_avg, double global_avg,
                                                 const int32_t* __restrict__ nbr_idx, const double* __restrict__ nbr_sim,
                                                 const int32_t* __restrict__ nbr_cnt, double* __restrict__ pred) {
    __shared__ uint32_t off[RB_TILE + 1];          // per item: entries (count), then first entry (prefix), then cursor (scatter)
    __shared__ uint32_t seg_b[RB_MAX_K];           // per neighbour: first position of its row inside the tile
    __shared__ uint16_t seg_len[RB_MAX_K];         //                and the number of its entries there
    __shared__ unsigned long long e_key[RB_CAP];   // (train file row << 32) | neighbour slot
    __shared__ double e_dev[RB_CAP];
    __shared__ uint32_t wave_tot[TPB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t slot = blockIdx.y;
    const int32_t i0 = (int32_t)blockIdx.x * RB_TILE;
    const int32_t T = min(RB_TILE, I - i0);
    if (T <= 0) return;
    const int32_t i1 = i0 + T;
    const int32_t u = slot_user[slot];
    const double ua = (u >= 0) ? user_avg[u] : -1.0;  // usersAvgValue.getOrElse(u, -1.0) :572
    const bool flat = ua < 0.0;
    const int32_t cnt = (flat || kcap <= 0) ? 0 : min(min(nbr_cnt[u], kcap), RB_MAX_K);
    const int64_t nb = (u >= 0) ? (int64_t)u * kcap : 0;
    double* out = pred + (int64_t)slot * I;

    for (int32_t c = tid; c <= RB_TILE; c += TPB) off[c] = 0;
    __syncthreads();
    // the tile's part of every neighbour's row, counted per item
    for (int32_t j = tid; j < cnt; j += TPB) {
        const int32_t v = nbr_idx[nb + j];
        const int64_t b = u_ptr[v], e = u_ptr[v + 1];
        const int64_t pb = rb_lower_bound(s_col, b, e, i0);
        int64_t p = pb;
        for (; p < e; ++p) {
            const int32_t c = s_col[p];
            if (c >= i1) break;
            atomicAdd(&off[c - i0], 1u);
        }
        seg_b[j] = (uint32_t)pb;
        seg_len[j] = (uint16_t)(p - pb);
    }
    __syncthreads();
    // exclusive prefix over the items: 8 consecutive items per thread, DPP scan inside the wave, the waves' totals through LDS
    {
        uint32_t mine[8], sum = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            mine[q] = off[tid * 8 + q];
            sum += mine[q];
        }
        const uint32_t incl = wave_incl_scan(sum);
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        uint32_t run = incl - sum;
        for (int w = 0; w < wave; ++w) run += wave_tot[w];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            off[tid * 8 + q] = run;
            run += mine[q];
        }
        if (tid == TPB - 1) off[RB_TILE] = run;
    }
    __syncthreads();
    // item ranges [a, b) whose lists fit the entry store together (one range when the tile holds <= RB_CAP entries: the usual case)
    int32_t a = 0;
    while (a < T) {
        const uint32_t base = off[a];  // (cells from a on still hold their prefix: only cells below a have been cursors)
        int32_t lo = a + 1, hi = T;
        while (lo < hi) {              // largest b in (a, T] with off[b] - base <= RB_CAP; one item's list always fits
            const int32_t mid = (lo + hi + 1) >> 1;
            if (off[mid] - base <= (uint32_t)RB_CAP) lo = mid;
            else hi = mid - 1;
        }
        const int32_t b = lo;
        const uint32_t next_base = off[b];
        __syncthreads();
        if (next_base != base) {
            for (int32_t j = tid; j < cnt; j += TPB) {
                const int64_t pb = seg_b[j];
                const int32_t len = seg_len[j];
                for (int32_t x = 0; x < len; ++x) {
                    const int32_t c = s_col[pb + x] - i0;
                    if (c >= b) break;
                    if (c < a) continue;
                    const uint32_t pos = atomicAdd(&off[c], 1u) - base;
                    if (pos < (uint32_t)RB_CAP) {  // (always: the range was sized for it)
                        e_key[pos] = ((unsigned long long)s_t[pb + x] << 32) | (unsigned long long)(uint32_t)j;
                        e_dev[pos] = s_dev[pb + x];
                    }
                }
            }
        }
        __syncthreads();
        // weightedSumDeviation :517-545 per item: the list in ascending key = training-file order, smallest remaining key first
        for (int32_t c = a + tid; c < b; c += TPB) {
            const uint32_t start = ((c == a) ? base : off[c - 1]) - base, end = min(off[c] - base, (uint32_t)RB_CAP);
            double num = 0.0, den = 0.0;
            unsigned long long prev = 0;
            for (uint32_t r = start; r < end; ++r) {
                unsigned long long best = ~0ull;
                uint32_t bx = start;
                for (uint32_t x = start; x < end; ++x) {
                    const unsigned long long k = e_key[x];
                    if ((r == start || k > prev) && k < best) {
                        best = k;
                        bx = x;
                    }
                }
                const double s = nbr_sim[nb + (uint32_t)best];
                num = num + e_dev[bx] * s;
                den = den + fabs(s);
                prev = best;
            }
            const double w = (den > 0) ? num / den : 0.0;
            out[i0 + c] = flat ? global_avg : combine(ua, w);
        }
        __syncthreads();
        a = b;
    }
}

// the chunk's prediction rows for the general batch: row s * I + i = (raw user of slot s, raw id of dense item i)
__global__ void k_rb_rows(int32_t C, int32_t I, const int32_t* __restrict__ slot_raw, const int32_t* __restrict__ iid,
                          int32_t* __restrict__ users, int32_t* __restrict__ items) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (int64_t)C * I) return;
    const int32_t s = (int32_t)(g / I);
    users[g] = slot_raw[s];
    items[g] = iid[g - (int64_t)s * I];
}

// rated[s][i] = 1 for the items slot s has rated (the cells were cleared); grid (blocks, C)
__global__ void k_rb_mark(int32_t I, const int32_t* __restrict__ slot_user, const int64_t* __restrict__ u_ptr,
                          const int32_t* __restrict__ s_col, uint8_t* __restrict__ rated) {
    const int32_t s = blockIdx.y, u = slot_user[s];
    if (u < 0) return;
    const int64_t b = u_ptr[u], e = u_ptr[u + 1];
    for (int64_t p = b + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < e; p += (int64_t)gridDim.x * blockDim.x)
        rated[(int64_t)s * I + s_col[p]] = 1;
}

// info[4 s + 1] = items slot s has rated (k_qb_take's layout), counts[s] = min(n, I - that)
__global__ void k_rb_info(int32_t C, int32_t I, int32_t n, const int32_t* __restrict__ slot_user,
                          const int64_t* __restrict__ u_ptr, long long* __restrict__ info, int32_t* __restrict__ counts) {
    const int32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= C) return;
    const int32_t u = slot_user[s];
    const int64_t r = (u >= 0) ? u_ptr[u + 1] - u_ptr[u] : 0;
    info[4 * s] = 0;
    info[4 * s + 1] = r;
    info[4 * s + 2] = 0;
    info[4 * s + 3] = 0;
    const int64_t left = (int64_t)I - r;
    counts[s] = left <= 0 ? 0 : (left < (int64_t)n ? (int32_t)left : n);
}

// id_rank[dense item] = its place in ascending raw-id order (the inverse of launch_reco_id_order's list)
__global__ void k_rb_inverse(int32_t I, const uint32_t* __restrict__ by_id, uint32_t* __restrict__ id_rank) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < I) id_rank[by_id[r]] = (uint32_t)r;
}

// Workgroup arg-min over m candidates (key, rank), smallest key first and the smaller rank among equal keys — the reference's
// (prediction descending, raw id ascending) on k_reco_pred_keys' key.  Returns the candidate's index, the same in every
// thread, or 0xffffffff when only spent candidates (key ~0, rank 0xffffffff) are left.  Ends on a barrier.
__device__ uint32_t rb_argmin(const unsigned long long* key, const uint32_t* rank, int32_t m, unsigned long long* w_key,
                              uint32_t* w_rank, uint32_t* w_idx) {
    unsigned long long bk = ~0ull;
    uint32_t br = 0xffffffffu, bi = 0xffffffffu;
    for (int32_t x = threadIdx.x; x < m; x += TPB) {
        const unsigned long long k = key[x];
        const uint32_t q = rank[x];
        if (k < bk || (k == bk && q < br)) {
            bk = k;
            br = q;
            bi = (uint32_t)x;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t klo = __shfl_xor((uint32_t)bk, o), khi = __shfl_xor((uint32_t)(bk >> 32), o);
        const uint32_t qr = __shfl_xor(br, o), qi = __shfl_xor(bi, o);
        const unsigned long long k = ((unsigned long long)khi << 32) | klo;
        if (k < bk || (k == bk && qr < br)) {
            bk = k;
            br = qr;
            bi = qi;
        }
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        w_key[wave] = bk;
        w_rank[wave] = br;
        w_idx[wave] = bi;
    }
    __syncthreads();
    bk = w_key[0];
    br = w_rank[0];
    bi = w_idx[0];
    for (int w = 1; w < TPB / 64; ++w) {
        const unsigned long long k = w_key[w];
        const uint32_t q = w_rank[w];
        if (k < bk || (k == bk && q < br)) {
            bk = k;
            br = q;
            bi = w_idx[w];
        }
    }
    __syncthreads();
    return (bk == ~0ull && br == 0xffffffffu) ? 0xffffffffu : bi;
}

// grid (tiles, C): the n best items of the tile -> cells ((s * tiles + tile) * n ..) of p_key / p_rank / p_item; cells the
// tile cannot fill are spent candidates
__global__ void __launch_bounds__(TPB) k_rb_select_tile(int32_t I, int32_t n, const double* __restrict__ pred,
                                                        const uint8_t* __restrict__ rated, const uint32_t* __restrict__ id_rank,
                                                        unsigned long long* __restrict__ p_key, uint32_t* __restrict__ p_rank,
                                                        uint32_t* __restrict__ p_item) {
    __shared__ unsigned long long key[RB_TILE];
    __shared__ uint32_t rank[RB_TILE];
    __shared__ unsigned long long w_key[TPB / 64];
    __shared__ uint32_t w_rank[TPB / 64], w_idx[TPB / 64];
    const int32_t s = blockIdx.y;
    const int32_t i0 = (int32_t)blockIdx.x * RB_TILE;
    const int32_t T = min(RB_TILE, I - i0);
    if (T <= 0) return;
    const int64_t row = (int64_t)s * I;
    for (int32_t c = threadIdx.x; c < T; c += TPB) {
        double p = pred[row + i0 + c];
        if (p == 0.0) p = 0.0;  // -0.0 and +0.0 compare equal in the reference
        const uint64_t bits = (uint64_t)__double_as_longlong(p);
        const uint64_t asc = (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
        const bool r = rated[row + i0 + c] != 0;
        key[c] = r ? ~0ull : ~asc;
        rank[c] = r ? 0xffffffffu : id_rank[i0 + c];
    }
    __syncthreads();
    const int64_t o = ((int64_t)s * gridDim.x + blockIdx.x) * n;
    for (int32_t r = 0; r < n; ++r) {
        const uint32_t win = rb_argmin(key, rank, T, w_key, w_rank, w_idx);
        if (threadIdx.x == 0) {
            if (win != 0xffffffffu) {
                p_key[o + r] = key[win];
                p_rank[o + r] = rank[win];
                p_item[o + r] = (uint32_t)(i0 + (int32_t)win);
                key[win] = ~0ull;
                rank[win] = 0xffffffffu;
            } else {
                p_key[o + r] = ~0ull;
                p_rank[o + r] = 0xffffffffu;
                p_item[o + r] = 0;
            }
        }
        __syncthreads();
    }
}

// grid (C): the counts[s] best of slot s's m = tiles * n tile winners -> out_items / out_preds [s][n]
__global__ void __launch_bounds__(TPB) k_rb_merge(int32_t I, int32_t n, int32_t m, const int32_t* __restrict__ counts,
                                                  unsigned long long* __restrict__ p_key, uint32_t* __restrict__ p_rank,
                                                  const uint32_t* __restrict__ p_item, const int32_t* __restrict__ iid,
                                                  const double* __restrict__ pred, int32_t* __restrict__ out_items,
                                                  double* __restrict__ out_preds) {
    __shared__ unsigned long long w_key[TPB / 64];
    __shared__ uint32_t w_rank[TPB / 64], w_idx[TPB / 64];
    const int32_t s = blockIdx.x;
    unsigned long long* key = p_key + (int64_t)s * m;
    uint32_t* rank = p_rank + (int64_t)s * m;
    const uint32_t* item = p_item + (int64_t)s * m;
    const int32_t take = min(counts[s], n);
    for (int32_t r = 0; r < take; ++r) {
        const uint32_t win = rb_argmin(key, rank, m, w_key, w_rank, w_idx);
        if (win == 0xffffffffu) break;  // (never: counts[s] unrated items exist and every tile offered its n best)
        if (threadIdx.x == 0) {
            const uint32_t d = item[win];
            out_items[(int64_t)s * n + r] = iid[d];
            out_preds[(int64_t)s * n + r] = pred[(int64_t)s * I + d];
            key[win] = ~0ull;
            rank[win] = 0xffffffffu;
        }
        __syncthreads();
    }
}

void reco_batch_id_rank(const Train& tr, QueryBatchScratch& bs, RecoBatchScratch& rb, SortWorkspace& ws, hipStream_t st) {
    const int32_t I = tr.I;
    bs.k64_a.ensure(I); bs.k64_b.ensure(I); bs.v32_a.ensure(I); bs.by_id.ensure(I);
    rb.id_rank.ensure(I);
    launch_reco_id_order(tr, ws, bs.k64_a.p, bs.k64_b.p, bs.v32_a.p, bs.by_id.p, st);
    k_rb_inverse<<<(unsigned)ceil_div(I, TPB), TPB, 0, st>>>(I, bs.by_id.p, rb.id_rank.p);
    KN_HIP(hipGetLastError());
}

void reco_batch_fold(const Train& tr, const NeighborTable& nt, const RecoBatchScratch& rb, int32_t C, double* d_pred,
                     hipStream_t st) {
    KN_REQUIRE(nt.kcap <= RB_MAX_K && C >= 1 && C <= RB_MAX_CHUNK, KNNCF_E_INVALID, "recommend batch: fold out of range");
    const dim3 grid((unsigned)ceil_div(tr.I, RB_TILE), (unsigned)C);
    k_rb_fold<<<grid, TPB, 0, st>>>(tr.I, nt.kcap, rb.slot_user.p, tr.u_ptr.p, tr.s_col.p, tr.s_t.p, tr.s_dev.p, tr.user_avg.p,
                                    tr.global_avg, nt.idx.p, nt.sim.p, nt.cnt.p, d_pred);
    KN_HIP(hipGetLastError());
}

void reco_batch_rows(const Train& tr, const RecoBatchScratch& rb, int32_t C, int32_t* d_users, int32_t* d_items, hipStream_t st) {
    const int64_t cells = (int64_t)C * tr.I;
    k_rb_rows<<<(unsigned)ceil_div(cells, TPB), TPB, 0, st>>>(C, tr.I, rb.slot_raw.p, tr.iid.p, d_users, d_items);
    KN_HIP(hipGetLastError());
}

void reco_batch_mark(const Train& tr, const RecoBatchScratch& rb, int32_t C, int32_t n, uint8_t* d_rated, long long* d_info,
                     hipStream_t st) {
    KN_HIP(hipMemsetAsync(d_rated, 0, (size_t)C * (size_t)tr.I, st));
    k_rb_mark<<<dim3(4, (unsigned)C), TPB, 0, st>>>(tr.I, rb.slot_user.p, tr.u_ptr.p, tr.s_col.p, d_rated);
    k_rb_info<<<(unsigned)ceil_div(C, TPB), TPB, 0, st>>>(C, tr.I, n, rb.slot_user.p, tr.u_ptr.p, d_info, rb.counts.p);
    KN_HIP(hipGetLastError());
}

void reco_batch_select(const Train& tr, RecoBatchScratch& rb, int32_t C, int32_t n, const double* d_pred, const uint8_t* d_rated,
                       int32_t* d_items, double* d_preds, hipStream_t st) {
    KN_REQUIRE(n >= 1 && n <= RB_FAST_N, KNNCF_E_INVALID, "recommend batch: select out of range");
    const int64_t tiles = ceil_div(tr.I, RB_TILE);
    const size_t cells = (size_t)C * (size_t)tiles * (size_t)n;
    rb.p_key.ensure(cells); rb.p_rank.ensure(cells); rb.p_item.ensure(cells);
    k_rb_select_tile<<<dim3((unsigned)tiles, (unsigned)C), TPB, 0, st>>>(tr.I, n, d_pred, d_rated, rb.id_rank.p,
                                                                        (unsigned long long*)rb.p_key.p, rb.p_rank.p, rb.p_item.p);
    k_rb_merge<<<(unsigned)C, TPB, 0, st>>>(tr.I, n, (int32_t)(tiles * n), rb.counts.p, (unsigned long long*)rb.p_key.p, rb.p_rank.p,
                                            rb.p_item.p, tr.iid.p, d_pred, d_items, d_preds);
    KN_HIP(hipGetLastError());
}

}  // namespace knncf
