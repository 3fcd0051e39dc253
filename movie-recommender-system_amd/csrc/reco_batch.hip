// reco_batch.hip — recommendations shared/predictions.scala:651-674 for users of the fit (knncf_recommend_batch, and
// knncf_recommend as the call over one user; DESIGN.md "Batched recommendations"): every train item a user has not rated,
// ordered by (prediction descending, raw item id ascending), first n.  A chunk of C users ("slots") is answered by a few
// launches over the chunk:
//   k_rb_rows          the chunk's C x I (user, item) rows for the prediction batch of predict.hip, whatever the predictor
//   k_rb_mark / k_rb_info   the items each slot has rated; the slots' counts min(n, I - #rated)
//   k_rb_select_tile / k_rb_merge   n <= RB_FAST_N: the n best of every tile of RB_TILE items by repeated workgroup arg-min on
//                      the (order key, raw-id rank) pair, then the n best of a slot's tile winners.  Nothing is sorted.
//   larger n           the segmented full order of foldin.hip (foldin_batch_recommend)
#include <math.h>

#include <algorithm>

#include "engine.h"

namespace knncf {

static constexpr int TPB = RB_TPB;

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

__global__ void k_reco_id_keys(int32_t I, const int32_t* __restrict__ iid, uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= I) return;
    key[j] = (uint64_t)(uint32_t)(iid[j] ^ 0x80000000);  // signed ids in ascending order
    val[j] = (uint32_t)j;
}

// id_rank[dense item] = its place in ascending raw-id order (the inverse of launch_reco_id_order's list)
__global__ void k_rb_inverse(int32_t I, const uint32_t* __restrict__ by_id, uint32_t* __restrict__ id_rank) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < I) id_rank[by_id[r]] = (uint32_t)r;
}

// Workgroup arg-min over m candidates (key, rank), smallest key first and the smaller rank among equal keys — the reference's
// (prediction descending, raw id ascending) on k_qb_reco_keys' key (foldin.hip).  Returns the candidate's index, the same in every
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

void launch_reco_id_order(const Train& tr, SortWorkspace& ws, uint64_t* k_a, uint64_t* k_b, uint32_t* v_a, uint32_t* by_id, hipStream_t st) {
    k_reco_id_keys<<<(unsigned)ceil_div(tr.I, TPB), TPB, 0, st>>>(tr.I, tr.iid.p, k_a, v_a);
    sort_pairs_u64_u32(ws, k_a, k_b, v_a, by_id, tr.I, 32, st);
    KN_HIP(hipGetLastError());
}

void reco_batch_id_rank(const Train& tr, QueryBatchScratch& bs, RecoBatchScratch& rb, SortWorkspace& ws, hipStream_t st) {
    const int32_t I = tr.I;
    bs.k64_a.ensure(I); bs.k64_b.ensure(I); bs.v32_a.ensure(I); bs.by_id.ensure(I);
    rb.id_rank.ensure(I);
    launch_reco_id_order(tr, ws, bs.k64_a.p, bs.k64_b.p, bs.v32_a.p, bs.by_id.p, st);
    k_rb_inverse<<<(unsigned)ceil_div(I, TPB), TPB, 0, st>>>(I, bs.by_id.p, rb.id_rank.p);
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
