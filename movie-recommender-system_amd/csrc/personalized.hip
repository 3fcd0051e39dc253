// personalized.hip — PERSONALIZED (no k) beyond the U x U table: exact similarity rows streamed by user.
//
// predictor(train, weightedSumDeviation(train, sim)) with sim = adjustedCosineSimilarityFunction(train) or
// jaccardCoefficient(train) (predict/Personalized.scala:61-72; shared/predictions.scala:489-585).  For a test pair (u, i):
//     num = fold over i's raters v in train FILE order of dev(v, i) * s(u, v),  den = fold of |s(u, v)|   (both from +0.0)
// u itself included when (u, i) is a training pair.  Two kernels per block of users:
//   k_sim_rows  — every user's full exact row s(u, .) against all U users, by item instead of by pair: for each item j of u
//                 in ascending dense order, acc[v] += pre(u, j) * pre(v, j) over j's raters v.  One workgroup per (user,
//                 column tile of PTC users) holds the tile's fp64 accumulators in LDS; the raters of one item are distinct,
//                 so its updates never collide, and a barrier between items keeps every cell's products in ascending item
//                 order — the reference's left fold over the common items, one v_mul_f64 + one v_add_f64 per
//                 product (-ffp-contract=off), no atomics, no reassociation.  Jaccard counts the common items with LDS
//                 integer atomics (order-free) and forms count / (|I(u)| + |I(v)| - count) in fp64 as rerank.hip does.
//   k_fold_rows — one wave per test row: the item's raters in file order (pf_user / pf_dev), s gathered from the user's row,
//                 products formed in parallel, the two left folds run serially over LDS.  Then the finishing code of
//                 k_predict_knn (combine, unknown user -> global average, unknown item -> wsd = 0).
// Raters with s = 0 add +-0 terms to accumulators that cannot hold -0.0: the folds run over every rater and stay exact.
#include <math.h>

#include <algorithm>

#include "engine.h"
#include "wave_helpers.h"

namespace knncf {

static constexpr int TPB = 256;
static inline int nblocks(int64_t n, int per = TPB) { return (int)std::max<int64_t>(1, ceil_div(n, per)); }

// ---- first-use copies ---------------------------------------------------------------------------------------------------
__global__ void k_pcol_keys(int64_t n, const int32_t* __restrict__ s_col, uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    key[p] = (uint32_t)s_col[p];
    val[p] = (uint32_t)p;
}

__global__ void k_pfile_keys(int64_t n, const int32_t* __restrict__ s_col, const uint32_t* __restrict__ s_t, int tbits,
                             uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    key[p] = ((uint64_t)(uint32_t)s_col[p] << tbits) | s_t[p];
    val[p] = (uint32_t)p;
}

// pi_pre[q] = pre of the q-th entry in (item, user ascending) order — the order of it_user
__global__ void k_pgather_pre(int64_t n, const uint32_t* __restrict__ perm, const double* __restrict__ s_pre, double* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    out[q] = s_pre[perm[q]];
}

// (rater, deviation) of the k-th entry in (item, file row) order
__global__ void k_pgather_file(int64_t n, const uint32_t* __restrict__ perm, const int32_t* __restrict__ s_user,
                               const double* __restrict__ s_dev, int32_t* __restrict__ pf_user, double* __restrict__ pf_dev) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t p = perm[k];
    pf_user[k] = s_user[p];
    pf_dev[k] = s_dev[p];
}

// p_tile[i][t] = lower bound of t * PTC in item i's ascending rater list (absolute entry index), t = 0 .. tiles
__global__ void k_ptiles(int32_t I, int32_t stride, const int64_t* __restrict__ i_ptr, const int32_t* __restrict__ it_user,
                         uint32_t* __restrict__ tile) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (int64_t)I * stride) return;
    const int32_t i = (int32_t)(g / stride), t = (int32_t)(g - (int64_t)i * stride);
    int64_t lo = i_ptr[i], hi = i_ptr[i + 1];
    const int64_t bound = (int64_t)t * PERSONAL_TCOLS;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (it_user[mid] < bound) lo = mid + 1;
        else hi = mid;
    }
    tile[g] = (uint32_t)lo;
}

void personalized_prepare(const Train& tr, PrepScratch& sc, PersonalRows& pr, hipStream_t st) {
    const int64_t n = tr.n;
    const int32_t I = tr.I;
    pr.pi_pre.alloc(n);
    pr.pf_user.alloc(n);
    pr.pf_dev.alloc(n);
    pr.tiles = (int32_t)ceil_div(tr.U, PERSONAL_TCOLS);
    pr.tile.ensure((size_t)I * (pr.tiles + 1));
    sc.k32_a.ensure(n); sc.k32_b.ensure(n); sc.v32_a.ensure(n); sc.v32_b.ensure(n);
    sc.k64_a.ensure(n); sc.k64_b.ensure(n);
    // (item, user ascending): a stable sort of the user-major positions by item
    k_pcol_keys<<<nblocks(n), TPB, 0, st>>>(n, tr.s_col.p, sc.k32_a.p, sc.v32_a.p);
    KN_HIP(hipGetLastError());
    sort_pairs_u32_u32(sc.sort, sc.k32_a.p, sc.k32_b.p, sc.v32_a.p, sc.v32_b.p, n, bits_for((uint64_t)I), st);
    k_pgather_pre<<<nblocks(n), TPB, 0, st>>>(n, sc.v32_b.p, tr.s_pre.p, pr.pi_pre.p);
    KN_HIP(hipGetLastError());
    // (item, file row): ratings.groupBy(_.item) keeps file order
    const int tbits = bits_for((uint64_t)n), ibits = bits_for((uint64_t)I);
    k_pfile_keys<<<nblocks(n), TPB, 0, st>>>(n, tr.s_col.p, tr.s_t.p, tbits, sc.k64_a.p, sc.v32_a.p);
    KN_HIP(hipGetLastError());
    sort_pairs_u64_u32(sc.sort, sc.k64_a.p, sc.k64_b.p, sc.v32_a.p, sc.v32_b.p, n, tbits + ibits, st);
    k_pgather_file<<<nblocks(n), TPB, 0, st>>>(n, sc.v32_b.p, tr.s_user.p, tr.s_dev.p, pr.pf_user.p, pr.pf_dev.p);
    k_ptiles<<<nblocks((int64_t)I * (pr.tiles + 1)), TPB, 0, st>>>(I, pr.tiles + 1, tr.i_ptr.p, tr.it_user.p, pr.tile.p);
    KN_HIP(hipGetLastError());
}

// ---- test rows by (user, item) ----------------------------------------------------------------------------------------
__global__ void k_prow_keys(int64_t n, const int32_t* __restrict__ du, const int32_t* __restrict__ di, int32_t U, int32_t I, int ibits,
                            uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t u = du[t] < 0 ? (uint32_t)U : (uint32_t)du[t];
    const uint32_t i = di[t] < 0 ? (uint32_t)I : (uint32_t)di[t];
    key[t] = ((uint64_t)u << ibits) | i;
    val[t] = (uint32_t)t;
}

void launch_personal_row_keys(const Train& tr, int64_t n, const int32_t* d_du, const int32_t* d_di, uint64_t* d_key, uint32_t* d_val,
                              hipStream_t st) {
    k_prow_keys<<<nblocks(n), TPB, 0, st>>>(n, d_du, d_di, tr.U, tr.I, bits_for((uint64_t)tr.I), d_key, d_val);
    KN_HIP(hipGetLastError());
}

// ---- K-P1: exact similarity rows ---------------------------------------------------------------------------------------
static constexpr int ROW_TPB = 512;
static constexpr int ROW_CHUNK = 512;  // items of u whose tile bounds and pre values are staged in LDS at a time

template <bool JACCARD>
__global__ void __launch_bounds__(ROW_TPB) k_sim_rows(const int64_t* __restrict__ u_ptr, const int32_t* __restrict__ s_col,
                                                      const double* __restrict__ s_pre, const uint32_t* __restrict__ tile,
                                                      int32_t tiles, const int32_t* __restrict__ it_user,
                                                      const double* __restrict__ pi_pre, const int32_t* __restrict__ users,
                                                      int32_t U, double* __restrict__ S) {
    // cosine: fp64 accumulators of the tile's PTC columns; Jaccard: their common-item counts (the first half of the space)
    __shared__ double acc[PERSONAL_TCOLS];
    __shared__ uint32_t s_q0[ROW_CHUNK], s_q1[ROW_CHUNK];
    __shared__ double s_x[ROW_CHUNK];
    uint32_t* cnt = reinterpret_cast<uint32_t*>(acc);
    const int32_t r = blockIdx.x / tiles, t = blockIdx.x - r * tiles;
    const int32_t u = users[r];
    const int32_t col0 = t * PERSONAL_TCOLS;
    const int32_t ncols = min(PERSONAL_TCOLS, U - col0);
    const int tid = threadIdx.x;
    for (int c = tid; c < PERSONAL_TCOLS; c += ROW_TPB) acc[c] = 0.0;  // +0.0 (Jaccard: two zero counts)
    const int64_t pb = u_ptr[u], pe = u_ptr[u + 1];
    const int32_t stride = tiles + 1;
    for (int64_t c0 = pb; c0 < pe; c0 += ROW_CHUNK) {
        const int m = (int)min<int64_t>(ROW_CHUNK, pe - c0);
        __syncthreads();  // (the accumulators are cleared / the previous chunk's bounds are consumed)
        for (int k = tid; k < m; k += ROW_TPB) {
            const int32_t j = s_col[c0 + k];
            s_q0[k] = tile[(int64_t)j * stride + t];
            s_q1[k] = tile[(int64_t)j * stride + t + 1];
            s_x[k] = s_pre[c0 + k];
        }
        __syncthreads();
        if (JACCARD) {
            for (int k = 0; k < m; ++k) {  // counts: any order; no barrier between items
                for (uint32_t q = s_q0[k] + tid; q < s_q1[k]; q += ROW_TPB) atomicAdd(&cnt[it_user[q] - col0], 1u);
            }
        } else {
            // the first ROW_TPB entries of the next item are loaded before the barrier that ends the current one
            uint32_t q0 = s_q0[0], q1 = s_q1[0];
            int32_t nv = 0;
            double ny = 0.0;
            if (q0 + tid < q1) { nv = it_user[q0 + tid]; ny = pi_pre[q0 + tid]; }
            for (int k = 0; k < m; ++k) {
                const double x = s_x[k];
                const uint32_t cq0 = q0, cq1 = q1;
                const int32_t v = nv;
                const double y = ny;
                if (k + 1 < m) {
                    q0 = s_q0[k + 1];
                    q1 = s_q1[k + 1];
                    if (q0 + tid < q1) { nv = it_user[q0 + tid]; ny = pi_pre[q0 + tid]; }
                }
                if (cq0 == cq1) continue;  // (uniform: no entry of this item in the tile, nothing to order)
                if (cq0 + tid < cq1) {
                    const double prod = x * y;
                    acc[v - col0] = acc[v - col0] + prod;
                }
                for (uint32_t q = cq0 + ROW_TPB + tid; q < cq1; q += ROW_TPB) {
                    const double prod = x * pi_pre[q];
                    const int32_t c = it_user[q] - col0;
                    acc[c] = acc[c] + prod;
                }
                __syncthreads();  // every cell sees the items in ascending order
            }
        }
    }
    __syncthreads();
    double* out = S + (int64_t)r * U + col0;
    if (JACCARD) {
        const int64_t nu = pe - pb;
        for (int c = tid; c < ncols; c += ROW_TPB) {
            const int64_t both = cnt[c];
            const int64_t nv = u_ptr[col0 + c + 1] - u_ptr[col0 + c];
            out[c] = (double)both / (double)(nu + nv - both);
        }
    } else {
        for (int c = tid; c < ncols; c += ROW_TPB) out[c] = acc[c];
    }
}

void launch_sim_rows(const Train& tr, const PersonalRows& pr, const int32_t* d_users, int32_t n_users, double* d_S, hipStream_t st) {
    if (n_users <= 0) return;
    const int64_t grid = (int64_t)n_users * pr.tiles;
    KN_REQUIRE(grid < (1ll << 31), KNNCF_E_UNSUPPORTED, "PERSONALIZED: too many similarity rows in one block");
    KN_TRACE_DISPATCH("sim_rows sim=%s users=%d tiles=%d", tr.jaccard ? "jaccard" : "cosine", (int)n_users, (int)pr.tiles);
    if (tr.jaccard)
        k_sim_rows<true><<<(int)grid, ROW_TPB, 0, st>>>(tr.u_ptr.p, tr.s_col.p, tr.s_pre.p, pr.tile.p, pr.tiles, tr.it_user.p,
                                                         pr.pi_pre.p, d_users, tr.U, d_S);
    else
        k_sim_rows<false><<<(int)grid, ROW_TPB, 0, st>>>(tr.u_ptr.p, tr.s_col.p, tr.s_pre.p, pr.tile.p, pr.tiles, tr.it_user.p,
                                                          pr.pi_pre.p, d_users, tr.U, d_S);
    KN_HIP(hipGetLastError());
}

// ---- K-P2: the weighted-sum folds in file order ------------------------------------------------------------------------
static constexpr int FOLD_WAVES = 4;

__global__ void __launch_bounds__(FOLD_WAVES * 64) k_fold_rows(int64_t n_rows, const uint32_t* __restrict__ order,
                                                              const int32_t* __restrict__ du, const int32_t* __restrict__ di,
                                                              const double* __restrict__ ratings, const int32_t* __restrict__ slot,
                                                              const double* __restrict__ S, int32_t U, const int64_t* __restrict__ i_ptr,
                                                              const int32_t* __restrict__ pf_user, const double* __restrict__ pf_dev,
                                                              const double* __restrict__ user_avg, double global_avg,
                                                              double* __restrict__ pred, double* __restrict__ abs_err,
                                                              uint8_t* __restrict__ owned) {
    __shared__ double s_prod[FOLD_WAVES][64], s_abs[FOLD_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * FOLD_WAVES + wave;
    if (w >= n_rows) return;
    const int64_t t = order[w];
    const int32_t u = du[t], i = di[t];
    double p;
    const double ua = (u >= 0) ? user_avg[u] : -1.0;  // usersAvgValue.getOrElse(u, -1.0) :572
    if (ua < 0.0) {
        p = global_avg;
    } else if (i < 0) {
        p = combine(ua, 0.0);  // no rater: den = 0 -> 0.0 :527-529
    } else {
        const double* row = S + (int64_t)slot[u] * U;
        const int64_t rb = i_ptr[i], re = i_ptr[i + 1];
        double* sp = s_prod[wave];
        double* sa = s_abs[wave];
        double num = 0.0, den = 0.0;
        // software-pipelined: the row gathers of the next chunk and the rater ids of the one after are in flight while the
        // current chunk's two serial chains of 64 additions run
        const int32_t v0 = (rb + lane < re) ? pf_user[rb + lane] : 0;
        double dv = (rb + lane < re) ? pf_dev[rb + lane] : 0.0;
        double s = (rb + lane < re) ? row[v0] : 0.0;
        int32_t vn = (rb + 64 + lane < re) ? pf_user[rb + 64 + lane] : 0;
        for (int64_t c0 = rb; c0 < re; c0 += 64) {
            const double prod = dv * s, a = fabs(s);  // (a lane past the end: stale or 0 values that the fold never reads)
            if (c0 + 64 + lane < re) {
                dv = pf_dev[c0 + 64 + lane];
                s = row[vn];
            }
            if (c0 + 128 + lane < re) vn = pf_user[c0 + 128 + lane];
            sp[lane] = prod;
            sa[lane] = a;
            wave_sync();
            const int m = (int)min<int64_t>(64, re - c0);
            for (int k = 0; k < m; ++k) {  // every lane folds the same sequence (LDS broadcast)
                num = num + sp[k];
                den = den + sa[k];
            }
            wave_sync();
        }
        const double wsd = (den > 0) ? num / den : 0.0;
        p = combine(ua, wsd);
    }
    if (lane == 0) {
        pred[t] = p;
        abs_err[t] = ratings ? fabs(ratings[t] - p) : 0.0;
        owned[t] = 1;
    }
}

void launch_fold_rows(const Train& tr, const PersonalRows& pr, int64_t n_rows, const uint32_t* d_order, const int32_t* d_du,
                      const int32_t* d_di, const double* d_ratings, const int32_t* d_slot, const double* d_S, double* d_pred,
                      double* d_abs_err, uint8_t* d_owned, hipStream_t st) {
    if (n_rows <= 0) return;
    KN_TRACE_DISPATCH("fold_rows rows=%lld", (long long)n_rows);
    k_fold_rows<<<nblocks(n_rows, FOLD_WAVES), FOLD_WAVES * 64, 0, st>>>(
        n_rows, d_order, d_du, d_di, d_ratings, d_slot, d_S, tr.U, tr.i_ptr.p, pr.pf_user.p, pr.pf_dev.p, tr.user_avg.p,
        tr.global_avg, d_pred, d_abs_err, d_owned);
    KN_HIP(hipGetLastError());
}

}  // namespace knncf
