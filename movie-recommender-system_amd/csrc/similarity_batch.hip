// similarity_batch.hip — many fresh-closure pair similarities in one pass (knncf_similarity_batch*, knncf_knn_similarity_batch;
// DESIGN.md "Bulk similarities").  One WAVE per pair, grid-stride: the raw ids are looked up by two lanes, the shorter row is
// walked in 64-entry pieces with coalesced loads, every lane binary-searches the other row for its item, and the hits are
// folded in lane order.  The adjusted cosine :415-432 is a left fold from 0.0 over the common items in the item-set order of the
// FIRST argument, so the fold stays ONE serial fp64 chain (a tree or per-lane partial sums round differently): what the wave
// does in parallel is finding the common items and forming the products.  The Jaccard coefficient :446-463 only counts hits.
// rerank.hip's merge_dot / owner_dot stay the single-pair path; nothing here is shared with them.
#include <algorithm>

#include "engine.h"

namespace knncf {

static constexpr int PAIR_TPB = 256;              // 4 waves: 4 pairs in flight per workgroup
static constexpr int PAIR_WAVES = PAIR_TPB / 64;
static constexpr int PAIR_MAX_BLOCKS = 8192;      // 8 workgroups on each of the 256 CUs, x 4: the tail of a launch stays short

// raw user id -> dense index, -1 when absent from train: the direct table when the fit has one (launch_dense_ids' rule)
struct UserIds {
    const int32_t* table;
    int32_t table_n;
    const uint32_t* keys;
    int32_t U;
};
__device__ __forceinline__ int32_t dense_user_of(const UserIds& ids, int32_t raw) {
    if (ids.table_n > 0) return (raw >= 0 && raw < ids.table_n) ? ids.table[raw] : -1;
    return dense_lookup(ids.keys, ids.U, raw);
}

__device__ __forceinline__ int32_t wave_i32(int32_t x, int lane) { return __builtin_amdgcn_readlane(x, lane); }
__device__ __forceinline__ double wave_f64(double x, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane), hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

// first position in [lo, hi) whose column is >= c
__device__ __forceinline__ int64_t pair_lower_bound(const int32_t* __restrict__ s_col, int64_t lo, int64_t hi, int32_t c) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (s_col[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the dense users of pair j, the same in every lane: lane 0 looks up us[j], lane 1 vs[j]
__device__ __forceinline__ void pair_users(const UserIds& ids, const int32_t* __restrict__ us, const int32_t* __restrict__ vs, int64_t j,
                                           int lane, int32_t& du, int32_t& dv) {
    int32_t d = -1;
    if (lane < 2) d = dense_user_of(ids, lane == 0 ? us[j] : vs[j]);
    du = wave_i32(d, 0);
    dv = wave_i32(d, 1);
}

// out[j] = adjustedCosine(train)(us[j], vs[j]) on a closure of its own
__global__ void __launch_bounds__(PAIR_TPB) k_pair_cosine(UserIds ids, const int64_t* __restrict__ u_ptr, const int32_t* __restrict__ s_col,
                                                          const uint32_t* __restrict__ s_t, const double* __restrict__ s_pre,
                                                          const int32_t* __restrict__ us, const int32_t* __restrict__ vs, int64_t n,
                                                          double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * PAIR_WAVES;
    for (int64_t j = (int64_t)blockIdx.x * PAIR_WAVES + (threadIdx.x >> 6); j < n; j += stride) {
        int32_t du, dv;
        pair_users(ids, us, vs, j, lane, du, dv);
        double s = 0.0;
        if (du >= 0 && dv >= 0) {  // (an absent user has no row: u_ptr[-1] is never read)
            const int64_t pu = u_ptr[du], eu = u_ptr[du + 1], pv = u_ptr[dv], ev = u_ptr[dv + 1];
            const int64_t nu = eu - pu;
            if (nu <= 4) {
                // Set1..Set4 iterate in insertion order: u's entries by ascending file row, each searched in v's row
                const bool mine = lane < nu;
                uint32_t t = 0;
                int32_t c = 0;
                double x = 0.0;
                if (mine) { t = s_t[pu + lane]; c = s_col[pu + lane]; x = s_pre[pu + lane]; }
                int32_t rank = 0;  // place of this lane's entry in file order (file rows are distinct)
                for (int q = 0; q < 4; ++q) {
                    const uint32_t tq = (uint32_t)wave_i32((int32_t)t, q);
                    if (q < nu && tq < t) ++rank;
                }
                bool hit = false;
                double prod = 0.0;
                if (mine) {
                    const int64_t p = pair_lower_bound(s_col, pv, ev, c);
                    if (p < ev && s_col[p] == c) { hit = true; prod = x * s_pre[p]; }
                }
                for (int32_t step = 0; step < (int32_t)nu; ++step) {
                    const unsigned long long m = __ballot(hit && rank == step);
                    if (m) s = s + wave_f64(prod, __builtin_amdgcn_readfirstlane((int)__ffsll((long long)m) - 1));
                }
            } else {
                // both iterate in trie order (ascending dense item): walk the shorter row, search the longer one — the common
                // items come out ascending whichever row is walked, and a product does not depend on its operands' order
                const bool u_short = nu <= ev - pv;
                const int64_t pa = u_short ? pu : pv, ea = u_short ? eu : ev;
                int64_t lo = u_short ? pv : pu;
                const int64_t eb = u_short ? ev : eu;
                for (int64_t base = pa; base < ea && lo < eb; base += 64) {
                    const int64_t left = ea - base;
                    const int last = (int)(left < 64 ? left : 64) - 1;  // last lane of this piece with an entry
                    bool hit = false;
                    double prod = 0.0;
                    int64_t p = eb;
                    if (lane <= last) {
                        const int32_t c = s_col[base + lane];
                        const double x = s_pre[base + lane];
                        p = pair_lower_bound(s_col, lo, eb, c);
                        if (p < eb && s_col[p] == c) { hit = true; prod = x * s_pre[p]; }
                    }
                    unsigned long long m = __ballot(hit);
                    while (m) {  // the fold: one serial chain in lane order, carried across the pieces
                        const int l = __builtin_amdgcn_readfirstlane((int)__ffsll((long long)m) - 1);
                        s = s + wave_f64(prod, l);
                        m &= m - 1;
                    }
                    // everything below the piece's largest item is behind every later piece
                    const int32_t p_lo = wave_i32((int32_t)(p - lo), last);  // (a row is shorter than 2^31)
                    lo += p_lo;
                }
            }
        }
        if (lane == 0) out[j] = s;
    }
}

// out[j] = jaccardCoefficient(train)(us[j], vs[j]): an absent user has the empty set; 0.0 / 0 is NaN, as in Scala
__global__ void __launch_bounds__(PAIR_TPB) k_pair_jaccard(UserIds ids, const int64_t* __restrict__ u_ptr, const int32_t* __restrict__ s_col,
                                                           const int32_t* __restrict__ us, const int32_t* __restrict__ vs, int64_t n,
                                                           double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * PAIR_WAVES;
    for (int64_t j = (int64_t)blockIdx.x * PAIR_WAVES + (threadIdx.x >> 6); j < n; j += stride) {
        int32_t du, dv;
        pair_users(ids, us, vs, j, lane, du, dv);
        int64_t pu = 0, eu = 0, pv = 0, ev = 0;
        if (du >= 0) { pu = u_ptr[du]; eu = u_ptr[du + 1]; }
        if (dv >= 0) { pv = u_ptr[dv]; ev = u_ptr[dv + 1]; }
        const int64_t nu = eu - pu, nv = ev - pv;
        const bool u_short = nu <= nv;
        const int64_t pa = u_short ? pu : pv, ea = u_short ? eu : ev;
        int64_t lo = u_short ? pv : pu;
        const int64_t eb = u_short ? ev : eu;
        int64_t both = 0;
        for (int64_t base = pa; base < ea && lo < eb; base += 64) {
            const int64_t left = ea - base;
            const int last = (int)(left < 64 ? left : 64) - 1;
            bool hit = false;
            int64_t p = eb;
            if (lane <= last) {
                const int32_t c = s_col[base + lane];
                p = pair_lower_bound(s_col, lo, eb, c);
                hit = p < eb && s_col[p] == c;
            }
            both += __popcll(__ballot(hit));
            lo += wave_i32((int32_t)(p - lo), last);
        }
        if (lane == 0) out[j] = (double)both / (double)(nu + nv - both);
    }
}

// out[j] = 0.0 + (similarity of vs[j] in us[j]'s neighbour list), 0.0 when it is not there: one thread per pair searches the
// id-sorted copy of the list
__global__ void __launch_bounds__(PAIR_TPB) k_pair_knn_lookup(UserIds ids, int32_t kcap, const int32_t* __restrict__ nbr_cnt,
                                                              const int32_t* __restrict__ uidx, const double* __restrict__ usim,
                                                              const int32_t* __restrict__ us, const int32_t* __restrict__ vs, int64_t n,
                                                              double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * PAIR_TPB + threadIdx.x;
    if (j >= n) return;
    const int32_t du = dense_user_of(ids, us[j]), dv = dense_user_of(ids, vs[j]);
    double r = 0.0;
    if (du >= 0 && dv >= 0 && kcap > 0) {
        const int64_t base = (int64_t)du * kcap;
        int32_t lo = 0, hi = nbr_cnt[du];
        const int32_t cnt = hi;
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (uidx[base + mid] < dv) lo = mid + 1;
            else hi = mid;
        }
        if (lo < cnt && uidx[base + lo] == dv) r = 0.0 + usim[base + lo];  // (.sum from 0.0: -0.0 becomes +0.0)
    }
    out[j] = r;
}

static UserIds user_ids(const Train& tr) { return UserIds{tr.u_table.p, tr.u_table_n, tr.ukeys.p, tr.U}; }

static unsigned pair_blocks(int64_t n) { return (unsigned)std::min<int64_t>(PAIR_MAX_BLOCKS, ceil_div(n, PAIR_WAVES)); }

void launch_pair_similarity(const Train& tr, bool jaccard, const int32_t* d_us, const int32_t* d_vs, int64_t n, double* d_out,
                            hipStream_t st) {
    if (n <= 0) return;
    KN_TRACE_DISPATCH("pairs %s n=%lld", jaccard ? "jaccard" : "cosine", (long long)n);
    if (jaccard) k_pair_jaccard<<<pair_blocks(n), PAIR_TPB, 0, st>>>(user_ids(tr), tr.u_ptr.p, tr.s_col.p, d_us, d_vs, n, d_out);
    else k_pair_cosine<<<pair_blocks(n), PAIR_TPB, 0, st>>>(user_ids(tr), tr.u_ptr.p, tr.s_col.p, tr.s_t.p, tr.s_pre.p, d_us, d_vs, n, d_out);
    KN_HIP(hipGetLastError());
}

void launch_pair_knn_lookup(const Train& tr, NeighborTable& nt, const int32_t* d_us, const int32_t* d_vs, int64_t n, double* d_out,
                            hipStream_t st) {
    if (n <= 0) return;
    const bool lists = tr.U >= 2 && nt.kcap > 0;
    if (lists && !nt.by_id_valid) {
        launch_sort_neighbors(nt, tr.U, tr.U, nullptr, st);
        nt.by_id_valid = true;
    }
    KN_TRACE_DISPATCH("pairs lookup n=%lld", (long long)n);
    k_pair_knn_lookup<<<(unsigned)ceil_div(n, PAIR_TPB), PAIR_TPB, 0, st>>>(user_ids(tr), lists ? nt.kcap : 0, nt.cnt.p, nt.uidx.p, nt.usim.p,
                                                                            d_us, d_vs, n, d_out);
    KN_HIP(hipGetLastError());
}

}  // namespace knncf
