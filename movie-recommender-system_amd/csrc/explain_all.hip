// explain_all.hip — the terms behind a Personalized prediction of a fitted user (knncf_explain_personalized*; DESIGN.md
// "Explanations of Personalized predictions").
//
// predictor(train, weightedSumDeviation(train, sim)) predict/Personalized.scala:61-72 has no neighbourhood cut: simVal
// shared/predictions.scala:513-517 pairs EVERY rating of the item, in training file order, with sim(u, rater), and the fold
// :520-524 runs over all of them.  The TERMS of a row (u, i) are the elements whose similarity is not exactly 0.0, u itself
// among them when (u, i) is a training pair.  A popular item has 10^4 .. 10^5 of them, so KNNCF_EXPLAIN_BY_WEIGHT cannot rank
// the segment as explain.hip does: it SELECTS the cap heaviest terms first and ranks only those.  One wavefront per row:
//   walk    the item's raters [i_ptr[i], i_ptr[i + 1]) in file order (pf_user / pf_dev), 64 per coalesced load, s gathered from
//           the user's exact row S[slot[u]][rater]; the two left folds of k_fold_rows (personalized.hip) restated: every rater's
//           product and magnitude through LDS, added serially in file order — zero similarities add +-0.0 to sums that start
//           at +0.0.  The non-zero entries are counted by ballot / mbcnt: the running count is the term's place in the fold.
//           SUM_ORDER stores a term while its place is below cap.  BY_WEIGHT counts the top byte of |s| into an LDS histogram.
//   select / emit / rank   (BY_WEIGHT) the steps of explain_select.h over this row's raters (FitTerms below): the radix select
//           of the cap heaviest when count > cap, the staging of the selected terms in place order, their rank by counting.
//           k_qb_explain_all (foldin.hip) runs the same steps over a query's terms.
// Cost per row of L raters, C = count of terms, m = min(C, cap), in wave steps: the walk is ceil(L / 64) loads + L serial
// additions (k_fold_rows's); BY_WEIGHT adds at most 7 histogram passes + 1 emit pass of ceil(L / 256) four-deep load groups each
// (none of the 7 when C <= cap) and ceil(m / 256) * m compare steps for the rank.  Nothing grows with L^2; cap >= C ranks all C
// terms, which is the caller's choice.
// Bounds, by construction: a lane reads pf_user / pf_dev only at c < i_ptr[i + 1] and S only at a rater it read there (a dense
// user < U, in the row slot[u] < R that launch_sim_rows wrote for this block); a lane past the segment's end contributes
// similarity 0.0, which is no term.  Histogram bins are one byte of the key: < 256.  A term is stored at place / staged index
// < min(count, cap) <= cap inside row w's cap cells (checked at the store); a rank counts staged terms other than its own: <
// the staged number.  Row w < n of the launch owns cells [w * cap, (w + 1) * cap) of the outputs and of the staging.
#include <math.h>

#include "explain_select.h"

namespace knncf {

static constexpr int XA_WAVES = 4;  // rows per workgroup

struct ExplainAllArgs {
    const uint32_t* order;  // row w of the launch is row order[w] of du / di
    const int32_t* du;
    const int32_t* di;
    const int32_t* slot;    // row of S of a user of the block
    const double* S;
    int32_t U;
    const int64_t* i_ptr;
    const int32_t* pf_user;
    const double* pf_dev;
    const double* user_avg;
    double global_avg;
    const int32_t* uid;     // raw id of a dense user
    ExplainCells out;       // rows [0, n) of the launch
    ExplainStage st;        // BY_WEIGHT staging
};

// the term reader of explain_select.h over a fitted row: position p is entry p of pf_user / pf_dev, [lo, hi) the item's raters in
// file order
struct FitTerms {
    int64_t lo, hi;
    const int32_t* pf_user;
    const double* pf_dev;
    const double* row;       // the user's exact similarity row
    const int32_t* uid;
    __device__ __forceinline__ int32_t rater(int64_t p) const { return pf_user[p]; }
    __device__ __forceinline__ double sim(int64_t, int32_t v) const { return row[v]; }
    __device__ __forceinline__ double dev(int64_t p, int32_t) const { return pf_dev[p]; }
    __device__ __forceinline__ int32_t raw(int64_t, int32_t v) const { return uid[v]; }
};

__global__ void __launch_bounds__(XA_WAVES * 64) k_explain_all(ExplainAllArgs A, int64_t n) {
    __shared__ double s_prod[XA_WAVES][64], s_abs[XA_WAVES][64];
    __shared__ uint32_t s_hist[XA_WAVES][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * XA_WAVES + wave;
    if (w >= n) return;
    const int64_t t = A.order[w];
    const int32_t u = A.du[t], i = A.di[t];
    const int32_t cap = A.out.cap;
    const double ua = (u >= 0) ? A.user_avg[u] : -1.0;  // usersAvgValue.getOrElse(u, -1.0) :572
    int32_t total = 0;
    double num = 0.0, den = 0.0, p;
    if (ua < 0.0) {
        p = A.global_avg;  // (:573 — wsd is not evaluated: no terms)
    } else if (i < 0) {
        p = combine(ua, 0.0);  // no rater: den = 0 -> 0.0 :527-529
    } else {
        const double* row = A.S + (int64_t)A.slot[u] * A.U;
        const int64_t rb = A.i_ptr[i], re = A.i_ptr[i + 1];
        const int64_t ob = w * (int64_t)cap;
        const bool by_weight = A.out.order == KNNCF_EXPLAIN_BY_WEIGHT && cap > 0;
        double* sp = s_prod[wave];
        double* sa = s_abs[wave];
        uint32_t* hist = s_hist[wave];
        if (by_weight) {
            for (int b = lane; b < 256; b += 64) hist[b] = 0;
            wave_sync();
        }
        // ---- walk: k_fold_rows's software pipeline (the next trip's gathers and the ids of the one after are in flight while
        // the two serial chains of 64 additions run) and its additions, in its order
        int32_t v = (rb + lane < re) ? A.pf_user[rb + lane] : 0;
        double dv = (rb + lane < re) ? A.pf_dev[rb + lane] : 0.0;
        double s = (rb + lane < re) ? row[v] : 0.0;
        int32_t vn = (rb + 64 + lane < re) ? A.pf_user[rb + 64 + lane] : 0;
        for (int64_t c0 = rb; c0 < re; c0 += 64) {
            const bool live = c0 + lane < re;
            const int32_t cv = v;
            const double cd = dv, cs = live ? s : 0.0;
            const double prod = cd * cs, a = fabs(cs);
            if (c0 + 64 + lane < re) {
                v = vn;
                dv = A.pf_dev[c0 + 64 + lane];
                s = row[vn];
            }
            if (c0 + 128 + lane < re) vn = A.pf_user[c0 + 128 + lane];
            sp[lane] = prod;
            sa[lane] = a;
            wave_sync();
            const int m = (int)min<int64_t>(64, re - c0);
            for (int k = 0; k < m; ++k) {  // every lane folds the same sequence (LDS broadcast)
                num = num + sp[k];
                den = den + sa[k];
            }
            wave_sync();
            const bool nz = cs != 0.0;
            const unsigned long long hit = __ballot(nz);
            if (nz) {
                if (by_weight) {
                    atomicAdd(&hist[(uint32_t)(mag_key(cs) >> 56)], 1u);
                } else {
                    const int32_t place = total + lanes_below(hit);
                    if (place < cap) {
                        A.out.raters[ob + place] = A.uid[cv];
                        A.out.sims[ob + place] = cs;
                        A.out.devs[ob + place] = cd;
                    }
                }
            }
            total += __popcll(hit);
        }
        const double wsd = (den > 0) ? num / den : 0.0;
        p = combine(ua, wsd);
        if (by_weight && total > 0) {
            const FitTerms rd{rb, re, A.pf_user, A.pf_dev, row, A.uid};
            explain_by_weight(rd, lane, total, A.out, A.st, ob, hist, sa);
        }
    }
    if (lane == 0) {
        A.out.counts[w] = total;
        A.out.sums[2 * w] = num;
        A.out.sums[2 * w + 1] = den;
        A.out.pred[w] = p;
    }
}

void launch_explain_all(const Train& tr, const PersonalRows& pr, int64_t n_rows, const uint32_t* d_order, const int32_t* d_du,
                        const int32_t* d_di, const int32_t* d_slot, const double* d_S, const ExplainCells& out, double* d_stage,
                        hipStream_t st) {
    if (n_rows <= 0) return;
    ExplainAllArgs A{};
    A.order = d_order; A.du = d_du; A.di = d_di; A.slot = d_slot; A.S = d_S; A.U = tr.U;
    A.i_ptr = tr.i_ptr.p; A.pf_user = pr.pf_user.p; A.pf_dev = pr.pf_dev.p;
    A.user_avg = tr.user_avg.p; A.global_avg = tr.global_avg; A.uid = tr.uid.p;
    A.out = out;
    A.st = explain_stage(d_stage, n_rows, out.cap);
    KN_TRACE_DISPATCH("explain_all order=%d cap=%d rows=%lld", (int)out.order, (int)out.cap, (long long)n_rows);
    k_explain_all<<<(unsigned)ceil_div(n_rows, XA_WAVES), XA_WAVES * 64, 0, st>>>(A, n_rows);
    KN_HIP(hipGetLastError());
}

}  // namespace knncf
