// explain.hip — the neighbour terms behind a kNN prediction (knncf_explain*; DESIGN.md "Explanations").
//
// weightedSumDeviation shared/predictions.scala:504-548 maps the item's raters, in training file order, to
// simVal = (deviation, getSimilarity(u, rater)) :513-517 and folds (num + dev * sim, den + |sim|) from (0.0, 0.0) :520-524.
// The TERMS of a row (u, i) are the elements of simVal whose similarity is non-zero: the neighbours of u that rated i and
// whose similarity is not exactly 0.0.  k_predict_knn (predict.hip) finds them, orders them and folds them with the steps of
// knn_terms.h; this kernel takes the same steps with TERMS: the zero-similarity matches are dropped before the fold (they add
// +-0.0: identities) and what that kernel discards is kept: who the raters were and what each of them contributed.  One
// wavefront per row:
//   terms   wave_knn_matches<CAP, true> + fold_terms: probe, compaction, file order, the additions of k_predict_knn
//   weight  KNNCF_EXPLAIN_BY_WEIGHT: a second counting rank by (|similarity| descending, summation order ascending)
//   emit    lane l writes output cells l, l + 64, ... of the row: adjacent lanes, adjacent cells
#include <math.h>
#include <stdio.h>

#include "knn_terms.h"

namespace knncf {

struct ExplainArgs {
    const double* user_avg;
    double global_avg;
    ProbeArgs P;  // (the lists sorted by id)
    const int32_t* uid;  // raw id of a dense user
    int32_t order, cap;
    // outputs: term arrays [n * cap] (unused with cap == 0), counts [n], sums [2 n] and pred [n] (either may be null)
    int32_t* raters;
    double* sims;
    double* devs;
    int32_t* counts;
    double* sums;
    double* pred;
};

template <int CAP, int WAVES>  // per-wave match capacity (power of two >= kcap), waves per block
__global__ void __launch_bounds__(WAVES * 64) k_explain(ExplainArgs A, int64_t n, const int32_t* __restrict__ du,
                                                        const int32_t* __restrict__ di) {
    // 24 B per match and wave: file row (then the BY_WEIGHT order), place in the item's rater list, deviation, similarity
    __shared__ __attribute__((aligned(16))) uint32_t m_t[WAVES][CAP];
    __shared__ uint32_t m_q[WAVES][CAP];
    __shared__ double m_dev[WAVES][CAP];
    __shared__ double m_sim[WAVES][CAP];
    constexpr int TR = CAP / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * WAVES + wave;
    if (t >= n) return;
    const int32_t u = du[t], i = di[t];
    const double ua = (u >= 0) ? A.user_avg[u] : -1.0;  // usersAvgValue.getOrElse(u, -1.0) :572
    int32_t total = 0;
    NumDen f{0.0, 0.0};  // the fold over all terms
    double p;
    if (ua < 0.0) {
        p = A.global_avg;  // (:573 — wsd is not evaluated: no terms)
    } else if (i < 0) {
        p = combine(ua, 0.0);  // no rater: den = 0 -> 0.0 :527-529
    } else {
        uint32_t* mt = m_t[wave];
        uint32_t* mq = m_q[wave];
        double* md = m_dev[wave];
        double* ms = m_sim[wave];
        const int64_t rb = A.P.i_ptr[i];
        total = wave_knn_matches<CAP, true>(A.P, u, i, rb, A.P.i_ptr[i + 1], lane, mt, mq, md, ms);
        const int nslot = (total + 63) >> 6;  // wave-uniform
        f = fold_terms(md, ms, total);  // :520-524
        const double wsd = (f.den > 0) ? f.num / f.den : 0.0;
        p = combine(ua, wsd);
        const int32_t m = min(total, A.cap);  // terms to write
        const bool by_weight = A.order == KNNCF_EXPLAIN_BY_WEIGHT;
        if (by_weight && m > 0) {
            // place of each term under (|similarity| descending, summation order ascending): every lane streams all magnitudes
            // and counts the terms that go first.  The file rows in mt are spent: it takes the order, mt[place] = term.
            double a[TR];
            uint32_t place[TR];
#pragma unroll
            for (int k = 0; k < TR; ++k) {
                const int32_t c = 64 * k + lane;
                place[k] = 0;
                a[k] = (c < total) ? fabs(ms[c]) : 0.0;
            }
            for (int32_t c2 = 0; c2 < total; ++c2) {
                const double b = fabs(ms[c2]);
#pragma unroll
                for (int k = 0; k < TR; ++k) {
                    if (k < nslot) place[k] += (uint32_t)(b > a[k] || (b == a[k] && c2 < 64 * k + lane));
                }
            }
#pragma unroll
            for (int k = 0; k < TR; ++k) {
                if (64 * k + lane < total) mt[place[k]] = (uint32_t)(64 * k + lane);
            }
            wave_sync();
        }
        const int64_t ob = t * (int64_t)A.cap;
        for (int32_t o = lane; o < m; o += 64) {
            const uint32_t c = by_weight ? mt[o] : (uint32_t)o;
            A.raters[ob + o] = A.uid[A.P.it_user[rb + mq[c]]];
            A.sims[ob + o] = ms[c];
            A.devs[ob + o] = md[c];
        }
    }
    if (lane == 0) {
        A.counts[t] = total;
        if (A.sums) {
            A.sums[2 * t] = f.num;
            A.sums[2 * t + 1] = f.den;
        }
        if (A.pred) A.pred[t] = p;
    }
}

void launch_explain(const Train& tr, NeighborTable& nt, int64_t n, const int32_t* d_du, const int32_t* d_di, const ExplainCells& out,
                    hipStream_t st) {
    if (n <= 0) return;
    ExplainArgs A{};
    A.user_avg = tr.user_avg.p; A.global_avg = tr.global_avg;
    A.P = probe_args(tr, nt, /*by_id=*/true, st);
    A.uid = tr.uid.p;
    A.order = out.order; A.cap = out.cap;
    A.raters = out.raters; A.sims = out.sims; A.devs = out.devs; A.counts = out.counts; A.sums = out.sums; A.pred = out.pred;
#define KN_LAUNCH_EXPLAIN(CAPV, WV)                                                                           \
    do {                                                                                                      \
        KN_TRACE_DISPATCH("explain CAP=%d bits=%d order=%d", CAPV, tr.ib_words > 0 ? 1 : 0, (int)out.order);  \
        k_explain<CAPV, WV><<<(unsigned)ceil_div(n, WV), WV * 64, 0, st>>>(A, n, d_du, d_di);                \
    } while (0)
    if (nt.kcap <= 64) KN_LAUNCH_EXPLAIN(64, 4);
    else if (nt.kcap <= 128) KN_LAUNCH_EXPLAIN(128, 4);
    else if (nt.kcap <= 256) KN_LAUNCH_EXPLAIN(256, 4);
    else if (nt.kcap <= 512) KN_LAUNCH_EXPLAIN(512, 4);
    else if (nt.kcap <= 1024) KN_LAUNCH_EXPLAIN(1024, 2);
    else if (nt.kcap <= 2048) KN_LAUNCH_EXPLAIN(2048, 1);
    else throw Error(KNNCF_E_UNSUPPORTED, "explain: k > 2048 (the engine-wide limit of the kNN prediction kernels)");
#undef KN_LAUNCH_EXPLAIN
    KN_HIP(hipGetLastError());
}

}  // namespace knncf
