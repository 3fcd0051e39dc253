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
//   select  (BY_WEIGHT, count > cap) radix select on the bit pattern of |s| (non-negative doubles order as unsigned integers; the
//           sign bit is cleared, so the top byte is below 128): per 8-bit digit, from the top, the histogram of the entries that
//           agree with the digits chosen so far, a scan from bin 255 down to the bin that holds the cap-th largest, descent into
//           it.  It stops as soon as that bin holds no more than what is still wanted (everything >= the prefix is taken) or
//           after the eighth digit (the prefix is the threshold magnitude t, and `want` of the entries equal to t are taken).
//   emit    one more pass writes, in place order, every term with |s| > t and the FIRST `want` terms with |s| == t — the
//           reference's stable order among ties — into the row's staging cells: min(count, cap) terms, places ascending.
//   rank    the staged terms by counting under (|s| descending, staged index ascending), the strict total order of k_explain;
//           each goes to its rank in the output row.
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

#include "engine.h"

namespace knncf {

static constexpr int XA_WAVES = 4;  // rows per workgroup
static constexpr int XA_DEEP = 4;   // trips of 64 whose loads a select / emit pass has in flight together
static constexpr int XA_OWN = 4;    // staged terms per lane that one sweep over the staged keys ranks

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
    double* st_sim;         // BY_WEIGHT staging, the layout of out's term arrays
    double* st_dev;
    int32_t* st_rater;
};

__device__ __forceinline__ void wave_sync() {
    // lanes of one wave exchange data through LDS: order the accesses for the compiler (the LDS queue is in order per wave)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int32_t lanes_below(unsigned long long mask) {
    return (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// |s| as an unsigned integer: the order of the magnitudes; 0 for +-0.0, which is no term
__device__ __forceinline__ uint64_t mag_key(double s) { return (uint64_t)__double_as_longlong(s) & 0x7fffffffffffffffull; }

// f(c0, rater, s) for every trip of 64 raters [c0, c0 + 64) of [rb, re) in file order, until it returns false (the same in every
// lane); a lane past the segment's end gets rater 0 and s = 0.0.  XA_DEEP trips' loads are issued together
template <class F>
__device__ __forceinline__ void walk_raters(int64_t rb, int64_t re, int lane, const int32_t* pf_user, const double* row, F&& f) {
    for (int64_t c0 = rb; c0 < re; c0 += 64 * XA_DEEP) {
        int32_t v[XA_DEEP];
        double s[XA_DEEP];
#pragma unroll
        for (int k = 0; k < XA_DEEP; ++k) v[k] = (c0 + 64 * k + lane < re) ? pf_user[c0 + 64 * k + lane] : 0;
#pragma unroll
        for (int k = 0; k < XA_DEEP; ++k) s[k] = (c0 + 64 * k + lane < re) ? row[v[k]] : 0.0;
#pragma unroll
        for (int k = 0; k < XA_DEEP; ++k) {
            if (c0 + 64 * k < re) {  // (uniform)
                if (!f(c0 + 64 * k, v[k], s[k])) return;
            }
        }
    }
}

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
            const int32_t m = min(total, cap);
            // ---- select: every key >= ge is taken, and the first take_eq of those equal to eq
            uint64_t ge = 1, eq = 0;
            int32_t take_eq = 0;
            if (total > cap) {
                uint64_t prefix = 0;
                int32_t want = cap;  // 1 <= want <= the entries that agree with prefix, throughout
                for (int d = 0; d < 8; ++d) {
                    const int shift = 56 - 8 * d;
                    if (d > 0) {  // (the top digit was counted by the walk)
                        for (int b = lane; b < 256; b += 64) hist[b] = 0;
                        wave_sync();
                        walk_raters(rb, re, lane, A.pf_user, row, [&](int64_t, int32_t, double x) {
                            const uint64_t key = mag_key(x);
                            if (key != 0 && (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
                            return true;
                        });
                    }
                    wave_sync();
                    int b = 255;
                    int32_t above = 0;  // entries of the bins above b
                    while (b > 0 && above + (int32_t)hist[b] < want) {  // (uniform: every lane reads the same bins)
                        above += (int32_t)hist[b];
                        --b;
                    }
                    const int32_t bucket = (int32_t)hist[b];
                    want -= above;
                    prefix |= (uint64_t)b << shift;
                    if (bucket <= want) {  // the whole bin is wanted: no need to tell its entries apart
                        ge = prefix;
                        break;
                    }
                    if (d == 7) {
                        ge = prefix + 1;
                        eq = prefix;
                        take_eq = want;
                    }
                    wave_sync();  // (the bins are read before the next digit clears them)
                }
            }
            // ---- emit into the staging row, in place order
            int32_t staged = 0, eq_seen = 0;
            walk_raters(rb, re, lane, A.pf_user, row, [&](int64_t c0, int32_t x, double sx) {
                const uint64_t key = mag_key(sx);
                const bool is_eq = take_eq > 0 && key == eq;  // (eq != 0 when take_eq > 0)
                const unsigned long long eqm = __ballot(is_eq);
                const bool em = key != 0 && (key >= ge || (is_eq && eq_seen + lanes_below(eqm) < take_eq));
                const unsigned long long emm = __ballot(em);
                if (em) {
                    const int32_t at = staged + lanes_below(emm);
                    if (at < m) {
                        A.st_sim[ob + at] = sx;
                        A.st_dev[ob + at] = A.pf_dev[c0 + lane];
                        A.st_rater[ob + at] = A.uid[x];
                    }
                }
                staged += __popcll(emm);
                eq_seen += __popcll(eqm);
                return staged < m;  // (uniform) nothing further is wanted
            });
            staged = min(staged, m);
            // the staged cells were written by other lanes of this wave: complete the stores before they are read back
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_wave_barrier();
            // ---- rank: lane l owns staged terms e0 + l, e0 + 64 + l, ...; every lane streams all staged magnitudes, 64 at a
            // time through LDS (broadcast reads), and counts the terms that go first
            for (int32_t e0 = 0; e0 < staged; e0 += 64 * XA_OWN) {
                double a[XA_OWN];
                uint32_t rank[XA_OWN];
#pragma unroll
                for (int k = 0; k < XA_OWN; ++k) {
                    const int32_t e = e0 + 64 * k + lane;
                    a[k] = (e < staged) ? fabs(A.st_sim[ob + e]) : 0.0;  // (past the end: precedes nothing, is not written)
                    rank[k] = 0;
                }
                for (int32_t t0 = 0; t0 < staged; t0 += 64) {
                    sa[lane] = (t0 + lane < staged) ? fabs(A.st_sim[ob + t0 + lane]) : 0.0;
                    wave_sync();
                    const int tm = min(64, staged - t0);
                    for (int f = 0; f < tm; ++f) {
                        const double b = sa[f];
#pragma unroll
                        for (int k = 0; k < XA_OWN; ++k) rank[k] += (uint32_t)(b > a[k] || (b == a[k] && t0 + f < e0 + 64 * k + lane));
                    }
                    wave_sync();
                }
#pragma unroll
                for (int k = 0; k < XA_OWN; ++k) {
                    const int32_t e = e0 + 64 * k + lane;
                    if (e < staged && rank[k] < (uint32_t)staged) {
                        A.out.raters[ob + rank[k]] = A.st_rater[ob + e];
                        A.out.sims[ob + rank[k]] = A.st_sim[ob + e];
                        A.out.devs[ob + rank[k]] = A.st_dev[ob + e];
                    }
                }
            }
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
    const size_t cells = (size_t)n_rows * (size_t)out.cap;
    A.st_sim = d_stage; A.st_dev = d_stage + cells; A.st_rater = reinterpret_cast<int32_t*>(d_stage + 2 * cells);
    KN_TRACE_DISPATCH("explain_all order=%d cap=%d rows=%lld", (int)out.order, (int)out.cap, (long long)n_rows);
    k_explain_all<<<(unsigned)ceil_div(n_rows, XA_WAVES), XA_WAVES * 64, 0, st>>>(A, n_rows);
    KN_HIP(hipGetLastError());
}

}  // namespace knncf
