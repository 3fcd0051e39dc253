// explain_select.h — the wave-level steps that the explanations of Personalized predictions share: k_explain_all
// (explain_all.hip, users as the fit holds them) and k_qb_explain_all (foldin.hip, fold-in / update / revise queries).
//
// Both kernels give one wavefront a row whose candidate terms form a SEQUENCE of positions in summation order, far longer
// than cap, and pick the cap heaviest without ordering it.  What differs is where a position's values come from, so the steps
// are templates over a lane-level TERM READER R:
//     int64_t lo, hi                           positions [lo, hi) in summation order
//     int32_t rater(int64_t p)                 lo <= p < hi: the handle by which the other three find the position's values
//     double  sim(int64_t p, int32_t v)        lo <= p < hi, v = rater(p): the similarity; 0.0 means "no term"
//     double  dev(int64_t p, int32_t v)        the rater's normalized deviation on the row's item
//     int32_t raw(int64_t p, int32_t v)        the rater's raw id
// A position past the end is never read: it contributes similarity 0.0.
//   walk_terms     f(p0, v, s) for every trip of 64 positions, XA_DEEP trips' loads in flight together
//   select_heaviest the radix select on the bit pattern of |s| (non-negative doubles order as unsigned integers; the sign bit is
//                  cleared, so the top byte is below 128): per 8-bit digit, from the top, the histogram of the entries that agree
//                  with the digits chosen so far, a scan from bin 255 down to the bin that holds the cap-th largest, descent
//                  into it.  It stops as soon as that bin holds no more than what is still wanted (everything >= the prefix is
//                  taken) or after the eighth digit (the prefix is the threshold magnitude t, and `want` of the entries equal
//                  to t are taken).  The top digit's histogram is the caller's: it is counted during the caller's own walk.
//   emit_heaviest  one more pass writes, in place order, every term with |s| > t and the FIRST `want` terms with |s| == t — the
//                  reference's stable order among ties — into the row's staging cells: min(count, cap) terms, places ascending
//   rank_staged    the staged terms by counting under (|s| descending, staged index ascending), a strict total order; each goes
//                  to its rank in the output row
// Bounds.  Histogram bins are one byte of the key: < 256.  A term is staged at an index < m = min(count, cap) (checked at the
// store) inside the row's cap cells at ob; a rank counts staged terms other than its own: < the staged number (checked at the
// store).  `hist` is 256 words and `sa` 64 doubles of LDS owned by the wave.
#pragma once

#include <math.h>

#include "knn_terms.h"

namespace knncf {

static constexpr int XA_DEEP = 4;  // trips of 64 whose loads a walk / select / emit pass has in flight together
static constexpr int XA_OWN = 4;   // staged terms per lane that one sweep over the staged keys ranks

// |s| as an unsigned integer: the order of the magnitudes; 0 for +-0.0, which is no term
__device__ __forceinline__ uint64_t mag_key(double s) { return (uint64_t)__double_as_longlong(s) & 0x7fffffffffffffffull; }

// the BY_WEIGHT staging cells of a launch, the layout of the outputs' term arrays
struct ExplainStage {
    double* sim;
    double* dev;
    int32_t* rater;
};
__host__ __device__ inline ExplainStage explain_stage(double* base, int64_t n_rows, int32_t cap) {
    const size_t cells = (size_t)n_rows * (size_t)cap;
    return {base, base + cells, reinterpret_cast<int32_t*>(base + 2 * cells)};
}

// f(p0, v, s) for every trip of 64 positions [p0, p0 + 64) of the reader in order, until it returns false (the same in every
// lane); a lane past the end gets v = 0 and s = 0.0.  XA_DEEP trips' loads are issued together
template <class R, class F>
__device__ __forceinline__ void walk_terms(const R& rd, int lane, F&& f) {
    for (int64_t p0 = rd.lo; p0 < rd.hi; p0 += 64 * XA_DEEP) {
        int32_t v[XA_DEEP];
        double s[XA_DEEP];
#pragma unroll
        for (int k = 0; k < XA_DEEP; ++k) v[k] = (p0 + 64 * k + lane < rd.hi) ? rd.rater(p0 + 64 * k + lane) : 0;
#pragma unroll
        for (int k = 0; k < XA_DEEP; ++k) s[k] = (p0 + 64 * k + lane < rd.hi) ? rd.sim(p0 + 64 * k + lane, v[k]) : 0.0;
#pragma unroll
        for (int k = 0; k < XA_DEEP; ++k) {
            if (p0 + 64 * k < rd.hi) {  // (uniform)
                if (!f(p0 + 64 * k, v[k], s[k])) return;
            }
        }
    }
}

// what emit_heaviest takes: every key >= ge, and the first take_eq of those equal to eq
struct HeavyCut {
    uint64_t ge = 1, eq = 0;
    int32_t take_eq = 0;
};

// total > cap > 0 terms; hist holds the counts of the terms' top key bytes (complete and visible to the wave)
template <class R>
__device__ __forceinline__ HeavyCut select_heaviest(const R& rd, int lane, int32_t cap, uint32_t* hist) {
    HeavyCut cut;
    uint64_t prefix = 0;
    int32_t want = cap;  // 1 <= want <= the entries that agree with prefix, throughout
    for (int d = 0; d < 8; ++d) {
        const int shift = 56 - 8 * d;
        if (d > 0) {  // (the top digit was counted by the caller's walk)
            for (int b = lane; b < 256; b += 64) hist[b] = 0;
            wave_sync();
            walk_terms(rd, lane, [&](int64_t, int32_t, double x) {
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
            cut.ge = prefix;
            break;
        }
        if (d == 7) {
            cut.ge = prefix + 1;
            cut.eq = prefix;
            cut.take_eq = want;
        }
        wave_sync();  // (the bins are read before the next digit clears them)
    }
    return cut;
}

// the terms the cut takes, in place order, into staging cells [ob, ob + m); returns their number (<= m)
template <class R>
__device__ __forceinline__ int32_t emit_heaviest(const R& rd, int lane, const HeavyCut& cut, int32_t m, const ExplainStage& st, int64_t ob) {
    int32_t staged = 0, eq_seen = 0;
    walk_terms(rd, lane, [&](int64_t p0, int32_t x, double sx) {
        const uint64_t key = mag_key(sx);
        const bool is_eq = cut.take_eq > 0 && key == cut.eq;  // (eq != 0 when take_eq > 0)
        const unsigned long long eqm = __ballot(is_eq);
        const bool em = key != 0 && (key >= cut.ge || (is_eq && eq_seen + lanes_below(eqm) < cut.take_eq));
        const unsigned long long emm = __ballot(em);
        if (em) {
            const int32_t at = staged + lanes_below(emm);
            if (at < m) {
                st.sim[ob + at] = sx;
                st.dev[ob + at] = rd.dev(p0 + lane, x);
                st.rater[ob + at] = rd.raw(p0 + lane, x);
            }
        }
        staged += __popcll(emm);
        eq_seen += __popcll(eqm);
        return staged < m;  // (uniform) nothing further is wanted
    });
    return min(staged, m);
}

// lane l owns staged terms e0 + l, e0 + 64 + l, ...; every lane streams all staged magnitudes, 64 at a time through LDS
// (broadcast reads), and counts the terms that go first
__device__ __forceinline__ void rank_staged(int lane, int32_t staged, const ExplainStage& st, int64_t ob, const ExplainCells& out, double* sa) {
    // the staged cells were written by other lanes of this wave: complete the stores before they are read back
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    for (int32_t e0 = 0; e0 < staged; e0 += 64 * XA_OWN) {
        double a[XA_OWN];
        uint32_t rank[XA_OWN];
#pragma unroll
        for (int k = 0; k < XA_OWN; ++k) {
            const int32_t e = e0 + 64 * k + lane;
            a[k] = (e < staged) ? fabs(st.sim[ob + e]) : 0.0;  // (past the end: precedes nothing, is not written)
            rank[k] = 0;
        }
        for (int32_t t0 = 0; t0 < staged; t0 += 64) {
            sa[lane] = (t0 + lane < staged) ? fabs(st.sim[ob + t0 + lane]) : 0.0;
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
                out.raters[ob + rank[k]] = st.rater[ob + e];
                out.sims[ob + rank[k]] = st.sim[ob + e];
                out.devs[ob + rank[k]] = st.dev[ob + e];
            }
        }
    }
}

// KNNCF_EXPLAIN_BY_WEIGHT for a row of total > 0 terms and cap > 0, after the caller's walk has counted the terms' top key
// bytes into hist: select (only when total > cap), emit, rank
template <class R>
__device__ __forceinline__ void explain_by_weight(const R& rd, int lane, int32_t total, const ExplainCells& out, const ExplainStage& st,
                                                  int64_t ob, uint32_t* hist, double* sa) {
    const int32_t m = min(total, out.cap);
    HeavyCut cut;
    if (total > out.cap) cut = select_heaviest(rd, lane, out.cap, hist);
    const int32_t staged = emit_heaviest(rd, lane, cut, m, st, ob);
    rank_staged(lane, staged, st, ob, out, sa);
}

}  // namespace knncf
