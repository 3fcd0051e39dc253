// explain.hip — the neighbour terms behind a kNN prediction (knncf_explain*; DESIGN.md "Explanations").
//
// weightedSumDeviation shared/predictions.scala:504-548 maps the item's raters, in training file order, to
// simVal = (deviation, getSimilarity(u, rater)) :513-517 and folds (num + dev * sim, den + |sim|) from (0.0, 0.0) :520-524.
// The TERMS of a row (u, i) are the elements of simVal whose similarity is non-zero: the neighbours of u that rated i and
// whose similarity is not exactly 0.0.  k_predict_knn (predict.hip) finds them, orders them and folds them; this kernel does
// the same, drops the zero-similarity matches before the fold (they add +-0.0: identities) and keeps what that kernel
// discards: who the raters were and what each of them contributed.  One wavefront per row:
//   probe   lanes stride over u's id-sorted neighbour list and ask "did neighbour v rate item i, and where": the item's
//           rater bitmap + rank prefixes (tr.ib_words > 0) or a binary search in the item's rater list
//   order   matches compacted into LDS (ballot / mbcnt), ranked by training file row by counting, moved to their ranks,
//           folded left in fp64 — the additions of k_predict_knn in the same order
//   weight  KNNCF_EXPLAIN_BY_WEIGHT: a second counting rank by (|similarity| descending, summation order ascending)
//   emit    lane l writes output cells l, l + 64, ... of the row: adjacent lanes, adjacent cells
#include <math.h>
#include <stdio.h>

#include "engine.h"

namespace knncf {

struct ExplainArgs {
    const double* user_avg;
    double global_avg;
    // neighbour table, ids ascending
    const int32_t* nbr_uidx;
    const double* nbr_usim;
    const int32_t* nbr_cnt;
    int32_t kcap;
    // item-major rows, raters ascending
    const int64_t* i_ptr;
    const int32_t* it_user;
    const double* it_dev;
    const uint32_t* it_t;
    // per-item rater bitmaps (ib_words == 0: not built, binary search instead)
    int64_t ib_words;
    const unsigned long long* item_bits;
    const uint32_t* item_rank;
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

__device__ __forceinline__ void wave_sync() {
    // lanes of one wave exchange data through LDS: order the accesses for the compiler (the LDS queue is in order per wave)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// a pointer whose value is the same in every lane, moved to scalar registers (buffer descriptors must be uniform)
template <class T>
__device__ __forceinline__ T* uniform_ptr(T* p) {
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return reinterpret_cast<T*>(((uint64_t)hi << 32) | lo);
}

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
    double num = 0.0, den = 0.0, p;
    if (ua < 0.0) {
        p = A.global_avg;  // (:573 — wsd is not evaluated: no terms)
    } else if (i < 0) {
        p = combine(ua, 0.0);  // no rater: den = 0 -> 0.0 :527-529
    } else {
        uint32_t* mt = m_t[wave];
        uint32_t* mq = m_q[wave];
        double* md = m_dev[wave];
        double* ms = m_sim[wave];
        const int32_t cnt = __builtin_amdgcn_readfirstlane(A.nbr_cnt[u]);  // (u is the same in every lane)
        const int64_t base = (int64_t)u * A.kcap;
        const int64_t rb = A.i_ptr[i], re = A.i_ptr[i + 1];
        if (A.ib_words > 0) {
            // item i's rater bitmap (U bits) + rank prefixes: one 8-byte + one 4-byte read per neighbour.  Three levels of
            // dependent gathers (neighbour ids -> bitmap words -> the matched ratings), each issued for ALL neighbours at once
            // through buffer descriptors rooted at the wave's own rows: a lane without a neighbour, or without a match, uses an
            // out-of-range offset and gets 0 (k_predict_knn's scheme)
            const int32_t rowlen = __builtin_amdgcn_readfirstlane((int32_t)(re - rb));
            const int32_t ibw = __builtin_amdgcn_readfirstlane((int32_t)A.ib_words);
            const auto r_uidx = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(uniform_ptr(A.nbr_uidx + base)), 0, (uint32_t)cnt * 4u, 0x00020000);
            const auto r_usim = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(uniform_ptr(A.nbr_usim + base)), 0, (uint32_t)cnt * 8u, 0x00020000);
            const auto r_bits = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned long long*>(uniform_ptr(A.item_bits + (int64_t)i * A.ib_words)), 0, (uint32_t)ibw * 8u, 0x00020000);
            const auto r_rank = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(uniform_ptr(A.item_rank + (int64_t)i * A.ib_words)), 0, (uint32_t)ibw * 4u, 0x00020000);
            const auto r_t = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(uniform_ptr(A.it_t + rb)), 0, (uint32_t)rowlen * 4u, 0x00020000);
            const auto r_dev = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(uniform_ptr(A.it_dev + rb)), 0, (uint32_t)rowlen * 8u, 0x00020000);
            typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
            uint32_t x[TR], rk[TR], mtv[TR], qv[TR];
            u32x2 sv[TR], wd[TR], dv[TR];
#pragma unroll
            for (int k = 0; k < TR; ++k) {  // level 1: neighbour ids and similarities (offsets past cnt are out of range)
                const uint32_t j = 64u * k + lane;
                x[k] = __builtin_amdgcn_raw_buffer_load_b32(r_uidx, (int)(j * 4u), 0, 0);
                sv[k] = __builtin_amdgcn_raw_buffer_load_b64(r_usim, (int)(j * 8u), 0, 0);
            }
#pragma unroll
            for (int k = 0; k < TR; ++k) {  // level 2: the bitmap word of each neighbour and the raters before that word
                const uint32_t wi = (64u * k + lane < (uint32_t)cnt) ? (x[k] >> 6) : 0x0fffffffu;
                wd[k] = __builtin_amdgcn_raw_buffer_load_b64(r_bits, (int)(wi * 8u), 0, 0);
                rk[k] = __builtin_amdgcn_raw_buffer_load_b32(r_rank, (int)(wi * 4u), 0, 0);
            }
            bool fnd[TR];
#pragma unroll
            for (int k = 0; k < TR; ++k) {  // level 3: the matched ratings (file row, deviation) of the non-zero neighbours
                const unsigned long long word = ((unsigned long long)wd[k].y << 32) | wd[k].x;  // (absent neighbour: 0)
                fnd[k] = ((word >> (x[k] & 63u)) & 1ull) && __hiloint2double((int)sv[k].y, (int)sv[k].x) != 0.0;
                qv[k] = fnd[k] ? rk[k] + (uint32_t)__popcll(word & ((1ull << (x[k] & 63u)) - 1ull)) : 0x0fffffffu;
                mtv[k] = __builtin_amdgcn_raw_buffer_load_b32(r_t, (int)(qv[k] * 4u), 0, 0);
                dv[k] = __builtin_amdgcn_raw_buffer_load_b64(r_dev, (int)(qv[k] * 8u), 0, 0);
            }
#pragma unroll
            for (int k = 0; k < TR; ++k) {
                const unsigned long long hit = __ballot(fnd[k]);
                if (fnd[k]) {
                    const int32_t slot = total + __builtin_amdgcn_mbcnt_hi((uint32_t)(hit >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hit, 0u));
                    mt[slot] = mtv[k];
                    mq[slot] = qv[k];
                    md[slot] = __hiloint2double((int)dv[k].y, (int)dv[k].x);
                    ms[slot] = __hiloint2double((int)sv[k].y, (int)sv[k].x);
                }
                total += __popcll(hit);
            }
        } else {
            // bitmaps not built (they would not fit): u's neighbour ids (sorted ascending) are looked up in the item's rater
            // list (sorted the same way) by binary search
            for (int32_t j0 = 0; j0 < cnt; j0 += 64) {
                const int32_t j = j0 + lane;
                int64_t lo = rb, hi = rb;
                int32_t x = 0;
                double s = 0.0;
                if (j < cnt) {
                    x = A.nbr_uidx[base + j];
                    s = A.nbr_usim[base + j];
                    hi = re;
                }
                while (__any(lo < hi)) {
                    if (lo < hi) {
                        const int64_t mid = (lo + hi) >> 1;
                        if (A.it_user[mid] < x) lo = mid + 1;
                        else hi = mid;
                    }
                }
                const bool found = j < cnt && s != 0.0 && lo < re && A.it_user[lo] == x;
                const unsigned long long hit = __ballot(found);
                if (found) {
                    const int32_t slot = total + __popcll(hit & ((1ull << lane) - 1ull));
                    mt[slot] = A.it_t[lo];
                    mq[slot] = (uint32_t)(lo - rb);
                    md[slot] = A.it_dev[lo];
                    ms[slot] = s;
                }
                total += __popcll(hit);
            }
        }
        const int nslot = (total + 63) >> 6;  // wave-uniform
        // order the matches by training file row (the order of ratedI(i) :508-517): rank by counting, as k_predict_knn does.
        // Lane l owns the matches in slots l, l + 64, ...; every lane streams all keys (LDS broadcast reads, 4 keys per read)
        // and counts the smaller ones; then each match moves to its rank.
        {
            for (int32_t c = total + lane; c < ((total + 3) & ~3); c += 64) mt[c] = 0xffffffffu;  // pad to a multiple of 4
            wave_sync();
            uint32_t my_t[TR], my_q[TR], rank[TR];
            double my_d[TR], my_s[TR];
#pragma unroll
            for (int k = 0; k < TR; ++k) {
                const int32_t slot = 64 * k + lane;
                rank[k] = 0;
                my_t[k] = 0;  // (a slot past `total` counts nothing and is not written back)
                my_q[k] = 0;
                my_d[k] = 0.0;
                my_s[k] = 0.0;
                if (slot < total) {
                    my_t[k] = mt[slot];
                    my_q[k] = mq[slot];
                    my_d[k] = md[slot];
                    my_s[k] = ms[slot];
                }
            }
            const uint4* keys4 = reinterpret_cast<const uint4*>(mt);
            for (int32_t c = 0; c < ((total + 3) >> 2); ++c) {
                const uint4 kq = keys4[c];
#pragma unroll
                for (int k = 0; k < TR; ++k) {
                    if (k < nslot) rank[k] += (uint32_t)(kq.x < my_t[k]) + (uint32_t)(kq.y < my_t[k]) + (uint32_t)(kq.z < my_t[k]) + (uint32_t)(kq.w < my_t[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < TR; ++k) {
                if (64 * k + lane < total) {
                    mq[rank[k]] = my_q[k];
                    md[rank[k]] = my_d[k];
                    ms[rank[k]] = my_s[k];
                }
            }
            wave_sync();
        }
        for (int32_t c = 0; c < total; ++c) {  // every lane folds the same sequence (LDS broadcast) :520-524
            const double s = ms[c];
            num = num + md[c] * s;
            den = den + fabs(s);
        }
        const double wsd = (den > 0) ? num / den : 0.0;
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
            A.raters[ob + o] = A.uid[A.it_user[rb + mq[c]]];
            A.sims[ob + o] = ms[c];
            A.devs[ob + o] = md[c];
        }
    }
    if (lane == 0) {
        A.counts[t] = total;
        if (A.sums) {
            A.sums[2 * t] = num;
            A.sums[2 * t + 1] = den;
        }
        if (A.pred) A.pred[t] = p;
    }
}

void launch_explain(const Train& tr, NeighborTable& nt, int64_t n, const int32_t* d_du, const int32_t* d_di, const ExplainCells& out,
                    hipStream_t st) {
    if (n <= 0) return;
    ExplainArgs A{};
    A.user_avg = tr.user_avg.p; A.global_avg = tr.global_avg;
    // the probes want neighbouring lanes on neighbouring ids: the id-sorted copies, made on first need as in launch_predict
    if (!nt.by_id_valid) {
        launch_sort_neighbors(nt, tr.U, tr.U, nullptr, st);
        nt.by_id_valid = true;
    }
    A.nbr_uidx = nt.uidx.p; A.nbr_usim = nt.usim.p; A.nbr_cnt = nt.cnt.p; A.kcap = nt.kcap;
    A.i_ptr = tr.i_ptr.p; A.it_user = tr.it_user.p; A.it_dev = tr.it_dev.p; A.it_t = tr.it_t.p;
    A.ib_words = tr.ib_words; A.item_bits = reinterpret_cast<const unsigned long long*>(tr.item_bits.p); A.item_rank = tr.item_rank.p;
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
