// knn_terms.h — the wave-level steps that every kNN answer is made of: for a row (u, i), WHICH of u's neighbours rated i (probe),
// those matches in the order of the training file (rank), and the left fold (num + dev * sim, den + |sim|) in fp64 over them.
// The comparison with the reference is bitwise, so the additions and their order are the contract.  Who takes what:
//   k_predict_knn, k_explain (predict.hip, explain.hip)   wave_knn_matches + fold_terms: the whole core, written once for both
//   k_predict_knn_sweep (ksweep.hip)                      lds_pair_probe, pad_file_rows (its rank writes a permutation and its
//                                                         fold filters by list position: its own)
//   k_predict_knn_rows, k_predict_knn_items (predict.hip) raw_buffer, as_double, NO_ENTRY, pad_file_rows (items), lanes_below
// The ordering rule is therefore NOT in one place: the rows and items kernels keep their own probe, counting rank and fold,
// because their instruction streams are kept as they are (DESIGN.md "The shared kNN term core"), and the sweep keeps its rank.
// A correction to the sentinel, the padding or a bound is made here, in those two kernels and in the sweep; the comments at
// those sites name the step of this header that they spell out.
#pragma once

#include <math.h>

#include "engine.h"
#include "wave_helpers.h"

namespace knncf {

typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

// raw buffer descriptor over [base, base + bytes), base the same in every lane: a load at a byte offset >= bytes touches no
// memory and returns 0, which is how the probes below switch a lane off (offsets of 0x0fffffff elements; bytes < 2^32)
template <class T>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t raw_buffer(const T* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(base), 0, bytes, 0x00020000);
}
static constexpr uint32_t NO_ENTRY = 0x0fffffffu;  // element offset that is out of range of every such buffer (times 8 < 2^32)

__device__ __forceinline__ double as_double(u32x2 v) { return __hiloint2double((int)v.y, (int)v.x); }

// "did user x rate the item, and where": `word` is word x / 64 of the item's rater bitmap (0 for an absent neighbour: not
// rated), `before` the raters in front of that word.  bitmap_place = x's entry in the item's rater list (raters ascending),
// meaningful only when bitmap_has, and then below the list's length
__device__ __forceinline__ bool bitmap_has(unsigned long long word, uint32_t x) { return (word >> (x & 63u)) & 1ull; }
__device__ __forceinline__ uint32_t bitmap_place(unsigned long long word, uint32_t x, uint32_t before) {
    return before + (uint32_t)__popcll(word & ((1ull << (x & 63u)) - 1ull));
}

// the same on a bitmap in LDS: bits[2 * ibw2] the words, rnk[ibw2] the raters before every SECOND word (an odd word adds the
// popcount of its even neighbour, which comes with the same 16-byte read).  x < 128 * ibw2; place counts from `base`
__device__ __forceinline__ bool lds_pair_probe(const unsigned long long* bits, const uint32_t* rnk, uint32_t x, uint32_t base, uint32_t& place) {
    const uint32_t wi = x >> 6;
    const ulonglong2 pair = *reinterpret_cast<const ulonglong2*>(bits + (wi & ~1u));
    const unsigned long long word = (wi & 1u) ? pair.y : pair.x;
    place = bitmap_place(word, x, base + rnk[wi >> 1] + ((wi & 1u) ? (uint32_t)__popcll(pair.x) : 0u));
    return bitmap_has(word, x);
}

// Order by training file row (the order of ratedI(i) :508-517): rank by counting.  mt[0 .. total) holds the file rows of a wave's
// matches, which are distinct; mt holds a multiple of 64 words >= total.
//   pad_file_rows      fills mt up to a multiple of 4 with 0xffffffff — no file row (there are fewer than 2^32 - 1 ratings), so
//                      it is smaller than no key — and makes the wave's stores to the match buffers visible to all its lanes
//   rank_by_file_row   the whole step for matches compacted into mt / md / ms (and mq with TERMS) [0 .. total), total <= 64 TR:
//                      lane l owns the matches in slots l, l + 64, ...; all keys stream past every lane (LDS broadcast reads, 4
//                      keys per read), which counts for each of its keys the smaller ones — its rank < total — and moves the
//                      match there.  No dependent LDS round trips, unlike a sorting network's 20-40 compare-exchange stages.
//                      mt keeps the slot order
__device__ __forceinline__ void pad_file_rows(uint32_t* mt, int32_t total, int lane) {
    for (int32_t c = total + lane; c < ((total + 3) & ~3); c += 64) mt[c] = 0xffffffffu;
    wave_sync();
}
template <int TR, bool TERMS = false>
__device__ __forceinline__ void rank_by_file_row(uint32_t* mt, uint32_t* mq, double* md, double* ms, int32_t total, int lane) {
    pad_file_rows(mt, total, lane);
    uint32_t key[TR], rank[TR];
    [[maybe_unused]] uint32_t pq[TR];
    double kd[TR], ks[TR];
#pragma unroll
    for (int k = 0; k < TR; ++k) {
        const int32_t slot = 64 * k + lane;
        rank[k] = 0;
        key[k] = 0;  // (a slot past `total` counts nothing and is not written back)
        if constexpr (TERMS) pq[k] = 0;
        kd[k] = 0.0;
        ks[k] = 0.0;
        if (slot < total) {
            key[k] = mt[slot];
            if constexpr (TERMS) pq[k] = mq[slot];
            kd[k] = md[slot];
            ks[k] = ms[slot];
        }
    }
    const int nslot = (total + 63) >> 6;  // wave-uniform
    const uint4* keys4 = reinterpret_cast<const uint4*>(mt);
    for (int32_t c = 0; c < ((total + 3) >> 2); ++c) {
        const uint4 kq = keys4[c];
#pragma unroll
        for (int k = 0; k < TR; ++k) {
            if (k < nslot) rank[k] += (uint32_t)(kq.x < key[k]) + (uint32_t)(kq.y < key[k]) + (uint32_t)(kq.z < key[k]) + (uint32_t)(kq.w < key[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < TR; ++k) {
        if (64 * k + lane < total) {
            if constexpr (TERMS) mq[rank[k]] = pq[k];
            md[rank[k]] = kd[k];
            ms[rank[k]] = ks[k];
        }
    }
    wave_sync();
}

// the left fold of weightedSumDeviation :520-524 over terms 0 .. n) in the order they lie in: every lane folds the same
// sequence (LDS broadcast reads).  These additions, in this order, are what the reference computes
struct NumDen {
    double num, den;
};
__device__ __forceinline__ NumDen fold_terms(const double* md, const double* ms, int32_t n) {
    double num = 0.0, den = 0.0;
    for (int32_t c = 0; c < n; ++c) {
        const double s = ms[c];
        num = num + md[c] * s;
        den = den + fabs(s);
    }
    return {num, den};
}

// One wave, one row (u, i) with rater list [rb, re) = i_ptr[i], i_ptr[i + 1]: the neighbours of u (ids ascending) that rated i,
// in training-file order, in md / ms (deviation, similarity) [0 .. returned count).  TERMS: matches whose similarity is exactly
// 0.0 are dropped (they add +-0.0: identities) and mq gets each match's place in the item's rater list; without TERMS mq is not
// touched (pass nullptr).  u and i are the same in every lane; CAP (a power of two >= 64) >= kcap words in each of mt (16-byte
// aligned) / mq / md / ms, owned by the wave; count <= nbr_cnt[u] <= kcap.
//   probe   the item's rater bitmap + rank prefixes (ib_words > 0): three levels of dependent gathers (neighbour ids -> bitmap
//           words -> the matched ratings), each issued for ALL neighbours at once through buffer descriptors rooted at the wave's
//           own rows, so that the loads are unconditional — a lane without a neighbour, or without a match, uses an out-of-range
//           offset and gets 0 — and the compiler can count them instead of waiting for everything at every use.  Bitmaps not
//           built (they would not fit): a binary search in the item's rater list; all lanes search the SAME array and
//           neighbouring lanes look for neighbouring ids, so the searches share their cache sectors
//   compact ballot / lanes_below into slots 0 .. count) of the buffers
//   order   rank_by_file_row
template <int CAP, bool TERMS>
__device__ __forceinline__ int32_t wave_knn_matches(const ProbeArgs& P, int32_t u, int32_t i, int64_t rb, int64_t re, int lane, uint32_t* mt,
                                                    uint32_t* mq, double* md, double* ms) {
    constexpr int TR = CAP / 64;
    const int32_t cnt = __builtin_amdgcn_readfirstlane(P.nbr_cnt[u]);
    const int64_t base = (int64_t)u * P.kcap;
    int32_t total = 0;
    if (P.ib_words > 0) {
        const int32_t rowlen = __builtin_amdgcn_readfirstlane((int32_t)(re - rb));
        const int32_t ibw = __builtin_amdgcn_readfirstlane((int32_t)P.ib_words);
        const auto r_uidx = raw_buffer(uniform_ptr(P.nbr_idx + base), (uint32_t)cnt * 4u);
        const auto r_usim = raw_buffer(uniform_ptr(P.nbr_sim + base), (uint32_t)cnt * 8u);
        const auto r_bits = raw_buffer(uniform_ptr(P.item_bits + (int64_t)i * P.ib_words), (uint32_t)ibw * 8u);
        const auto r_rank = raw_buffer(uniform_ptr(P.item_rank + (int64_t)i * P.ib_words), (uint32_t)ibw * 4u);
        const auto r_t = raw_buffer(uniform_ptr(P.it_t + rb), (uint32_t)rowlen * 4u);
        const auto r_dev = raw_buffer(uniform_ptr(P.it_dev + rb), (uint32_t)rowlen * 8u);
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
            const uint32_t wi = (64u * k + lane < (uint32_t)cnt) ? (x[k] >> 6) : NO_ENTRY;
            wd[k] = __builtin_amdgcn_raw_buffer_load_b64(r_bits, (int)(wi * 8u), 0, 0);
            rk[k] = __builtin_amdgcn_raw_buffer_load_b32(r_rank, (int)(wi * 4u), 0, 0);
        }
        bool fnd[TR];
#pragma unroll
        for (int k = 0; k < TR; ++k) {  // level 3: the matched ratings (file row, deviation); TERMS: of the non-zero neighbours
            const unsigned long long word = ((unsigned long long)wd[k].y << 32) | wd[k].x;  // (absent neighbour: 0)
            fnd[k] = bitmap_has(word, x[k]) && (!TERMS || as_double(sv[k]) != 0.0);
            qv[k] = fnd[k] ? bitmap_place(word, x[k], rk[k]) : NO_ENTRY;
            mtv[k] = __builtin_amdgcn_raw_buffer_load_b32(r_t, (int)(qv[k] * 4u), 0, 0);
            dv[k] = __builtin_amdgcn_raw_buffer_load_b64(r_dev, (int)(qv[k] * 8u), 0, 0);
        }
#pragma unroll
        for (int k = 0; k < TR; ++k) {
            const unsigned long long hit = __ballot(fnd[k]);
            if (fnd[k]) {
                const int32_t slot = total + lanes_below(hit);
                mt[slot] = mtv[k];
                if constexpr (TERMS) mq[slot] = qv[k];
                md[slot] = as_double(dv[k]);
                ms[slot] = as_double(sv[k]);
            }
            total += __popcll(hit);
        }
    } else {
        for (int32_t j0 = 0; j0 < cnt; j0 += 64) {
            const int32_t j = j0 + lane;
            int64_t lo = rb, hi = rb;
            int32_t x = 0;
            double s = 0.0;
            if (j < cnt) {
                x = P.nbr_idx[base + j];
                s = P.nbr_sim[base + j];
                hi = re;
            }
            while (__any(lo < hi)) {
                if (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (P.it_user[mid] < x) lo = mid + 1;
                    else hi = mid;
                }
            }
            const bool found = j < cnt && (!TERMS || s != 0.0) && lo < re && P.it_user[lo] == x;
            const unsigned long long hit = __ballot(found);
            if (found) {
                const int32_t slot = total + __popcll(hit & ((1ull << lane) - 1ull));  // (= lanes_below(hit))
                // Not a rule: a measured accident of code placement.  With the two v_mbcnt the code in front of k_predict_knn<512,4>'s
                // search loop was 16 bytes shorter, the loop lay in three 64-byte instruction lines instead of two, and the kernel
                // measured 1.2 % slower; any later edit above the loop moves it again and is to be measured, not this line kept.
                mt[slot] = P.it_t[lo];
                if constexpr (TERMS) mq[slot] = (uint32_t)(lo - rb);
                md[slot] = P.it_dev[lo];
                ms[slot] = s;
            }
            total += __popcll(hit);
        }
    }
    rank_by_file_row<TR, TERMS>(mt, mq, md, ms, total, lane);
    return total;
}

}  // namespace knncf
