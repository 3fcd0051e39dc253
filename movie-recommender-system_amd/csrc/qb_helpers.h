// qb_helpers.h — the device helpers that the query kernels of foldin.hip, bystander.hip and entered.hip share, each defined once.
#pragma once

#include <algorithm>

#include "common.h"

namespace knncf {

static constexpr int ONE_BLOCK = 1024;

// one workgroup: exclusive prefix of cnt(i) over i < m (cnt = popcount of a bitmap word, or a neighbour's row length);
// out[m] = the total, which every thread returns
template <class F>
__device__ int64_t block_exclusive_scan(int64_t m, F cnt, int64_t* __restrict__ out) {
    __shared__ int64_t part[ONE_BLOCK];
    const int t = threadIdx.x;
    const int64_t per = (m + ONE_BLOCK - 1) / ONE_BLOCK;
    const int64_t lo = std::min<int64_t>(m, t * per), hi = std::min<int64_t>(m, lo + per);
    int64_t c = 0;
    for (int64_t i = lo; i < hi; ++i) c += cnt(i);
    part[t] = c;
    __syncthreads();
    for (int off = 1; off < ONE_BLOCK; off <<= 1) {
        const int64_t add = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int64_t run = part[t] - c;
    for (int64_t i = lo; i < hi; ++i) {
        out[i] = run;
        run += cnt(i);
    }
    if (t == ONE_BLOCK - 1) out[m] = part[t];
    return part[ONE_BLOCK - 1];
}

__device__ __forceinline__ int32_t bit_rank(const unsigned long long* bits, const int64_t* rank, int32_t c) {
    const unsigned long long below = bits[c >> 6] & ((1ull << (c & 63)) - 1ull);
    return (int32_t)rank[c >> 6] + __popcll(below);
}

// slot of chunk row j: the last b with qo[b] <= j
__device__ __forceinline__ int32_t qb_slot(const int64_t* __restrict__ qo, int32_t C, int64_t j) {
    int32_t lo = 0, hi = C - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (qo[mid] <= j) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// neighbours a slot returns: (allUsers - u) :608 has U - 1 users for a user of the fit.  self == nullptr: fold-in queries.
__device__ __forceinline__ int32_t qb_take(const int32_t* __restrict__ self, int32_t b, int32_t take, int32_t U) {
    return (self && self[b] >= 0) ? min(take, U - 1) : take;
}

// the order key of a similarity in a neighbour list, as k_fallback_keys of neighbours.hip makes it: ascending key <=> descending
// similarity, -0.0 with +0.0
__device__ __forceinline__ uint64_t by_sim_key(double s) {
    if (s == 0.0) s = 0.0;
    const uint64_t b = (uint64_t)__double_as_longlong(s);
    return ~((b >> 63) ? ~b : (b | 0x8000000000000000ull));
}

}  // namespace knncf
