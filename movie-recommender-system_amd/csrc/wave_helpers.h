// wave_helpers.h — the three wave-level helpers that kernels all over the library use, each defined once.
#pragma once

#include <stdint.h>

namespace knncf {

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

// the set bits of a ballot below this lane: a lane's place among the lanes that voted
__device__ __forceinline__ int32_t lanes_below(unsigned long long mask) {
    return (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

}  // namespace knncf
