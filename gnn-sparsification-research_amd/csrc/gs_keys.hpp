// gs_keys.hpp -- the order-preserving 64-bit key of an fp64 score, shared by the
// global radix select (gs_topk.hip), the segmented one (gs_segtopk.hip) and the
// spanning forest's ranking (gs_forest.hip; its host check compiles this for the CPU):
// key(a) < key(b) iff np.sort puts a before b; -0.0 == +0.0; every NaN is the one
// largest key ~0 (no other double maps to it).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gs {

__host__ __device__ __forceinline__ uint64_t order_key(double x) {
    if (x != x) return ~0ull;
    if (x == 0.0) x = 0.0;  // -0.0 -> +0.0
    uint64_t b = __builtin_bit_cast(uint64_t, x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

}  // namespace gs
