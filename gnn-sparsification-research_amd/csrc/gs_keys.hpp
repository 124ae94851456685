// gs_keys.hpp -- the order-preserving 64-bit key of an fp64 score, shared by the
// global radix select (gs_topk.hip) and the segmented one (gs_segtopk.hip):
// key(a) < key(b) iff np.sort puts a before b; -0.0 == +0.0; every NaN is the one
// largest key ~0 (no other double maps to it).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gs {

__device__ __forceinline__ uint64_t order_key(double x) {
    if (x != x) return ~0ull;
    if (x == 0.0) x = 0.0;  // -0.0 -> +0.0
    uint64_t b = (uint64_t)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

}  // namespace gs
