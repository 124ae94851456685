// gs_forest.hpp -- the per-element rules of the maximum spanning forest
// (gs_spanning_forest), for the device kernels of gs_forest.hip and, compiled for the
// host, tools/forest_host_check.cpp.
//
// The order: column i is better than column j when (order_key(score), index) is
// lexicographically larger (keep_lowest: smaller) -- gs_topk_mask's stable rule, a
// strict total order.  One stable radix sort of (key, column) by key puts the columns
// in ascending (key, index) order; a column's *rank* counts the columns better than it
// (0 = the best), so rank r sits at sorted position E - 1 - r (keep_lowest: r).
//
// A Boruvka round: every component takes the smallest rank among its crossing columns
// (integer atomicMin, the index is part of the rank); its root hooks onto the other
// side's root.  Under a strict total order the only cycles among the picks are pairs
// of components that picked the same column: there the smaller root hooks and the
// larger stays, so the column is counted once and the hooks form a forest.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gs_keys.hpp"

namespace gs {

// both ids in [0, n) (n < 2^31 is the caller's check)
__host__ __device__ __forceinline__ bool forest_in_range(int64_t s, int64_t d, int64_t n) {
    return s >= 0 && s < n && d >= 0 && d < n;
}

// the strict total order itself (the sort realises it; the host check compares the two)
__host__ __device__ __forceinline__ bool forest_better(double si, int64_t i, double sj, int64_t j,
                                                       int keep_lowest) {
    const uint64_t ki = order_key(si), kj = order_key(sj);
    if (ki != kj) return keep_lowest ? ki < kj : ki > kj;
    return keep_lowest ? i < j : i > j;
}

// rank <-> sorted position (ascending (key, index)); its own inverse
__host__ __device__ __forceinline__ int64_t forest_flip(int64_t x, int64_t E, int keep_lowest) {
    return keep_lowest ? x : E - 1 - x;
}

// a column takes part in a round while its ends lie in different components
// (a self-loop never does)
__host__ __device__ __forceinline__ bool forest_crossing(int32_t la, int32_t lb) { return la != lb; }

// the root on the far side of root a's pick, whose ends carry the labels la and lb
__host__ __device__ __forceinline__ int32_t forest_other(int32_t a, int32_t la, int32_t lb) {
    return la == a ? lb : la;
}

// root a hooks onto `other` unless both picked the same column and a is the larger
__host__ __device__ __forceinline__ bool forest_hooks(int32_t a, int32_t other, bool mutual) {
    return !(mutual && a > other);
}

}  // namespace gs
