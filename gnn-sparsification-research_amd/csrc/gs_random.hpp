// gs_random.hpp -- the per-element logic of the symmetric random baseline
// (precompute_random_scores / random_sparsify, random.py:14-52), for the device
// kernels of gs_random.hip and, compiled for the host, tools/random_host_check.cpp.
//
// The result is defined by NumPy:
//   keys = minimum(src, dst) * (n + 1) + maximum(src, dst)       random.py:26-28
//   _, inverse = np.unique(keys, return_inverse=True)            random.py:29
//     inverse[i] = the rank of keys[i] among the distinct keys, ascending:
//     (key, column) pairs sorted by key, a head flag where the key changes, the
//     inclusive scan of the flags minus one, scattered back to the columns
//   mask = keep_undir[inverse]                                   random.py:49
//     NumPy's index rule: j in [0, m) as is, j in [-m, 0) wraps to j + m, anything
//     else is an IndexError
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gs {

// the device contract of the id build: both ids in [0, n) (n < 2^31 is the caller's check)
__host__ __device__ __forceinline__ bool undirected_in_range(int64_t s, int64_t d, int64_t n) {
    return s >= 0 && s < n && d >= 0 && d < n;
}

// random.py:26-28; ids in [0, n), n < 2^31: the key is below (n + 1)^2 <= 2^62
__host__ __device__ __forceinline__ uint64_t undirected_key(int64_t s, int64_t d, int64_t n) {
    const uint64_t u = (uint64_t)(s < d ? s : d), v = (uint64_t)(s < d ? d : s);
    return u * (uint64_t)(n + 1) + v;
}

// 1 where sorted position i starts a run of equal keys
__host__ __device__ __forceinline__ int64_t undirected_head(const uint64_t *keys, int64_t i) {
    return (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

// rank of sorted position i from the exclusive scan of the head flags
__host__ __device__ __forceinline__ int64_t undirected_rank(int64_t before, int64_t head) {
    return before + head - 1;
}

// NumPy's index rule for an axis of m entries: the entry read, or -1 (IndexError)
__host__ __device__ __forceinline__ int64_t wrap_index(int64_t j, int64_t m) {
    if (j >= 0) return j < m ? j : -1;
    return j >= -m ? j + m : -1;
}

}  // namespace gs
