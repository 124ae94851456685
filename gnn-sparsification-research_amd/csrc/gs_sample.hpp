// gs_sample.hpp -- the per-element logic of score-proportional sampling without
// replacement (GraphSparsifier.sparsify_sampled, core.py:333-350), for the device
// kernels of gs_sample.hip and, compiled for the host, tools/sample_host_check.cpp.
//
// The result is defined by NumPy 2.x:
//   s = nan_to_num(scores, nan=1e-8, posinf=1e-8, neginf=1e-8); p = maximum(s, 1e-8)
//   p /= p.sum()                       np.sum of E contiguous doubles: the pairwise sums of
//                                      its 8192-element buffer blocks, folded in order
//   Generator.choice(E, size, replace=False, p=p):
//     while n_uniq < size:
//       x = rng.random(size - n_uniq)  (next_uint64 >> 11) * 2^-53, one uint64 each
//       p[found] = 0
//       cdf = cumsum(p); cdf /= cdf[-1]    sequential adds, IEEE divides
//       new = cdf.searchsorted(x, 'right'); found += the distinct values of new
// Needs -ffp-contract=off, IEEE fp64 division and fp64 denormals kept.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gs_pairwise.hpp"
#include "gs_ziggurat.hpp"

namespace gs {

static constexpr double kSampleFloor = 1e-8;

// maximum(nan_to_num(s), floor): NaN, +-inf, -0.0 and everything below the floor -> floor
__host__ __device__ __forceinline__ double sample_prep(double s) {
    return s > kSampleFloor && s < __builtin_inf() ? s : kSampleFloor;
}

// Generator.random's double of one raw draw
__host__ __device__ __forceinline__ double sample_double(uint64_t u) {
    return (double)(u >> 11) * (1.0 / 9007199254740992.0);
}

// cdf.searchsorted(x, side='right'): the first i with cdf[i] > x (n if none)
__host__ __device__ __forceinline__ int64_t sample_search(const double *cdf, int64_t n, double x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// NumPy's pairwise sum of p[off, off + n), n <= the subtree size of the caller's cut
__host__ __device__ inline double sample_subtree_sum(const double *p, int64_t off, int64_t n) {
    const double *q = p + off;
    auto get = [q](int64_t i) { return q[i]; };
    return pw_tree<double>(n, 128, [&get](int64_t o, int64_t m) { return pw_leaf<double>(o, m, get); });
}

// np.sum of n contiguous doubles: add.reduce hands its inner loop one block of the
// ufunc buffer size (8192 elements, NumPy's default) at a time, so the result is
// ((0 + pw(block 0)) + pw(block 1)) + ... with pw the pairwise tree of gs_pairwise.hpp.
// Every block's tree is cut at `cut` terms; leaf(off, m) gives the pairwise sum of the
// subtree [off, off + m) and is called in ascending offset.
static constexpr int64_t kNumpyBufsize = 8192;
template <class L>
__host__ __device__ inline double sample_total(int64_t n, int64_t cut, L leaf) {
    double tot = 0.0;
    for (int64_t b = 0; b < n; b += kNumpyBufsize) {
        const int64_t nb = n - b < kNumpyBufsize ? n - b : kNumpyBufsize;
        tot = tot + pw_tree<double>(nb, cut, [&leaf, b](int64_t off, int64_t m) { return leaf(b + off, m); });
    }
    return tot;
}

// the degenerate gate: NumPy raises (or takes another branch) on these
__host__ __device__ __forceinline__ bool sample_total_ok(double total) {
    return total > 0.0 && total < __builtin_inf();
}

}  // namespace gs
