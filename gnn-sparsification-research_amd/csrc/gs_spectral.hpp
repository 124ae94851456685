// gs_spectral.hpp -- the per-element rules of spectral sparsification by
// effective-resistance sampling (selection.spectral_sample), for the device kernels of
// gs_spectral.hip and, compiled for the host, tools/spectral_host_check.cpp.
//
// The result is defined by NumPy (selection.spectral_sample):
//   inverse = np.unique(min(src, dst) * (n + 1) + max(src, dst), return_inverse=True)[1]
//   first[j] = the lowest column of pair j;  r[j] = scores[first[j]], or 0 for a loop
//              and a score that is NaN, +-inf or <= 0
//   p = r / np.sum(r)                  gs_sample.hpp's blocked pairwise total
//   multinomial:  cdf = cumsum(p) / cumsum(p)[-1]; draw j is double j of the stream,
//                 searched side='right' (gs_sample.hpp's sample_search);
//                 weight = count / fl(q * p)
//   independent:  pair j is kept when double j of the stream is < pk = min(1, fl(q * p));
//                 weight = 1 / pk
// Needs -ffp-contract=off, IEEE fp64 division and fp64 denormals kept.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gs {

enum { kSpectralMultinomial = 0, kSpectralIndependent = 1 };

// the sampling rate of a pair before normalisation: loops, NaN, +-inf, -0.0 and
// everything <= 0 give 0
__host__ __device__ __forceinline__ double spectral_rate(double s, bool loop) {
    return (!loop && s > 0.0 && s < __builtin_inf()) ? s : 0.0;
}

// a pair present in one direction only, or in more than two columns, gives an
// asymmetric weighted graph; loops are never kept, so they do not count
__host__ __device__ __forceinline__ bool spectral_irregular(uint64_t ncols, bool loop) {
    return !loop && ncols != 2;
}

// min(1, fl(q * p)): the keep probability of the independent method
__host__ __device__ __forceinline__ double spectral_keep_prob(double q, double p) {
    const double qp = q * p;
    return qp < 1.0 ? qp : 1.0;  // p is finite and >= 0: no NaN to order
}

// the weight of a pair drawn count times
__host__ __device__ __forceinline__ double spectral_weight(uint32_t count, double q, double p, int method) {
    if (!count) return 0.0;
    return method == kSpectralIndependent ? 1.0 / spectral_keep_prob(q, p) : (double)count / (q * p);
}

}  // namespace gs
