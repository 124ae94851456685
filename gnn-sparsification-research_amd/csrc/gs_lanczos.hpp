// gs_lanczos.hpp -- what the two forms of the algebraic connectivity share: the dense
// one (gs_topology.hip: Lanczos on the Cholesky inverse, one workgroup per step) and
// the sparse one (gs_fiedler_sparse.hip: Lanczos on preconditioned-CG solves, grid-wide
// steps).  Both build the same tridiagonal T and read its largest eigenvalue the same way
// (gs_tridiag.hpp, which the spectral bounds of gs_spectral_bounds.hip read both ends of).
#pragma once

#include <cmath>

#include "gs_internal.hpp"
#include "gs_tridiag.hpp"

namespace gs {

// gs_fiedler takes the dense form up to this many nodes and the sparse form above
static constexpr int64_t kFiedlerDenseMax = 32768;
// the inner solve of the sparse form when gs_fiedler dispatches to it: relative residual
// ||r|| / ||P v_j|| and the iteration cap of one solve
static constexpr double kFiedlerCgRtol = 1e-10;
static constexpr int32_t kFiedlerCgMaxIter = 5000;

// element i of the fixed pseudo-random start vector, before the mean is removed and the
// norm taken (deterministic)
__device__ inline double lz_start(int64_t i) {
    const uint64_t h = ((uint64_t)i + 1) * 0x9E3779B97F4A7C15ull;
    return (double)(h >> 11) * 0x1p-53 - 0.5;
}

// gs_fiedler_sparse.hip: the sparse form on a symmetric resident graph with n >= 2 and
// max_iter in [2, 500] (the caller has checked both); throws GS_EINVAL for several
// components and GS_ENOCONV at a cap, *value untouched then
void fiedler_sparse(gs_ctx *c, double tol, int32_t max_iter, double cg_rtol, int32_t cg_max_iter,
                    double *value, int32_t *iterations, int64_t *cg_iterations);

}  // namespace gs
