// gs_dense.hpp -- the dense grounded-Laplacian machinery shared by the exact effective
// resistance (gs_exact_er.hip) and the algebraic connectivity (gs_topology.hip).
//
// Grounding one node per connected component (row and column of L replaced by the
// identity) leaves M sparse and SPD; N = dense_pad(n) with the padding rows identity
// too.  Units: gs_components.hip (component labels and their statistics), gs_chol.hip
// (the default inverse: blocked Cholesky M = L L^T and W = L^{-1}), gs_xer_ns.hip (the
// other inverse, Newton-Schulz behind GSPARSE_XER_METHOD=ns, with its own read-out),
// gs_exact_er.hip (knobs, grounding, drivers), gs_xer_sparse.hip (the exact effective
// resistance with no dense matrix: a CG batched over the inverse's columns).  A unit
// launches its own kernels only.
#pragma once

#include "gs_internal.hpp"

namespace gs {

static constexpr int kCb = 64;       // block size of the factorisation and its tiles
static constexpr int kGemmPad = 64;  // N is padded to a multiple of this
inline int64_t dense_pad(int64_t n) { return ((n + kGemmPad - 1) / kGemmPad) * kGemmPad; }

// The GSPARSE_XER_* variables as they are now.  xer_knobs() (gs_exact_er.hip) is the only
// reader of the environment in the dense units; gs_exact_er and gs_fiedler call it once
// per call.  A field holds the parsed value, not the text.
struct XerKnobs {
    bool ns = false;     // METHOD is exactly "ns": Newton-Schulz instead of the Cholesky
    int panel = 8;       // PANEL in 1..16 (else 8): block columns per Cholesky panel
    int tile = 64;       // TILE == 128: k_dgemm's 128-wide tiles (taken when N % 128 == 0)
    bool full = false;   // FULL present: Newton-Schulz runs every tile, not the upper triangle
    bool debug = false;  // DEBUG present: Newton-Schulz prints its residual per step
    int batch = 0;       // BATCH > 0: the sparse form's columns per batch (xer_sparse_plan clamps it)
};
XerKnobs xer_knobs();

// The two N x N fp64 matrices both users factor and invert in (shared on purpose: one
// context never runs both at once, and at n = 32768 each is 8.6 GB).
struct DenseScratch {
    double *A, *W;
};
DenseScratch dense_scratch(gs_ctx *c, int64_t N);

// gs_components.hip: component labels of the resident graph (smallest node id per
// component, device buffer); their number and the largest one's size (synchronises)
int32_t *components(gs_ctx *c);
void component_stats(gs_ctx *c, const int32_t *lab, int64_t *count, int64_t *largest);

// gs_chol.hip: W = L^{-1} of M = L L^T for the grounded M (identity rows where flag[u];
// A ends holding L); U = W^T
void grounded_inverse(gs_ctx *c, const XerKnobs &k, int64_t N, const uint8_t *flag, double *A,
                      double *W);
void transpose_square(gs_ctx *c, int64_t N, const double *W, double *U);

// gs_xer_ns.hip: M^{-1} by Newton-Schulz and the scores read off it into device out[nnz];
// returns the index of the last step
int32_t newton_schulz_scores(gs_ctx *c, const XerKnobs &k, int64_t N, const uint8_t *flag,
                             double *out);

// gs_xer_sparse.hip: the columns of the grounded inverse by a batched Jacobi-CG, B columns
// at a time, and the scores read off them into device out[nnz]; flag[n] as
// ground_components gives it.  *batches and *cg_iterations (the columns' iterations summed)
// are written before it throws GS_ENOCONV; out is written only when every batch converged.
static constexpr int64_t kXsBudgetBytes = (int64_t)8 << 30;  // the four n x B fp64 blocks
static constexpr int kXsMaxBatch = 1024;
static constexpr int kXsDefaultBatch = 256;
struct XsPlan {
    int32_t batch = 64;  // B: columns per batch, a multiple of 64
    int64_t budget = 0;  // bytes the four blocks may take (B = 64 is the floor: n <= 4.19 M fits)
    int32_t nb = 1;      // row chunks of the vector passes: a function of n alone
    int64_t chunk = 4;   // rows per chunk
};
// pure host logic: B from n and the device's CU count (cus <= 0: 256); override_b > 0
// replaces the default and is clamped to [64, kXsMaxBatch], a multiple of 64, and the budget
XsPlan xer_sparse_plan(int64_t n, int cus, int override_b);
void xer_sparse_scores(gs_ctx *c, const XerKnobs &k, const uint8_t *flag, double cg_rtol,
                       int32_t cg_max_iter, double *out, int32_t *batches, int64_t *cg_iterations);

}  // namespace gs
