// gs_sp_solve.hpp -- what the Lanczos iterations on the resident weighted CSR share
// (gs_fiedler_sparse.hip: the algebraic connectivity; gs_spectral_bounds.hip: the pencil of
// two Laplacians): the Laplacian apply by row class, the geometry and the folds of the
// vector passes, and the solve of L y = P v by Jacobi-preconditioned CG on the mean-free
// vectors.  The kernels and the host routines are gs_fiedler_sparse.hip's: declared here
// once, defined there once.  The folds are per-element device code, defined here.
//
// Every reduction is two-stage: one partial per workgroup over a fixed contiguous chunk,
// then a fold in a fixed order that every consumer workgroup repeats for itself.  No
// floating-point atomic, so two calls give the same bits.
#pragma once

#include "gs_internal.hpp"

namespace gs {

static constexpr int kSpThreads = 256;
static constexpr int kSpWaves = kSpThreads / 64;
static constexpr int kSpMaxBlocks = 1024;  // partials per reduction (a fold reads them all)
static constexpr int kSpShort = 32;        // rows up to this many entries: one lane each
static constexpr int kSpWide = 512;        // rows above this: workgroups (else one wave each)
static constexpr int kSpSeg = 2048;        // ... one per this many entries of the row
static constexpr int kCgPoll = 8;          // the host reads the residual every this many iterations

// slots of the CG's scalar block (doubles); RZ and RR are ping-pong pairs indexed by the
// iteration's parity, so no launch reads a slot that one of its own workgroups writes
enum { S_RZ = 0, S_RR = 2, S_THRESH = 4, S_RRNOW = 5, S_ITS = 6, S_COUNT = 8 };

// sum over the workgroup, the same value in every thread: shuffles, then the waves' sums
// left to right
__device__ inline double sp_block_sum(double v, double *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < kSpWaves; ++w) s += red[w];
    return s;
}

// the fixed fold of nb <= kSpMaxBlocks partials (every workgroup that needs the total
// folds it itself, in this one order)
__device__ inline double sp_fold(const double *__restrict__ part, int nb, double *red) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += kSpThreads) s += part[i];
    return sp_block_sum(s, red);
}

// Workgroup b owns elements [b chunk, min(n, (b + 1) chunk)) in every vector pass.
struct SpGeom {
    int64_t n, chunk;
    int nb;
};

#define SP_OWN(g)                                                        \
    const int64_t lo = blockIdx.x * (g).chunk;                           \
    const int64_t hi = lo + (g).chunk < (g).n ? lo + (g).chunk : (g).n

// the chunks of n elements: at most kSpMaxBlocks of them, each a multiple of the workgroup
inline SpGeom sp_geometry(int64_t n) {
    SpGeom geo;
    geo.n = n;
    const int64_t nb = std::min<int64_t>(kSpMaxBlocks, (n + kSpThreads - 1) / kSpThreads);
    geo.chunk = ((n + nb - 1) / nb + kSpThreads - 1) / kSpThreads * kSpThreads;
    geo.nb = (int)((n + geo.chunk - 1) / geo.chunk);
    return geo;
}

// L = D - W on the resident CSR's pattern: d the weight per entry (the resident ones, or a
// caller's in the same entry order), deg its weighted degrees over the off-diagonal
// entries; a stored diagonal entry is no part of L.  Rows by length: one lane, one wave,
// or one workgroup per kSpSeg entries (wpart: the segments' sums).
struct SpOp {
    gs_ctx *c;
    hipStream_t st;
    int64_t n;
    const int64_t *ip;
    const int32_t *ix;
    const double *d;
    const int32_t *lwave, *lwide, *wbase, *segrow, *segoff;
    int32_t nwave, nwide, nseg;
    double *deg, *wpart;
    const char *label;  // the profile entry of an apply

    // q = L p; scal / par: the solve whose freeze the launches obey (nullptr: none)
    void apply(const double *p, double *q, const double *scal, int par) const;
    // out = the weighted degrees of d (the DEG form of the same kernels)
    void degrees(double *out) const;
};

// The rows of the resident graph by length, once per call: the lists live in the
// context's fs_* buffers, d is the resident weights, deg and label are the caller's to
// set.  what: the caller's name in the error message.  Synchronises the stream.
SpOp sp_row_classes(gs_ctx *c, const char *what);

// inv[i] = 1 / deg[i] (0 for an isolated node)
void sp_inverse_degrees(const SpOp &op, const double *deg, double *inv);

// the vectors, partials and scalars of one CG solve (n doubles each, 4 nb, S_COUNT)
struct SpCg {
    SpGeom geo;
    const double *inv;  // the Jacobi preconditioner: 1 / deg of the operator
    double *x, *r, *p, *q;
    double *part;       // part3 = part + nb: three rows of partials
    double *scal;
    const char *label;  // the profile entry of the vector passes
};

// x = L^+ P v by CG from x = 0 to ||r|| <= rtol ||P v|| within max_iter iterations.  A
// solve that has met its tolerance freezes itself, so the host polls every kCgPoll
// iterations.  h receives the scalar block (h[S_ITS]: the iterations done, h[S_RRNOW] /
// h[S_THRESH]: the squared residual and its bound); false: stopped at the cap.
bool sp_solve(const SpOp &op, const SpCg &cg, const double *v, double rtol, int32_t max_iter,
              double h[S_COUNT]);

}  // namespace gs
