// gs_xer_sparse.hip -- exact effective resistance without a dense matrix: the columns of
// the grounded inverse G = M^{-1} (gs_exact_er.hip, header comment) by a Jacobi-
// preconditioned CG that runs B columns at a time.
//
// M is L = D - W (off-diagonal entries; stored diagonal entries dropped) with the rows
// and columns of the grounded nodes (ground_components: one per component, so every
// isolated node too) replaced by the identity.  For every other node u the column
// g_u solves M g_u = e_u; its grounded rows are zero and stay zero, so the solve runs
// on the ungrounded rows alone, where M is SPD.  R(u,v) = (G_uu + G_vv) - 2 G_uv needs
// G_uu and, per CSR entry (u,v) with u < v, G_vu: both are read from the column of u when
// its batch has converged, and no n x n array ever exists.
//
// Layout: X, R, P, Q are row-major n x B, B a multiple of 64; the 64 lanes of a wave are
// 64 consecutive columns of one row.  A column has its own alpha, beta, residual and
// stopping test (this is not block-CG); one that has met ||r|| <= cg_rtol ||r_0|| freezes
// (its lanes store nothing more) while the batch goes on.
//
// Nothing here is a persistent kernel: an iteration is a chain of plain
// launches on the context's stream -- the apply, p . q, the x / r update, the p update --
// and every dot is two-stage: a lane sums its own column over the rows of its wave, a
// workgroup writes one partial per column over a fixed row chunk, and every consumer
// workgroup folds the partials in one fixed order (xs_fold).  The chunks depend on n
// alone, and a (row, column) sum walks the row's entries in CSR order, so a column's
// bits depend neither on B nor on where it sits in its batch, and there is no
// floating-point atomic.  The per-column scalars are ping-pong pairs by the iteration's
// parity, as gs_fiedler_sparse.hip's.
//
// The row classification and degree kernels are this unit's own, not shared with
// gs_fiedler_sparse.hip: the classes differ (a wave walks a row here, so there is no
// one-lane class and the segment length is another), and moving that unit's kernels
// into a header would change its generated code ("The unit split").
#include <cmath>
#include <cstdlib>

#include "gs_dense.hpp"

namespace gs {

static constexpr int kXsThreads = 256;
static constexpr int kXsWaves = kXsThreads / 64;
static constexpr int kXsMaxBlocks = 128;  // row chunks, i.e. partials per column and dot
static constexpr int kXsSeg = 256;        // rows above this many entries: one wave per this many
static constexpr int kXsPoll = 4;         // the host reads the open-column count every this many iterations

// ------------------------------------------------------------------ the batch plan
XsPlan xer_sparse_plan(int64_t n, int cus, int override_b) {
    XsPlan p;
    p.budget = kXsBudgetBytes;
    if (n < 1) n = 1;
    if (cus < 1) cus = 256;
    // the widest B whose four blocks fit the budget, never below one wave of columns
    int64_t cap = p.budget / (4 * 8 * n) / 64 * 64;
    cap = std::max<int64_t>(64, std::min<int64_t>(cap, kXsMaxBatch));
    int64_t b;
    if (override_b > 0) {
        b = std::max<int64_t>(64, std::min<int64_t>(override_b, kXsMaxBatch)) / 64 * 64;
    } else {
        // the apply runs n B / 64 waves: at least eight per CU, and no more columns than
        // the graph has nodes
        const int64_t fill = ((int64_t)cus * 8 + n - 1) / n * 64;
        b = std::max<int64_t>(kXsDefaultBatch, fill);
        b = std::min<int64_t>(b, (n + 63) / 64 * 64);
    }
    p.batch = (int32_t)std::min<int64_t>(b, cap);
    p.chunk = ((n + kXsMaxBlocks - 1) / kXsMaxBlocks + kXsWaves - 1) / kXsWaves * kXsWaves;
    p.nb = (int32_t)((n + p.chunk - 1) / p.chunk);
    return p;
}

// ------------------------------------------------------------------ device helpers
// the wave's index in its workgroup, as a scalar: what is indexed by it (row pointers,
// column indices, weights) is then loaded by the scalar unit
__device__ __forceinline__ int xs_wave() {
    return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

struct XsScal {
    double *rz, *rr;  // [2][B] by parity
    double *thresh;   // [B]
    int32_t *its;     // [B] iterations the column took
    int32_t *open;    // [B / 64] columns of the group still open after the last p update
};

__device__ __forceinline__ bool xs_frozen(const XsScal &s, int B, int par, int col) {
    return s.rr[par * B + col] <= s.thresh[col];
}

// every column of the workgroup's group is frozen (the same answer in all its waves)
__device__ __forceinline__ bool xs_group_done(const XsScal &s, int B, int par, int col) {
    return __ballot(!xs_frozen(s, B, par, col)) == 0ull;
}

// the workgroup's sum per column: the waves' values left to right
__device__ __forceinline__ double xs_block_sum(double v, double (*red)[64]) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    red[w][lane] = v;
    __syncthreads();
    double s = red[0][lane];
    for (int k = 1; k < kXsWaves; ++k) s += red[k][lane];
    return s;
}

// the fixed fold of a column's nb partials (every workgroup that needs the total folds it
// itself, in this one order): wave w takes chunks w, w + 4, ..., then the waves left to right
__device__ __forceinline__ double xs_fold(const double *__restrict__ part, int nb, int B, int col,
                                          double (*red)[64]) {
    double s = 0.0;
    for (int b = threadIdx.x >> 6; b < nb; b += kXsWaves) s += part[(int64_t)b * B + col];
    return xs_block_sum(s, red);
}

struct XsGeom {
    int64_t n, chunk;
    int nb, B;
};

#define XS_OWN(g)                                                                  \
    const int lane = threadIdx.x & 63, wv = xs_wave();                             \
    const int col = blockIdx.y * 64 + lane;                                        \
    (void)lane;                                                                    \
    const int64_t lo = blockIdx.x * (g).chunk;                                     \
    const int64_t hi = lo + (g).chunk < (g).n ? lo + (g).chunk : (g).n

// ------------------------------------------------------------------ set-up, once per call
// deg[i] = the sum of row i's off-diagonal weights, inv[i] = 1 / deg[i] (0 on a grounded
// row), wm[e] = the weight M applies for entry e: 0 on the diagonal, in a grounded row and
// for a grounded neighbour.  One wave per row.
__global__ void __launch_bounds__(kXsThreads)
k_xs_rows(int64_t n, const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
          const double *__restrict__ d, const uint8_t *__restrict__ flag, double *__restrict__ deg,
          double *__restrict__ inv, double *__restrict__ wm) {
    const int64_t i = blockIdx.x * (int64_t)kXsWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const bool fi = flag[i];
    double s = 0.0;
    for (int64_t e = ip[i] + lane; e < ip[i + 1]; e += 64) {
        const int32_t k = ix[e];
        const bool edge = k != i;
        if (edge) s += d[e];
        wm[e] = edge && !fi && !flag[k] ? d[e] : 0.0;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) {
        deg[i] = s;
        inv[i] = !fi && s > 0.0 ? 1.0 / s : 0.0;
    }
}

// rows of more than kXsSeg entries: their segments are consecutive in the segment table
// from wbase on.  cnt: wide rows, segments.
__global__ void k_xs_classify(int64_t n, const int64_t *__restrict__ ip, int32_t *__restrict__ cnt,
                              int32_t *__restrict__ lwide, int32_t *__restrict__ wbase,
                              int32_t *__restrict__ segrow, int32_t *__restrict__ segoff) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t len = ip[i + 1] - ip[i];
        if (len <= kXsSeg) continue;
        const int32_t ns = (int32_t)((len + kXsSeg - 1) / kXsSeg);
        const int32_t slot = atomicAdd(&cnt[0], 1), base = atomicAdd(&cnt[1], ns);
        lwide[slot] = (int32_t)i;
        wbase[slot] = base;
        for (int32_t t = 0; t < ns; ++t) {
            segrow[base + t] = (int32_t)i;
            segoff[base + t] = t;
        }
    }
}

// ------------------------------------------------------------------ Q = M P
// sum over entries [e0, e1) of one row of wm[e] P[ix[e], col]: e is wave-uniform, so the
// index and the weight are scalar loads and P's row is one coalesced 512-byte read
__device__ __forceinline__ double xs_walk(int64_t e0, int64_t e1, const int32_t *__restrict__ ix,
                                          const double *__restrict__ wm,
                                          const double *__restrict__ p, int B, int col) {
    double s = 0.0;
#pragma unroll 4
    for (int64_t e = e0; e < e1; ++e) s += wm[e] * p[(int64_t)ix[e] * B + col];
    return s;
}

// a wave owns (row, 64-column group); rows of more than kXsSeg entries are k_xs_seg's
__global__ void __launch_bounds__(kXsThreads)
k_xs_apply(int64_t n, int B, const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
           const double *__restrict__ wm, const double *__restrict__ deg,
           const uint8_t *__restrict__ flag, const double *__restrict__ p, double *__restrict__ q,
           XsScal sc, int par) {
    const int lane = threadIdx.x & 63;
    const int col = blockIdx.y * 64 + lane;
    if (xs_group_done(sc, B, par, col)) return;
    const int64_t i = blockIdx.x * (int64_t)kXsWaves + xs_wave();
    if (i >= n) return;
    const int64_t e0 = ip[i], e1 = ip[i + 1];
    if (e1 - e0 > kXsSeg) return;
    double out = 0.0;  // a grounded row of Q is zero, as P's
    if (!flag[i]) {
        const double s = xs_walk(e0, e1, ix, wm, p, B, col);
        out = deg[i] * p[i * B + col] - s;
    }
    q[i * B + col] = out;
}

// one segment of a wide row: wpart[segment, col] = the sum of its terms
__global__ void __launch_bounds__(kXsThreads)
k_xs_seg(int32_t nseg, int B, const int32_t *__restrict__ segrow, const int32_t *__restrict__ segoff,
         const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
         const double *__restrict__ wm, const double *__restrict__ p, double *__restrict__ wpart,
         XsScal sc, int par) {
    const int lane = threadIdx.x & 63;
    const int col = blockIdx.y * 64 + lane;
    if (xs_group_done(sc, B, par, col)) return;
    const int64_t s = blockIdx.x * (int64_t)kXsWaves + xs_wave();
    if (s >= nseg) return;
    const int64_t i = segrow[s];
    const int64_t e0 = ip[i] + (int64_t)segoff[s] * kXsSeg;
    const int64_t e1 = e0 + kXsSeg < ip[i + 1] ? e0 + kXsSeg : ip[i + 1];
    wpart[s * B + col] = xs_walk(e0, e1, ix, wm, p, B, col);
}

// a wide row's segments, left to right: a wave per (wide row, group)
__global__ void __launch_bounds__(kXsThreads)
k_xs_wide(int32_t nwide, int B, const int32_t *__restrict__ lwide, const int32_t *__restrict__ wbase,
          const int64_t *__restrict__ ip, const double *__restrict__ wpart,
          const double *__restrict__ deg, const uint8_t *__restrict__ flag,
          const double *__restrict__ p, double *__restrict__ q, XsScal sc, int par) {
    const int lane = threadIdx.x & 63;
    const int col = blockIdx.y * 64 + lane;
    if (xs_group_done(sc, B, par, col)) return;
    const int64_t slot = blockIdx.x * (int64_t)kXsWaves + xs_wave();
    if (slot >= nwide) return;
    const int64_t i = lwide[slot], base = wbase[slot];
    const int64_t ns = (ip[i + 1] - ip[i] + kXsSeg - 1) / kXsSeg;
    double out = 0.0;
    if (!flag[i]) {
        double s = 0.0;
        for (int64_t t = 0; t < ns; ++t) s += wpart[(base + t) * B + col];
        out = deg[i] * p[i * B + col] - s;
    }
    q[i * B + col] = out;
}

// ------------------------------------------------------------------ vector passes
// Workgroup (b, g) owns rows [b chunk, min(n, (b + 1) chunk)) of column group g; its wave w
// takes rows lo + w, lo + w + 4, ...
//
// A batch's start: column j is node cols[c0 + j] (none past ncols: such a column is
// frozen from the start); x = 0, r = e_u, p = z = r / D.
__global__ void __launch_bounds__(kXsThreads)
k_xs_init(XsGeom g, const int32_t *__restrict__ cols, int64_t c0, int64_t ncols,
          const double *__restrict__ inv, double *__restrict__ x, double *__restrict__ r,
          double *__restrict__ p, XsScal sc, double rtol) {
    XS_OWN(g);
    const int64_t u = c0 + col < ncols ? cols[c0 + col] : -1;
    for (int64_t i = lo + wv; i < hi; i += kXsWaves) {
        const double ri = i == u ? 1.0 : 0.0;
        x[i * g.B + col] = 0.0;
        r[i * g.B + col] = ri;
        p[i * g.B + col] = ri * inv[i];
    }
    if (blockIdx.x == 0 && wv == 0) {
        sc.rz[col] = u >= 0 ? inv[u] : 0.0;
        sc.rr[col] = u >= 0 ? 1.0 : 0.0;
        sc.thresh[col] = u >= 0 ? rtol * rtol : 0.0;
        sc.its[col] = 0;
        const unsigned long long open = __ballot(u >= 0);
        if (lane == 0) sc.open[blockIdx.y] = __popcll(open);
    }
}

// part[b, col] = p . q over the chunk
__global__ void __launch_bounds__(kXsThreads)
k_xs_dot(XsGeom g, const double *__restrict__ p, const double *__restrict__ q,
         double *__restrict__ part, XsScal sc, int par) {
    __shared__ double red[kXsWaves][64];
    XS_OWN(g);
    if (xs_group_done(sc, g.B, par, col)) return;
    double s = 0.0;
#pragma unroll 4
    for (int64_t i = lo + wv; i < hi; i += kXsWaves) s += p[i * g.B + col] * q[i * g.B + col];
    s = xs_block_sum(s, red);
    if (wv == 0) part[(int64_t)blockIdx.x * g.B + col] = s;
}

// alpha = (r . z) / (p . q) from the fold of pin; x += alpha p, r -= alpha q, and the
// chunk's ||r||^2 and r . z (z = r / D, not stored).  pout: two planes of nb x B partials.
__global__ void __launch_bounds__(kXsThreads)
k_xs_xr(XsGeom g, const double *__restrict__ p, const double *__restrict__ q,
        const double *__restrict__ inv, double *__restrict__ x, double *__restrict__ r,
        const double *__restrict__ pin, double *__restrict__ pout, XsScal sc, int par) {
    __shared__ double red[kXsWaves][64];
    XS_OWN(g);
    if (xs_group_done(sc, g.B, par, col)) return;
    const bool live = !xs_frozen(sc, g.B, par, col);
    const double pq = xs_fold(pin, g.nb, g.B, col, red);
    const double a = pq > 0.0 ? sc.rz[par * g.B + col] / pq : 0.0;  // p . q = 0 only for p = 0
    double rr = 0.0, rz = 0.0;
    if (live) {
#pragma unroll 2
        for (int64_t i = lo + wv; i < hi; i += kXsWaves) {
            const int64_t k = i * g.B + col;
            x[k] = x[k] + a * p[k];
            const double ri = r[k] - a * q[k];
            r[k] = ri;
            const double zi = ri * inv[i];
            rr += ri * ri;
            rz += ri * zi;
        }
    }
    rr = xs_block_sum(rr, red);
    rz = xs_block_sum(rz, red);
    if (wv == 0) {
        pout[(int64_t)blockIdx.x * g.B + col] = rr;
        pout[((int64_t)g.nb + blockIdx.x) * g.B + col] = rz;
    }
}

// beta = (r . z) / (r . z)_previous; p = z + beta p.  Workgroup (0, g) publishes the folded
// scalars for the next parity, counts the iteration and the columns still open; a frozen
// column only carries its scalars over.
__global__ void __launch_bounds__(kXsThreads)
k_xs_p(XsGeom g, const double *__restrict__ r, const double *__restrict__ inv,
       double *__restrict__ p, const double *__restrict__ pin, XsScal sc, int par) {
    __shared__ double red[kXsWaves][64];
    XS_OWN(g);
    if (xs_group_done(sc, g.B, par, col)) {
        if (blockIdx.x == 0 && wv == 0) {
            sc.rr[(par ^ 1) * g.B + col] = sc.rr[par * g.B + col];
            sc.rz[(par ^ 1) * g.B + col] = sc.rz[par * g.B + col];
            if (lane == 0) sc.open[blockIdx.y] = 0;
        }
        return;
    }
    const bool live = !xs_frozen(sc, g.B, par, col);
    const double rr = xs_fold(pin, g.nb, g.B, col, red);
    const double rz = xs_fold(pin + (int64_t)g.nb * g.B, g.nb, g.B, col, red);
    const double old = sc.rz[par * g.B + col];
    const double beta = old > 0.0 ? rz / old : 0.0;
    if (live) {
#pragma unroll 2
        for (int64_t i = lo + wv; i < hi; i += kXsWaves) {
            const int64_t k = i * g.B + col;
            p[k] = r[k] * inv[i] + beta * p[k];
        }
    }
    if (blockIdx.x == 0 && wv == 0) {
        const double nrr = live ? rr : sc.rr[par * g.B + col];
        sc.rr[(par ^ 1) * g.B + col] = nrr;
        sc.rz[(par ^ 1) * g.B + col] = live ? rz : old;
        if (live) sc.its[col] = sc.its[col] + 1;
        const unsigned long long open = __ballot(nrr > sc.thresh[col]);
        if (lane == 0) sc.open[blockIdx.y] = __popcll(open);
    }
}

// ------------------------------------------------------------------ read-out
// a converged batch: workgroup j reads column j (node u): G_uu, and G_vu for every entry
// (u, v) of row u with u < v
__global__ void __launch_bounds__(kXsThreads)
k_xs_read(int B, const int32_t *__restrict__ cols, int64_t c0, const int64_t *__restrict__ ip,
          const int32_t *__restrict__ ix, const double *__restrict__ x, double *__restrict__ diag,
          double *__restrict__ guv) {
    const int64_t j = blockIdx.x, u = cols[c0 + j];
    if (threadIdx.x == 0) diag[u] = x[u * B + j];
    for (int64_t e = ip[u] + threadIdx.x; e < ip[u + 1]; e += kXsThreads) {
        const int64_t v = ix[e];
        if (v > u) guv[e] = x[v * B + j];
    }
}

// R per CSR entry; (v, u) takes the value of (u, v), u < v, through the transpose positions
__global__ void k_xs_scores(int64_t nnz, const int32_t *__restrict__ rows,
                            const int32_t *__restrict__ ix, const int64_t *__restrict__ tpos,
                            const double *__restrict__ diag, const double *__restrict__ guv,
                            double *__restrict__ out) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t u = rows[e], v = ix[e];
        const double a = u < v ? diag[u] : diag[v], b = u < v ? diag[v] : diag[u];
        const double g = u == v ? diag[u] : guv[u < v ? e : tpos[e]];
        const double r = (a + b) - 2.0 * g;
        out[e] = r > 1e-10 ? r : 1e-10;
    }
}

// ------------------------------------------------------------------ driver
void xer_sparse_scores(gs_ctx *c, const XerKnobs &kn, const uint8_t *flag, double cg_rtol,
                       int32_t cg_max_iter, double *out, int32_t *batches, int64_t *cg_iterations) {
    Graph &g = c->g;
    hipStream_t st = c->stream;
    const int64_t n = g.n, nnz = g.nnz;
    const int64_t *ip = g.indptr.as<int64_t>();
    const int32_t *ix = g.indices.as<int32_t>();
    if (batches) *batches = 0;
    if (cg_iterations) *cg_iterations = 0;
    if (!nnz) return;

    int cus = 0;
    GS_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    const XsPlan plan = xer_sparse_plan(n, cus, kn.batch);
    const int B = plan.batch, G = B / 64;
    const XsGeom geo{n, plan.chunk, plan.nb, B};

    // the columns: every node that is not grounded, ascending
    std::vector<uint8_t> hflag((size_t)n);
    GS_HIP(hipMemcpyAsync(hflag.data(), flag, (size_t)n, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    std::vector<int32_t> hcols;
    hcols.reserve((size_t)n);
    for (int64_t u = 0; u < n; ++u)
        if (!hflag[(size_t)u]) hcols.push_back((int32_t)u);
    const int64_t ncols = (int64_t)hcols.size();
    int32_t *cols = (int32_t *)c->buf("xs_cols").ensure(sizeof(int32_t) * (size_t)std::max<int64_t>(ncols, 1));
    if (ncols)
        GS_HIP(hipMemcpyAsync(cols, hcols.data(), sizeof(int32_t) * (size_t)ncols,
                              hipMemcpyHostToDevice, st));

    // degrees, masked weights, wide rows: once per call (a wide row has more than kXsSeg
    // entries and at most len / kXsSeg + 1 segments)
    const size_t wcap = (size_t)(nnz / kXsSeg + 1), scap = (size_t)(nnz / kXsSeg + 1) + wcap;
    double *vec = (double *)c->buf("xs_vec").ensure(sizeof(double) * 3 * (size_t)n);
    double *deg = vec, *inv = vec + n, *diag = vec + 2 * n;
    double *wm = (double *)c->buf("xs_wm").ensure(sizeof(double) * (size_t)nnz);
    double *guv = (double *)c->buf("xs_guv").ensure(sizeof(double) * (size_t)nnz);
    int32_t *cnt = (int32_t *)c->buf("xs_cnt").ensure(sizeof(int32_t) * 2);
    int32_t *lwide = (int32_t *)c->buf("xs_lwide").ensure(sizeof(int32_t) * 2 * wcap);
    int32_t *wbase = lwide + wcap;
    int32_t *segrow = (int32_t *)c->buf("xs_seg").ensure(sizeof(int32_t) * 2 * scap);
    int32_t *segoff = segrow + scap;
    GS_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * 2, st));
    GS_HIP(hipMemsetAsync(diag, 0, sizeof(double) * (size_t)n, st));
    GS_HIP(hipMemsetAsync(guv, 0, sizeof(double) * (size_t)nnz, st));
    k_xs_rows<<<(unsigned)((n + kXsWaves - 1) / kXsWaves), kXsThreads, 0, st>>>(
        n, ip, ix, g.data.as<double>(), flag, deg, inv, wm);
    k_xs_classify<<<grid_for(n, kXsThreads, 1 << 16), kXsThreads, 0, st>>>(n, ip, cnt, lwide, wbase,
                                                                          segrow, segoff);
    GS_HIP(hipGetLastError());
    int32_t hcnt[2] = {0, 0};
    GS_HIP(hipMemcpyAsync(hcnt, cnt, sizeof(hcnt), hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));  // also: hcols has been uploaded
    GS_CHECK((size_t)hcnt[0] <= wcap && (size_t)hcnt[1] <= scap, GS_EHIP,
             "exact effective resistance: the wide-row tables overflowed");
    const int32_t nwide = hcnt[0], nseg = hcnt[1];

    // the four blocks, the partials (one plane for p . q, two for ||r||^2 and r . z), the
    // wide rows' segment sums, the per-column scalars
    const size_t blk = (size_t)n * (size_t)B;
    double *blocks = (double *)c->buf("xs_blocks").ensure(sizeof(double) * 4 * blk);
    double *X = blocks, *R = blocks + blk, *P = blocks + 2 * blk, *Q = blocks + 3 * blk;
    double *part = (double *)c->buf("xs_part").ensure(sizeof(double) * 3 * (size_t)plan.nb * B);
    double *part2 = part + (size_t)plan.nb * B;
    double *wpart = (double *)c->buf("xs_wpart").ensure(sizeof(double) * (size_t)std::max(nseg, 1) * B);
    double *sd = (double *)c->buf("xs_scal").ensure(sizeof(double) * 5 * (size_t)B +
                                                    sizeof(int32_t) * ((size_t)B + (size_t)G));
    XsScal sc;
    sc.rz = sd;
    sc.rr = sd + 2 * B;
    sc.thresh = sd + 4 * B;
    sc.its = (int32_t *)(sd + 5 * B);
    sc.open = sc.its + B;

    const dim3 vgrid((unsigned)plan.nb, (unsigned)G);
    const dim3 agrid((unsigned)((n + kXsWaves - 1) / kXsWaves), (unsigned)G);
    const dim3 sgrid((unsigned)((nseg + kXsWaves - 1) / kXsWaves), (unsigned)G);
    const dim3 wgrid((unsigned)((nwide + kXsWaves - 1) / kXsWaves), (unsigned)G);
    std::vector<int32_t> hopen((size_t)G), hits((size_t)B);
    int64_t cg_total = 0;
    int32_t nbatch = 0;
    for (int64_t c0 = 0; c0 < ncols; c0 += B, ++nbatch) {
        const int64_t ncb = std::min<int64_t>(B, ncols - c0);
        k_xs_init<<<vgrid, kXsThreads, 0, st>>>(geo, cols, c0, ncols, inv, X, R, P, sc, cg_rtol);
        GS_HIP(hipGetLastError());
        int64_t open = ncb;
        int32_t it = 0;
        while (it < cg_max_iter && open) {
            const int32_t stop = (int32_t)std::min<int64_t>(cg_max_iter, (int64_t)it + kXsPoll);
            for (; it < stop; ++it) {
                const int par = it & 1;
                hipEvent_t e = prof_begin(c);
                k_xs_apply<<<agrid, kXsThreads, 0, st>>>(n, B, ip, ix, wm, deg, flag, P, Q, sc, par);
                if (nwide) {
                    k_xs_seg<<<sgrid, kXsThreads, 0, st>>>(nseg, B, segrow, segoff, ip, ix, wm, P,
                                                          wpart, sc, par);
                    k_xs_wide<<<wgrid, kXsThreads, 0, st>>>(nwide, B, lwide, wbase, ip, wpart, deg,
                                                           flag, P, Q, sc, par);
                }
                prof_end(c, e, "xer_sparse_apply", 0.0);
                e = prof_begin(c);
                k_xs_dot<<<vgrid, kXsThreads, 0, st>>>(geo, P, Q, part, sc, par);
                k_xs_xr<<<vgrid, kXsThreads, 0, st>>>(geo, P, Q, inv, X, R, part, part2, sc, par);
                k_xs_p<<<vgrid, kXsThreads, 0, st>>>(geo, R, inv, P, part2, sc, par);
                prof_end(c, e, "xer_sparse_vector", 0.0);
            }
            GS_HIP(hipGetLastError());
            GS_HIP(hipMemcpyAsync(hopen.data(), sc.open, sizeof(int32_t) * (size_t)G,
                                  hipMemcpyDeviceToHost, st));
            GS_HIP(hipStreamSynchronize(st));
            open = 0;
            for (int32_t v : hopen) open += v;
        }
        GS_HIP(hipMemcpyAsync(hits.data(), sc.its, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost,
                              st));
        GS_HIP(hipStreamSynchronize(st));
        for (int32_t v : hits) cg_total += v;
        if (batches) *batches = nbatch + (open ? 0 : 1);
        if (cg_iterations) *cg_iterations = cg_total;
        if (open) {
            // the worst column: its residual is the parity's that the next iteration would read
            std::vector<double> hs(5 * (size_t)B);
            GS_HIP(hipMemcpy(hs.data(), sd, sizeof(double) * hs.size(), hipMemcpyDeviceToHost));
            const double *rr = hs.data() + 2 * B + (size_t)(it & 1) * B;
            double worst = 0.0;
            for (int64_t j = 0; j < ncb; ++j) worst = std::max(worst, rr[j]);  // ||r_0|| = 1
            GS_CHECK(false, GS_ENOCONV,
                     "exact effective resistance: batch %d (columns %lld to %lld of %lld) stopped "
                     "at cg_max_iter=%d with %lld columns open, worst relative residual %.3e > "
                     "cg_rtol=%.3e (%lld CG iterations in all)",
                     (int)nbatch, (long long)c0, (long long)(c0 + ncb), (long long)ncols,
                     (int)cg_max_iter, (long long)open, sqrt(worst), cg_rtol, (long long)cg_total);
        }
        hipEvent_t e = prof_begin(c);
        k_xs_read<<<(unsigned)ncb, kXsThreads, 0, st>>>(B, cols, c0, ip, ix, X, diag, guv);
        prof_end(c, e, "xer_sparse_read", 0.0);
        GS_HIP(hipGetLastError());
    }
    k_xs_scores<<<grid_for(nnz, kXsThreads, 1 << 16), kXsThreads, 0, st>>>(
        nnz, g.rows.as<int32_t>(), ix, g.tpos.as<int64_t>(), diag, guv, out);
    GS_HIP(hipGetLastError());
}

}  // namespace gs

using namespace gs;

extern "C" int gs_xer_sparse_plan(int64_t n, int32_t cus, int64_t out[4]) {
    return guard([&] {
        GS_CHECK(out, GS_EINVAL, "null output");
        GS_CHECK(n >= 0, GS_EINVAL, "n >= 0");
        const XsPlan p = xer_sparse_plan(n, cus, xer_knobs().batch);
        out[0] = p.batch;
        out[1] = p.budget;
        out[2] = p.nb;
        out[3] = p.chunk;
    });
}
