// gs_exact_er.hip -- exact effective resistance (calculate_effective_resistance_scores,
// metrics.py:124-175) on the device, fp64 MFMA.
//
// The reference takes the dense pseudo-inverse of L + 1e-10 I by SVD and reads
// R(u,v) = P_uu + P_vv - 2 P_uv.  Within a connected component that is the
// effective resistance, which grounding one node g per component computes
// exactly: with M = L with row/column g replaced by the identity (SPD, sparse)
// and G = M^{-1} with row/column g zeroed, R(u,v) = G_uu + G_vv - 2 G_uv.  The
// reference's own value carries the rounding of its 1e10/|C| direction (1e-6 ..
// 5e-5 absolute on the fixtures); this computation has none of it.  g = the
// component's node of largest degree (smallest id on ties).
//
// G by the blocked Cholesky of gs_chol.hip: M = L L^T, W = L^{-1}, and
// G_uv = (W^T W)_uv = sum_{k >= max(u,v)} W_ku W_kv read from U = W^T, one wave per
// CSR entry.  GSPARSE_XER_METHOD=ns takes gs_xer_ns.hip's Newton-Schulz instead.
// This unit: the GSPARSE_XER_* knobs, the checks, the grounding, the read-out.  Above
// kXerDenseMax nodes, and through gs_exact_er_sparse at any size, G's columns come from
// gs_xer_sparse.hip's batched CG instead and no dense matrix exists.
#include <cstdlib>
#include <cstring>

#include "gs_dense.hpp"

namespace gs {

XerKnobs xer_knobs() {
    XerKnobs k;
    const char *e = getenv("GSPARSE_XER_METHOD");
    k.ns = e && strcmp(e, "ns") == 0;
    if ((e = getenv("GSPARSE_XER_PANEL"))) {
        const int p = atoi(e);
        k.panel = p >= 1 && p <= 16 ? p : 8;
    }
    if ((e = getenv("GSPARSE_XER_TILE"))) k.tile = atoi(e) == 128 ? 128 : 64;
    k.full = getenv("GSPARSE_XER_FULL") != nullptr;
    k.debug = getenv("GSPARSE_XER_DEBUG") != nullptr;
    if ((e = getenv("GSPARSE_XER_BATCH"))) k.batch = atoi(e) > 0 ? atoi(e) : 0;
    return k;
}

// value symmetry: A_uv == A_vu for every entry (the pattern check is ensure_transpose's)
__global__ void k_er_valsym(const int64_t *__restrict__ tpos, const double *__restrict__ d,
                            int64_t nnz, int *__restrict__ asym) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz;
         e += (int64_t)gridDim.x * blockDim.x)
        if (d[e] != d[tpos[e]]) atomicOr(asym, 1);
}

// grounded node per component: largest row length, smallest id on ties
__global__ void k_er_ground_pick(int64_t n, const int64_t *__restrict__ ip,
                                 const int32_t *__restrict__ lab,
                                 unsigned long long *__restrict__ best) {
    for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < n;
         u += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = ((unsigned long long)(ip[u + 1] - ip[u]) << 32) |
                                       (unsigned long long)(0xffffffffu - (uint32_t)u);
        atomicMax(&best[lab[u]], key);
    }
}

// flag[u] = 1 for identity rows of M (grounded nodes and the padding up to N)
__global__ void k_er_ground_mark(int64_t n, int64_t N, const int32_t *__restrict__ lab,
                                 const unsigned long long *__restrict__ best,
                                 uint8_t *__restrict__ flag) {
    for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < N;
         u += (int64_t)gridDim.x * blockDim.x) {
        if (u >= n) {
            flag[u] = 1;
            continue;
        }
        const uint32_t g = 0xffffffffu - (uint32_t)(best[lab[u]] & 0xffffffffu);
        flag[u] = g == (uint32_t)u;
    }
}

// g[u] = G_uu = sum_{k >= u} U_uk^2, one wave per row
__global__ void __launch_bounds__(256) k_er_gdiag(int64_t n, int64_t N, const double *__restrict__ U,
                                                  double *__restrict__ g) {
    const int64_t u = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (u >= n) return;
    double s = 0.0;
    for (int64_t k = u + lane; k < N; k += 64) {
        const double x = U[u * N + k];
        s += x * x;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) g[u] = s;
}

// r_eff in CSR order, one wave per entry: G_uv = sum_{k >= max(u,v)} U_uk U_vk
__global__ void __launch_bounds__(256) k_er_chol_scores(int64_t N, const int32_t *__restrict__ rows,
                                                        const int32_t *__restrict__ ix, int64_t nnz,
                                                        const uint8_t *__restrict__ flag,
                                                        const double *__restrict__ U,
                                                        const double *__restrict__ g,
                                                        double *__restrict__ out) {
    const int64_t e = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (e >= nnz) return;
    const int64_t u = rows[e], v = ix[e];
    const bool fu = flag[u], fv = flag[v];
    double s = 0.0;
    if (!fu && !fv) {
        const int64_t k0 = u > v ? u : v;
        for (int64_t k = k0 + lane; k < N; k += 64) s += U[u * N + k] * U[v * N + k];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) {
        const double guu = fu ? 0.0 : g[u];
        const double gvv = fv ? 0.0 : g[v];
        const double guv = (fu || fv) ? 0.0 : s;
        const double r = (guu + gvv) - 2.0 * guv;
        out[e] = r > 1e-10 ? r : 1e-10;
    }
}

static void check_symmetric_weights(gs_ctx *c) {
    Graph &g = c->g;
    hipStream_t st = c->stream;
    if (!g.nnz) return;
    auto *flags = (int *)c->buf("xer_flags").ensure(64);
    GS_HIP(hipMemsetAsync(flags, 0, 4, st));
    k_er_valsym<<<grid_for(g.nnz, 256, 8192), 256, 0, st>>>(g.tpos.as<int64_t>(),
                                                           g.data.as<double>(), g.nnz, flags);
    int asym = 0;
    GS_HIP(hipMemcpyAsync(&asym, flags, 4, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    GS_CHECK(!asym, GS_EUNSUPPORTED, "exact effective resistance needs symmetric edge weights");
}

// flag[N]: the identity rows of M, one grounded node per component and the padding
static uint8_t *ground_components(gs_ctx *c, int64_t N) {
    hipStream_t st = c->stream;
    const int64_t n = c->g.n;
    int32_t *lab = components(c);
    auto *best = (unsigned long long *)c->buf("xer_best").ensure(8 * n);
    auto *flag = (uint8_t *)c->buf("xer_flag").ensure(N);
    GS_HIP(hipMemsetAsync(best, 0, 8 * n, st));
    k_er_ground_pick<<<grid_for(n, 256, 8192), 256, 0, st>>>(n, c->g.indptr.as<int64_t>(), lab, best);
    k_er_ground_mark<<<grid_for(N, 256, 8192), 256, 0, st>>>(n, N, lab, best, flag);
    return flag;
}

// the default method: blocked Cholesky + triangular inverse, scores from U = W^T;
// returns the block count
static int32_t cholesky_scores(gs_ctx *c, const XerKnobs &kn, int64_t N, const uint8_t *flag,
                               double *out) {
    Graph &g = c->g;
    hipStream_t st = c->stream;
    const int64_t n = g.n, nnz = g.nnz;
    const DenseScratch ds = dense_scratch(c, N);
    double *gd = (double *)c->buf("xer_g").ensure(sizeof(double) * (size_t)n);
    grounded_inverse(c, kn, N, flag, ds.A, ds.W);
    transpose_square(c, N, ds.W, ds.A);
    k_er_gdiag<<<(unsigned)((n + 3) / 4), 256, 0, st>>>(n, N, ds.A, gd);
    if (nnz)
        k_er_chol_scores<<<(unsigned)((nnz + 3) / 4), 256, 0, st>>>(
            N, g.rows.as<int32_t>(), g.indices.as<int32_t>(), nnz, flag, ds.A, gd, out);
    GS_HIP(hipGetLastError());
    return (int32_t)(N / kCb);
}

}  // namespace gs

using namespace gs;

static constexpr int64_t kXerDenseMax = 32768;  // the dense form's limit
static constexpr double kXerCgRtol = 1e-12;     // the sparse form's defaults
static constexpr int32_t kXerCgMaxIter = 5000;

// the sparse form behind both entry points: checks and grounding as the dense form's
static void exact_er_sparse(gs_ctx *c, double *out, int loc, double cg_rtol, int32_t cg_max_iter,
                            int32_t *batches, int64_t *cg_iterations) {
    Graph &g = c->g;
    GS_CHECK(cg_rtol > 0.0 && cg_rtol < 1.0, GS_EINVAL, "cg_rtol in (0, 1)");
    GS_CHECK(cg_max_iter >= 1, GS_EINVAL, "cg_max_iter >= 1");
    GS_HIP(hipSetDevice(c->device));
    const XerKnobs kn = xer_knobs();
    const int64_t nnz = g.nnz;
    if (batches) *batches = 0;
    if (cg_iterations) *cg_iterations = 0;
    double *dout = (double *)out_device(c, c->outbuf, out, sizeof(double) * (nnz ? nnz : 1), loc);
    if (g.n > 0) {
        check_symmetric_weights(c);
        const uint8_t *flag = ground_components(c, g.n);
        xer_sparse_scores(c, kn, flag, cg_rtol, cg_max_iter, dout, batches, cg_iterations);
    }
    finish_out(c, out, dout, sizeof(double) * nnz, loc);
}

extern "C" int gs_exact_er_sparse(gs_ctx *c, double *out, int loc, double cg_rtol,
                                  int32_t cg_max_iter, int32_t *batches, int64_t *cg_iterations) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        ensure_transpose(c);
        GS_CHECK(c->g.symmetric, GS_EUNSUPPORTED,
                 "exact effective resistance needs a symmetric adjacency (metrics.py:138)");
        exact_er_sparse(c, out, loc, cg_rtol, cg_max_iter, batches, cg_iterations);
    });
}

extern "C" int gs_exact_er(gs_ctx *c, double *out, int loc, int32_t *iterations) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        Graph &g = c->g;
        ensure_transpose(c);
        GS_CHECK(g.symmetric, GS_EUNSUPPORTED,
                 "exact effective resistance needs a symmetric adjacency (metrics.py:138)");
        if (g.n > kXerDenseMax) {
            exact_er_sparse(c, out, loc, kXerCgRtol, kXerCgMaxIter, iterations, nullptr);
            return;
        }
        GS_HIP(hipSetDevice(c->device));
        const XerKnobs kn = xer_knobs();
        const int64_t nnz = g.nnz, N = dense_pad(g.n);
        double *dout = (double *)out_device(c, c->outbuf, out, sizeof(double) * (nnz ? nnz : 1), loc);
        int32_t it_done = 0;
        if (g.n > 0) {
            check_symmetric_weights(c);
            const uint8_t *flag = ground_components(c, N);
            it_done = kn.ns ? newton_schulz_scores(c, kn, N, flag, dout)
                            : cholesky_scores(c, kn, N, flag, dout);
        }
        finish_out(c, out, dout, sizeof(double) * nnz, loc);
        if (iterations) *iterations = it_done;
    });
}
