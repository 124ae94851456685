// gs_xer_ns.hip -- the other dense inverse of the grounded Laplacian M, behind
// GSPARSE_XER_METHOD=ns: Newton-Schulz on fp64 MFMA, and the scores read off it.
//
// M^{-1} by Newton-Schulz in its symmetric form, X <- 2X - X (M X) with
// X0 = I / ||M||_inf (Gershgorin, so every eigenvalue of X0 M is in (0, 1]):
// S = M X is a sparse-times-dense product (nnz N per step, HBM-bound), X S =
// X M X is exactly symmetric in exact arithmetic for any symmetric X, so only
// its upper-triangle tiles run (N^3 flops per step on v_mfma_f64_16x16x4_f64)
// and X stays exactly symmetric.  ||I - M X||_F is folded into the S kernel.
#include <cmath>

#include "gs_dense.hpp"

namespace gs {

static constexpr int kGemmK = 16;  // K slice staged in LDS

// Workgroup -> output tile.  Dispatch deals consecutive workgroup ids round-robin
// over the 8 XCDs; regroup so each XCD walks a contiguous run of tiles (shared
// A rows / B columns stay in its own L2).  SYM: only tiles bi <= bj (row-major
// over the upper triangle), the result mirrored into (bj, bi).
template <bool SYM>
__device__ __forceinline__ void gemm_tile(int nb, int &bi, int &bj) {
    const int nblk = gridDim.x;
    int t = blockIdx.x;
    if ((nblk & 7) == 0) t = (t & 7) * (nblk >> 3) + (t >> 3);
    if (!SYM) {
        bi = t / nb;
        bj = t % nb;
        return;
    }
    // row bi starts at s(bi) = bi*nb - bi*(bi-1)/2
    const double q = 2.0 * nb + 1.0;
    int r = (int)((q - sqrt(q * q - 8.0 * t)) * 0.5);
    while (r > 0 && (int64_t)r * nb - (int64_t)r * (r - 1) / 2 > t) --r;
    while ((int64_t)(r + 1) * nb - (int64_t)(r + 1) * r / 2 <= t) ++r;
    bi = r;
    bj = r + (t - (r * nb - r * (r - 1) / 2));
}

// C = alpha * A * B + beta * Cin  (N x N row-major, N a multiple of TM, fp64).
// TM x TM output tile per 256-thread workgroup, four waves in 2x2, each wave
// (TM/2)^2 as (TM/32)^2 v_mfma_f64_16x16x4_f64 tiles.  K advances 16 at a time
// through LDS; the next slice is loaded into registers (16-byte loads) while
// the current one feeds the MFMAs.  SYM: the product is symmetric (X (M X) with
// X, M symmetric): upper-triangle tiles only, each written to both triangles.
template <bool SYM, int TM>
__global__ void __launch_bounds__(256) k_dgemm(int64_t N, const double *__restrict__ A,
                                               const double *__restrict__ B, double alpha,
                                               double beta, const double *__restrict__ Cin,
                                               double *__restrict__ C) {
    constexpr int FT = TM / 32;          // MFMA tiles per wave per dimension
    constexpr int LA = TM * kGemmK / 512;  // 16-byte loads per thread per operand
    __shared__ double As[TM][kGemmK + 2];
    __shared__ double Bs[kGemmK][TM + 2];
    typedef double d2 __attribute__((ext_vector_type(2)));
    typedef double d4 __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bi, bj;
    gemm_tile<SYM>((int)(N / TM), bi, bj);
    const int64_t r0 = (int64_t)bi * TM, c0 = (int64_t)bj * TM;
    const int wr = (wave >> 1) * (TM / 2), wc = (wave & 1) * (TM / 2);
    d4 acc[FT][FT];
#pragma unroll
    for (int i = 0; i < FT; ++i)
#pragma unroll
        for (int j = 0; j < FT; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
    d2 ra[LA], rb[LA];
    auto load = [&](int64_t k0) {
#pragma unroll
        for (int q = 0; q < LA; ++q) {
            const int e = tid + q * 256;  // d2 index within the slice
            const int ar = e / (kGemmK / 2), ac = (e % (kGemmK / 2)) * 2;
            ra[q] = *(const d2 *)(A + (r0 + ar) * N + k0 + ac);
            const int br = e / (TM / 2), bc = (e % (TM / 2)) * 2;
            rb[q] = *(const d2 *)(B + (k0 + br) * N + c0 + bc);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int q = 0; q < LA; ++q) {
            const int e = tid + q * 256;
            const int ar = e / (kGemmK / 2), ac = (e % (kGemmK / 2)) * 2;
            *(d2 *)&As[ar][ac] = ra[q];
            const int br = e / (TM / 2), bc = (e % (TM / 2)) * 2;
            *(d2 *)&Bs[br][bc] = rb[q];
        }
    };
    load(0);
    for (int64_t k0 = 0; k0 < N; k0 += kGemmK) {
        stage();
        __syncthreads();
        if (k0 + kGemmK < N) load(k0 + kGemmK);
#pragma unroll
        for (int s = 0; s < kGemmK / 4; ++s) {
            const int kk = s * 4 + (lane >> 4);
            double a[FT], b[FT];
#pragma unroll
            for (int i = 0; i < FT; ++i) a[i] = As[wr + i * 16 + (lane & 15)][kk];
#pragma unroll
            for (int j = 0; j < FT; ++j) b[j] = Bs[kk][wc + j * 16 + (lane & 15)];
#pragma unroll
            for (int i = 0; i < FT; ++i)
#pragma unroll
                for (int j = 0; j < FT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D map of the f64 16x16x4 form: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int i = 0; i < FT; ++i)
#pragma unroll
        for (int j = 0; j < FT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = r0 + wr + i * 16 + (lane >> 4) + 4 * r;
                const int64_t col = c0 + wc + j * 16 + (lane & 15);
                const int64_t o = row * N + col;
                const double v = alpha * acc[i][j][r];
                const double w = beta != 0.0 ? v + beta * Cin[o] : v;
                C[o] = w;
                if (SYM && bi != bj) C[col * N + row] = w;
            }
}

// Gershgorin bound ||M||_inf (max via the bits of a non-negative double)
__global__ void k_er_rownorm(int64_t n, const int64_t *__restrict__ ip,
                             const int32_t *__restrict__ ix, const double *__restrict__ d,
                             const uint8_t *__restrict__ flag, unsigned long long *__restrict__ mx) {
    double m = 1.0;  // identity rows
    for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < n;
         u += (int64_t)gridDim.x * blockDim.x) {
        if (flag[u]) continue;
        double deg = 0.0, diag = 0.0, off = 0.0;
        for (int64_t e = ip[u]; e < ip[u + 1]; ++e) {
            deg += d[e];
            if (ix[e] == u) diag += d[e];
            else if (!flag[ix[e]]) off += d[e];
        }
        const double r = fabs(deg - diag) + off;
        m = r > m ? r : m;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double t = __shfl_down(m, o, 64);
        m = t > m ? t : m;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(mx, (unsigned long long)__double_as_longlong(m));
}

__global__ void k_er_xinit(int64_t N, const unsigned long long *__restrict__ mx,
                           double *__restrict__ X) {
    const double c = 1.0 / __longlong_as_double((long long)*mx);
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < N * N;
         idx += (int64_t)gridDim.x * blockDim.x)
        X[idx] = (idx / N == idx % N) ? c : 0.0;
}

// S = M X, row i of S from row i of the CSR: (deg_i - A_ii) X_i - sum A_ij X_j over
// non-grounded j != i; S_i = X_i on identity rows.  One workgroup per (row,
// 256-column slice); each block also leaves its share of ||I - S||_F^2.
__global__ void __launch_bounds__(256) k_er_spmm(int64_t n, int64_t N, const int64_t *__restrict__ ip,
                                                 const int32_t *__restrict__ ix,
                                                 const double *__restrict__ d,
                                                 const uint8_t *__restrict__ flag,
                                                 const double *__restrict__ X,
                                                 double *__restrict__ S, double *__restrict__ part) {
    __shared__ double red[4];
    const int64_t slices = (N + 255) / 256;
    const int64_t i = blockIdx.x / slices;
    const int64_t j = (blockIdx.x % slices) * 256 + threadIdx.x;
    double v = 0.0;
    if (j >= N) {
        // past the last column: contributes nothing
    } else if (flag[i]) {
        v = X[i * N + j];
    } else {
        double deg = 0.0, diag = 0.0, acc = 0.0;
        for (int64_t e = ip[i]; e < ip[i + 1]; ++e) {
            const int32_t k = ix[e];
            const double w = d[e];
            deg += w;
            if (k == i) diag += w;
            else if (!flag[k]) acc += w * X[(int64_t)k * N + j];
        }
        v = (deg - diag) * X[i * N + j] - acc;
    }
    if (j < N) S[i * N + j] = v;
    const double r = j < N ? (i == j ? 1.0 : 0.0) - v : 0.0;
    double s2 = r * r;
    for (int o = 32; o > 0; o >>= 1) s2 += __shfl_down(s2, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s2;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ||I - S||_F from the per-block shares, folded in a fixed order (deterministic)
__global__ void __launch_bounds__(256) k_er_resid_fin(const double *__restrict__ part, int64_t np,
                                                      double *__restrict__ res) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < np; i += 256) s += part[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *res = sqrt(red[0]);
}

// r_eff in CSR order: (G_uu + G_vv) - 2 G_uv, then max(., 1e-10) (metrics.py:171-173);
// G = X with grounded rows/columns read as zero
__global__ void k_er_exact_scores(int64_t N, const int32_t *__restrict__ rows,
                                  const int32_t *__restrict__ ix, int64_t nnz,
                                  const uint8_t *__restrict__ flag,
                                  const double *__restrict__ X, double *__restrict__ out) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t u = rows[e], v = ix[e];
        const bool fu = flag[u], fv = flag[v];
        const double guu = fu ? 0.0 : X[u * N + u];
        const double gvv = fv ? 0.0 : X[v * N + v];
        const double guv = (fu || fv) ? 0.0 : X[u * N + v];
        const double r = (guu + gvv) - 2.0 * guv;
        out[e] = r > 1e-10 ? r : 1e-10;
    }
}

// X2 = 2X - X S over gg tiles of width tm
static void launch_step(hipStream_t st, bool sym, int tm, unsigned gg, int64_t N, const double *X,
                        const double *S, double *X2) {
    if (sym && tm == 128)
        k_dgemm<true, 128><<<gg, 256, 0, st>>>(N, X, S, -1.0, 2.0, X, X2);
    else if (sym)
        k_dgemm<true, 64><<<gg, 256, 0, st>>>(N, X, S, -1.0, 2.0, X, X2);
    else if (tm == 128)
        k_dgemm<false, 128><<<gg, 256, 0, st>>>(N, X, S, -1.0, 2.0, X, X2);
    else
        k_dgemm<false, 64><<<gg, 256, 0, st>>>(N, X, S, -1.0, 2.0, X, X2);
}

int32_t newton_schulz_scores(gs_ctx *c, const XerKnobs &kn, int64_t N, const uint8_t *flag,
                             double *out) {
    Graph &g = c->g;
    hipStream_t st = c->stream;
    const int64_t n = g.n, nnz = g.nnz;
    const int64_t *ip = g.indptr.as<int64_t>();
    const int32_t *ix = g.indices.as<int32_t>();
    const double *dd = g.data.as<double>();
    auto *mx = (unsigned long long *)c->buf("xer_mx").ensure(64);
    GS_HIP(hipMemsetAsync(mx, 0, 64, st));
    k_er_rownorm<<<grid_for(n, 256, 2048), 256, 0, st>>>(n, ip, ix, dd, flag, mx);
    const DenseScratch ds = dense_scratch(c, N);
    double *X = ds.A, *S = ds.W;
    double *X2 = (double *)c->buf("xer_X2").ensure(sizeof(double) * (size_t)N * (size_t)N);
    const int64_t sblocks = N * ((N + 255) / 256);
    auto *rpart = (double *)c->buf("xer_resid").ensure(8 * (sblocks + 1));
    k_er_xinit<<<grid_for(N * N, 256, 65536), 256, 0, st>>>(N, mx, X);
    const bool sym = !kn.full;
    // 64-wide tiles (4 waves/SIMD); the 128-wide form holds 1 wave/SIMD and
    // measured slower at every size, kept behind the knob
    const int tm = (kn.tile == 128 && N % 128 == 0) ? 128 : 64;
    const int64_t nb = N / tm;
    const unsigned gg = (unsigned)(sym ? nb * (nb + 1) / 2 : nb * nb);
    // flops one launch executes (the symmetric form runs nb(nb+1)/2 of nb^2 tiles)
    const double flops = 2.0 * tm * tm * (double)N * (double)gg;
    // algorithmic bytes of S = M X: X row gathers per entry + X_i + S_i per row
    const double sbytes = 8.0 * (double)N * (double)(nnz + 2 * N);
    double prev = 1e300;
    int32_t it_done = 0;
    for (int it = 0; it < 256; ++it) {
        hipEvent_t t0 = prof_begin(c);
        k_er_spmm<<<(unsigned)sblocks, 256, 0, st>>>(n, N, ip, ix, dd, flag, X, S, rpart);
        prof_end(c, t0, "exact_er_spmm", sbytes);
        k_er_resid_fin<<<1, 256, 0, st>>>(rpart, sblocks, rpart + sblocks);
        double res = 0.0;
        GS_HIP(hipMemcpyAsync(&res, rpart + sblocks, 8, hipMemcpyDeviceToHost, st));
        GS_HIP(hipStreamSynchronize(st));
        it_done = it;
        if (kn.debug) fprintf(stderr, "[gs_exact_er] it=%d residual=%.6e\n", it, res);
        GS_CHECK(std::isfinite(res), GS_EHIP, "Newton-Schulz diverged at step %d", it);
        // converged, or rounding has taken over: in the quadratic phase each
        // step squares the residual, at the rounding floor it stalls
        if (res < 1e-14 * (double)N || (prev < 1e-2 && res > 0.5 * prev)) break;
        GS_CHECK(it < 255, GS_EHIP, "Newton-Schulz did not converge (residual %g)", res);
        prev = res;
        t0 = prof_begin(c);
        launch_step(st, sym, tm, gg, N, X, S, X2);
        prof_end(c, t0, "exact_er_dgemm", flops);
        std::swap(X, X2);
    }
    if (nnz)
        k_er_exact_scores<<<grid_for(nnz, 256, 8192), 256, 0, st>>>(N, g.rows.as<int32_t>(), ix, nnz,
                                                                    flag, X, out);
    GS_HIP(hipGetLastError());
    return it_done;
}

}  // namespace gs
