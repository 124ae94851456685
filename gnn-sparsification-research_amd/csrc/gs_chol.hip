// gs_chol.hip -- the default dense inverse of the grounded Laplacian M: a blocked
// Cholesky factorisation M = L L^T and W = L^{-1} on fp64 MFMA.
//
// 64 x 64 blocks, N^3/3 + N^3/3 flops; G = M^{-1} = W^T W is never formed: its users
// read G_uv = sum_{k >= max(u,v)} W_ku W_kv from U = W^T, or apply G x = U (W x).
// Block columns are taken in panels of P (XerKnobs::panel, 8).  Per panel [k0, kend),
// for each block step k in it:
//   k_chol_diag       : A_kk = L_kk L_kk^T in LDS, D_k = L_kk^{-1}
//   k_tile_mm<false>  : A_ik <- A_ik D_k^T                 (i > k: the panel column L_ik)
//   k_tile_upd<false> : A_ij -= A_ik A_jk^T                (the panel's own later columns,
//                                                           k < j < kend, i >= j; K = 64)
// and once per panel, over the trailing lower triangle (kend <= j <= i):
//   k_tile_upd<false> : A_ij -= sum_{k in panel} A_ik A_jk^T      (K = 64 (kend - k0))
// Then, with W = I, over the same panels, for each k:
//   k_tile_mm<true>   : W_kj <- D_k W_kj                   (j <= k)
//   k_tile_upd<true>  : W_ij -= A_ik W_kj                  (rows of the panel below k,
//                                                           k < i < kend, j <= k; K = 64)
// and once per panel, for the rows below it (i >= kend, j < kend):
//   k_tile_upd<true>  : W_ij -= sum_{k in panel} A_ik W_kj        (K = 64 (kend - k0))
// A K = 64 update reads and rewrites its C tile per block step (about 4 flops per
// byte); the wide ones touch each C tile once per P steps.  Every tile product is
// 64 x 64 x 64 on v_mfma_f64_16x16x4_f64 (four waves of 2 x 2 MFMA tiles), both
// operands staged whole in LDS.
#include <cmath>

#include "gs_dense.hpp"

namespace gs {

__global__ void k_er_dense_rows(int64_t n, int64_t N, const int64_t *__restrict__ ip,
                                const int32_t *__restrict__ ix, const double *__restrict__ d,
                                const uint8_t *__restrict__ flag, double *__restrict__ A) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (i >= n || flag[i]) {
            A[i * N + i] = 1.0;
            continue;
        }
        double deg = 0.0, diag = 0.0;
        for (int64_t e = ip[i]; e < ip[i + 1]; ++e) {
            const int32_t k = ix[e];
            deg += d[e];
            if (k == i) diag += d[e];
            else if (!flag[k]) A[i * N + k] = -d[e];
        }
        A[i * N + i] = deg - diag;
    }
}

__global__ void k_er_identity(int64_t N, double *__restrict__ W) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N;
         i += (int64_t)gridDim.x * blockDim.x)
        W[i * N + i] = 1.0;
}

// factor the diagonal block in LDS (right-looking, all 256 threads); *bad = 1 on
// a non-positive pivot.  D = L^{-1} by 2 x 2 blocks of 32:
// T11 = L11^{-1}, T22 = L22^{-1} (one thread per column, both halves at once),
// then T21 = -T22 (L21 T11) on all 256 threads.
__global__ void __launch_bounds__(256) k_chol_diag(int64_t N, int k, double *__restrict__ A,
                                                   double *__restrict__ D, int *__restrict__ bad) {
    __shared__ double S[kCb][kCb + 1];
    __shared__ double T[kCb][kCb + 1];
    __shared__ double Z[32][33];
    const int tid = threadIdx.x;
    double *Akk = A + (int64_t)k * kCb * N + (int64_t)k * kCb;
    for (int e = tid; e < kCb * kCb; e += 256) {
        const int r = e / kCb, c = e % kCb;
        S[r][c] = c <= r ? Akk[(int64_t)r * N + c] : 0.0;
        T[r][c] = 0.0;
    }
    __syncthreads();
    for (int j = 0; j < kCb; ++j) {
        if (tid == 0) {
            const double p = S[j][j];
            if (!(p > 0.0)) *bad = 1;
            S[j][j] = sqrt(p > 0.0 ? p : 1.0);
        }
        __syncthreads();
        for (int i = j + 1 + tid; i < kCb; i += 256) S[i][j] = S[i][j] / S[j][j];
        __syncthreads();
        const int m = kCb - 1 - j;
        for (int e = tid; e < m * m; e += 256) {
            const int i = j + 1 + e / m, l = j + 1 + e % m;
            if (l <= i) S[i][l] -= S[i][j] * S[l][j];
        }
        __syncthreads();
    }
    // diagonal halves: thread c < 32 -> column c of T11, 32 <= c < 64 -> column of T22
    if (tid < 64) {
        const int c = tid, hi = c < 32 ? 32 : 64;
        for (int i = c; i < hi; ++i) {
            double s = i == c ? 1.0 : 0.0;
            for (int q = c; q < i; ++q) s -= S[i][q] * T[q][c];
            T[i][c] = s / S[i][i];
        }
    }
    __syncthreads();
    // Z = L21 T11 (32 x 32), then T21 = -T22 Z
    for (int e = tid; e < 32 * 32; e += 256) {
        const int r = e / 32, c = e % 32;
        double s = 0.0;
        for (int q = c; q < 32; ++q) s += S[32 + r][q] * T[q][c];
        Z[r][c] = s;
    }
    __syncthreads();
    for (int e = tid; e < 32 * 32; e += 256) {
        const int r = e / 32, c = e % 32;
        double s = 0.0;
        for (int q = 0; q <= r; ++q) s += T[32 + r][32 + q] * Z[q][c];
        T[32 + r][c] = -s;
    }
    __syncthreads();
    double *Dk = D + (int64_t)k * kCb * kCb;
    for (int e = tid; e < kCb * kCb; e += 256) {
        const int r = e / kCb, c = e % kCb;
        Akk[(int64_t)r * N + c] = S[r][c];  // L_kk (zeros above the diagonal)
        Dk[e] = T[r][c];
    }
}

// row r of the lower triangle (r >= c) holding linear index t of an m x m triangle
__device__ __forceinline__ void tri_index(int64_t t, int &r, int &c) {
    int64_t rr = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (rr * (rr + 1) / 2 > t) --rr;
    while ((rr + 1) * (rr + 2) / 2 <= t) ++rr;
    r = (int)rr;
    c = (int)(t - rr * (rr + 1) / 2);
}

// The 64 x 64 x 64 tile product of a 256-thread workgroup, as both kernels below write
// it out: wave w owns the 32 x 32 quarter at (wr, wc) = ((w >> 1) * 32, (w & 1) * 32) as
// 2 x 2 MFMA tiles over Xs[row][kk], Ys[kk][col], and stores by the C/D map of the f64
// 16x16x4 form (col = lane & 15, row = (lane >> 4) + 4 * reg).  Shared __forceinline__
// helpers for it (zero, accumulate, store) were tried and each one moved instructions
// or accumulator registers in these kernels, so the product stays written out twice.
typedef double d4 __attribute__((ext_vector_type(4)));

// One tile product per workgroup against the diagonal block's inverse D_k:
//   !INVROW: A_ik <- A_ik D_k^T, i = k + 1 + blockIdx.x
//   INVROW : W_kj <- D_k W_kj,   j = blockIdx.x
template <bool INVROW>
__global__ void __launch_bounds__(256) k_tile_mm(int64_t N, int nb, int k, double *__restrict__ A,
                                                 double *__restrict__ W, const double *__restrict__ D) {
    __shared__ double Xs[kCb][kCb + 1];  // Xs[row][kk]
    __shared__ double Ys[kCb][kCb + 1];  // Ys[kk][col]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t t = blockIdx.x;
    const double *X;
    const double *Y;
    int64_t ldx = N, ldy = N;
    double *C;
    const double *Dk = D + (int64_t)k * kCb * kCb;
    if (!INVROW) {
        const int bi = k + 1 + (int)t;
        X = A + (int64_t)bi * kCb * N + (int64_t)k * kCb;
        Y = Dk;  // Y = D_k^T
        ldy = kCb;
        C = A + (int64_t)bi * kCb * N + (int64_t)k * kCb;
    } else {
        const int bj = (int)t;
        X = Dk;
        ldx = kCb;
        Y = W + (int64_t)k * kCb * N + (int64_t)bj * kCb;
        C = W + (int64_t)k * kCb * N + (int64_t)bj * kCb;
    }
    for (int e = tid; e < kCb * kCb; e += 256) {
        const int r = e / kCb, c = e % kCb;
        Xs[r][c] = X[(int64_t)r * ldx + c];
        const double yv = Y[(int64_t)r * ldy + c];
        if (!INVROW) Ys[c][r] = yv;
        else Ys[r][c] = yv;
    }
    __syncthreads();
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    d4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < kCb / 4; ++s) {
        const int kk = s * 4 + (lane >> 4);
        double a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = Xs[wr + i * 16 + (lane & 15)][kk];
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = Ys[kk][wc + j * 16 + (lane & 15)];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wr + i * 16 + (lane >> 4) + 4 * r;
                const int col = wc + j * 16 + (lane & 15);
                double *cp = C + (int64_t)row * N + col;
                *cp = acc[i][j][r];
            }
}

// Rank-(64 kb) tile updates, C -= sum_{q < kb} X_q Y_q over a tile region:
//   CHOL: C = A_ij, X_q = A_{i,k0+q}, Y_q = A_{j,k0+q}^T   (trailing lower triangle)
//   INV : C = W_ij, X_q = A_{i,k0+q}, Y_q = W_{k0+q,j}
// tri: tiles (i, j) with lo <= j <= i < hi; else i in [ilo, ihi), j in [jlo, jhi).
// Wider K (kb = 4: 256) reads and rewrites each C tile once per 4 block steps.
struct TileJob {
    int k0, kb;
    int ilo, ihi, jlo, jhi;
    int tri;
};

template <bool INV>
__global__ void __launch_bounds__(256) k_tile_upd(int64_t N, TileJob J, double *__restrict__ A,
                                                  double *__restrict__ W) {
    __shared__ double Xs[kCb][kCb + 1];
    __shared__ double Ys[kCb][kCb + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t t = blockIdx.x;
    int bi, bj;
    if (J.tri) {
        int r, c;
        tri_index(t, r, c);
        bi = J.ilo + r;
        bj = J.ilo + c;
    } else {
        const int w = J.jhi - J.jlo;
        bi = J.ilo + (int)(t / w);
        bj = J.jlo + (int)(t % w);
    }
    double *C = (INV ? W : A) + (int64_t)bi * kCb * N + (int64_t)bj * kCb;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    d4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < J.kb; ++q) {
        const int kq = J.k0 + q;
        const double *X = A + (int64_t)bi * kCb * N + (int64_t)kq * kCb;
        const double *Y = INV ? W + (int64_t)kq * kCb * N + (int64_t)bj * kCb
                              : A + (int64_t)bj * kCb * N + (int64_t)kq * kCb;
        for (int e = tid; e < kCb * kCb; e += 256) {
            const int r = e / kCb, c = e % kCb;
            Xs[r][c] = X[(int64_t)r * N + c];
            const double yv = Y[(int64_t)r * N + c];
            if (INV) Ys[r][c] = yv;
            else Ys[c][r] = yv;
        }
        __syncthreads();
#pragma unroll
    for (int s = 0; s < kCb / 4; ++s) {
        const int kk = s * 4 + (lane >> 4);
        double a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = Xs[wr + i * 16 + (lane & 15)][kk];
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = Ys[kk][wc + j * 16 + (lane & 15)];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wr + i * 16 + (lane >> 4) + 4 * r;
                const int col = wc + j * 16 + (lane & 15);
                double *cp = C + (int64_t)row * N + col;
                *cp = *cp - acc[i][j][r];
            }
}

static unsigned tile_count(const TileJob &J) {
    if (J.tri) {
        const int64_t m = J.ihi - J.ilo;
        return (unsigned)(m * (m + 1) / 2);
    }
    return (unsigned)((int64_t)(J.ihi - J.ilo) * (J.jhi - J.jlo));
}

// U = W^T (64 x 64 tiles through LDS)
__global__ void __launch_bounds__(256) k_er_transpose(int64_t N, const double *__restrict__ W,
                                                      double *__restrict__ U) {
    __shared__ double T[kCb][kCb + 1];
    const int64_t nb = N / kCb;
    const int64_t bi = blockIdx.x / nb, bj = blockIdx.x % nb;
    for (int e = threadIdx.x; e < kCb * kCb; e += 256) {
        const int r = e / kCb, c = e % kCb;
        T[r][c] = W[(bi * kCb + r) * N + bj * kCb + c];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kCb * kCb; e += 256) {
        const int r = e / kCb, c = e % kCb;
        U[(bj * kCb + r) * N + bi * kCb + c] = T[c][r];
    }
}

DenseScratch dense_scratch(gs_ctx *c, int64_t N) {
    const size_t mb = sizeof(double) * (size_t)N * (size_t)N;
    DenseScratch s;
    s.A = (double *)c->buf("xer_X").ensure(mb);
    s.W = (double *)c->buf("xer_S").ensure(mb);
    return s;
}

// U = W^T for an N x N matrix (N a multiple of 64)
void transpose_square(gs_ctx *c, int64_t N, const double *W, double *U) {
    const int64_t nb = N / kCb;
    k_er_transpose<<<(unsigned)(nb * nb), 256, 0, c->stream>>>(N, W, U);
    GS_HIP(hipGetLastError());
}

void grounded_inverse(gs_ctx *c, const XerKnobs &kn, int64_t N, const uint8_t *flag, double *A,
                      double *W) {
    Graph &g = c->g;
    hipStream_t st = c->stream;
    const int64_t n = g.n;
    const size_t mb = sizeof(double) * (size_t)N * (size_t)N;
    const int64_t *ip = g.indptr.as<int64_t>();
    const int32_t *ix = g.indices.as<int32_t>();
    const double *dd = g.data.as<double>();
    auto *flags = (int *)c->buf("chol_flags").ensure(64);
    const int nb = (int)(N / kCb);
    double *D = (double *)c->buf("xer_D").ensure(sizeof(double) * (size_t)nb * kCb * kCb);
    GS_HIP(hipMemsetAsync(flags, 0, 4, st));
    GS_HIP(hipMemsetAsync(A, 0, mb, st));
    k_er_dense_rows<<<grid_for(N, 256, 8192), 256, 0, st>>>(n, N, ip, ix, dd, flag, A);
    double fl_upd = 0.0;
    const double tf = 2.0 * kCb * kCb * kCb;  // flops of one 64^3 tile product
    // block columns per panel: the trailing update runs at K = 64 P and rewrites
    // each C tile once per P block steps (Roman-like n = 22,662: P = 1 0.59 s,
    // 2 0.47 s, 4 0.39 s, 8 0.37 s)
    const int P = kn.panel;
    auto upd = [&](bool inv, const TileJob &J) {
        const unsigned cnt = tile_count(J);
        if (!cnt || J.kb <= 0) return;
        if (inv) k_tile_upd<true><<<cnt, 256, 0, st>>>(N, J, A, W);
        else k_tile_upd<false><<<cnt, 256, 0, st>>>(N, J, A, W);
        fl_upd += tf * J.kb * (double)cnt;
    };
    hipEvent_t t0 = prof_begin(c);
    for (int k0 = 0; k0 < nb; k0 += P) {
        const int kend = k0 + P < nb ? k0 + P : nb;
        for (int k = k0; k < kend; ++k) {
            k_chol_diag<<<1, 256, 0, st>>>(N, k, A, D, flags);
            const int m = nb - 1 - k;
            if (m > 0) {
                k_tile_mm<false><<<(unsigned)m, 256, 0, st>>>(N, nb, k, A, W, D);
                fl_upd += tf * m;
            }
            // the panel's own later columns (i >= j, k < j < kend), one K = 64 step
            for (int j = k + 1; j < kend; ++j) upd(false, TileJob{k, 1, j, nb, j, j + 1, 0});
        }
        // the trailing lower triangle, K = 64 (kend - k0)
        upd(false, TileJob{k0, kend - k0, kend, nb, kend, nb, 1});
    }
    GS_HIP(hipMemsetAsync(W, 0, mb, st));
    k_er_identity<<<grid_for(N, 256, 8192), 256, 0, st>>>(N, W);
    for (int k0 = 0; k0 < nb; k0 += P) {
        const int kend = k0 + P < nb ? k0 + P : nb;
        for (int k = k0; k < kend; ++k) {
            k_tile_mm<true><<<(unsigned)(k + 1), 256, 0, st>>>(N, nb, k, A, W, D);
            fl_upd += tf * (k + 1);
            // rows of the panel below k (W_ij -= L_ik W_kj, j <= k)
            upd(true, TileJob{k, 1, k + 1, kend, 0, k + 1, 0});
        }
        // rows below the panel: W_ij -= sum_{k in panel} L_ik W_kj, j < kend
        upd(true, TileJob{k0, kend - k0, kend, nb, 0, kend, 0});
    }
    // the factorisation + inverse as one profiled region (flops executed on MFMA)
    prof_end(c, t0, "exact_er_dgemm", fl_upd);
    int bad = 0;
    GS_HIP(hipMemcpyAsync(&bad, flags, 4, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    GS_CHECK(!bad, GS_EHIP, "Cholesky: non-positive pivot (M not positive definite)");
}

}  // namespace gs
