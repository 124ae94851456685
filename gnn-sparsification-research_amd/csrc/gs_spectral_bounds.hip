// gs_spectral_bounds.hip -- how well a reweighted subgraph H approximates the resident
// graph G spectrally: the extreme eigenvalues of the pencil L_H x = lambda L_G x over the
// mean-free vectors,
//   lambda_min = min x'L_H x / x'L_G x,   lambda_max = max x'L_H x / x'L_G x,
// so that H is a (1 +- eps) approximation of G with eps = max(lambda_max - 1, 1 - lambda_min).
//
// Lanczos on A = L_G^+ L_H, which is self-adjoint in the L_G inner product.  The basis
// v_0 .. v_j is L_G-orthonormal and u_q = L_G v_q is kept beside v_q, so an inner product
// <v_q, x> = u_q . x costs no SpMV.  Step j:
//   t = L_H v_j;  alpha_j = v_j . t;  x = L_G^+ t (gs_sp_solve.hpp's CG);
//   x -= alpha_j v_j + beta_{j-1} v_{j-1};  two Gram-Schmidt passes x -= sum (u_q . x) v_q;
//   u = L_G x;  beta_j = sqrt(x . u);  v_{j+1} = x / beta_j,  u_{j+1} = u / beta_j.
// The L_G inner product cannot see the constant vector, so Gram-Schmidt alone never
// removes a constant component of x and the recurrence would amplify it by about
// alpha / beta per step; each pass therefore subtracts the mean of x as well (slot j + 1
// of the coefficients, as gs_fiedler_sparse.hip's passes do).
//
// L_H is applied by L_G's own row-class kernels with the caller's weights in place of the
// stored ones and H's own weighted degrees (the DEG form of the apply, once per call).
//
// Both extreme Ritz values are read from the same tridiagonal T on the host after every
// step (T has at most max_iter rows; the step has synchronised in its solve anyway).
// The stopping test is the residual bound of both extreme Ritz pairs,
//   beta_j |s_last| <= tol theta_max   for the eigenvectors s of theta_min and theta_max,
// or an invariant subspace: beta_j <= max(1e-14, 100 cg_rtol) theta_max.  The solve leaves
// x with a relative error of the order of cg_rtol times the root of the preconditioned
// condition number, so a beta_j below that level is the solve's error, not a direction of
// the Krylov space (H = c G ends this way after one step, a tree's two-valued reweighting
// after two).  Or the Krylov space is full (j + 1 = n - 1).
//
// Every reduction is two-stage in a fixed order, there is no floating-point atomic: two
// calls give the same bits.
#include <cmath>

#include "gs_dense.hpp"
#include "gs_lanczos.hpp"
#include "gs_sp_solve.hpp"

namespace gs {

enum { SB_BAD = 1, SB_ASYM = 2 };

// flags |= SB_BAD for an entry that is negative or not finite, SB_ASYM for an entry whose
// transposed entry holds other bits (a diagonal entry is its own transpose)
__global__ void k_sb_check(int64_t nnz, const double *__restrict__ hw,
                           const int64_t *__restrict__ tpos, int *__restrict__ flags) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz;
         e += (int64_t)gridDim.x * blockDim.x) {
        const double w = hw[e];
        if (!(w >= 0.0 && w < __builtin_inf())) atomicOr(flags, SB_BAD);
        if (__double_as_longlong(w) != __double_as_longlong(hw[tpos[e]])) atomicOr(flags, SB_ASYM);
    }
}

// the start vector's raw values (gs_lanczos.hpp's lz_start) and their partial sums
__global__ void __launch_bounds__(kSpThreads)
k_sb_start_raw(SpGeom g, double *__restrict__ v, double *__restrict__ part) {
    __shared__ double red[kSpWaves];
    SP_OWN(g);
    double s = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kSpThreads) {
        const double t = lz_start(i);
        v[i] = t;
        s += t;
    }
    s = sp_block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// v -= mean(v) (pin: the partial sums of v)
__global__ void __launch_bounds__(kSpThreads)
k_sb_centre(SpGeom g, double *__restrict__ v, const double *__restrict__ pin) {
    __shared__ double red[kSpWaves];
    SP_OWN(g);
    const double mean = sp_fold(pin, g.nb, red) / (double)g.n;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kSpThreads) v[i] -= mean;
}

// part[b] = a . b over the chunk
__global__ void __launch_bounds__(kSpThreads)
k_sb_dot(SpGeom g, const double *__restrict__ a, const double *__restrict__ b,
         double *__restrict__ part) {
    __shared__ double red[kSpWaves];
    SP_OWN(g);
    double s = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kSpThreads) s += a[i] * b[i];
    s = sp_block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// The next basis pair: b = sqrt(x . L_G x) from the fold of pin (rounding can leave a
// vanishing x . L_G x below zero), vn = x / b, un = ux / b; be (may be null) receives b.
// In place (vn == x, un == ux) for the start vector.
__global__ void __launch_bounds__(kSpThreads)
k_sb_next(SpGeom g, const double *x, const double *ux, const double *__restrict__ pin, double *vn,
          double *un, double *__restrict__ be) {
    __shared__ double red[kSpWaves];
    SP_OWN(g);
    const double b = sqrt(fmax(sp_fold(pin, g.nb, red), 0.0));
    for (int64_t i = lo + threadIdx.x; i < hi; i += kSpThreads) {
        vn[i] = b > 0.0 ? x[i] / b : 0.0;
        un[i] = b > 0.0 ? ux[i] / b : 0.0;
    }
    if (be && blockIdx.x == 0 && threadIdx.x == 0) *be = b;
}

// c_q's partial over the chunk for every basis vector q <= j in one pass over the chunk
// of x: one wave per q, c_q = u_q . x (cpart[q nb + b]).  Slot j + 1 is the constant
// vector's, the plain sum of x.
__device__ void sb_basis_dots(SpGeom g, int64_t lo, int64_t hi, int64_t ldv, int j,
                              const double *__restrict__ U, const double *x,
                              double *__restrict__ cpart) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int q = wv; q <= j + 1; q += kSpWaves) {
        const double *uq = U + (int64_t)q * ldv;
        double d = 0.0;
        if (q <= j)
            for (int64_t i = lo + lane; i < hi; i += 64) d += uq[i] * x[i];
        else
            for (int64_t i = lo + lane; i < hi; i += 64) d += x[i];
        for (int o = 32; o > 0; o >>= 1) d += __shfl_down(d, o, 64);
        if (lane == 0) cpart[(int64_t)q * g.nb + blockIdx.x] = d;
    }
}

// alpha_j from the fold of pin; the three-term recurrence; the first Gram-Schmidt pass's
// dots.  ab: alpha_j and beta_j interleaved (ab[2 j], ab[2 j + 1]).
__global__ void __launch_bounds__(kSpThreads)
k_sb_rec(SpGeom g, int64_t ldv, int j, const double *__restrict__ V, const double *__restrict__ U,
         double *x, const double *__restrict__ pin, double *__restrict__ ab,
         double *__restrict__ cpart) {
    __shared__ double red[kSpWaves];
    SP_OWN(g);
    const double a = sp_fold(pin, g.nb, red);
    const double *vj = V + (int64_t)j * ldv;
    const double bprev = j ? ab[2 * (j - 1) + 1] : 0.0;
    const double *vp = j ? V + (int64_t)(j - 1) * ldv : vj;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kSpThreads)
        x[i] = x[i] - a * vj[i] - bprev * vp[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) ab[2 * j] = a;
    __syncthreads();  // the chunk of x is this workgroup's own: its dots can follow
    sb_basis_dots(g, lo, hi, ldv, j, U, x, cpart);
}

// c[q] = the fold of q's partials (workgroup q; j + 2 of them)
__global__ void __launch_bounds__(kSpThreads)
k_sb_foldc(int nb, const double *__restrict__ cpart, double *__restrict__ c) {
    __shared__ double red[kSpWaves];
    const double s = sp_fold(cpart + (int64_t)blockIdx.x * nb, nb, red);
    if (threadIdx.x == 0) c[blockIdx.x] = s;
}

// x -= V c + mean(x) (c[j + 1] is the sum of x), then the second pass's dots (LAST: none)
template <bool LAST>
__global__ void __launch_bounds__(kSpThreads)
k_sb_orth(SpGeom g, int64_t ldv, int j, const double *__restrict__ V,
          const double *__restrict__ U, double *x, const double *__restrict__ c,
          double *__restrict__ cpart) {
    __shared__ double s_c[kLzMaxBasis];
    SP_OWN(g);
    for (int q = threadIdx.x; q <= j + 1; q += kSpThreads) s_c[q] = c[q];
    __syncthreads();
    const double mean = s_c[j + 1] / (double)g.n;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kSpThreads) {
        double t = x[i];
        for (int q = 0; q <= j; ++q) t -= s_c[q] * V[(int64_t)q * ldv + i];
        x[i] = t - mean;
    }
    if (!LAST) {
        __syncthreads();
        sb_basis_dots(g, lo, hi, ldv, j, U, x, cpart);
    }
}

void spectral_bounds(gs_ctx *c, const double *hw, int hw_loc, int64_t nhw, double tol,
                     int32_t max_iter, double cg_rtol, int32_t cg_max_iter, double *lambda_min,
                     double *lambda_max, int32_t *iterations, int64_t *cg_iterations) {
    Graph &g = c->g;
    const int64_t n = g.n;
    GS_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    GS_CHECK(nhw == g.nnz, GS_EINVAL, "spectral bounds: %lld weights for %lld CSR entries",
             (long long)nhw, (long long)g.nnz);
    GS_CHECK(hw || !g.nnz, GS_EINVAL, "spectral bounds: null weights");
    const double *dhw =
        (const double *)to_device(c, c->buf("sb_hw"), hw, sizeof(double) * (size_t)g.nnz, hw_loc);
    if (g.nnz) {
        int *flags = (int *)c->buf("sb_flags").ensure(64);
        GS_HIP(hipMemsetAsync(flags, 0, sizeof(int), st));
        k_sb_check<<<grid_for(g.nnz, 256, 8192), 256, 0, st>>>(g.nnz, dhw, g.tpos.as<int64_t>(),
                                                              flags);
        GS_HIP(hipGetLastError());
        int hf = 0;
        GS_HIP(hipMemcpyAsync(&hf, flags, sizeof(int), hipMemcpyDeviceToHost, st));
        GS_HIP(hipStreamSynchronize(st));
        GS_CHECK(!(hf & SB_BAD), GS_EINVAL,
                 "spectral bounds: a weight of the sparsifier is negative or not finite");
        GS_CHECK(!(hf & SB_ASYM), GS_EUNSUPPORTED,
                 "spectral bounds need symmetric sparsifier weights");
    }
    int64_t ncomp = 0;
    component_stats(c, components(c), &ncomp, nullptr);
    GS_CHECK(ncomp == 1, GS_EINVAL, "spectral bounds: graph has %lld components", (long long)ncomp);

    const SpGeom geo = sp_geometry(n);
    const int64_t nb = geo.nb;
    const int64_t ldv = (n + 63) & ~(int64_t)63;
    const unsigned G = (unsigned)nb;

    // the rows by length and both graphs' weighted degrees: once per call
    double *vec = (double *)c->buf("sb_vec").ensure(sizeof(double) * 9 * (size_t)n);
    double *deg = vec, *inv = vec + n, *x = vec + 2 * n, *r = vec + 3 * n, *p = vec + 4 * n,
           *q = vec + 5 * n, *degh = vec + 6 * n, *t = vec + 7 * n, *ux = vec + 8 * n;
    SpOp opg = sp_row_classes(c, "spectral bounds");
    opg.deg = deg;
    opg.label = "spectral_bounds_spmv_g";
    opg.degrees(deg);
    sp_inverse_degrees(opg, deg, inv);
    SpOp oph = opg;  // the same pattern and row classes, H's weights and degrees
    oph.d = dhw;
    oph.deg = degh;
    oph.label = "spectral_bounds_spmv_h";
    oph.degrees(degh);

    const size_t basis = sizeof(double) * (size_t)(max_iter + 1) * ldv;
    double *V = (double *)c->buf("lz_V").ensure(basis);
    double *U = (double *)c->buf("sb_U").ensure(basis);
    double *ab = (double *)c->buf("sb_ab").ensure(sizeof(double) * 2 * (size_t)max_iter);
    double *part = (double *)c->buf("fs_part").ensure(sizeof(double) * 4 * (size_t)nb);
    double *cpart = (double *)c->buf("fs_cpart").ensure(sizeof(double) * (size_t)(max_iter + 2) * nb);
    double *cvec = (double *)c->buf("fs_c").ensure(sizeof(double) * kLzMaxBasis);
    double *scal = (double *)c->buf("fs_scal").ensure(sizeof(double) * S_COUNT);
    const SpCg cg{geo, inv, x, r, p, q, part, scal, "spectral_bounds_vector"};

    // v_0: the fixed start vector, mean-free, of L_G-norm 1; u_0 = L_G v_0
    hipEvent_t e = prof_begin(c);
    k_sb_start_raw<<<G, kSpThreads, 0, st>>>(geo, V, part);
    k_sb_centre<<<G, kSpThreads, 0, st>>>(geo, V, part);
    prof_end(c, e, "spectral_bounds_lanczos", 0.0);
    opg.apply(V, U, nullptr, 0);
    e = prof_begin(c);
    k_sb_dot<<<G, kSpThreads, 0, st>>>(geo, V, U, part);
    k_sb_next<<<G, kSpThreads, 0, st>>>(geo, V, U, part, V, U, nullptr);
    prof_end(c, e, "spectral_bounds_lanczos", 0.0);
    GS_HIP(hipGetLastError());

    std::vector<double> al, be;
    double tmin = 0.0, tmax = 0.0, res = 0.0;
    int32_t done = 0;
    int64_t cg_total = 0;
    bool converged = false;
    for (int j = 0; j < max_iter; ++j) {
        const double *vj = V + (int64_t)j * ldv;
        // ---- t = L_H v_j, alpha_j's partials, L_G x = t
        oph.apply(vj, t, nullptr, 0);
        double h[S_COUNT];
        const bool solved = sp_solve(opg, cg, t, cg_rtol, cg_max_iter, h);
        cg_total += (int64_t)h[S_ITS];
        if (!solved) {
            if (iterations) *iterations = j;
            if (cg_iterations) *cg_iterations = cg_total;
            const double rel = h[S_THRESH] > 0.0 ? cg_rtol * sqrt(h[S_RRNOW] / h[S_THRESH]) : NAN;
            GS_CHECK(false, GS_ENOCONV,
                     "spectral bounds: the CG solve of Lanczos step %d stopped at "
                     "cg_max_iter=%d with relative residual %.3e > cg_rtol=%.3e (%d outer steps "
                     "done, %lld CG iterations in all)",
                     j, (int)cg_max_iter, rel, cg_rtol, j, (long long)cg_total);
        }
        // ---- the Lanczos step on x (the solve is done with part: alpha_j's partials go there)
        e = prof_begin(c);
        k_sb_dot<<<G, kSpThreads, 0, st>>>(geo, vj, t, part);
        k_sb_rec<<<G, kSpThreads, 0, st>>>(geo, ldv, j, V, U, x, part, ab, cpart);
        k_sb_foldc<<<(unsigned)(j + 2), kSpThreads, 0, st>>>(geo.nb, cpart, cvec);
        k_sb_orth<false><<<G, kSpThreads, 0, st>>>(geo, ldv, j, V, U, x, cvec, cpart);
        k_sb_foldc<<<(unsigned)(j + 2), kSpThreads, 0, st>>>(geo.nb, cpart, cvec);
        k_sb_orth<true><<<G, kSpThreads, 0, st>>>(geo, ldv, j, V, U, x, cvec, cpart);
        prof_end(c, e, "spectral_bounds_lanczos", 0.0);
        opg.apply(x, ux, nullptr, 0);
        e = prof_begin(c);
        k_sb_dot<<<G, kSpThreads, 0, st>>>(geo, x, ux, part);
        k_sb_next<<<G, kSpThreads, 0, st>>>(geo, x, ux, part, V + (int64_t)(j + 1) * ldv,
                                            U + (int64_t)(j + 1) * ldv, ab + 2 * j + 1);
        prof_end(c, e, "spectral_bounds_lanczos", 0.0);
        GS_HIP(hipGetLastError());
        double hab[2];
        GS_HIP(hipMemcpyAsync(hab, ab + 2 * j, sizeof(hab), hipMemcpyDeviceToHost, st));
        GS_HIP(hipStreamSynchronize(st));
        al.push_back(hab[0]);
        be.push_back(hab[1]);
        done = j + 1;
        // ---- both ends of T_{j+1} and their residual bounds, on the host
        GS_CHECK(std::isfinite(hab[0]) && std::isfinite(hab[1]), GS_EHIP,
                 "spectral bounds: Lanczos step %d is not finite", j);
        tmax = lz_ritz_max(al.data(), be.data(), done);
        tmin = lz_ritz_min(al.data(), be.data(), done);
        const double bj = hab[1];
        res = bj * std::max(lz_ritz_last(al.data(), be.data(), done, tmax),
                            lz_ritz_last(al.data(), be.data(), done, tmin));
        const double floor_ = std::max(1e-14, 100.0 * cg_rtol) * fabs(tmax);
        if (res <= tol * fabs(tmax) || bj <= floor_ || j + 1 >= n - 1) {
            converged = true;
            break;
        }
    }
    if (iterations) *iterations = done;
    if (cg_iterations) *cg_iterations = cg_total;
    GS_CHECK(converged, GS_ENOCONV,
             "spectral bounds: Lanczos stopped at max_iter=%d with the residual bound of the "
             "extreme Ritz pairs at %.3e relative > tol=%.3e (%lld CG iterations in all)",
             (int)max_iter, tmax != 0.0 ? res / fabs(tmax) : NAN, tol, (long long)cg_total);
    // L_H and L_G are positive semi-definite: a Ritz value below 0 is rounding
    if (lambda_min) *lambda_min = tmin > 0.0 ? tmin : 0.0;
    if (lambda_max) *lambda_max = tmax > 0.0 ? tmax : 0.0;
}

}  // namespace gs

using namespace gs;

extern "C" {

int gs_spectral_bounds(gs_ctx *c, const double *hw, int hw_loc, int64_t nhw, double tol,
                       int32_t max_iter, double cg_rtol, int32_t cg_max_iter, double *lambda_min,
                       double *lambda_max, int32_t *iterations, int64_t *cg_iterations) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        if (iterations) *iterations = 0;
        if (cg_iterations) *cg_iterations = 0;
        GS_CHECK(tol > 0.0, GS_EINVAL, "tol > 0");
        GS_CHECK(max_iter >= 2 && max_iter <= 500, GS_EINVAL, "max_iter in [2, 500]");
        GS_CHECK(cg_rtol > 0.0 && cg_rtol < 1.0, GS_EINVAL, "cg_rtol in (0, 1)");
        GS_CHECK(cg_max_iter >= 1, GS_EINVAL, "cg_max_iter >= 1");
        ensure_transpose(c);
        GS_CHECK(c->g.symmetric, GS_EUNSUPPORTED, "spectral bounds need a symmetric graph");
        GS_CHECK(c->g.n >= 2, GS_EINVAL, "spectral bounds need n >= 2");
        spectral_bounds(c, hw, hw_loc, nhw, tol, max_iter, cg_rtol, cg_max_iter, lambda_min,
                        lambda_max, iterations, cg_iterations);
    });
}

}  // extern "C"
