// gs_fiedler_sparse.hip -- the algebraic connectivity without a dense matrix:
// lambda_2(L) = 1 / lambda_max(L^+) by Lanczos on L^+ restricted to the mean-free
// vectors (P = I - 11^T / n), as gs_topology.hip's dense form, with the two GEMVs that
// apply the grounded inverse replaced by a preconditioned CG solve of L y = P v_j.
//
// L = D - W from the resident symmetric CSR: D the weighted degrees over the
// off-diagonal entries, stored diagonal entries (self-loops) dropped, as
// k_er_dense_rows builds the dense L.  The preconditioner is Jacobi (1 / D_ii) followed
// by the projection P, so every iterate stays mean-free and CG runs on the subspace
// where L is positive definite.
//
// Nothing here is a persistent kernel: every reduction is two-stage (one partial per
// workgroup over a fixed contiguous chunk, then a fold in a fixed order that every
// consumer workgroup repeats for itself), so a step is a chain of plain launches on the
// context's stream, there is no floating-point atomic, and two calls give the same
// bits.  alpha and beta of the CG are formed on the device from the folds; a solve
// that has met its tolerance freezes itself (its launches return at once), so the
// host only polls every kCgPoll iterations.
//
// The Laplacian apply by row class (SpOp), the row classes, the chunk geometry and the
// solve of L y = P v (sp_solve) are defined here and declared in gs_sp_solve.hpp, which
// gs_spectral_bounds.hip shares; the folds are that header's.
#include <cmath>

#include "gs_dense.hpp"
#include "gs_lanczos.hpp"
#include "gs_sp_solve.hpp"

namespace gs {

// a solve that has met its tolerance: the residual of the current parity is below it
__device__ bool cg_frozen(const double *scal, int par) {
    return scal && scal[S_RR + par] <= scal[S_THRESH];
}

// ------------------------------------------------------------------ Laplacian apply
// rows by length: <= kSpShort one lane, <= kSpWide one wave (list lwave), above one
// workgroup per kSpSeg entries (a row's segments are consecutive in the segment table
// from wbase on; their sums are folded in segment order).  The order of the lists is
// whatever the append order was; a row's own sum does not depend on it.
// cnt: wave rows, wide rows, segments.
__global__ void k_sp_classify(int64_t n, const int64_t *__restrict__ ip, int32_t *__restrict__ cnt,
                              int32_t *__restrict__ lwave, int32_t *__restrict__ lwide,
                              int32_t *__restrict__ wbase, int32_t *__restrict__ segrow,
                              int32_t *__restrict__ segoff) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t len = ip[i + 1] - ip[i];
        if (len > kSpWide) {
            const int32_t ns = (int32_t)((len + kSpSeg - 1) / kSpSeg);
            const int32_t slot = atomicAdd(&cnt[1], 1), base = atomicAdd(&cnt[2], ns);
            lwide[slot] = (int32_t)i;
            wbase[slot] = base;
            for (int32_t t = 0; t < ns; ++t) {
                segrow[base + t] = (int32_t)i;
                segoff[base + t] = t;
            }
        } else if (len > kSpShort) {
            lwave[atomicAdd(&cnt[0], 1)] = (int32_t)i;
        }
    }
}

// one entry's term of row i: DEG the weight itself (the weighted degree), else weight x p
template <bool DEG>
__device__ __forceinline__ double sp_term(int64_t i, int32_t k, double d, const double *p) {
    if (k == i) return 0.0;  // a stored diagonal entry is no edge of L
    return DEG ? d : d * p[k];
}

template <bool DEG>
__device__ __forceinline__ void sp_row_out(int64_t i, double s, const double *deg, const double *p,
                                           double *q) {
    q[i] = DEG ? s : deg[i] * p[i] - s;
}

template <bool DEG>
__global__ void __launch_bounds__(kSpThreads)
k_sp_lap_short(int64_t n, const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
               const double *__restrict__ d, const double *__restrict__ deg,
               const double *__restrict__ p, double *__restrict__ q, const double *scal, int par) {
    if (cg_frozen(scal, par)) return;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e0 = ip[i], e1 = ip[i + 1];
        if (e1 - e0 > kSpShort) continue;
        double s = 0.0;
        for (int64_t e = e0; e < e1; ++e) s += sp_term<DEG>(i, ix[e], d[e], p);
        sp_row_out<DEG>(i, s, deg, p, q);
    }
}

template <bool DEG>
__global__ void __launch_bounds__(kSpThreads)
k_sp_lap_wave(int32_t cnt, const int32_t *__restrict__ list, const int64_t *__restrict__ ip,
              const int32_t *__restrict__ ix, const double *__restrict__ d,
              const double *__restrict__ deg, const double *__restrict__ p, double *__restrict__ q,
              const double *scal, int par) {
    if (cg_frozen(scal, par)) return;
    const int64_t slot = blockIdx.x * (int64_t)kSpWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (slot >= cnt) return;
    const int64_t i = list[slot];
    double s = 0.0;
    for (int64_t e = ip[i] + lane; e < ip[i + 1]; e += 64) s += sp_term<DEG>(i, ix[e], d[e], p);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) sp_row_out<DEG>(i, s, deg, p, q);
}

// one segment of a wide row: wpart[segment] = the sum of its terms
template <bool DEG>
__global__ void __launch_bounds__(kSpThreads)
k_sp_lap_seg(const int32_t *__restrict__ segrow, const int32_t *__restrict__ segoff,
             const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
             const double *__restrict__ d, const double *__restrict__ p,
             double *__restrict__ wpart, const double *scal, int par) {
    __shared__ double red[kSpWaves];
    if (cg_frozen(scal, par)) return;
    const int64_t i = segrow[blockIdx.x];
    const int64_t e0 = ip[i] + (int64_t)segoff[blockIdx.x] * kSpSeg;
    const int64_t e1 = e0 + kSpSeg < ip[i + 1] ? e0 + kSpSeg : ip[i + 1];
    double s = 0.0;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += kSpThreads) s += sp_term<DEG>(i, ix[e], d[e], p);
    s = sp_block_sum(s, red);
    if (threadIdx.x == 0) wpart[blockIdx.x] = s;
}

// a wide row's segments, left to right (one lane per wide row)
template <bool DEG>
__global__ void __launch_bounds__(kSpThreads)
k_sp_lap_wide(int32_t cnt, const int32_t *__restrict__ list, const int32_t *__restrict__ wbase,
              const int64_t *__restrict__ ip, const double *__restrict__ wpart,
              const double *__restrict__ deg, const double *__restrict__ p, double *__restrict__ q,
              const double *scal, int par) {
    if (cg_frozen(scal, par)) return;
    const int64_t slot = blockIdx.x * (int64_t)kSpThreads + threadIdx.x;
    if (slot >= cnt) return;
    const int64_t i = list[slot];
    const int64_t ns = (ip[i + 1] - ip[i] + kSpSeg - 1) / kSpSeg;
    double s = 0.0;
    for (int64_t t = 0; t < ns; ++t) s += wpart[wbase[slot] + t];
    sp_row_out<DEG>(i, s, deg, p, q);
}

__global__ void k_sp_invdeg(int64_t n, const double *__restrict__ deg, double *__restrict__ inv) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        inv[i] = deg[i] > 0.0 ? 1.0 / deg[i] : 0.0;
}

// ------------------------------------------------------------------ vector passes
// Workgroup b owns elements [b chunk, min(n, (b + 1) chunk)) in every pass below (SpGeom).
// part[b] = sum of x over the chunk
__global__ void __launch_bounds__(kSpThreads)
k_sp_sum(SpGeom g, const double *__restrict__ x, double *__restrict__ part) {
    __shared__ double red[kSpWaves];
    SP_OWN(g);
    double s = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kSpThreads) s += x[i];
    s = sp_block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// part[b] = p . q over the chunk
__global__ void __launch_bounds__(kSpThreads)
k_sp_dot(SpGeom g, const double *__restrict__ p, const double *__restrict__ q,
         double *__restrict__ part, const double *scal, int par) {
    __shared__ double red[kSpWaves];
    if (cg_frozen(scal, par)) return;
    SP_OWN(g);
    double s = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kSpThreads) s += p[i] * q[i];
    s = sp_block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// The x / r update fused with ||r||^2 and with the preconditioner's r . z and sum z
// (z = r / D, not stored).  FIRST: the solve's start instead, x = 0 and r = v - mean(v)
// (pin holds the partial sums of v); else alpha = (r . z) / (p . q) from the fold of pin.
// pout: three rows of nb partials (||r||^2, r . z, sum z).
template <bool FIRST>
__global__ void __launch_bounds__(kSpThreads)
k_sp_xr(SpGeom g, const double *__restrict__ v, const double *__restrict__ p,
        const double *__restrict__ q, const double *__restrict__ inv, double *__restrict__ x,
        double *__restrict__ r, const double *__restrict__ pin, double *__restrict__ pout,
        const double *scal, int par) {
    __shared__ double red[kSpWaves];
    if (!FIRST && cg_frozen(scal, par)) return;
    SP_OWN(g);
    const double f = sp_fold(pin, g.nb, red);
    double a = 0.0;
    if (FIRST) a = f / (double)g.n;               // the mean of v
    else if (f > 0.0) a = scal[S_RZ + par] / f;   // alpha (p . q = 0 only for p = 0)
    double rr = 0.0, rz = 0.0, sz = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kSpThreads) {
        double ri;
        if (FIRST) {
            x[i] = 0.0;
            ri = v[i] - a;
        } else {
            x[i] = x[i] + a * p[i];
            ri = r[i] - a * q[i];
        }
        r[i] = ri;
        const double zi = ri * inv[i];
        rr += ri * ri;
        rz += ri * zi;
        sz += zi;
    }
    rr = sp_block_sum(rr, red);
    rz = sp_block_sum(rz, red);
    sz = sp_block_sum(sz, red);
    if (threadIdx.x == 0) {
        pout[blockIdx.x] = rr;
        pout[g.nb + blockIdx.x] = rz;
        pout[2 * g.nb + blockIdx.x] = sz;
    }
}

// The p update: p = (z - mean z) + beta p, beta = (r . z) / (r . z)_previous (FIRST: 0,
// and the tolerance of the solve is set: rtol^2 ||r_0||^2).  Workgroup 0 publishes the
// folded scalars for the next parity and counts the iteration; a frozen solve only carries
// its residual over to the next parity.
template <bool FIRST>
__global__ void __launch_bounds__(kSpThreads)
k_sp_p(SpGeom g, const double *__restrict__ r, const double *__restrict__ inv,
       double *__restrict__ p, const double *__restrict__ pin, double *scal, int par, double rtol) {
    __shared__ double red[kSpWaves];
    const int nxt = FIRST ? 0 : par ^ 1;
    if (!FIRST && cg_frozen(scal, par)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) scal[S_RR + nxt] = scal[S_RR + par];
        return;
    }
    SP_OWN(g);
    const double rr = sp_fold(pin, g.nb, red);
    const double rz = sp_fold(pin + g.nb, g.nb, red);
    const double mean = sp_fold(pin + 2 * g.nb, g.nb, red) / (double)g.n;
    double beta = 0.0;
    if (!FIRST) {
        const double old = scal[S_RZ + par];
        beta = old > 0.0 ? rz / old : 0.0;
    }
    for (int64_t i = lo + threadIdx.x; i < hi; i += kSpThreads) {
        const double zi = r[i] * inv[i] - mean;
        p[i] = FIRST ? zi : zi + beta * p[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        scal[S_RZ + nxt] = rz;
        scal[S_RR + nxt] = rr;
        scal[S_RRNOW] = rr;
        if (FIRST) {
            scal[S_THRESH] = rtol * rtol * rr;
            scal[S_ITS] = 0.0;
        } else {
            scal[S_ITS] = scal[S_ITS] + 1.0;
        }
    }
}

// ------------------------------------------------------------------ Lanczos, grid-wide
// the start vector by k_lz_init's formula, in three passes: the raw values and their sum;
// the mean removed and the squares' sum; the norm divided out
__global__ void __launch_bounds__(kSpThreads)
k_sp_start_raw(SpGeom g, double *__restrict__ v, double *__restrict__ part) {
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

__global__ void __launch_bounds__(kSpThreads)
k_sp_start_centre(SpGeom g, double *__restrict__ v, const double *__restrict__ pin,
                  double *__restrict__ pout) {
    __shared__ double red[kSpWaves];
    SP_OWN(g);
    const double mean = sp_fold(pin, g.nb, red) / (double)g.n;
    double s = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kSpThreads) {
        const double t = v[i] - mean;
        v[i] = t;
        s += t * t;
    }
    s = sp_block_sum(s, red);
    if (threadIdx.x == 0) pout[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kSpThreads)
k_sp_start_scale(SpGeom g, double *__restrict__ v, const double *__restrict__ pin) {
    __shared__ double red[kSpWaves];
    SP_OWN(g);
    const double nrm = sqrt(sp_fold(pin, g.nb, red));
    for (int64_t i = lo + threadIdx.x; i < hi; i += kSpThreads) v[i] /= nrm;
}

// w <- P w (pin: the partial sums of w), pout[b] = v_j . w over the chunk
__global__ void __launch_bounds__(kSpThreads)
k_sp_lz_alpha(SpGeom g, const double *__restrict__ vj, double *__restrict__ w,
              const double *__restrict__ pin, double *__restrict__ pout) {
    __shared__ double red[kSpWaves];
    SP_OWN(g);
    const double mean = sp_fold(pin, g.nb, red) / (double)g.n;
    double s = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kSpThreads) {
        const double t = w[i] - mean;
        w[i] = t;
        s += vj[i] * t;
    }
    s = sp_block_sum(s, red);
    if (threadIdx.x == 0) pout[blockIdx.x] = s;
}

// c_q's partial over the chunk for every basis vector q <= j, in one pass over the
// chunk of w: one wave per q (cpart[q nb + b]).  Slot j + 1 is the constant vector's, the
// plain sum of w: a tiny w (beta ~ 0) is rounding noise, whose mean the normalisation
// would blow up into a basis vector that P then maps to nothing, so the Gram-Schmidt
// passes keep w orthogonal to 1 as well (in exact arithmetic it already is).
__device__ void sp_basis_dots(SpGeom g, int64_t lo, int64_t hi, int64_t ldv, int j,
                              const double *__restrict__ V, const double *w,
                              double *__restrict__ cpart) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int q = wv; q <= j + 1; q += kSpWaves) {
        const double *vq = V + (int64_t)q * ldv;
        double d = 0.0;
        if (q <= j)
            for (int64_t i = lo + lane; i < hi; i += 64) d += vq[i] * w[i];
        else
            for (int64_t i = lo + lane; i < hi; i += 64) d += w[i];
        for (int o = 32; o > 0; o >>= 1) d += __shfl_down(d, o, 64);
        if (lane == 0) cpart[(int64_t)q * g.nb + blockIdx.x] = d;
    }
}

// alpha_j from the fold of pin; the three-term recurrence; the first Gram-Schmidt
// pass's dots
__global__ void __launch_bounds__(kSpThreads)
k_sp_lz_rec(SpGeom g, int64_t ldv, int j, const double *__restrict__ V, double *w,
            const double *__restrict__ pin, double *__restrict__ al,
            const double *__restrict__ be, double *__restrict__ cpart) {
    __shared__ double red[kSpWaves];
    SP_OWN(g);
    const double a = sp_fold(pin, g.nb, red);
    const double *vj = V + (int64_t)j * ldv;
    const double bprev = j ? be[j - 1] : 0.0;
    const double *vp = j ? V + (int64_t)(j - 1) * ldv : vj;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kSpThreads)
        w[i] = w[i] - a * vj[i] - bprev * vp[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) al[j] = a;
    __syncthreads();  // the chunk of w is this workgroup's own: its dots can follow
    sp_basis_dots(g, lo, hi, ldv, j, V, w, cpart);
}

// c[q] = the fold of q's partials (workgroup q; j + 2 of them)
__global__ void __launch_bounds__(kSpThreads)
k_sp_lz_foldc(int nb, const double *__restrict__ cpart, double *__restrict__ c) {
    __shared__ double red[kSpWaves];
    const double s = sp_fold(cpart + (int64_t)blockIdx.x * nb, nb, red);
    if (threadIdx.x == 0) c[blockIdx.x] = s;
}

// w -= V c + mean(w) (c[j + 1] is the sum of w), then the second pass's dots (LAST: the
// partial of ||w||^2 instead)
template <bool LAST>
__global__ void __launch_bounds__(kSpThreads)
k_sp_lz_orth(SpGeom g, int64_t ldv, int j, const double *__restrict__ V, double *w,
             const double *__restrict__ c, double *__restrict__ out) {
    __shared__ double red[kSpWaves];
    __shared__ double s_c[kLzMaxBasis];
    SP_OWN(g);
    for (int q = threadIdx.x; q <= j + 1; q += kSpThreads) s_c[q] = c[q];
    __syncthreads();
    const double mean = s_c[j + 1] / (double)g.n;
    double s = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kSpThreads) {
        double t = w[i];
        for (int q = 0; q <= j; ++q) t -= s_c[q] * V[(int64_t)q * ldv + i];
        t -= mean;
        w[i] = t;
        s += t * t;
    }
    if (LAST) {
        s = sp_block_sum(s, red);
        if (threadIdx.x == 0) out[blockIdx.x] = s;
    } else {
        __syncthreads();
        sp_basis_dots(g, lo, hi, ldv, j, V, w, out);
    }
}

// beta_j from the fold of pin, v_{j+1} = w / beta_j; workgroup 0 also reads the largest
// eigenvalue of T_{j+1} (alpha_j is k_sp_lz_rec's)
__global__ void __launch_bounds__(kSpThreads)
k_sp_lz_next(SpGeom g, int64_t ldv, int j, double *__restrict__ V, const double *__restrict__ w,
             const double *__restrict__ pin, const double *al, double *be,
             double *__restrict__ theta) {
    __shared__ double red[kSpWaves];
    SP_OWN(g);
    const double b = sqrt(sp_fold(pin, g.nb, red));
    double *vn = V + (int64_t)(j + 1) * ldv;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kSpThreads) vn[i] = b > 0.0 ? w[i] / b : 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        be[j] = b;
        theta[j] = lz_ritz_max(al, be, j + 1);
    }
}

namespace {

// q = L p (DEG: q = the weighted degrees); scal / par: the solve whose freeze it obeys
template <bool DEG>
void sp_apply(const SpOp &o, const double *p, double *q, const double *scal, int par) {
    hipEvent_t e = prof_begin(o.c);
    k_sp_lap_short<DEG><<<grid_for(o.n, kSpThreads, 1 << 16), kSpThreads, 0, o.st>>>(
        o.n, o.ip, o.ix, o.d, o.deg, p, q, scal, par);
    if (o.nwave)
        k_sp_lap_wave<DEG><<<(unsigned)((o.nwave + kSpWaves - 1) / kSpWaves), kSpThreads, 0, o.st>>>(
            o.nwave, o.lwave, o.ip, o.ix, o.d, o.deg, p, q, scal, par);
    if (o.nwide) {
        k_sp_lap_seg<DEG><<<(unsigned)o.nseg, kSpThreads, 0, o.st>>>(o.segrow, o.segoff, o.ip, o.ix,
                                                                    o.d, p, o.wpart, scal, par);
        k_sp_lap_wide<DEG><<<grid_for(o.nwide, kSpThreads), kSpThreads, 0, o.st>>>(
            o.nwide, o.lwide, o.wbase, o.ip, o.wpart, o.deg, p, q, scal, par);
    }
    prof_end(o.c, e, o.label, 0.0);
}

}  // namespace

void SpOp::apply(const double *p, double *q, const double *scal, int par) const {
    sp_apply<false>(*this, p, q, scal, par);
}

void SpOp::degrees(double *out) const { sp_apply<true>(*this, nullptr, out, nullptr, 0); }

SpOp sp_row_classes(gs_ctx *c, const char *what) {
    Graph &g = c->g;
    const int64_t n = g.n;
    hipStream_t st = c->stream;
    // a wide row has more than kSpWide entries and at most len / kSpSeg + 1 segments, so
    // there are fewer than nnz / kSpWide wide rows and nnz (1 / kSpSeg + 1 / kSpWide) segments
    const size_t wcap = (size_t)(g.nnz / kSpWide + 1), scap = (size_t)(g.nnz / kSpSeg + 1) + wcap;
    int32_t *cnt = (int32_t *)c->buf("fs_cnt").ensure(sizeof(int32_t) * 3);
    int32_t *lwave = (int32_t *)c->buf("fs_lwave").ensure(sizeof(int32_t) * (size_t)n);
    int32_t *lwide = (int32_t *)c->buf("fs_lwide").ensure(sizeof(int32_t) * 2 * wcap);
    int32_t *wbase = lwide + wcap;
    int32_t *segrow = (int32_t *)c->buf("fs_seg").ensure(sizeof(int32_t) * 2 * scap);
    int32_t *segoff = segrow + scap;
    double *wpart = (double *)c->buf("fs_wpart").ensure(sizeof(double) * scap);
    GS_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * 3, st));
    k_sp_classify<<<grid_for(n, kSpThreads, 1 << 16), kSpThreads, 0, st>>>(
        n, g.indptr.as<int64_t>(), cnt, lwave, lwide, wbase, segrow, segoff);
    GS_HIP(hipGetLastError());
    int32_t hcnt[3] = {0, 0, 0};
    GS_HIP(hipMemcpyAsync(hcnt, cnt, sizeof(hcnt), hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    GS_CHECK((size_t)hcnt[1] <= wcap && (size_t)hcnt[2] <= scap, GS_EHIP,
             "%s: the wide-row tables overflowed", what);
    return SpOp{c,      st,     n,       g.indptr.as<int64_t>(), g.indices.as<int32_t>(),
                g.data.as<double>(), lwave, lwide, wbase, segrow, segoff, hcnt[0], hcnt[1],
                hcnt[2], nullptr, wpart, nullptr};
}

void sp_inverse_degrees(const SpOp &op, const double *deg, double *inv) {
    k_sp_invdeg<<<grid_for(op.n, kSpThreads, 1 << 16), kSpThreads, 0, op.st>>>(op.n, deg, inv);
    GS_HIP(hipGetLastError());
}

bool sp_solve(const SpOp &op, const SpCg &cg, const double *v, double rtol, int32_t max_iter,
              double h[S_COUNT]) {
    gs_ctx *c = op.c;
    hipStream_t st = op.st;
    const SpGeom &geo = cg.geo;
    const unsigned G = (unsigned)geo.nb;
    double *part = cg.part, *part3 = cg.part + geo.nb;
    hipEvent_t e = prof_begin(c);
    k_sp_sum<<<G, kSpThreads, 0, st>>>(geo, v, part);
    k_sp_xr<true><<<G, kSpThreads, 0, st>>>(geo, v, cg.p, cg.q, cg.inv, cg.x, cg.r, part, part3,
                                            cg.scal, 0);
    k_sp_p<true><<<G, kSpThreads, 0, st>>>(geo, cg.r, cg.inv, cg.p, part3, cg.scal, 0, rtol);
    prof_end(c, e, cg.label, 0.0);
    GS_HIP(hipGetLastError());
    for (int i = 0; i < S_COUNT; ++i) h[i] = 0.0;
    bool solved = false;
    for (int32_t it = 0; it < max_iter && !solved;) {
        const int32_t stop = std::min<int64_t>(max_iter, (int64_t)it + kCgPoll);
        for (; it < stop; ++it) {
            const int par = it & 1;
            op.apply(cg.p, cg.q, cg.scal, par);
            e = prof_begin(c);
            k_sp_dot<<<G, kSpThreads, 0, st>>>(geo, cg.p, cg.q, part, cg.scal, par);
            k_sp_xr<false><<<G, kSpThreads, 0, st>>>(geo, v, cg.p, cg.q, cg.inv, cg.x, cg.r, part,
                                                     part3, cg.scal, par);
            k_sp_p<false><<<G, kSpThreads, 0, st>>>(geo, cg.r, cg.inv, cg.p, part3, cg.scal, par,
                                                    rtol);
            prof_end(c, e, cg.label, 0.0);
        }
        GS_HIP(hipGetLastError());
        GS_HIP(hipMemcpyAsync(h, cg.scal, sizeof(double) * S_COUNT, hipMemcpyDeviceToHost, st));
        GS_HIP(hipStreamSynchronize(st));
        solved = h[S_RRNOW] <= h[S_THRESH];
    }
    return solved;
}

void fiedler_sparse(gs_ctx *c, double tol, int32_t max_iter, double cg_rtol, int32_t cg_max_iter,
                    double *value, int32_t *iterations, int64_t *cg_iterations) {
    Graph &g = c->g;
    const int64_t n = g.n;
    GS_CHECK(cg_rtol > 0.0 && cg_rtol < 1.0, GS_EINVAL, "cg_rtol in (0, 1)");
    GS_CHECK(cg_max_iter >= 1, GS_EINVAL, "cg_max_iter >= 1");
    GS_CHECK(max_iter + 2 <= kLzMaxBasis, GS_EINVAL, "max_iter in [2, 500]");
    GS_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    int64_t ncomp = 0;
    component_stats(c, components(c), &ncomp, nullptr);
    GS_CHECK(ncomp == 1, GS_EINVAL, "algebraic connectivity: graph has %lld components",
             (long long)ncomp);

    const SpGeom geo = sp_geometry(n);
    const int64_t nb = geo.nb;
    const int64_t ldv = (n + 63) & ~(int64_t)63;

    // the rows by length, the weighted degrees and their reciprocals: once per call
    double *vec = (double *)c->buf("fs_vec").ensure(sizeof(double) * 6 * (size_t)n);
    double *deg = vec, *inv = vec + n, *x = vec + 2 * n, *r = vec + 3 * n, *p = vec + 4 * n,
           *q = vec + 5 * n;
    SpOp op = sp_row_classes(c, "algebraic connectivity");
    op.deg = deg;
    op.label = "fiedler_sparse_spmv";
    op.degrees(deg);
    sp_inverse_degrees(op, deg, inv);

    double *V = (double *)c->buf("lz_V").ensure(sizeof(double) * (size_t)(max_iter + 1) * ldv);
    double *ab = (double *)c->buf("lz_ab").ensure(sizeof(double) * (3 * (size_t)max_iter + 8));
    double *al = ab, *be = ab + max_iter, *th = ab + 2 * max_iter;
    // partials: one row for a scalar's, three for the CG pass's; the Gram-Schmidt dots'
    double *part = (double *)c->buf("fs_part").ensure(sizeof(double) * 4 * (size_t)nb);
    double *part3 = part + nb;
    double *cpart = (double *)c->buf("fs_cpart").ensure(sizeof(double) * (size_t)(max_iter + 2) * nb);
    double *cvec = (double *)c->buf("fs_c").ensure(sizeof(double) * kLzMaxBasis);
    double *scal = (double *)c->buf("fs_scal").ensure(sizeof(double) * S_COUNT);

    const SpCg cg{geo, inv, x, r, p, q, part, scal, "fiedler_sparse_vector"};
    const unsigned G = (unsigned)nb;
    k_sp_start_raw<<<G, kSpThreads, 0, st>>>(geo, V, part);
    k_sp_start_centre<<<G, kSpThreads, 0, st>>>(geo, V, part, part3);
    k_sp_start_scale<<<G, kSpThreads, 0, st>>>(geo, V, part3);
    GS_HIP(hipGetLastError());

    double prev = 0.0, theta = 0.0;
    int32_t done = 0;
    int64_t cg_total = 0;
    bool converged = false;
    for (int j = 0; j < max_iter; ++j) {
        const double *vj = V + (int64_t)j * ldv;
        // ---- L x = P v_j by Jacobi-preconditioned CG on the mean-free subspace
        double h[S_COUNT];
        const bool solved = sp_solve(op, cg, vj, cg_rtol, cg_max_iter, h);
        cg_total += (int64_t)h[S_ITS];
        if (!solved) {
            if (iterations) *iterations = j;
            if (cg_iterations) *cg_iterations = cg_total;
            const double rel = h[S_THRESH] > 0.0 ? cg_rtol * sqrt(h[S_RRNOW] / h[S_THRESH]) : NAN;
            GS_CHECK(false, GS_ENOCONV,
                     "algebraic connectivity: the CG solve of Lanczos step %d stopped at "
                     "cg_max_iter=%d with relative residual %.3e > cg_rtol=%.3e (%d outer steps "
                     "done, %lld CG iterations in all)",
                     j, (int)cg_max_iter, rel, cg_rtol, j, (long long)cg_total);
        }
        // ---- the Lanczos step on w = x
        hipEvent_t e = prof_begin(c);
        k_sp_sum<<<G, kSpThreads, 0, st>>>(geo, x, part);
        k_sp_lz_alpha<<<G, kSpThreads, 0, st>>>(geo, vj, x, part, part3);
        k_sp_lz_rec<<<G, kSpThreads, 0, st>>>(geo, ldv, j, V, x, part3, al, be, cpart);
        k_sp_lz_foldc<<<(unsigned)(j + 2), kSpThreads, 0, st>>>(geo.nb, cpart, cvec);
        k_sp_lz_orth<false><<<G, kSpThreads, 0, st>>>(geo, ldv, j, V, x, cvec, cpart);
        k_sp_lz_foldc<<<(unsigned)(j + 2), kSpThreads, 0, st>>>(geo.nb, cpart, cvec);
        k_sp_lz_orth<true><<<G, kSpThreads, 0, st>>>(geo, ldv, j, V, x, cvec, part);
        k_sp_lz_next<<<G, kSpThreads, 0, st>>>(geo, ldv, j, V, x, part, al, be, th);
        prof_end(c, e, "fiedler_sparse_lanczos", 0.0);
        GS_HIP(hipGetLastError());
        done = j + 1;
        if (j % 4 != 3 && j + 1 < max_iter && j + 1 < n - 1) continue;
        double hb[2];
        GS_HIP(hipMemcpyAsync(&hb[0], th + j, sizeof(double), hipMemcpyDeviceToHost, st));
        GS_HIP(hipMemcpyAsync(&hb[1], be + j, sizeof(double), hipMemcpyDeviceToHost, st));
        GS_HIP(hipStreamSynchronize(st));
        theta = hb[0];
        // converged, an invariant subspace (beta ~ 0), or the Krylov space is full
        if (fabs(theta - prev) <= tol * fabs(theta) || !(hb[1] > 1e-14 * fabs(theta)) ||
            j + 1 >= n - 1) {
            converged = true;
            break;
        }
        prev = theta;
    }
    if (iterations) *iterations = done;
    if (cg_iterations) *cg_iterations = cg_total;
    GS_CHECK(converged, GS_ENOCONV,
             "algebraic connectivity: Lanczos stopped at max_iter=%d with the Ritz value still "
             "moving by %.3e relative > tol=%.3e (%lld CG iterations in all)",
             (int)max_iter, theta != 0.0 ? fabs(theta - prev) / fabs(theta) : NAN, tol,
             (long long)cg_total);
    GS_CHECK(theta > 0.0, GS_EHIP, "Lanczos: non-positive lambda_max(L^+)");
    if (value) *value = 1.0 / theta;
}

}  // namespace gs

using namespace gs;

extern "C" {

int gs_fiedler_sparse(gs_ctx *c, double tol, int32_t max_iter, double cg_rtol, int32_t cg_max_iter,
                      double *value, int32_t *iterations, int64_t *cg_iterations) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        ensure_transpose(c);
        GS_CHECK(c->g.symmetric, GS_EUNSUPPORTED, "algebraic connectivity needs a symmetric graph");
        GS_CHECK(c->g.n >= 2, GS_EINVAL, "algebraic connectivity needs n >= 2");
        GS_CHECK(max_iter >= 2 && max_iter <= 500, GS_EINVAL, "max_iter in [2, 500]");
        fiedler_sparse(c, tol, max_iter, cg_rtol, cg_max_iter, value, iterations, cg_iterations);
    });
}

}  // extern "C"
