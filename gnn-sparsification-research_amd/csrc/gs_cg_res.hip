// gs_cg_res.hip -- the resident CG of ApproxER (cg_plan's mode 4): one workgroup solves
// whole columns inside one launch, from a SELL-16 (or ELL) copy of L_reg.  Also what
// it shares with the register-resident solver (mode 5, gs_cg_reg.hip): the facts about
// L_reg's weights, the column-major x and the common tail of a solve.
#include "gs_cg.hpp"

namespace gs {

// ---------------------------------------------------------------- resident CG (mode 4)
// One workgroup (1024 threads, one per CU) owns whole columns: every iteration
// of a column's solve runs inside one launch, the dot products are workgroup
// reductions (no grid-wide step, no per-iteration launches), and the column's
// vectors live in column-major slots -- r, p, q per workgroup (reused from
// column to column) and x in its column of Xc.  256 resident columns x 4
// vectors fit the 256 MiB Infinity Cache for n up to ~24K, so the CG streams
// are served on-die rather than from HBM.  Per iteration:
//   p   (row-flat)  x += fl(alpha_{t-1} p_{t-1}); p = fl(fl(beta p) + r)
//   q   (row-flat)  q = L_reg p from a SELL-16 copy of L_reg (coalesced index
//                   loads, all gathers of a trip in flight), stored
//   pq  (chains)    thread `chain` = (BLAS chunk t, residue j) folds
//                   fma(p_i, q_i) over rows a_t + j, +32, ... -- the OpenBLAS
//                   accumulator chain -- then wave 0 finishes (ddot_finish_wave)
//   r   (chains)    r -= fl(alpha q), chains of dot(r, r), finish
static constexpr int kResThreads = 1024;
static constexpr int kResWaves = kResThreads / 64;
static constexpr int kSell = 16;  // SELL slice height: rows per block (padding to the block's longest row)

struct ResArgs {
    int64_t n, ld, ldn, col0, ncols;
    const int64_t *lp;
    const int32_t *li;
    const double *lv;
    const double *Rr;        // b = Y, row-major (stride ld)
    double *Xc;              // x, column-major: column col0 + i at Xc + i * ldn
    double *slots;           // per workgroup r, p, q (ldn each)
    const int64_t *ca, *cl;  // chunk starts / lengths (device, read by the finish)
    int32_t maxiter;
    double rtol;
    int32_t *iters;          // [k] iterations executed per column
    // SELL-16 copy of L_reg: block b = rows 16 b + l (l < 16); entry k of
    // row 16 b + l at soff[b] + 16 k + l
    const int64_t *soff;     // entry offset of each block
    const int32_t *swid;     // width (longest row) of each block
    const int32_t *scol;     // column, -1 = padding
    const double *sval;      // weight (nullptr in the unit-weight form)
    const double *sdiag;     // unit-weight form: L_reg_ii (off-diagonal entries are -1.0)
    // ELL copy of L_reg when every row has <= 16 entries: entry k of row i at
    // ecol[k * lde + i] (column-major, so a wave's loads are contiguous)
    const int32_t *ecol;     // column, -1 = padding
    const double *eval;      // weight (nullptr in the unit-weight form)
    int64_t lde;
    int64_t ql;              // rows of q mirrored in LDS (dynamic shared memory)
    int64_t nstab;           // SELL slices whose (offset, width) are staged in LDS after q (0: none)
    long long *prof;         // optional: workgroup 0's phase times (wall clock ticks)
    int32_t dcount;          // unit form: every L_reg_ii == fl((entries of row i) - 1 + 1e-6)
};

// a wave-uniform copy of v (read from lane 0): loop and branch conditions that
// depend on it compile as scalar branches, so every barrier stays in uniform
// control flow
__device__ __forceinline__ double wave_uniform(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// q = L_reg p over all rows, row-flat: wave w takes SELL blocks w, w + 16, ...,
// RB blocks per trip; fold from 0.0 in ascending column with rounded products
// (SciPy csr_matvec).  The first W entries of each row are loaded at once
// (then all their gathers), wider rows finish in a tail loop.
template <int RB, int W, bool UNIT>
__device__ __forceinline__ void res_spmv(const ResArgs &A, const double *p, double *q, double *sq, int64_t ql,
                                         const int2 *stab) {
    const int64_t n = A.n;
    const int64_t ntile = (n + 63) >> 6;  // 64-row tiles, one per wave-trip row
    for (int64_t t0 = threadIdx.x >> 6; t0 < ntile; t0 += (int64_t)kResWaves * RB) {
        int64_t o[RB], row[RB];
        int32_t w[RB], wmax = 0;
        double acc[RB], dg[RB];
        bool ok[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int64_t t = t0 + (int64_t)kResWaves * i;
            const int64_t rw = (t < ntile ? t : t0) * 64 + (threadIdx.x & 63);
            ok[i] = t < ntile && rw < n;
            row[i] = ok[i] ? rw : 0;
            const int64_t b = row[i] / kSell;
            int32_t wb;
            if (stab) {  // slice table staged in LDS: no dependent global load
                const int2 t = stab[b];
                o[i] = (int64_t)t.x + row[i] % kSell;
                wb = t.y;
            } else {
                o[i] = A.soff[b] + row[i] % kSell;
                wb = A.swid[b];
            }
            w[i] = ok[i] ? wb : 0;
            wmax = w[i] > wmax ? w[i] : wmax;
            // the diagonal: derived from the row's entry count when the whole row is in
            // the first W entries (dcount graphs), else loaded
            dg[i] = (UNIT && !(A.dcount && w[i] <= W)) ? A.sdiag[row[i]] : 0.0;
            acc[i] = 0.0;
        }
        {
            int32_t col[RB][W];
            double v[RB][W], pv[RB][W];
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    const int64_t idx = o[i] + (k < w[i] ? kSell * k : 0);
                    col[i][k] = A.scol[idx];
                    if (!UNIT) v[i][k] = A.sval[idx];
                }
            if (UNIT && A.dcount) {
#pragma unroll
                for (int i = 0; i < RB; ++i)
                    if (w[i] <= W) {
                        int cnt = 0;
#pragma unroll
                        for (int k = 0; k < W; ++k) cnt += (k < w[i] && col[i][k] >= 0) ? 1 : 0;
                        dg[i] = (double)(cnt - 1) + 1e-6;
                    }
            }
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int k = 0; k < W; ++k) pv[i][k] = p[col[i][k] >= 0 ? col[i][k] : 0];
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    if (UNIT) v[i][k] = col[i][k] == row[i] ? dg[i] : -1.0;
                    const double prod = v[i][k] * pv[i][k];
                    const double qn = acc[i] + prod;
                    acc[i] = (k < w[i] && col[i][k] >= 0) ? qn : acc[i];
                }
        }
        for (int32_t k = W; k < wmax; ++k) {
            int32_t col[RB];
            double v[RB], pv[RB];
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                const int64_t idx = o[i] + (k < w[i] ? (int64_t)kSell * k : 0);
                col[i] = A.scol[idx];
                v[i] = UNIT ? 0.0 : A.sval[idx];
            }
#pragma unroll
            for (int i = 0; i < RB; ++i) pv[i] = p[col[i] >= 0 ? col[i] : 0];
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                if (UNIT) v[i] = col[i] == row[i] ? dg[i] : -1.0;
                const double prod = v[i] * pv[i];
                const double qn = acc[i] + prod;
                acc[i] = (k < w[i] && col[i] >= 0) ? qn : acc[i];
            }
        }
#pragma unroll
        for (int i = 0; i < RB; ++i)
            if (ok[i]) {  // rows mirrored in LDS live only there (chunk tails: copied below)
                if (row[i] < ql) sq[row[i]] = acc[i];
                else q[row[i]] = acc[i];
            }
    }
}

// q = L_reg p over all rows from the ELL copy: row-flat, RB rows per thread
// and trip, all W index loads, then all W gathers of each row in flight (two
// dependent memory latencies per trip); padding entries are masked.
template <int RB, int W, bool UNIT>
__device__ __forceinline__ void res_spmv_ell(const ResArgs &A, const double *p, double *q, double *sq, int64_t ql) {
    const int64_t n = A.n;
    for (int64_t r0 = threadIdx.x; r0 < n; r0 += (int64_t)kResThreads * RB) {
        int64_t row[RB];
        bool ok[RB];
        int32_t col[RB][W];
        double v[RB][W], pv[RB][W], dg[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int64_t rw = r0 + (int64_t)kResThreads * i;
            ok[i] = rw < n;
            row[i] = ok[i] ? rw : r0;
            dg[i] = UNIT ? A.sdiag[row[i]] : 0.0;
#pragma unroll
            for (int k = 0; k < W; ++k) {
                col[i][k] = A.ecol[k * A.lde + row[i]];
                if (!UNIT) v[i][k] = A.eval[k * A.lde + row[i]];
            }
        }
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
            for (int k = 0; k < W; ++k) pv[i][k] = p[col[i][k] >= 0 ? col[i][k] : 0];
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < W; ++k) {
                if (UNIT) v[i][k] = col[i][k] == row[i] ? dg[i] : -1.0;
                const double prod = v[i][k] * pv[i][k];
                const double qn = acc + prod;
                acc = col[i][k] >= 0 ? qn : acc;
            }
            if (ok[i]) {
                if (row[i] < ql) sq[row[i]] = acc;
                else q[row[i]] = acc;
            }
        }
    }
}

template <int RB, int W, int RC, bool UNIT, int EW>
__global__ void __launch_bounds__(kResThreads) k_cg_resident(ResArgs A, ChunkArg ch) {
    __shared__ double s_acc[kMaxChunks * 32];
    __shared__ double s_bc;
    extern __shared__ double sq[];  // q of rows < ql (LDS mirror of the q slot), then the slice table
    const int tid = threadIdx.x;
    const int nchains = ch.count * 32;
    const int64_t n = A.n, ql = A.ql;
    int2 *stab = reinterpret_cast<int2 *>(sq + ql);
    for (int64_t b = tid; b < A.nstab; b += kResThreads)
        stab[b] = make_int2((int)A.soff[b], A.swid[b]);
    __syncthreads();
    double *r = A.slots + (int64_t)blockIdx.x * 3 * A.ldn;
    double *p = r + A.ldn;
    double *q = p + A.ldn;

    // phase clock (workgroup 0, thread 0 writes it out at the end): p update,
    // SpMV, pq chains, r update, finish (incl. the barrier wait before it)
    long long tp[5] = {0, 0, 0, 0, 0};
    long long tmark = wall_clock64();
    auto lap = [&](int ph) {
        const long long t = wall_clock64();
        tp[ph] += t - tmark;
        tmark = t;
    };
    // chain partials are in s_acc: wave 0 finishes in OpenBLAS order, all read it
    auto finish = [&](const double *X, const double *Y) -> double {
        __syncthreads();
        if (tid < 64) {
            const double d = ddot_finish_impl(s_acc, A.ca, A.cl, ch.count, 1, 0, X, Y, nullptr);
            if (tid == 0) s_bc = d;
        }
        __syncthreads();
        lap(4);
        return wave_uniform(s_bc);
    };
    // chain (t, j): rows a_t + j + 32 s below e32 = a_t + (len_t rounded down to 32 after 16)
    auto chain_geom = [&](int chain, int64_t &a, int64_t &L, int64_t &e32) {
        const int t = chain >> 5;
        a = ch.a[t] + (chain & 31);
        L = ch.a[t] + ch.len[t];
        e32 = ch.a[t] + ((ch.len[t] & ~(int64_t)15) & ~(int64_t)31);
    };
    // fold fma(X_i, Y_i) along every chain into s_acc (loads of RC rows in flight);
    // YQ: Y is q, read from its LDS mirror where it has one
    auto chain_dot = [&](const double *X, const double *Y, bool YQ) {
        for (int chain = tid; chain < nchains; chain += kResThreads) {
            int64_t a, L, e32;
            chain_geom(chain, a, L, e32);
            double s = 0.0;
            for (int64_t base = a; base < e32; base += 32 * RC) {
                double xv[RC], yv[RC];
#pragma unroll
                for (int i = 0; i < RC; ++i) {
                    const int64_t rw = base + 32 * i < e32 ? base + 32 * i : base;
                    xv[i] = X[rw];
                    yv[i] = (YQ && rw < ql) ? sq[rw] : Y[rw];
                }
#pragma unroll
                for (int i = 0; i < RC; ++i)
                    if (base + 32 * i < e32) s = __builtin_fma(xv[i], yv[i], s);
            }
            s_acc[chain] = s;
        }
    };

    // columns dealt round-robin; every loop and branch below is workgroup-uniform
    for (int64_t ci = blockIdx.x; ci < A.ncols; ci += gridDim.x) {
        const int64_t c = A.col0 + ci;
        double *x = A.Xc + ci * A.ldn;
        for (int64_t i = tid; i < n; i += kResThreads) r[i] = A.Rr[i * A.ld + c];
        __syncthreads();
        chain_dot(r, r, false);  // ||b||^2 = rho_0 (r = b.copy())
        double rr = finish(r, r);
        const double bn = __builtin_sqrt(rr);
        const double atol = A.rtol * bn;  // max(atol=0, rtol*bnrm2)
        int32_t done = 0;
        double rho_prev = 0.0, alpha_prev = 0.0;
        const bool act = !(bn == 0.0) && !(__builtin_sqrt(rr) < atol);
        for (int32_t it = 0; act && it < A.maxiter; ++it) {
            if (it > 0 && __builtin_sqrt(rr) < atol) break;  // loop-top test
            const double rho_cur = rr;
            const double beta = it > 0 ? rho_cur / rho_prev : 0.0;
            lap(4);
            // p = beta p + r (two roundings); the x update of iteration it-1 rides along
            if (it == 0) {
                for (int64_t i = tid; i < n; i += kResThreads) p[i] = r[i];
            } else {
                // 8 rows per thread in flight as 4 row pairs (16-B loads; the odd row n of
                // an odd n is slot padding, written but never read)
                constexpr int U = 6;
                const int64_t n2 = (n + 1) >> 1;
                double2 *p2 = reinterpret_cast<double2 *>(p);
                const double2 *r2 = reinterpret_cast<const double2 *>(r);
                double2 *x2 = reinterpret_cast<double2 *>(x);
                for (int64_t j0 = tid; j0 < n2; j0 += kResThreads * U) {
                    double2 po[U], rv[U], xv[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int64_t j = j0 + (int64_t)u * kResThreads;
                        const int64_t jc = j < n2 ? j : j0;
                        po[u] = p2[jc];
                        rv[u] = r2[jc];
                        xv[u] = it > 1 ? x2[jc] : make_double2(0.0, 0.0);
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int64_t j = j0 + (int64_t)u * kResThreads;
                        if (j < n2) {
                            double2 xo, pn;
                            const double t1a = alpha_prev * po[u].x, t1b = alpha_prev * po[u].y;
                            xo.x = xv[u].x + t1a;
                            xo.y = xv[u].y + t1b;
                            const double pba = po[u].x * beta, pbb = po[u].y * beta;
                            pn.x = pba + rv[u].x;
                            pn.y = pbb + rv[u].y;
                            x2[j] = xo;
                            p2[j] = pn;
                        }
                    }
                }
            }
            __syncthreads();
            lap(0);
            if (EW) res_spmv_ell<EW <= 8 ? 2 : 1, EW, UNIT>(A, p, q, sq, ql);
            else res_spmv<RB, W, UNIT>(A, p, q, sq, ql, A.nstab ? stab : nullptr);
            __syncthreads();
            lap(1);
            chain_dot(p, q, true);
            // the chunk tails (< 32 rows past each chunk's chains) are read from the q slot
            // by the finish and the r update: copy the LDS-only ones there
            for (int k = tid; k < nchains; k += kResThreads) {
                int64_t a, L, e32;
                chain_geom(k, a, L, e32);
                const int64_t rw = e32 + (k & 31);
                if (rw < L && rw < ql) q[rw] = sq[rw];
            }
            lap(2);
            const double pq = finish(p, q);
            const double alpha = rho_cur / pq;
            // r -= alpha q, chains of dot(r, r); the < 32 leftover rows of each chunk too
            for (int chain = tid; chain < nchains; chain += kResThreads) {
                int64_t a, L, e32;
                chain_geom(chain, a, L, e32);
                double s = 0.0;
                for (int64_t base = a; base < e32; base += 32 * RC) {
                    double rv[RC], qv[RC];
#pragma unroll
                    for (int i = 0; i < RC; ++i) {
                        const int64_t rw = base + 32 * i < e32 ? base + 32 * i : base;
                        rv[i] = r[rw];
                        qv[i] = rw < ql ? sq[rw] : q[rw];
                    }
#pragma unroll
                    for (int i = 0; i < RC; ++i)
                        if (base + 32 * i < e32) {
                            const double t2 = alpha * qv[i];
                            const double rn = rv[i] - t2;
                            r[base + 32 * i] = rn;
                            s = __builtin_fma(rn, rn, s);
                        }
                }
                const int64_t lr = e32 + (chain & 31);
                if (lr < L) {
                    const double t2 = alpha * q[lr];
                    r[lr] = r[lr] - t2;
                }
                s_acc[chain] = s;
            }
            lap(3);
            rr = finish(r, r);
            rho_prev = rho_cur;
            alpha_prev = alpha;
            done = it + 1;
        }
        // x: b (||b|| == 0), 0 (no iteration), or the last pending update
        if (bn == 0.0) {
            for (int64_t i = tid; i < n; i += kResThreads) x[i] = r[i];
        } else if (done == 0) {
            for (int64_t i = tid; i < n; i += kResThreads) x[i] = 0.0;
        } else {
            for (int64_t i = tid; i < n; i += kResThreads) {
                const double t1 = alpha_prev * p[i];
                x[i] = (done > 1 ? x[i] : 0.0) + t1;
            }
        }
        if (tid == 0) A.iters[c] = done;
    }
    if (A.prof && blockIdx.x == 0 && tid == 0)
        for (int i = 0; i < 5; ++i) A.prof[i] = tp[i];
}

// unit-weight test: every off-diagonal entry of L_reg is -1.0 (clears *flag otherwise);
// diag[i] = L_reg_ii (0.0 where the diagonal entry was dropped)
__global__ void k_l_unit(const int64_t *__restrict__ lp, const int32_t *__restrict__ li,
                         const double *__restrict__ lv, int64_t n, double *__restrict__ diag,
                         int32_t *__restrict__ flag) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        double dg = 0.0;
        bool unit = true;
        for (int64_t e = lp[i]; e < lp[i + 1]; ++e) {
            if (li[e] == i) dg = lv[e];
            else unit = unit && lv[e] == -1.0;
        }
        diag[i] = dg;
        if (!unit) atomicAnd(flag, ~1);
        if (!(dg == (double)(lp[i + 1] - lp[i] - 1) + 1e-6)) atomicAnd(flag, ~2);
    }
}

// ELL build (rows of at most lde-independent width W): one thread per row
__global__ void k_ell_fill(int64_t n, int W, int64_t lde, const int64_t *__restrict__ lp,
                           const int32_t *__restrict__ li, const double *__restrict__ lv,
                           int32_t *__restrict__ ecol, double *__restrict__ eval) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e0 = lp[i], len = lp[i + 1] - e0;
        for (int k = 0; k < W; ++k) {
            ecol[k * lde + i] = k < len ? li[e0 + k] : -1;
            if (eval) eval[k * lde + i] = k < len ? lv[e0 + k] : 0.0;
        }
    }
}

// SELL-16 build: one thread per block (width), one per row (fill)
__global__ void k_sell_width(int64_t n, const int64_t *__restrict__ lp, int32_t *__restrict__ swid,
                             int64_t *__restrict__ cnt) {
    const int64_t nb = (n + kSell - 1) / kSell;
    for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < nb;
         b += (int64_t)gridDim.x * blockDim.x) {
        int64_t w = 0;
        for (int64_t r = b * kSell; r < (b + 1) * kSell && r < n; ++r) {
            const int64_t l = lp[r + 1] - lp[r];
            w = l > w ? l : w;
        }
        swid[b] = (int32_t)w;
        cnt[b] = kSell * w;
    }
}

__global__ void k_sell_fill(int64_t n, const int64_t *__restrict__ lp,
                            const int32_t *__restrict__ li, const double *__restrict__ lv,
                            const int64_t *__restrict__ soff, const int32_t *__restrict__ swid,
                            int32_t *__restrict__ scol, double *__restrict__ sval) {
    for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < n;
         g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = g / kSell;
        const int l = (int)(g % kSell);
        const int64_t e0 = lp[g], len = lp[g + 1] - e0;
        for (int64_t k = 0; k < swid[b]; ++k) {
            const int64_t idx = soff[b] + kSell * k + l;
            scol[idx] = k < len ? li[e0 + k] : -1;
            if (sval) sval[idx] = k < len ? lv[e0 + k] : 0.0;
        }
    }
}

// Xc (column-major, ncols x ldn) -> X (row-major, stride ld) columns [col0, col0+ncols)
__global__ void __launch_bounds__(256) k_cols_to_rows(const double *__restrict__ Xc, int64_t ldn,
                                                      int64_t n, int64_t col0, int64_t ncols,
                                                      double *__restrict__ X, int64_t ld) {
    __shared__ double tile[32][33];
    const int64_t r0 = (int64_t)blockIdx.x * 32, c0 = (int64_t)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int yy = ty; yy < 32; yy += 8) {
        const int64_t col = c0 + yy, row = r0 + tx;
        if (col < ncols && row < n) tile[yy][tx] = Xc[col * ldn + row];
    }
    __syncthreads();
    for (int yy = ty; yy < 32; yy += 8) {
        const int64_t row = r0 + yy, col = c0 + tx;
        if (col < ncols && row < n) X[row * ld + col0 + col] = tile[tx][yy];
    }
}

// out = sum of v[0..n) (one workgroup; profiling bookkeeping)
__global__ void __launch_bounds__(256) k_sum_i32(const int32_t *__restrict__ v, int64_t n,
                                                 int64_t *__restrict__ out) {
    __shared__ int64_t part[256];
    int64_t acc = 0;
    for (int64_t i = threadIdx.x; i < n; i += 256) acc += v[i];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = part[0];
}

// ---------------------------------------------------------------- shared with mode 5
// Unit-weight flags, diagonal, SELL slice widths / offsets: functions of L_reg,
// i.e. of (graph, reg) -- computed and read back once (er_prepare's key) into the
// ErState's unit_flags, sell_sent and sell_wid
static void res_lreg(gs_ctx *c, ResCommon &rc) {
    ErState &er = c->er;
    const int64_t n = er.n;
    const int64_t *lp = er.lp.as<int64_t>();
    const int32_t *li = er.li.as<int32_t>();
    const double *lv = er.lv.as<double>();
    auto *sdiag = (double *)c->buf("er_sell_diag").ensure(sizeof(double) * (n + 1));
    auto *uflag = (int32_t *)c->buf("er_unit_flag").ensure(sizeof(int32_t));
    const int64_t nbk = (n + kSell - 1) / kSell;
    auto *swid = (int32_t *)c->buf("er_sell_wid").ensure(sizeof(int32_t) * (nbk + 1));
    auto *soff = (int64_t *)c->buf("er_sell_off").ensure(sizeof(int64_t) * (nbk + 1));
    if (er.unit_key != er.prep_key) {
        int32_t one = 3;  // bit 0: unit weights, bit 1: diagonal = entries - 1 + 1e-6
        GS_HIP(hipMemcpyAsync(uflag, &one, sizeof(one), hipMemcpyHostToDevice, c->stream));
        if (n)
            k_l_unit<<<grid_for(n, 256, 8192), 256, 0, c->stream>>>(lp, li, lv, n, sdiag, uflag);
        auto *scnt = (int64_t *)c->scratch[0].ensure(sizeof(int64_t) * (nbk + 1));
        GS_HIP(hipMemsetAsync(scnt, 0, sizeof(int64_t) * (nbk + 1), c->stream));
        if (nbk) k_sell_width<<<grid_for(nbk, 256, 4096), 256, 0, c->stream>>>(n, lp, swid, scnt);
        exclusive_scan_i64(c, scnt, soff, nbk + 1);
        er.sell_wid.assign((size_t)nbk, 0);
        GS_HIP(hipMemcpyAsync(&er.sell_sent, soff + nbk, sizeof(int64_t), hipMemcpyDeviceToHost,
                              c->stream));
        GS_HIP(hipMemcpyAsync(&er.unit_flags, uflag, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        if (nbk)
            GS_HIP(hipMemcpyAsync(er.sell_wid.data(), swid, sizeof(int32_t) * nbk,
                                  hipMemcpyDeviceToHost, c->stream));
        GS_HIP(hipStreamSynchronize(c->stream));
        er.unit_key = er.prep_key;
    }
    rc.sdiag = sdiag;
    rc.swid = swid;
    rc.soff = soff;
    rc.nbk = nbk;
}

ResCommon res_begin(gs_ctx *c, const CgPlan &plan, int64_t ncols) {
    ErState &er = c->er;
    ResCommon rc{};
    rc.ldn = (er.n + 7) & ~(int64_t)7;
    rc.Xc = (double *)c->buf("er_xc").ensure(sizeof(double) * (size_t)ncols * rc.ldn);
    res_lreg(c, rc);
    // bit 0: unit weights, bit 1: diagonal = entries - 1 + 1e-6
    rc.unit = (er.unit_flags & 1) && plan.res_unit;
    rc.dcount = (er.unit_flags & 3) == 3 && plan.res_dcount;
    if (plan.res_prof) rc.prof = (long long *)c->buf("er_res_prof").ensure(8 * sizeof(long long));
    return rc;
}

void res_end(gs_ctx *c, const ResCommon &rc, hipEvent_t t0, const char *name, int64_t col0,
             int64_t ncols) {
    ErState &er = c->er;
    const int64_t n = er.n;
    GS_HIP(hipGetLastError());
    prof_end(c, t0, name, 0.0);
    const bool prof_rec = c->profiling && !c->pending.empty();
    if (n)
        k_cols_to_rows<<<dim3((unsigned)((n + 31) / 32), (unsigned)((ncols + 31) / 32)), 256, 0,
                         c->stream>>>(rc.Xc, rc.ldn, n, col0, ncols, er.X.as<double>(), er.ld);
    GS_HIP(hipGetLastError());
    if (prof_rec) {
        // algorithmic bytes (SURVEY 8(d) B_ER): 8 (nnz(L_reg) + 10 n) per column and
        // iteration, + b in and x out per column; the iterations are summed on the
        // device and read when the profile is flushed
        ProfPending &pp = c->pending.back();
        pp.bytes = 16.0 * n * ncols;
        pp.its_slot = (int64_t)c->pending.size() - 1;
        pp.its_bytes = 8.0 * ((double)er.lnnz + 10.0 * n);
        auto *slots = c->buf("prof_its").ensure(sizeof(int64_t) * kProfPendingMax);
        k_sum_i32<<<1, 256, 0, c->stream>>>(col_ptrs(er).iters + col0, ncols,
                                            (int64_t *)slots + pp.its_slot);
    }
    if (rc.prof) {
        long long h[5];
        GS_HIP(hipStreamSynchronize(c->stream));
        GS_HIP(hipMemcpy(h, rc.prof, sizeof(h), hipMemcpyDeviceToHost));
        fprintf(stderr,
                "[gsparse] resident CG, workgroup 0 (us): p %.1f spmv %.1f pq %.1f upd %.1f finish %.1f\n",
                h[0] / 100.0, h[1] / 100.0, h[2] / 100.0, h[3] / 100.0, h[4] / 100.0);
    }
    er.pcur = 0;
}

// ---------------------------------------------------------------- mode 4
// From the SELL slice widths hw: the ELL width that holds the longest row (4 / 8 / 12 /
// 16, 0: none does), and the entries per row the SELL SpMV loads at once
struct ResWidths {
    int ew, sell_w;
};
static ResWidths res_widths(const std::vector<int32_t> &hw) {
    const int64_t nbk = (int64_t)hw.size();
    int32_t maxw = 0;
    int sell_w = 8;
    for (int32_t v : hw) maxw = v > maxw ? v : maxw;
    // entries per row loaded at once: the smallest W in 6..8 that leaves at most
    // 1 in 10 of the 64-row tiles (a wave's rows, 4 slices) to the tail loop
    const int64_t ntl = (nbk + 3) / 4;
    for (int wc = 6; wc <= 8; ++wc) {
        int64_t over = 0;
        for (int64_t t = 0; t < ntl; ++t) {
            int32_t m = 0;
            for (int64_t b = 4 * t; b < 4 * t + 4 && b < nbk; ++b) m = hw[b] > m ? hw[b] : m;
            over += m > wc;
        }
        sell_w = wc;
        if (over * 10 <= ntl) break;
    }
    // (measured on the Roman layout: SELL-16 40 us per column-iteration vs ELL-12 48 us --
    // the padded index loads cost more than the dependent block-offset load saves)
    const int ew = maxw <= 4 ? 4 : maxw <= 8 ? 8 : maxw <= 12 ? 12 : maxw <= 16 ? 16 : 0;
    return {ew, sell_w};
}

// k_cg_resident by SpMV shape (rows per thread-trip x entries loaded at once), weight
// form and ELL width
template <int B, int W, bool U, int E>
static void res_launch(const ResArgs &ra, const ChunkArg &ch, unsigned slots, size_t dyn,
                       hipStream_t s) {
    GS_HIP(hipFuncSetAttribute((const void *)k_cg_resident<B, W, 16, U, E>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    k_cg_resident<B, W, 16, U, E><<<slots, kResThreads, dyn, s>>>(ra, ch);
}

template <int B, int W, int E, class... A>
static void res_launch_u(bool unit, const A &...a) {
    if (unit) res_launch<B, W, true, E>(a...);
    else res_launch<B, W, false, E>(a...);
}

template <int E, class... A>
static void res_launch_rbw(int rbw, bool unit, const A &...a) {
    switch (rbw) {
    case 28: res_launch_u<2, 8, E>(unit, a...); break;
    case 27: res_launch_u<2, 7, E>(unit, a...); break;
    case 26: res_launch_u<2, 6, E>(unit, a...); break;
    default: res_launch_u<4, 4, E>(unit, a...); break;
    }
}

template <class... A>
static void res_launch_ew(int ew, int rbw, bool unit, const A &...a) {
    switch (ew) {
    case 4: res_launch_rbw<4>(rbw, unit, a...); break;
    case 8: res_launch_rbw<8>(rbw, unit, a...); break;
    case 12: res_launch_rbw<12>(rbw, unit, a...); break;
    case 16: res_launch_rbw<16>(rbw, unit, a...); break;
    default: res_launch_rbw<0>(rbw, unit, a...); break;
    }
}

void cg_solve_resident(gs_ctx *c, const CgPlan &plan, int64_t col0, int64_t col1, int32_t maxiter,
                       double rtol) {
    ErState &er = c->er;
    const ChunkArg &ch = plan.ch;
    const int64_t n = er.n, ncols = col1 - col0, slots = plan.slots;
    const ColPtrs cp = col_ptrs(er);
    const int64_t *lp = er.lp.as<int64_t>();
    const int32_t *li = er.li.as<int32_t>();
    const double *lv = er.lv.as<double>();
    const ResCommon rc = res_begin(c, plan, ncols);
    const int64_t ldn = rc.ldn, nbk = rc.nbk, sent = er.sell_sent;
    const int32_t unit = rc.unit;
    const int32_t *swid = rc.swid;
    const int64_t *soff = rc.soff;
    double *sl = (double *)c->buf("er_slots").ensure(sizeof(double) * (size_t)slots * 3 * ldn);
    const int64_t *ca = chunks_to_device(c, ch), *cl = ca + kMaxChunks;
    const ResWidths wd = res_widths(er.sell_wid);
    const int ew = plan.res_ell ? wd.ew : 0;
    const int64_t lde = (n + 63) & ~(int64_t)63;
    int32_t *ecol = nullptr;
    double *evalp = nullptr;
    if (ew && n) {
        ecol = (int32_t *)c->buf("er_ell_col").ensure(sizeof(int32_t) * (size_t)ew * lde);
        if (!unit) evalp = (double *)c->buf("er_ell_val").ensure(sizeof(double) * (size_t)ew * lde);
        k_ell_fill<<<grid_for(n, 256, 16384), 256, 0, c->stream>>>(n, ew, lde, lp, li, lv, ecol,
                                                                  evalp);
    }
    auto *scol = (int32_t *)c->buf("er_sell_col").ensure(sizeof(int32_t) * (sent + 1));
    double *sval = unit ? nullptr
                        : (double *)c->buf("er_sell_val").ensure(sizeof(double) * (sent + 1));
    GS_HIP(hipMemsetAsync(scol, 0xff, sizeof(int32_t) * (sent + 1), c->stream));
    if (nbk)
        k_sell_fill<<<grid_for(n, 256, 16384), 256, 0, c->stream>>>(
            n, lp, li, lv, soff, swid, scol, sval);
    GS_HIP(hipGetLastError());
    ResArgs ra{n, er.ld, ldn, col0, ncols, lp, li, lv, er.Rr.as<double>(), rc.Xc, sl, ca, cl, maxiter,
               rtol, cp.iters, soff, swid, scol, sval, rc.sdiag, ecol, evalp, lde, 0, 0, rc.prof,
               rc.dcount};
    // q mirror in LDS: what the 160 KiB leave after the static 16 KiB
    // dynamic LDS (140 KiB next to the 16 KiB chain table): the SELL slice table
    // (8 B per 16 rows, when the offsets fit int32) and a mirror of q's first rows
    size_t lds = 140 * 1024;
    ra.nstab = (sent < (int64_t)1 << 31 && (size_t)nbk * 8 <= lds / 4) ? nbk : 0;
    if (!plan.res_stab) ra.nstab = 0;
    lds -= (size_t)ra.nstab * 8;
    const int64_t qlmax = plan.res_qlds ? (int64_t)(lds / 8) : 0;
    ra.ql = n < qlmax ? n : qlmax;
    const size_t dyn = sizeof(double) * (size_t)ra.ql + 8 * (size_t)ra.nstab + 8;
    hipEvent_t t0 = prof_begin(c);
    // SpMV rows per thread-trip and entries loaded at once: 2 x W, W from the slice
    // widths above (Roman: W = 7, 419 ms per step vs 439 with 8 and 427 with 6;
    // 4 x 4 was slower, its rows wider than 4 take the tail loop)
    const int rbw = plan.res_rbw ? plan.res_rbw : 20 + wd.sell_w;
    if (n)
        res_launch_ew(ew, rbw, unit != 0, ra, ch, (unsigned)slots, dyn, c->stream);
    else
        GS_HIP(hipMemsetAsync(cp.iters + col0, 0, sizeof(int32_t) * ncols, c->stream));
    res_end(c, rc, t0, "cg_res", col0, ncols);
}

}  // namespace gs
