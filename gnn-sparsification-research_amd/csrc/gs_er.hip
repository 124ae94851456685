// gs_er.hip -- ApproxER (calculate_approx_effective_resistance_scores,
// metrics.py:178-298) on the device, bit-exact with the reference.
//
// This unit: the setup (edge ids, incidence rows B, L_reg), the projection Y = B @ R,
// the scores, and the gs_er_* entry points.  The k CG solves (metrics.py:284-289) are
// planned by cg_plan (gs_cg.hpp) and run by one of three solvers: gs_cg_stream.hip,
// gs_cg_res.hip, gs_cg_reg.hip.
//
// Layout in HBM (row-major n x k, the JL columns contiguous per node):
//   Rr  residual, initialised with Y = B @ R           (metrics.py:275)
//   X   solution
#include "gs_cg.hpp"
#include "gs_pairwise.hpp"

namespace gs {

// ---------------------------------------------------------------- prepare
__global__ void k_upper_flags(const int32_t *__restrict__ rows, const int32_t *__restrict__ ix,
                              int64_t nnz, int64_t *__restrict__ flag) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz;
         e += (int64_t)gridDim.x * blockDim.x)
        flag[e] = rows[e] < ix[e] ? 1 : 0;
}

__global__ void k_edge_ids(const int64_t *__restrict__ flag, const int64_t *__restrict__ pos,
                           int64_t nnz, int64_t *__restrict__ eid) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz;
         e += (int64_t)gridDim.x * blockDim.x)
        eid[e] = flag[e] ? pos[e] : -1;
}

// B row counts: node i is incident to (u,i) u<i (transposed column i) and (i,j) j>i (row i).
__global__ void k_b_counts(const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
                           const int64_t *__restrict__ tp, const int32_t *__restrict__ ti,
                           int64_t n, int64_t *__restrict__ cnt) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        int64_t c = 0;
        for (int64_t t = tp[i]; t < tp[i + 1]; ++t) c += ti[t] < i;
        for (int64_t e = ip[i]; e < ip[i + 1]; ++e) c += ix[e] > i;
        cnt[i] = c;
    }
}

__global__ void k_b_fill(const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
                         const int64_t *__restrict__ tp, const int32_t *__restrict__ ti,
                         const int64_t *__restrict__ tpos, const int64_t *__restrict__ eid,
                         int64_t n, const int64_t *__restrict__ bptr, int64_t *__restrict__ bcol,
                         int8_t *__restrict__ bsgn, int64_t *__restrict__ bcur) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        int64_t o = bptr[i];
        bcur[i] = o;
        // (u, i) with u < i: edge ids ascending with u (row-major numbering), sign -1
        for (int64_t t = tp[i]; t < tp[i + 1]; ++t)
            if (ti[t] < i) {
                bcol[o] = eid[tpos[t]];
                bsgn[o] = -1;
                ++o;
            }
        // (i, j) with j > i: after every (u, i), sign +1
        for (int64_t e = ip[i]; e < ip[i + 1]; ++e)
            if (ix[e] > i) {
                bcol[o] = eid[e];
                bsgn[o] = 1;
                ++o;
            }
    }
}

// L = diag(rowsum A) - A (zeros dropped, SciPy csr_minus), L_reg = L + reg I.
__device__ __forceinline__ void lrow_diag(const int64_t *ip, const int32_t *ix, const double *d,
                                          int64_t i, double reg, double &diag, bool &has_diag) {
    double deg = 0.0, aii = 0.0;
    bool self = false;
    for (int64_t e = ip[i]; e < ip[i + 1]; ++e) {
        deg = deg + d[e];  // adj.sum(axis=1): fold ascending column from 0.0
        if (ix[e] == i) {
            self = true;
            aii = d[e];
        }
    }
    // D_ii present iff deg != 0 (dia->csr drops zeros)
    bool has_l = false;
    double l = 0.0;
    if (deg != 0.0 && self) {
        l = deg - aii;
        has_l = l != 0.0;
    } else if (deg != 0.0) {
        l = deg;
        has_l = true;
    } else if (self) {
        l = 0.0 - aii;
        has_l = l != 0.0;
    }
    diag = has_l ? l + reg : reg;
    has_diag = diag != 0.0;
}

__global__ void k_l_counts(const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
                           const double *__restrict__ d, int64_t n, double reg,
                           int64_t *__restrict__ cnt) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        double dg;
        bool hd;
        lrow_diag(ip, ix, d, i, reg, dg, hd);
        int64_t c = hd ? 1 : 0;
        for (int64_t e = ip[i]; e < ip[i + 1]; ++e)
            if (ix[e] != i && d[e] != 0.0) ++c;
        cnt[i] = c;
    }
}

__global__ void k_l_fill(const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
                         const double *__restrict__ d, int64_t n, double reg,
                         const int64_t *__restrict__ lp, int32_t *__restrict__ li,
                         double *__restrict__ lv) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        double dg;
        bool hd;
        lrow_diag(ip, ix, d, i, reg, dg, hd);
        int64_t o = lp[i];
        bool placed = !hd;
        for (int64_t e = ip[i]; e < ip[i + 1]; ++e) {
            int32_t j = ix[e];
            if (!placed && j >= i) {
                li[o] = (int32_t)i;
                lv[o] = dg;
                ++o;
                placed = true;
            }
            if (j != i && d[e] != 0.0) {
                li[o] = j;
                lv[o] = 0.0 - d[e];
                ++o;
            }
        }
        if (!placed) {
            li[o] = (int32_t)i;
            lv[o] = dg;
        }
    }
}

// ---------------------------------------------------------------- projection
// Y[i,c] += sign * raw[e - e0, c - rc0] / sqrt_k for node i's incident edges e in
// [e0, e1), in ascending e (metrics.py:272-275; SciPy csr_matvecs folds B's
// sorted row from 0.0, +-1 * R exact), for the columns c in [c0, c1).  One wave per
// node and 64-column slice.  raw is row-major with stride kraw, its column 0 being
// Y's column rc0 (NumPy's whole rows: kraw = k, rc0 = 0; a rank's slice: kraw =
// c1 - c0, rc0 = c0); Y has stride ld.  The first rows (e0 == 0) fold from 0.0,
// later row chunks from the Y the earlier ones left.
__global__ void __launch_bounds__(256) k_project(const int64_t *__restrict__ bptr,
                                                 const int64_t *__restrict__ bcol,
                                                 const int8_t *__restrict__ bsgn, int64_t n,
                                                 int64_t c0, int64_t c1, int64_t kraw, int64_t rc0,
                                                 int64_t ld, int64_t e0, int64_t e1,
                                                 const double *__restrict__ raw, double sqrt_k,
                                                 double *__restrict__ Y) {
    const int64_t k = c1;
    int64_t ncb = (c1 - c0 + 63) / 64;
    int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    int lane = threadIdx.x & 63;
    int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t w = wave; w < n * ncb; w += nwaves) {
        int64_t i = w / ncb, cb = w % ncb;
        int64_t c = c0 + cb * 64 + lane;
        // first incident edge id >= e0 (B rows are sorted): stateless, so the
        // column slices of one node need no shared cursor
        int64_t p = bptr[i], end = bptr[i + 1];
        {
            int64_t hi = end;
            while (p < hi) {
                int64_t mid = (p + hi) >> 1;
                if (bcol[mid] < e0) p = mid + 1;
                else hi = mid;
            }
        }
        double y = (c < k && e0 > 0) ? Y[i * ld + c] : 0.0;
        for (; p < end; ++p) {
            int64_t e = bcol[p];
            if (e >= e1) break;
            if (c < k) {
                double r = raw[(e - e0) * kraw + (c - rc0)] / sqrt_k;
                double t = bsgn[p] > 0 ? r : -r;
                y = y + t;
            }
        }
        if (c < k) Y[i * ld + c] = y;
    }
}

// ---------------------------------------------------------------- scores
// r_eff[e] = 0 + pw_sum_c (Z_u,c - Z_v,c)^2 over columns [col0,col1),
// Z = nan_to_num(X) (metrics.py:288,292-293); finalize: :296-297.
__global__ void k_er_scores(const int32_t *__restrict__ rows, const int32_t *__restrict__ ix,
                            const double *__restrict__ X, int64_t ld, int64_t col0, int64_t col1,
                            int64_t e0, int64_t e1, int finalize, double *__restrict__ out) {
    for (int64_t e = e0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < e1;
         e += (int64_t)gridDim.x * blockDim.x) {
        const double *zu = X + (int64_t)rows[e] * ld + col0;
        const double *zv = X + (int64_t)ix[e] * ld + col0;
        double s = pw_sum<double>(col1 - col0, [&](int64_t c) {
            double a = zu[c], b = zv[c];
            if (a != a || __builtin_isinf(a)) a = 0.0;
            if (b != b || __builtin_isinf(b)) b = 0.0;
            double d = a - b;
            return d * d;
        });
        if (finalize) {
            s = 0.0 + s;
            if (s != s || __builtin_isinf(s)) s = 1e-10;
            s = s > 1e-10 ? s : 1e-10;
        }
        out[e - e0] = s;
    }
}

// Y[:, col0:col1] (+)= B @ (raw rows [e0, e1) / sqrt_k): raw is device-resident,
// row-major with kraw columns -- the whole NumPy rows (kraw = k) or just the slice
// (kraw = col1 - col0).  Advances the streamed-row cursor.
void project_rows(gs_ctx *c, int64_t e0, int64_t e1, const double *draw, int64_t kraw,
                  int64_t col0, int64_t col1, double sqrt_k) {
    ErState &er = c->er;
    const int64_t kc = col1 - col0, rc0 = kraw == er.k ? 0 : col0;
    const int64_t ncb = (kc + 63) / 64;
    hipEvent_t t0 = prof_begin(c);
    k_project<<<grid_for(er.n * ncb * 64, 256, 65536), 256, 0, c->stream>>>(
        er.bptr.as<int64_t>(), er.bcol.as<int64_t>(), er.bsgn.as<int8_t>(), er.n, col0, col1, kraw,
        rc0, er.ld, e0, e1, draw, sqrt_k, er.Rr.as<double>());
    GS_HIP(hipGetLastError());
    prof_end(c, t0, "er_project", 8.0 * (double)(e1 - e0) * (double)kc * 3.0);
    er.proj_c0 = col0;
    er.proj_c1 = col1;
    er.proj_next = e1;
}
}  // namespace gs

using namespace gs;

// every column of [c0, c1) solved since the last gs_er_prepare (a read of
// columns another rank -- or no one -- solved must not return stale X)
static bool er_cols_solved(const ErState &er, int64_t c0, int64_t c1) {
    if ((int64_t)er.col_solved.size() < c1) return false;
    for (int64_t i = c0; i < c1; ++i)
        if (!er.col_solved[i]) return false;
    return true;
}

extern "C" {

int gs_er_prepare(gs_ctx *c, int64_t k, double reg, int64_t *m_out) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        GS_CHECK(k >= 1, GS_EINVAL, "k must be >= 1");
        GS_HIP(hipSetDevice(c->device));
        ensure_transpose(c);
        Graph &g = c->g;
        ErState &er = c->er;
        int64_t n = g.n, nnz = g.nnz;
        er.proj_next = 0;
        er.solved = false;
        er.proj_c0 = 0;
        er.proj_c1 = k;
        // the edge ids, B and L_reg are functions of (graph, k, reg) only: a repeated
        // prepare (every bench step, every rank) reuses them -- no kernels, no host sync
        int64_t regbits;
        memcpy(&regbits, &reg, sizeof(regbits));
        const std::vector<int64_t> pkey = {g.epoch, k, regbits};
        er.col_solved.assign((size_t)k, 0);
        if (pkey == er.prep_key) {
            // per-column scalars and iteration counts restart (async, no host sync): a
            // column not solved since this prepare reports 0 iterations, as before
            GS_HIP(hipMemsetAsync(er.colstate.ptr, 0, er.colstate.bytes, c->stream));
            GS_HIP(hipMemsetAsync(er.iters.ptr, 0, sizeof(int32_t) * k, c->stream));
            if (m_out) *m_out = er.m;
            return;
        }
        er.prep_key.clear();
        er.n = n;
        er.k = k;
        er.reg = reg;
        // undirected edge ids (u<v in CSR order, metrics.py:236-242)
        int64_t *eid = (int64_t *)er.edge_id.ensure(sizeof(int64_t) * (nnz ? nnz : 1));
        int64_t m = 0;
        if (nnz) {
            int64_t *flag = (int64_t *)c->scratch[0].ensure(sizeof(int64_t) * nnz);
            int64_t *pos = (int64_t *)c->scratch[1].ensure(sizeof(int64_t) * nnz);
            k_upper_flags<<<grid_for(nnz, 256, 8192), 256, 0, c->stream>>>(
                g.rows.as<int32_t>(), g.indices.as<int32_t>(), nnz, flag);
            exclusive_scan_i64(c, flag, pos, nnz);
            k_edge_ids<<<grid_for(nnz, 256, 8192), 256, 0, c->stream>>>(flag, pos, nnz, eid);
            int64_t last[2];
            GS_HIP(hipMemcpyAsync(&last[0], pos + nnz - 1, 8, hipMemcpyDeviceToHost, c->stream));
            GS_HIP(hipMemcpyAsync(&last[1], flag + nnz - 1, 8, hipMemcpyDeviceToHost, c->stream));
            GS_HIP(hipStreamSynchronize(c->stream));
            m = last[0] + last[1];
        }
        er.m = m;
        // incidence rows B (metrics.py:260-269)
        int64_t *cnt = (int64_t *)c->scratch[0].ensure(sizeof(int64_t) * (n + 1));
        GS_HIP(hipMemsetAsync(cnt, 0, sizeof(int64_t) * (n + 1), c->stream));
        int64_t *bptr = (int64_t *)er.bptr.ensure(sizeof(int64_t) * (n + 1));
        if (n)
            k_b_counts<<<grid_for(n, 256, 8192), 256, 0, c->stream>>>(
                g.indptr.as<int64_t>(), g.indices.as<int32_t>(), g.tptr.as<int64_t>(),
                g.tidx.as<int32_t>(), n, cnt);
        exclusive_scan_i64(c, cnt, bptr, n + 1);
        er.bcol.ensure(sizeof(int64_t) * (2 * m + 1));
        er.bsgn.ensure(2 * m + 1);
        er.bcur.ensure(sizeof(int64_t) * (n + 1));
        if (n)
            k_b_fill<<<grid_for(n, 256, 8192), 256, 0, c->stream>>>(
                g.indptr.as<int64_t>(), g.indices.as<int32_t>(), g.tptr.as<int64_t>(),
                g.tidx.as<int32_t>(), g.tpos.as<int64_t>(), eid, n, bptr, er.bcol.as<int64_t>(),
                er.bsgn.as<int8_t>(), er.bcur.as<int64_t>());
        // L_reg (metrics.py:251-256)
        GS_HIP(hipMemsetAsync(cnt, 0, sizeof(int64_t) * (n + 1), c->stream));
        int64_t *lp = (int64_t *)er.lp.ensure(sizeof(int64_t) * (n + 1));
        if (n)
            k_l_counts<<<grid_for(n, 256, 8192), 256, 0, c->stream>>>(
                g.indptr.as<int64_t>(), g.indices.as<int32_t>(), g.data.as<double>(), n, reg, cnt);
        exclusive_scan_i64(c, cnt, lp, n + 1);
        int64_t lnnz = 0;
        GS_HIP(hipMemcpyAsync(&lnnz, lp + n, 8, hipMemcpyDeviceToHost, c->stream));
        GS_HIP(hipStreamSynchronize(c->stream));
        er.lnnz = lnnz;
        er.li.ensure(sizeof(int32_t) * (lnnz + 1));
        er.lv.ensure(sizeof(double) * (lnnz + 1));
        if (n)
            k_l_fill<<<grid_for(n, 256, 8192), 256, 0, c->stream>>>(
                g.indptr.as<int64_t>(), g.indices.as<int32_t>(), g.data.as<double>(), n, reg, lp,
                er.li.as<int32_t>(), er.lv.as<double>());
        // state
        // row stride padded to 8 doubles: 64-B aligned rows, 16-B vector access
        er.ld = (k + 7) & ~(int64_t)7;
        // + slack: a 16-B access of a block's last (odd) column reads one column past
        // the block, which on the last row may be past the row's padding
        size_t nk = sizeof(double) * ((size_t)(n ? n : 1) * (size_t)er.ld + 256);
        er.X.ensure(nk);
        er.Rr.ensure(nk);
        er.P0.ensure(nk);
        er.P1.ensure(nk);
        er.Q.ensure(nk);
        // the projection writes every Y entry it covers (the first rows fold from 0.0);
        // the row padding past k is zeroed once per allocation
        if (er.rr_zeroed != er.Rr.ptr || er.rr_k != k) {
            GS_HIP(hipMemsetAsync(er.Rr.ptr, 0, er.Rr.bytes, c->stream));
            er.rr_zeroed = er.Rr.ptr;
            er.rr_k = k;
        }
        er.colstate.ensure(sizeof(double) * 5 * k + sizeof(int32_t) * (3 * k + 4));
        GS_HIP(hipMemsetAsync(er.colstate.ptr, 0, er.colstate.bytes, c->stream));
        er.acc.ensure(sizeof(double) * (size_t)k * kMaxChunks * 32);
        er.iters.ensure(sizeof(int32_t) * k);
        GS_HIP(hipMemsetAsync(er.iters.ptr, 0, sizeof(int32_t) * k, c->stream));
        GS_HIP(hipStreamSynchronize(c->stream));
        er.prep_key = pkey;
        if (m_out) *m_out = m;
    });
}

int gs_er_project_rows_cols(gs_ctx *c, int64_t e0, int64_t e1, const double *raw, int loc,
                            double sqrt_k, int64_t col0, int64_t col1) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        ErState &er = c->er;
        GS_CHECK(er.k > 0, GS_ESTATE, "gs_er_prepare first");
        GS_CHECK(e0 == er.proj_next && e0 <= e1 && e1 <= er.m, GS_EINVAL,
                 "rows must be streamed in order: expected %lld, got [%lld, %lld) of %lld",
                 (long long)er.proj_next, (long long)e0, (long long)e1, (long long)er.m);
        GS_CHECK(0 <= col0 && col0 < col1 && col1 <= er.k, GS_EINVAL, "bad column range");
        GS_CHECK(e0 == 0 || (col0 == er.proj_c0 && col1 == er.proj_c1), GS_EINVAL,
                 "every row chunk must project the same columns");
        GS_HIP(hipSetDevice(c->device));
        er.proj_c0 = col0;
        er.proj_c1 = col1;
        int64_t rowsn = e1 - e0;
        if (rowsn == 0) return;
        size_t bytes = sizeof(double) * (size_t)rowsn * (size_t)er.k;
        const double *draw = (const double *)to_device(c, er.rawbuf, raw, bytes, loc);
        project_rows(c, e0, e1, draw, er.k, col0, col1, sqrt_k);
        if (loc == GS_HOST) GS_HIP(hipStreamSynchronize(c->stream));  // rawbuf reuse
    });
}

int gs_er_project_rows(gs_ctx *c, int64_t e0, int64_t e1, const double *raw, int loc,
                       double sqrt_k) {
    const int64_t k = c ? c->er.k : 0;
    return gs_er_project_rows_cols(c, e0, e1, raw, loc, sqrt_k, 0, k > 0 ? k : 1);
}

int gs_er_solve(gs_ctx *c, int64_t col0, int64_t col1, int32_t maxiter, double rtol,
                int32_t blas_threads) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        ErState &er = c->er;
        GS_CHECK(er.k > 0, GS_ESTATE, "gs_er_prepare first");
        GS_CHECK(er.proj_next == er.m, GS_ESTATE, "projection incomplete: %lld of %lld rows",
                 (long long)er.proj_next, (long long)er.m);
        GS_CHECK(0 <= col0 && col0 < col1 && col1 <= er.k, GS_EINVAL, "bad column range");
        GS_CHECK(er.proj_c0 <= col0 && col1 <= er.proj_c1, GS_ESTATE,
                 "columns [%lld, %lld) were not projected (Y holds [%lld, %lld))", (long long)col0,
                 (long long)col1, (long long)er.proj_c0, (long long)er.proj_c1);
        GS_HIP(hipSetDevice(c->device));
        const CgPlan plan = cg_plan(er.n, er.lnnz, col1 - col0, blas_threads);
        switch (plan.mode) {
        case 5: cg_regres_solve(c, plan, col0, col1, maxiter, rtol); break;
        case 4: cg_solve_resident(c, plan, col0, col1, maxiter, rtol); break;
        default: cg_solve_streamed(c, plan, col0, col1, maxiter, rtol); break;
        }
        GS_HIP(hipMemcpyAsync(er.iters.ptr, col_ptrs(er).iters, sizeof(int32_t) * er.k,
                              hipMemcpyDeviceToDevice, c->stream));
        // a streamed solve always ends with a wait, a resident one only when the context
        // is not asynchronous
        if (plan.mode >= 4) sync_if_needed(c);
        else GS_HIP(hipStreamSynchronize(c->stream));
        er.solved = true;
        std::fill(er.col_solved.begin() + col0, er.col_solved.begin() + col1, 1);
    });
}

int gs_er_plan(int64_t n, int64_t lnnz, int64_t ncols, int32_t blas_threads, int32_t out[4]) {
    return guard([&] {
        GS_CHECK(out, GS_EINVAL, "out is NULL");
        GS_CHECK(n >= 0 && lnnz >= 0 && ncols >= 0, GS_EINVAL, "negative size");
        const CgPlan plan = cg_plan(n, lnnz, ncols, blas_threads);
        out[0] = plan.mode;
        out[1] = plan.cpl;
        out[2] = plan.ru;
        out[3] = plan.ch.count;
    });
}

int gs_er_reg_layout(int64_t n, int32_t blas_threads, int32_t unit, int64_t out[72]) {
    return guard([&] {
        GS_CHECK(out, GS_EINVAL, "out is NULL");
        GS_CHECK(n >= 0, GS_EINVAL, "negative size");
        std::fill(out, out + 72, (int64_t)0);
        const CgPlan plan = cg_plan(n, 0, 1, blas_threads);
        RegLayout L;
        if (!reg_layout(n, plan.ch, plan.reg_nt, plan.reg_keep, unit != 0, L)) return;
        const int64_t head[8] = {L.NT, L.G, L.R, L.T, L.zslot, L.dsl, (int64_t)L.dyn, 0};
        std::copy(head, head + 8, out);
        for (int t = 0; t < L.T; ++t) {
            out[8 + t] = plan.ch.a[t];
            out[8 + 16 + t] = plan.ch.len[t];
            out[8 + 32 + t] = L.keep[t];
            out[8 + 48 + t] = L.lbase[t];
        }
    });
}

// as gs_er_reg_layout with a p window of `window` wave-slots per chunk asked for (3 or 4;
// laid out only where the window kernel exists, else the plain layout): out[7] the window
// laid out (0: none), out[72 + t] its LDS base for chunk t
int gs_er_reg_layout_w(int64_t n, int32_t blas_threads, int32_t unit, int32_t window, int64_t out[88]) {
    return guard([&] {
        GS_CHECK(out, GS_EINVAL, "out is NULL");
        GS_CHECK(n >= 0, GS_EINVAL, "negative size");
        std::fill(out, out + 88, (int64_t)0);
        const CgPlan plan = cg_plan(n, 0, 1, blas_threads);
        RegLayout L;
        if (!reg_layout(n, plan.ch, plan.reg_nt, plan.reg_keep, unit != 0, L, window)) return;
        const int64_t head[8] = {L.NT, L.G, L.R, L.T, L.zslot, L.dsl, (int64_t)L.dyn, L.W};
        std::copy(head, head + 8, out);
        for (int t = 0; t < L.T; ++t) {
            out[8 + t] = plan.ch.a[t];
            out[8 + 16 + t] = plan.ch.len[t];
            out[8 + 32 + t] = L.keep[t];
            out[8 + 48 + t] = L.lbase[t];
            out[8 + 64 + t] = L.wbase[t];
        }
    });
}

// The p window of the last register-resident solve's ELL copy: its size in wave-slots (0:
// the plain layout), the wave-slots with a global p code under the plain and the windowed
// layout (-1 where no window was weighed), the window codes in the copy
int gs_er_reg_window(gs_ctx *c, int64_t out[4]) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        GS_CHECK(out, GS_EINVAL, "out is NULL");
        std::copy(c->reg_win, c->reg_win + 4, out);
    });
}

int gs_er_scores(gs_ctx *c, int64_t col0, int64_t col1, int64_t e0, int64_t e1, int finalize,
                 double *out, int loc) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        ErState &er = c->er;
        GS_CHECK(er.solved, GS_ESTATE, "gs_er_solve first");
        GS_CHECK(0 <= col0 && col0 <= col1 && col1 <= er.k, GS_EINVAL, "bad column range");
        GS_CHECK(0 <= e0 && e0 <= e1 && e1 <= c->g.nnz, GS_EINVAL, "bad edge range");
        GS_CHECK(er_cols_solved(er, col0, col1), GS_ESTATE,
                 "columns [%lld, %lld) were not all solved since gs_er_prepare", (long long)col0,
                 (long long)col1);
        GS_HIP(hipSetDevice(c->device));
        int64_t cnt = e1 - e0;
        double *dout = (double *)out_device(c, c->outbuf, out, sizeof(double) * cnt, loc);
        if (cnt) {
            hipEvent_t t0 = prof_begin(c);
            k_er_scores<<<grid_for(cnt, 64), 64, 0, c->stream>>>(
                c->g.rows.as<int32_t>(), c->g.indices.as<int32_t>(), er.X.as<double>(), er.ld, col0,
                col1, e0, e1, finalize, dout);
            GS_HIP(hipGetLastError());
            prof_end(c, t0, "er_scores", (16.0 * (col1 - col0) + 16.0) * cnt);
        }
        finish_out(c, out, dout, sizeof(double) * cnt, loc);
    });
}

int gs_er_copy_z(gs_ctx *c, int64_t col0, int64_t col1, double *out, int loc) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        ErState &er = c->er;
        GS_CHECK(er.solved, GS_ESTATE, "gs_er_solve first");
        GS_CHECK(out, GS_EINVAL, "out is NULL");
        GS_CHECK(0 <= col0 && col0 <= col1 && col1 <= er.k, GS_EINVAL, "bad column range");
        GS_CHECK(er_cols_solved(er, col0, col1), GS_ESTATE,
                 "columns [%lld, %lld) were not all solved since gs_er_prepare", (long long)col0,
                 (long long)col1);
        GS_HIP(hipSetDevice(c->device));
        const int64_t nc = col1 - col0;
        if (nc && er.n)
            GS_HIP(hipMemcpy2DAsync(out, sizeof(double) * nc, er.X.as<double>() + col0,
                                    sizeof(double) * er.ld, sizeof(double) * nc, er.n,
                                    loc == GS_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                                    c->stream));
        GS_HIP(hipStreamSynchronize(c->stream));
    });
}

int gs_er_iterations(gs_ctx *c, int32_t *iters, int loc) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        ErState &er = c->er;
        GS_CHECK(er.solved, GS_ESTATE, "gs_er_solve first");
        GS_HIP(hipMemcpyAsync(iters, er.iters.ptr, sizeof(int32_t) * er.k,
                              loc == GS_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                              c->stream));
        GS_HIP(hipStreamSynchronize(c->stream));
    });
}

int gs_er_split(int64_t k, int32_t parts, int64_t *bounds) {
    return guard([&] {
        GS_CHECK(parts >= 1 && (parts & (parts - 1)) == 0, GS_EINVAL, "parts must be a power of 2");
        GS_CHECK(bounds, GS_EINVAL, "bounds is NULL");
        std::vector<int64_t> b = {0, k};
        for (int32_t p = 1; p < parts; p *= 2) {
            std::vector<int64_t> nb = {0};
            for (size_t i = 0; i + 1 < b.size(); ++i) {
                int64_t lo = b[i], len = b[i + 1] - b[i];
                GS_CHECK(len > 128, GS_EINVAL,
                         "k=%lld too small to split %d ways along the pairwise tree",
                         (long long)k, parts);
                int64_t n2 = len / 2;
                n2 -= n2 % 8;
                nb.push_back(lo + n2);
                nb.push_back(b[i + 1]);
            }
            b.swap(nb);
        }
        for (size_t i = 0; i < b.size(); ++i) bounds[i] = b[i];
    });
}

}  // extern "C"