// gs_cg_stream.hip -- the streamed batched CG of ApproxER (cg_plan's modes 0-3):
// every column of the solve advances one iteration per round of launches.
//
// Layout in HBM (row-major n x k, the JL columns contiguous per node):
//   Rr  residual, initialised with Y = B @ R           (metrics.py:275)
//   X   solution, P0/P1 search direction (ping-pong), Q = L_reg p (whole in
//       modes 1-3, else only the leftover rows of each BLAS chunk)
// The k CG solves (metrics.py:284-289, SciPy 1.15 cg recurrence) run as one
// batched iteration.  Short rows (mode 0), two fused kernels per iteration:
//   k_cg_pq : x += fl(alpha_{t-1} p_{t-1}) (deferred x update of the previous
//             iteration); p = beta*p + r (two roundings), neighbours' p
//             recomputed; q = L_reg p (per-row fold from 0.0 in ascending
//             column, products rounded); partial dot(p,q)
//   k_cg_upd: q recomputed from the stored p; r -= fl(alpha q); partial dot(r,r)
// (64 B per entry and iteration).  Long rows (mode 3): k_cg_p_flat (p stream),
// k_spmv (column-block-major SpMV, q stored), k_dot_acc, k_cg_upd<STOREQ>.
// Plus two per-column finish kernels.  Every dot product reproduces
// OpenBLAS ddot (SkylakeX kernel) as np.dot calls it: T thread chunks for
// n > 10000, inside a chunk 32 FMA accumulator chains over rows j, j+32, ...,
// then the 32->16 fold, the optional 16-block, the 4-lane tree and the FMA
// tail (pinned in oracle.c, oracle_ddot).  A lane of k_cg_* owns one
// (column, chunk, residue j) chain: the chain IS the thread's row loop, so
// the reduction costs no extra pass over HBM.
#include "gs_cg.hpp"

namespace gs {

// Iteration t, kernel 1 (after beta_t is known):
//   x += fl(alpha_{t-1} p_{t-1})   for columns whose previous update is pending
//                                  (the x update of SciPy's iteration t-1, moved
//                                  here so the second kernel never touches x or p)
//   p_t = fl(fl(beta_t p_{t-1}) + r_t)  (own row stored; neighbours recomputed)
//   q_t = L_reg p_t (per-row fold from 0.0, ascending column), kept only for the
//         <32 leftover rows the ddot finish needs (qside); chains of dot(p_t, q_t).
template <bool FIRST, int CPL, bool STOREQ, int RU>
__global__ void __launch_bounds__(256) k_cg_pq(CgGeom G, ChunkArg ch,
                                               const int64_t *__restrict__ lp,
                                               const int32_t *__restrict__ li,
                                               const double *__restrict__ lv,
                                               const double *__restrict__ R,
                                               const double *__restrict__ Pold,
                                               double *__restrict__ Pnew, double *__restrict__ X,
                                               double *__restrict__ qside,
                                               double *__restrict__ Q,
                                               const double *__restrict__ rho,
                                               const double *__restrict__ rho_prev,
                                               const double *__restrict__ alpha,
                                               const int32_t *__restrict__ active,
                                               const int32_t *__restrict__ xstep, int32_t it,
                                               double *__restrict__ acc) {
    const CgLane ln = cg_lane<CPL>(G);
    if (!ln.ok) return;
    const int64_t ld = G.ld, c = ln.c;
    bool live[CPL], xp[CPL];
    double beta[CPL], al[CPL];
    bool any_live = false, any_x = false;
#pragma unroll
    for (int u = 0; u < CPL; ++u) {
        const bool in = (c + u) < G.col1;
        live[u] = in && active[c + u];
        xp[u] = !FIRST && in && xstep[c + u] == it - 1;
        beta[u] = (!FIRST && live[u]) ? rho[c + u] / rho_prev[c + u] : 0.0;
        al[u] = xp[u] ? alpha[c + u] : 0.0;
        any_live = any_live || live[u];
        any_x = any_x || xp[u];
    }
    if (!any_live && !any_x) return;
    const int64_t a = ch.a[ln.t], L = ch.len[ln.t];
    const int64_t n1 = L & ~(int64_t)15, n32 = n1 & ~(int64_t)31;
    double s[CPL];
#pragma unroll
    for (int u = 0; u < CPL; ++u) s[u] = 0.0;

    // RU rows of the chain per trip (rows ok[i]; ok[0] always holds).  The trip
    // is branch-free up to the stores: absent rows and entries past a row's
    // end load from valid addresses (row[0], the row's last entry) and are
    // masked by selects, so every load of a step is in flight at once.
    auto rows_pq = [&](const int64_t *row, const bool *ok, double (*pi)[CPL], double (*q)[CPL]) {
        int64_t rc[RU];
#pragma unroll
        for (int i = 0; i < RU; ++i) rc[i] = ok[i] ? row[i] : row[0];
        Vec<CPL> po[RU], xv[RU];
        if (!FIRST && any_x) {
#pragma unroll
            for (int i = 0; i < RU; ++i) {
                po[i].load(Pold + rc[i] * ld + c);
                xv[i].load(X + rc[i] * ld + c);
            }
        }
        int64_t e0[RU], len[RU], maxlen = 0;
        bool found[RU];
#pragma unroll
        for (int i = 0; i < RU; ++i) {
            e0[i] = lp[rc[i]];
            const int64_t e1 = lp[rc[i] + 1];  // unconditional: keeps the loads of all rows in flight
            len[i] = ok[i] ? e1 - e0[i] : 0;
            maxlen = len[i] > maxlen ? len[i] : maxlen;
            found[i] = false;
#pragma unroll
            for (int u = 0; u < CPL; ++u) {
                q[i][u] = 0.0;
                pi[i][u] = 0.0;
            }
        }
        if (!any_live) maxlen = 0;
        for (int64_t k = 0; k < maxlen; ++k) {
            int32_t col[RU];
            double w[RU];
            Vec<CPL> rv[RU], pv[RU];
#pragma unroll
            for (int i = 0; i < RU; ++i) {
                const int64_t kk = k < len[i] ? k : (len[i] > 0 ? len[i] - 1 : 0);
                col[i] = li[e0[i] + kk];
                w[i] = lv[e0[i] + kk];
            }
#pragma unroll
            for (int i = 0; i < RU; ++i) {
                rv[i].load(R + col[i] * ld + c);
                if (!FIRST) pv[i].load(Pold + col[i] * ld + c);
            }
#pragma unroll
            for (int i = 0; i < RU; ++i) {
                const bool act = k < len[i];
                const bool diag = act && col[i] == row[i];
#pragma unroll
                for (int u = 0; u < CPL; ++u) {
                    double pn;
                    if (FIRST) {
                        pn = rv[i].v[u];
                    } else {
                        double pb = pv[i].v[u] * beta[u];
                        pn = pb + rv[i].v[u];
                    }
                    pi[i][u] = diag ? pn : pi[i][u];
                    double prod = w[i] * pn;
                    double qn = q[i][u] + prod;
                    q[i][u] = act ? qn : q[i][u];
                }
                found[i] = found[i] || diag;
            }
        }
        if (!FIRST && any_x) {
#pragma unroll
            for (int i = 0; i < RU; ++i)
                if (ok[i]) {
#pragma unroll
                    for (int u = 0; u < CPL; ++u)
                        if (xp[u]) {
                            double t1 = al[u] * po[i].v[u];
                            xv[i].v[u] = xv[i].v[u] + t1;
                        }
                    xv[i].store(X + row[i] * ld + c);
                }
        }
        if (!any_live) return;
#pragma unroll
        for (int i = 0; i < RU; ++i) {
            if (!ok[i]) continue;
            if (!found[i]) {  // L_reg_ii dropped (== 0): p_i still needed
                Vec<CPL> rv, pv;
                rv.load(R + row[i] * ld + c);
                if (!FIRST) pv.load(Pold + row[i] * ld + c);
#pragma unroll
                for (int u = 0; u < CPL; ++u) {
                    if (FIRST) {
                        pi[i][u] = rv.v[u];
                    } else {
                        double pb = pv.v[u] * beta[u];
                        pi[i][u] = pb + rv.v[u];
                    }
                }
            }
            const int64_t o = row[i] * ld + c;
            Vec<CPL> pw;
#pragma unroll
            for (int u = 0; u < CPL; ++u) pw.v[u] = live[u] ? pi[i][u] : 0.0;
            // columns that are not live keep their last p (the flush may need it)
            if (CPL == 1 || (live[0] && live[CPL - 1])) {
                pw.store(Pnew + o);
            } else {
#pragma unroll
                for (int u = 0; u < CPL; ++u)
                    if (live[u]) Pnew[o + u] = pi[i][u];
            }
            if (STOREQ) {  // q kept, the update kernel streams it
                Vec<CPL> qw;
#pragma unroll
                for (int u = 0; u < CPL; ++u) qw.v[u] = q[i][u];
                if (CPL == 1 || (live[0] && live[CPL - 1])) {
                    qw.store(Q + o);
                } else {
#pragma unroll
                    for (int u = 0; u < CPL; ++u)
                        if (live[u]) Q[o + u] = q[i][u];
                }
            }
        }
    };

    for (int64_t base = a + ln.j; base < a + n32; base += 32 * RU) {
        int64_t row[RU];
        bool ok[RU];
#pragma unroll
        for (int i = 0; i < RU; ++i) {
            row[i] = base + 32 * i;
            ok[i] = row[i] < a + n32;
        }
        double pi[RU][CPL], q[RU][CPL];
        rows_pq(row, ok, pi, q);
#pragma unroll
        for (int i = 0; i < RU; ++i)
            if (ok[i])
#pragma unroll
                for (int u = 0; u < CPL; ++u) s[u] = __builtin_fma(pi[i][u], q[i][u], s[u]);
    }
    {  // leftover rows of the chunk (16-block + tail): q kept for the finish
        int64_t row[RU];
        bool ok[RU];
#pragma unroll
        for (int i = 0; i < RU; ++i) {
            row[i] = a + n32 + ln.j;
            ok[i] = i == 0 && row[i] < a + L;
        }
        if (ok[0]) {
            double pi[RU][CPL], q[RU][CPL];
            rows_pq(row, ok, pi, q);
            if (!STOREQ && any_live) {
                double *qs = qside + ((int64_t)ln.t * 32 + ln.j) * ld + c;
#pragma unroll
                for (int u = 0; u < CPL; ++u)
                    if (live[u]) qs[u] = q[0][u];
            }
        }
    }
    if (any_live) {
#pragma unroll
        for (int u = 0; u < CPL; ++u)
            if (live[u]) acc[((c + u - G.col0) * kMaxChunks + ln.t) * 32 + ln.j] = s[u];
    }
}

// Iteration t, kernel 2 (after alpha_t is known):
//   q_t = L_reg p_t recomputed from the stored p_t (same fold, same bits) or
//   read (STOREQ), r_{t+1} = r_t - fl(alpha_t q_t); chains of dot(r_{t+1}, r_{t+1}).
template <int CPL, bool STOREQ, int RU>
__global__ void __launch_bounds__(256) k_cg_upd(CgGeom G, ChunkArg ch,
                                                const int64_t *__restrict__ lp,
                                                const int32_t *__restrict__ li,
                                                const double *__restrict__ lv,
                                                const double *__restrict__ P,
                                                const double *__restrict__ Q,
                                                double *__restrict__ R,
                                                const double *__restrict__ alpha,
                                                const int32_t *__restrict__ active,
                                                double *__restrict__ acc) {
    const CgLane ln = cg_lane<CPL>(G);
    if (!ln.ok) return;
    const int64_t ld = G.ld, c = ln.c;
    double al[CPL];
    bool live[CPL];
    bool any = false;
#pragma unroll
    for (int u = 0; u < CPL; ++u) {
        live[u] = (c + u) < G.col1 && active[c + u];
        al[u] = live[u] ? alpha[c + u] : 0.0;
        any = any || live[u];
    }
    if (!any) return;
    const int64_t a = ch.a[ln.t], L = ch.len[ln.t];
    const int64_t n1 = L & ~(int64_t)15, n32 = n1 & ~(int64_t)31;
    double s[CPL];
#pragma unroll
    for (int u = 0; u < CPL; ++u) s[u] = 0.0;
    auto rows_upd = [&](const int64_t *row, const bool *ok, Vec<CPL> *rv) {
        double q[RU][CPL];
        int64_t rc[RU], e0[RU], len[RU], maxlen = 0;
#pragma unroll
        for (int i = 0; i < RU; ++i) {
            rc[i] = ok[i] ? row[i] : row[0];
            rv[i].load(R + rc[i] * ld + c);
#pragma unroll
            for (int u = 0; u < CPL; ++u) q[i][u] = 0.0;
            if (STOREQ) {
                Vec<CPL> qv;
                qv.load(Q + rc[i] * ld + c);
#pragma unroll
                for (int u = 0; u < CPL; ++u) q[i][u] = qv.v[u];
            }
            e0[i] = STOREQ ? 0 : lp[rc[i]];
            const int64_t e1 = STOREQ ? 0 : lp[rc[i] + 1];
            len[i] = (!STOREQ && ok[i]) ? e1 - e0[i] : 0;
            maxlen = len[i] > maxlen ? len[i] : maxlen;
        }
        for (int64_t k = 0; k < maxlen; ++k) {
            double w[RU];
            Vec<CPL> pv[RU];
#pragma unroll
            for (int i = 0; i < RU; ++i) {
                const int64_t kk = k < len[i] ? k : (len[i] > 0 ? len[i] - 1 : 0);
                const int32_t col = li[e0[i] + kk];
                w[i] = lv[e0[i] + kk];
                pv[i].load(P + col * ld + c);
            }
#pragma unroll
            for (int i = 0; i < RU; ++i) {
                const bool act = k < len[i];
#pragma unroll
                for (int u = 0; u < CPL; ++u) {
                    double prod = w[i] * pv[i].v[u];
                    double qn = q[i][u] + prod;
                    q[i][u] = act ? qn : q[i][u];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < RU; ++i)
            if (ok[i]) {
#pragma unroll
                for (int u = 0; u < CPL; ++u) {
                    double t2 = al[u] * q[i][u];
                    rv[i].v[u] = live[u] ? rv[i].v[u] - t2 : rv[i].v[u];
                }
                rv[i].store(R + row[i] * ld + c);
            }
    };
    for (int64_t base = a + ln.j; base < a + n32; base += 32 * RU) {
        int64_t row[RU];
        bool ok[RU];
#pragma unroll
        for (int i = 0; i < RU; ++i) {
            row[i] = base + 32 * i;
            ok[i] = row[i] < a + n32;
        }
        Vec<CPL> rv[RU];
        rows_upd(row, ok, rv);
#pragma unroll
        for (int i = 0; i < RU; ++i)
            if (ok[i])
#pragma unroll
                for (int u = 0; u < CPL; ++u) s[u] = __builtin_fma(rv[i].v[u], rv[i].v[u], s[u]);
    }
    {
        int64_t row[RU];
        bool ok[RU];
#pragma unroll
        for (int i = 0; i < RU; ++i) {
            row[i] = a + n32 + ln.j;
            ok[i] = i == 0 && row[i] < a + L;
        }
        if (ok[0]) {
            Vec<CPL> rv[RU];
            rows_upd(row, ok, rv);
        }
    }
#pragma unroll
    for (int u = 0; u < CPL; ++u)
        if (live[u]) acc[((c + u - G.col0) * kMaxChunks + ln.t) * 32 + ln.j] = s[u];
}

// Split modes (rows with many entries, where recomputing a neighbour's p costs
// two gathers, or few columns, where the chains give too few waves):
//   k_cg_p_flat : x += fl(alpha_{t-1} p_{t-1}) (pending columns); p_t = fl(fl(beta p) + r)
//   k_cg_q (mode 2) : q_t = L_reg p_t (gathers of the stored p), q stored, dot(p, q) chains
//   k_spmv + k_dot_acc (mode 3) : the same, SpMV in column-block-major order
//   k_cg_upd<STOREQ> : r -= fl(alpha q) streaming q
// The p update has no reduction, so it streams flat: threads own a column pair
// (16 B, flags loaded once), blockIdx.y a band of kFlatRows rows, rows
// walked in order -- each wave reads 1 KB contiguous per row.
static constexpr int kFlatRows = 16;

template <bool FIRST>
__global__ void __launch_bounds__(256) k_cg_p_flat(CgGeom G, const double *__restrict__ R,
                                                   const double *__restrict__ Pold,
                                                   double *__restrict__ Pnew,
                                                   double *__restrict__ X,
                                                   const double *__restrict__ rho,
                                                   const double *__restrict__ rho_prev,
                                                   const double *__restrict__ alpha,
                                                   const int32_t *__restrict__ active,
                                                   const int32_t *__restrict__ xstep, int32_t it) {
    const int64_t c = G.col0 + 2 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= G.col1) return;
    bool live[2], xp[2];
    double beta[2], al[2];
    bool any_live = false, any_x = false;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const bool in = (c + u) < G.col1;
        live[u] = in && active[c + u];
        xp[u] = !FIRST && in && xstep[c + u] == it - 1;
        beta[u] = (!FIRST && live[u]) ? rho[c + u] / rho_prev[c + u] : 0.0;
        al[u] = xp[u] ? alpha[c + u] : 0.0;
        any_live = any_live || live[u];
        any_x = any_x || xp[u];
    }
    if (!any_live && !any_x) return;
    const int64_t r0 = (int64_t)blockIdx.y * kFlatRows;
    const int64_t r1 = r0 + kFlatRows < G.n ? r0 + kFlatRows : G.n;
    for (int64_t row = r0; row < r1; ++row) {
        const int64_t o = row * G.ld + c;
        Vec<2> po, rv, xv;
        if (!FIRST) po.load(Pold + o);
        if (any_x) xv.load(X + o);
        if (any_live) rv.load(R + o);
        if (any_x) {
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (xp[u]) {
                    double t1 = al[u] * po.v[u];
                    xv.v[u] = xv.v[u] + t1;
                }
            if (xp[0] && xp[1]) xv.store(X + o);
            else
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    if (xp[u]) X[o + u] = xv.v[u];
        }
        if (!any_live) continue;
        Vec<2> pw;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            double pn;
            if (FIRST) {
                pn = rv.v[u];
            } else {
                double pb = po.v[u] * beta[u];
                pn = pb + rv.v[u];
            }
            pw.v[u] = pn;
        }
        if (live[0] && live[1]) pw.store(Pnew + o);
        else
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (live[u]) Pnew[o + u] = pw.v[u];
    }
}

template <int CPL>
__global__ void __launch_bounds__(256) k_cg_q(CgGeom G, ChunkArg ch, const int64_t *__restrict__ lp,
                                              const int32_t *__restrict__ li,
                                              const double *__restrict__ lv,
                                              const double *__restrict__ P,
                                              double *__restrict__ Q,
                                              const int32_t *__restrict__ active,
                                              double *__restrict__ acc) {
    const CgLane ln = cg_lane<CPL>(G);
    if (!ln.ok) return;
    const int64_t ld = G.ld, c = ln.c;
    bool live[CPL];
    bool any = false;
#pragma unroll
    for (int u = 0; u < CPL; ++u) {
        live[u] = (c + u) < G.col1 && active[c + u];
        any = any || live[u];
    }
    if (!any) return;
    const int64_t a = ch.a[ln.t], L = ch.len[ln.t];
    const int64_t n1 = L & ~(int64_t)15, n32 = n1 & ~(int64_t)31;
    double s[CPL];
#pragma unroll
    for (int u = 0; u < CPL; ++u) s[u] = 0.0;
    auto row_q = [&](int64_t row, double *pi, double *q) {
        const int64_t e0 = lp[row], e1 = lp[row + 1];
        bool found = false;
#pragma unroll
        for (int u = 0; u < CPL; ++u) q[u] = 0.0;
        for (int64_t e = e0; e < e1; ++e) {
            const int32_t col = li[e];
            const double w = lv[e];
            Vec<CPL> pv;
            pv.load(P + col * ld + c);
#pragma unroll
            for (int u = 0; u < CPL; ++u) {
                if (col == row) pi[u] = pv.v[u];
                double prod = w * pv.v[u];
                q[u] = q[u] + prod;
            }
            found = found || (col == row);
        }
        if (!found) {  // L_reg_ii dropped (== 0): p_i still needed
            Vec<CPL> pv;
            pv.load(P + row * ld + c);
#pragma unroll
            for (int u = 0; u < CPL; ++u) pi[u] = pv.v[u];
        }
        Vec<CPL> qw;
#pragma unroll
        for (int u = 0; u < CPL; ++u) qw.v[u] = q[u];
        if (CPL == 1 || (live[0] && live[CPL - 1])) {
            qw.store(Q + row * ld + c);
        } else {
#pragma unroll
            for (int u = 0; u < CPL; ++u)
                if (live[u]) Q[row * ld + c + u] = q[u];
        }
    };
    for (int64_t row = a + ln.j; row < a + n32; row += 32) {
        double pi[CPL], q[CPL];
        row_q(row, pi, q);
#pragma unroll
        for (int u = 0; u < CPL; ++u) s[u] = __builtin_fma(pi[u], q[u], s[u]);
    }
    {
        const int64_t row = a + n32 + ln.j;
        if (row < a + L) {
            double pi[CPL], q[CPL];
            row_q(row, pi, q);
        }
    }
#pragma unroll
    for (int u = 0; u < CPL; ++u)
        if (live[u]) acc[((c + u - G.col0) * kMaxChunks + ln.t) * 32 + ln.j] = s[u];
}

// q = L_reg p with no reduction attached, so any row order is allowed: waves
// walk row tiles with the column block as the SLOWEST index, so the blocks in
// flight (n x 64*CPL doubles each) stay resident in the Infinity Cache while
// their rows are gathered.  dot(p, q) then comes from k_dot_acc.
template <int CPL>
__global__ void __launch_bounds__(256) k_spmv(CgGeom G, int64_t rpw, int64_t ntiles,
                                              const int64_t *__restrict__ lp,
                                              const int32_t *__restrict__ li,
                                              const double *__restrict__ lv,
                                              const double *__restrict__ P,
                                              double *__restrict__ Q,
                                              const int32_t *__restrict__ active) {
    const int64_t gw = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t cb = gw / ntiles, tile = gw % ntiles;
    if (cb >= G.ncb) return;
    const int64_t ld = G.ld, c = G.col0 + cb * (64 * CPL) + (int64_t)(threadIdx.x & 63) * CPL;
    bool live[CPL];
    bool any = false;
#pragma unroll
    for (int u = 0; u < CPL; ++u) {
        live[u] = (c + u) < G.col1 && active[c + u];
        any = any || live[u];
    }
    if (!any) return;
    const int64_t r0 = tile * rpw, r1 = r0 + rpw < G.n ? r0 + rpw : G.n;
    for (int64_t row = r0; row < r1; ++row) {
        const int64_t e0 = lp[row], e1 = lp[row + 1];
        double q[CPL];
#pragma unroll
        for (int u = 0; u < CPL; ++u) q[u] = 0.0;
        for (int64_t e = e0; e < e1; ++e) {
            const int32_t col = li[e];
            const double w = lv[e];
            Vec<CPL> pv;
            pv.load(P + col * ld + c);
#pragma unroll
            for (int u = 0; u < CPL; ++u) {
                double prod = w * pv.v[u];
                q[u] = q[u] + prod;
            }
        }
        Vec<CPL> qw;
#pragma unroll
        for (int u = 0; u < CPL; ++u) qw.v[u] = q[u];
        if (CPL == 1 || (live[0] && live[CPL - 1])) {
            qw.store(Q + row * ld + c);
        } else {
#pragma unroll
            for (int u = 0; u < CPL; ++u)
                if (live[u]) Q[row * ld + c + u] = q[u];
        }
    }
}

// after the loop: the x update of the last executed iteration
__global__ void k_x_flush(CgGeom G, const double *__restrict__ P, const double *__restrict__ alpha,
                          const int32_t *__restrict__ xstep, int32_t it_last,
                          double *__restrict__ X) {
    int64_t ncol = G.col1 - G.col0;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < G.n * ncol;
         idx += (int64_t)gridDim.x * blockDim.x) {
        int64_t i = idx / ncol, c = G.col0 + idx % ncol;
        if (xstep[c] != it_last) continue;
        int64_t o = i * G.ld + c;
        double t1 = alpha[c] * P[o];
        X[o] = X[o] + t1;
    }
}

// plain dot accumulation (||b||^2 before the first iteration)
template <int CPL, int RU>
__global__ void __launch_bounds__(256) k_dot_acc(CgGeom G, ChunkArg ch,
                                                 const double *__restrict__ A,
                                                 const double *__restrict__ B,
                                                 double *__restrict__ acc) {
    const CgLane ln = cg_lane<CPL>(G);
    // lanes past the block's last column load nothing (their columns may lie
    // beyond the padded row, and past the buffer on the last row)
    if (!ln.ok || ln.c >= G.col1) return;
    const int64_t ld = G.ld, c = ln.c;
    const int64_t a = ch.a[ln.t], L = ch.len[ln.t];
    const int64_t n1 = L & ~(int64_t)15, n32 = n1 & ~(int64_t)31;
    double s[CPL];
#pragma unroll
    for (int u = 0; u < CPL; ++u) s[u] = 0.0;
    // RU chain rows per trip, loads first (absent rows re-read the first row)
    for (int64_t base = a + ln.j; base < a + n32; base += 32 * RU) {
        Vec<CPL> av[RU], bv[RU];
        bool ok[RU];
#pragma unroll
        for (int i = 0; i < RU; ++i) {
            ok[i] = base + 32 * i < a + n32;
            const int64_t row = ok[i] ? base + 32 * i : base;
            av[i].load(A + row * ld + c);
            bv[i].load(B + row * ld + c);
        }
#pragma unroll
        for (int i = 0; i < RU; ++i)
#pragma unroll
            for (int u = 0; u < CPL; ++u) {
                const double f = __builtin_fma(av[i].v[u], bv[i].v[u], s[u]);
                s[u] = ok[i] ? f : s[u];
            }
    }
#pragma unroll
    for (int u = 0; u < CPL; ++u)
        if (c + u < G.col1) acc[((c + u - G.col0) * kMaxChunks + ln.t) * 32 + ln.j] = s[u];
}

__device__ __noinline__ double ddot_finish_wave(const double *__restrict__ acc_c,
                                                   const int64_t *__restrict__ ca,
                                                   const int64_t *__restrict__ cl, int count,
                                                   int64_t ld, int64_t c,
                                                   const double *__restrict__ A,
                                                   const double *__restrict__ B,
                                                   const double *__restrict__ Bside) {
    return ddot_finish_impl(acc_c, ca, cl, count, ld, c, A, B, Bside);
}

// one wave per column: c = col0 + blockIdx.x * waves + wave
__device__ __forceinline__ int64_t fin_column(const CgGeom &G) {
    return G.col0 + (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
}

// init: rho = b.b, bn = sqrt(rho), atol = rtol*bn; bn == 0 -> done (x = b)
__global__ void __launch_bounds__(256) k_fin_init(CgGeom G, const int64_t *__restrict__ ca,
                                                  const int64_t *__restrict__ cl, int count,
                                                  const double *__restrict__ acc,
                                                  const double *__restrict__ Rr, double rtol,
                                                  double *__restrict__ bn, double *__restrict__ atol,
                                                  double *__restrict__ rho,
                                                  int32_t *__restrict__ active,
                                                  int32_t *__restrict__ iters,
                                                  int32_t *__restrict__ xstep,
                                                  int32_t *__restrict__ nactive) {
    const int64_t c = fin_column(G);
    if (c >= G.col1) return;
    const double d = ddot_finish_wave(acc + (c - G.col0) * kMaxChunks * 32, ca, cl, count, G.ld, c,
                                      Rr, Rr, nullptr);
    if ((threadIdx.x & 63) != 0) return;
    double b = __builtin_sqrt(d);
    bn[c] = b;
    double at = rtol * b;  // max(atol=0, rtol*bnrm2)
    atol[c] = at;
    rho[c] = d;
    iters[c] = 0;
    xstep[c] = -2;
    int act = 1;
    if (b == 0.0) act = 0;                     // cg returns b, info 0
    else if (__builtin_sqrt(d) < at) act = 0;  // converged at loop top, iteration 0
    active[c] = act;
    if (act) atomicAdd(nactive, 1);
}

__global__ void __launch_bounds__(256) k_fin_pq(CgGeom G, const int64_t *__restrict__ ca,
                                                const int64_t *__restrict__ cl, int count,
                                                const double *__restrict__ acc,
                                                const double *__restrict__ P,
                                                const double *__restrict__ Qfull,
                                                const double *__restrict__ qside,
                                                const double *__restrict__ rho,
                                                const int32_t *__restrict__ active, int32_t it,
                                                double *__restrict__ alpha,
                                                int32_t *__restrict__ xstep) {
    const int64_t c = fin_column(G);
    if (c >= G.col1 || !active[c]) return;
    const double pq = ddot_finish_wave(acc + (c - G.col0) * kMaxChunks * 32, ca, cl, count, G.ld,
                                       c, P, Qfull, qside);
    if ((threadIdx.x & 63) != 0) return;
    alpha[c] = rho[c] / pq;
    xstep[c] = it;  // x += alpha p is applied by the next k_cg_pq (or the flush)
}

// after the update of iteration `it`: rho_prev = rho; rho = r.r; loop-top test
__global__ void __launch_bounds__(256) k_fin_rr(CgGeom G, const int64_t *__restrict__ ca,
                                                const int64_t *__restrict__ cl, int count,
                                                const double *__restrict__ acc,
                                                const double *__restrict__ Rr, int32_t it,
                                                double *__restrict__ rho,
                                                double *__restrict__ rho_prev,
                                                const double *__restrict__ atol,
                                                int32_t *__restrict__ active,
                                                int32_t *__restrict__ iters,
                                                int32_t *__restrict__ nactive) {
    const int64_t c = fin_column(G);
    if (c >= G.col1 || !active[c]) return;
    const double rr = ddot_finish_wave(acc + (c - G.col0) * kMaxChunks * 32, ca, cl, count, G.ld,
                                       c, Rr, Rr, nullptr);
    if ((threadIdx.x & 63) != 0) return;
    rho_prev[c] = rho[c];
    rho[c] = rr;
    iters[c] = it + 1;
    if (__builtin_sqrt(rr) < atol[c]) {
        active[c] = 0;
        atomicSub(nactive, 1);
    }
}

// x = b for columns with ||b|| == 0 (cg returns b); zero X elsewhere
__global__ void k_x_init(CgGeom G, const double *__restrict__ Rr, const double *__restrict__ bn,
                         double *__restrict__ X) {
    int64_t ncol = G.col1 - G.col0;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < G.n * ncol;
         idx += (int64_t)gridDim.x * blockDim.x) {
        int64_t i = idx / ncol, c = G.col0 + idx % ncol;
        int64_t o = i * G.ld + c;
        X[o] = (bn[c] == 0.0) ? Rr[o] : 0.0;
    }
}

// ---------------------------------------------------------------- launches
// the fused kernels by (FIRST, CPL, STOREQ) and chain rows per trip
template <bool F, int C, bool S, class... A>
static void pq_ru(int ru, dim3 grid, hipStream_t s, const A &...a) {
    switch (ru) {
    case 1: k_cg_pq<F, C, S, 1><<<grid, 256, 0, s>>>(a...); break;
    case 2: k_cg_pq<F, C, S, 2><<<grid, 256, 0, s>>>(a...); break;
    case 4: k_cg_pq<F, C, S, 4><<<grid, 256, 0, s>>>(a...); break;
    default: k_cg_pq<F, C, S, 8><<<grid, 256, 0, s>>>(a...); break;
    }
}

template <class... A>
static void launch_pq(bool first, int cpl, bool storeq, int ru, dim3 grid, hipStream_t s,
                      const A &...a) {
    switch ((first ? 4 : 0) | (cpl == 2 ? 2 : 0) | (storeq ? 1 : 0)) {
    case 0: pq_ru<false, 1, false>(ru, grid, s, a...); break;
    case 1: pq_ru<false, 1, true>(ru, grid, s, a...); break;
    case 2: pq_ru<false, 2, false>(ru, grid, s, a...); break;
    case 3: pq_ru<false, 2, true>(ru, grid, s, a...); break;
    case 4: pq_ru<true, 1, false>(ru, grid, s, a...); break;
    case 5: pq_ru<true, 1, true>(ru, grid, s, a...); break;
    case 6: pq_ru<true, 2, false>(ru, grid, s, a...); break;
    default: pq_ru<true, 2, true>(ru, grid, s, a...); break;
    }
}

template <int C, bool S, class... A>
static void upd_ru(int ru, dim3 grid, hipStream_t s, const A &...a) {
    switch (ru) {
    case 1: k_cg_upd<C, S, 1><<<grid, 256, 0, s>>>(a...); break;
    case 2: k_cg_upd<C, S, 2><<<grid, 256, 0, s>>>(a...); break;
    case 4: k_cg_upd<C, S, 4><<<grid, 256, 0, s>>>(a...); break;
    default: k_cg_upd<C, S, 8><<<grid, 256, 0, s>>>(a...); break;
    }
}

template <class... A>
static void launch_upd(int cpl, bool storeq, int ru, dim3 grid, hipStream_t s, const A &...a) {
    switch ((cpl == 2 ? 2 : 0) | (storeq ? 1 : 0)) {
    case 0: upd_ru<1, false>(ru, grid, s, a...); break;
    case 1: upd_ru<1, true>(ru, grid, s, a...); break;
    case 2: upd_ru<2, false>(ru, grid, s, a...); break;
    default: upd_ru<2, true>(ru, grid, s, a...); break;
    }
}

void cg_solve_streamed(gs_ctx *c, const CgPlan &plan, int64_t col0, int64_t col1, int32_t maxiter,
                       double rtol) {
    ErState &er = c->er;
    const ChunkArg &ch = plan.ch;
    const int mode = plan.mode, cpl = plan.cpl, ru = plan.ru;
    const bool storeq = plan.storeq;
    const int64_t n = er.n, ncols = col1 - col0;
    CgGeom G;
    G.n = n;
    G.k = er.k;
    G.ld = er.ld;
    G.col0 = col0;
    G.col1 = col1;
    G.ncb = (int32_t)((ncols + 64 * cpl - 1) / (64 * cpl));
    G.npairs = G.ncb * ch.count;
    ColPtrs cp = col_ptrs(er);
    double *X = er.X.as<double>(), *Rr = er.Rr.as<double>();
    double *Qbuf = (double *)er.Q.ensure(
        storeq ? sizeof(double) * (size_t)n * (size_t)er.ld
               : sizeof(double) * (size_t)ch.count * 32 * (size_t)er.ld);
    double *qside = storeq ? nullptr : Qbuf;
    double *Qfull = storeq ? Qbuf : nullptr;
    double *P[2] = {er.P0.as<double>(), er.P1.as<double>()};
    double *acc = er.acc.as<double>();
    // 8 workgroups (32 residues) per (column block, chunk) pair, XCD-grouped
    dim3 grid((unsigned)(((G.npairs + 7) / 8) * 64)), block(256);
    // finish kernels: one wave per column, one lane per BLAS chunk
    const unsigned fgrid = grid_for(ncols, 4);
    const int64_t *ca = chunks_to_device(c, ch), *cl = ca + kMaxChunks;
    // algorithmic bytes, SURVEY 8(d) B_ER: per column and iteration 8 (nnz(L_reg) + 10 n),
    // i.e. one 8-B p read per L_reg entry (the SpMV) + the vector streams.  Attributed
    // to the kernel that does each part: pq reads x, p, r and writes x, p (first
    // iteration: r in, p out) and performs the SpMV (+ q written when stored); upd
    // reads p (or q), r and writes r (its q recompute is not counted again)
    const double qb = storeq ? 8.0 : 0.0;
    const double lnz = (double)er.lnnz;
    const double bytes_pq = ((40.0 + qb) * n + 8.0 * lnz) * ncols,
                 bytes_pq0 = ((16.0 + qb) * n + 8.0 * lnz) * ncols,
                 bytes_upd = 24.0 * n * ncols;
    const int64_t *lp = er.lp.as<int64_t>();
    const int32_t *li = er.li.as<int32_t>();
    const double *lv = er.lv.as<double>();
    GS_HIP(hipMemsetAsync(cp.nactive, 0, sizeof(int32_t), c->stream));
    // ||b|| and rho_0 (r = b.copy())
    if (cpl == 2) k_dot_acc<2, 4><<<grid, block, 0, c->stream>>>(G, ch, Rr, Rr, acc);
    else k_dot_acc<1, 4><<<grid, block, 0, c->stream>>>(G, ch, Rr, Rr, acc);
    k_fin_init<<<fgrid, 256, 0, c->stream>>>(G, ca, cl, ch.count, acc, Rr, rtol, cp.bn,
                                              cp.atol, cp.rho, cp.active, cp.iters, cp.xstep,
                                              cp.nactive);
    if (n)
        k_x_init<<<grid_for(n * ncols, 256, 65536), 256, 0, c->stream>>>(G, Rr, cp.bn, X);
    GS_HIP(hipGetLastError());
    int cur = 0;
    int32_t it_last = -1;
    for (int32_t it = 0; it < maxiter; ++it) {
        if (it % 8 == 0) {
            int32_t na = 0;
            GS_HIP(hipMemcpyAsync(&na, cp.nactive, sizeof(int32_t), hipMemcpyDeviceToHost,
                                  c->stream));
            GS_HIP(hipStreamSynchronize(c->stream));
            if (na == 0) break;
        }
        double *Pold = P[cur], *Pnew = P[cur ^ 1];
        hipEvent_t t0 = prof_begin(c);
        if (mode >= 2) {
            const dim3 pg((unsigned)(((ncols + 1) / 2 + 255) / 256),
                          (unsigned)((n + kFlatRows - 1) / kFlatRows));
            if (it == 0)
                k_cg_p_flat<true><<<pg, 256, 0, c->stream>>>(G, Rr, Pold, Pnew, X, cp.rho,
                                                             cp.rho_prev, cp.alpha, cp.active,
                                                             cp.xstep, it);
            else
                k_cg_p_flat<false><<<pg, 256, 0, c->stream>>>(G, Rr, Pold, Pnew, X, cp.rho,
                                                              cp.rho_prev, cp.alpha, cp.active,
                                                              cp.xstep, it);
            prof_end(c, t0, "cg_p", (it == 0 ? 16.0 : 40.0) * n * ncols);
            t0 = prof_begin(c);
            if (mode == 2) {
                if (cpl == 2)
                    k_cg_q<2><<<grid, block, 0, c->stream>>>(G, ch, lp, li, lv, Pnew, Qfull, cp.active, acc);
                else
                    k_cg_q<1><<<grid, block, 0, c->stream>>>(G, ch, lp, li, lv, Pnew, Qfull, cp.active, acc);
                prof_end(c, t0, "cg_q", (24.0 * n + 8.0 * lnz) * ncols);
            } else {
                // 4 rows per wave, 128 columns: best of {1..64} x {64, 128} on ogbn-arxiv size
                const int64_t rpw = 4;
                const int scpl = 2;
                CgGeom GS = G;
                GS.ncb = (int32_t)((ncols + 64 * scpl - 1) / (64 * scpl));
                const int64_t ntiles = (n + rpw - 1) / rpw;
                const unsigned sg = (unsigned)((GS.ncb * ntiles + 3) / 4);
                if (scpl == 2)
                    k_spmv<2><<<sg, 256, 0, c->stream>>>(GS, rpw, ntiles, lp, li, lv, Pnew, Qfull, cp.active);
                else
                    k_spmv<1><<<sg, 256, 0, c->stream>>>(GS, rpw, ntiles, lp, li, lv, Pnew, Qfull, cp.active);
                prof_end(c, t0, "cg_spmv", (8.0 * n + 8.0 * lnz) * ncols);
                t0 = prof_begin(c);
                if (cpl == 2) k_dot_acc<2, 4><<<grid, block, 0, c->stream>>>(G, ch, Pnew, Qfull, acc);
                else k_dot_acc<1, 4><<<grid, block, 0, c->stream>>>(G, ch, Pnew, Qfull, acc);
                prof_end(c, t0, "cg_dot", 16.0 * n * ncols);
            }
        } else {
            launch_pq(it == 0, cpl, storeq, ru, grid, c->stream, G, ch, lp, li, lv, Rr, Pold, Pnew,
                      X, qside, Qfull, cp.rho, cp.rho_prev, cp.alpha, cp.active, cp.xstep, it, acc);
            prof_end(c, t0, "cg_pq", it == 0 ? bytes_pq0 : bytes_pq);
        }
        k_fin_pq<<<fgrid, 256, 0, c->stream>>>(G, ca, cl, ch.count, acc, Pnew, Qfull, qside, cp.rho,
                                               cp.active, it, cp.alpha, cp.xstep);
        t0 = prof_begin(c);
        launch_upd(cpl, storeq, ru, grid, c->stream, G, ch, lp, li, lv, Pnew, Qfull, Rr, cp.alpha,
                   cp.active, acc);
        prof_end(c, t0, "cg_upd", bytes_upd);
        k_fin_rr<<<fgrid, 256, 0, c->stream>>>(G, ca, cl, ch.count, acc, Rr, it, cp.rho,
                                               cp.rho_prev, cp.atol,
                                              cp.active, cp.iters, cp.nactive);
        GS_HIP(hipGetLastError());
        cur ^= 1;
        it_last = it;
    }
    // the x update of the last executed iteration (P[cur] holds its p)
    if (it_last >= 0 && n)
        k_x_flush<<<grid_for(n * ncols, 256, 65536), 256, 0, c->stream>>>(G, P[cur], cp.alpha,
                                                                          cp.xstep, it_last, X);
    GS_HIP(hipGetLastError());
    er.pcur = cur;
}

}  // namespace gs
