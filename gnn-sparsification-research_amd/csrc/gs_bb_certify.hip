// gs_bb_certify.hip -- the metric backbone's certificates: the 2-hop witness, the
// degree-1 / landmark / local-bound rules, and the stage that runs them over a rank's
// column range (the meet-in-the-middle certificate is gs_bb_mitm.hip's).
#include "gs_bb.hpp"

namespace gs {

// 2-hop witness. state: 0 = unresolved, 1 = keep, 2 = prune.
// Columns [c0, c1) only (the staged multi-rank form splits them in ranges; the rest
// keep their state).  Pair form (nparts > 1): only the columns of this part
// (bb_col_part) are decided here: the other parts' columns are marked 3 and never
// decided by this part (k_bb_need, k_bb_keep).
// With the local bounds (mw != null; k_bb_certify has pruned every column heavier than
// its own G edge + eps): a column the 2-hop paths do not prune is kept when
// w <= LB (1 - 2m), LB = min(W2, max(Au' + mv', mu' + Av'), Au' + Av') -- W2 the least
// 2-edge fold (+inf: no common neighbour), mu' / mv' the least other edge weights of
// u / v, Au' = min over u's other neighbours a of w_ua + (a's least edge weight but
// (a, u)) (k_bb_minw2): a 3-edge path u-a-b-v is at least Au' + w_bv >= Au' + mv' and
// at least mu' + Av'; a longer one's first two and last two edges are distinct,
// >= Au' + Av'.  (R-MAT-15: 93.5 % of the kept columns certified, 66 % by mu' + mv'.)
__global__ void k_bb_witness(const int64_t *__restrict__ src, const int64_t *__restrict__ dst,
                             const double *__restrict__ w, int64_t c0, int64_t c1,
                             const int64_t *__restrict__ gp, const int32_t *__restrict__ gi,
                             const double *__restrict__ gw, double eps, int part, int nparts,
                             const double *__restrict__ mw, const int32_t *__restrict__ ma,
                             const double *__restrict__ aw, const int32_t *__restrict__ aa,
                             double m, uint8_t *__restrict__ state, uint8_t *__restrict__ why) {
    for (int64_t i = c0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < c1;
         i += (int64_t)gridDim.x * blockDim.x) {
        int64_t u = src[i], v = dst[i];
        if (nparts > 1 && bb_col_part(u, v, nparts) != part) {
            state[i] = 3;  // another part's column: not decided here
            continue;
        }
        if (state[i] != 0) continue;  // decided by k_bb_certify (it runs first)
        double wi = w[i];
        if (u == v) {  // d(u,u) = 0
            bb_set(state, why, i, (wi <= 0.0 + eps) ? 1 : 2, kWhySelf);
            continue;
        }
        int64_t a = gp[u], ae = gp[u + 1], b = gp[v], be = gp[v + 1];
        uint8_t st = 0, cls = kWhyOpen;
        double w2 = __builtin_inf();
        if (a == ae || b == be) {
            st = 1;  // u or v isolated in G: unreachable, d = inf -> keep
            cls = kWhyIsolated;
        } else {
            while (a < ae && b < be) {
                int32_t x = gi[a], y = gi[b];
                if (x == y) {
                    double path = gw[a] + gw[b];  // fl(fl(0 + w_ux) + w_xv)
                    if (wi > path + eps) {
                        st = 2;
                        cls = kWhyWitness;
                        break;
                    }
                    w2 = path < w2 ? path : w2;
                    ++a;
                    ++b;
                } else if (x < y) {
                    ++a;
                } else {
                    ++b;
                }
            }
            if (st == 0 && aw) {
                const double mu = ma[u] == (int32_t)v ? mw[2 * u + 1] : mw[2 * u];
                const double mv = ma[v] == (int32_t)u ? mw[2 * v + 1] : mw[2 * v];
                const double au = aa[u] == (int32_t)v ? aw[2 * u + 1] : aw[2 * u];
                const double av = aa[v] == (int32_t)u ? aw[2 * v + 1] : aw[2 * v];
                const double l3a = au + mv, l3b = mu + av, l3 = l3a > l3b ? l3a : l3b, l4 = au + av;
                double lb = w2 < l3 ? w2 : l3;
                lb = lb < l4 ? lb : l4;
                if (wi <= lb * (1.0 - 2.0 * m)) {
                    st = 1;
                    cls = kWhyLocal34;
                }
            }
        }
        state[i] = st;
        if (why && st) why[i] = cls;
    }
}

// Certificates for unresolved columns (state 0), each implying the exact
// comparison w <= fl(d + eps) the reference makes (d = the fl left-fold
// Dijkstra distance; fl sums of <= 2^31 terms are within 1e-9 relative of the
// exact path sums, which the margins below absorb):
//  * an endpoint of degree 1 in G whose only neighbour is the other one: every
//    path starts or ends with that edge, so d = w_G(u,v) exactly;
//  * landmark upper bound: the walk u -> l -> v has fold <= (D_l(u)+D_l(v))(1+m),
//    so w > fl(that + eps) proves w > fl(d + eps): prune;
//  * landmark lower bound: d >= |D_l(u)-D_l(v)| - m (D_l(u)+D_l(v)), so
//    w <= that proves w <= d <= fl(d + eps): keep; D_l(u) finite with D_l(v)
//    infinite (or the reverse) means u and v are disconnected: d = inf, keep.
//  * local bounds (mw != null): every u-v path but the edge itself starts with
//    another edge of u and ends with another edge of v, so its fold is at least
//    LB = fl(mu' + mv') (1 - 2m), mu' / mv' the least weights of u's / v's other
//    G edges (+inf: none).  With the edge in G (weight w_G, d <= w_G):
//    w > fl(w_G + eps) proves w > fl(d + eps): prune; else w <= LB proves
//    w <= fl(d + eps) whichever path is shortest: keep.  Without it every path is
//    another one: w <= LB keeps.  (A column whose endpoint's edges all cost far more
//    than the column -- the Jaccard-0 edges of R-MAT -- is kept here instead of by a
//    search exhausting the giant component.)
// m = max(1e-8, 8 n 2^-53) bounds the relative rounding of folds over simple
// paths (< n terms each, two of them per walk).
// per node of G: its least edge weight mw[2x] and the second least mw[2x + 1] (equal
// when tied, +inf when missing), ma[x] the neighbour of the least; one wave per node
__global__ void k_bb_minw(const int64_t *__restrict__ gp, const int32_t *__restrict__ gi,
                          const double *__restrict__ gw, int64_t n, double *__restrict__ mw,
                          int32_t *__restrict__ ma) {
    const int lane = threadIdx.x & 63;
    const int64_t w0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const double inf = __builtin_inf();
    for (int64_t x = w0; x < n; x += nw) {
        double m1 = inf, m2 = inf;
        int32_t a1 = 0x7fffffff;
        for (int64_t e = gp[x] + lane; e < gp[x + 1]; e += 64) {
            const double we = gw[e];
            const int32_t y = gi[e];
            if (we < m1 || (we == m1 && y < a1)) {
                m2 = m1;
                m1 = we;
                a1 = y;
            } else if (we < m2) {
                m2 = we;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {  // merge the lanes' (least, neighbour, second)
            const double o1 = __shfl_xor(m1, off, 64), o2 = __shfl_xor(m2, off, 64);
            const int32_t oa = __shfl_xor(a1, off, 64);
            if (o1 < m1 || (o1 == m1 && oa < a1)) {
                m2 = m1 < o2 ? m1 : o2;
                m1 = o1;
                a1 = oa;
            } else {
                m2 = o1 < m2 ? o1 : m2;
            }
        }
        if (lane == 0) {
            mw[2 * x] = m1;
            mw[2 * x + 1] = m2;
            ma[x] = a1;
        }
    }
}

// per node u: the least of w_ua + (a's least edge weight but (a, u)) over u's neighbours
// a, aw[2u], its a in aa[u], the second least aw[2u + 1] (k_bb_witness's 3-edge bound);
// one wave per node
__global__ void k_bb_minw2(const int64_t *__restrict__ gp, const int32_t *__restrict__ gi,
                           const double *__restrict__ gw, int64_t n, const double *__restrict__ mw,
                           const int32_t *__restrict__ ma, double *__restrict__ aw,
                           int32_t *__restrict__ aa) {
    const int lane = threadIdx.x & 63;
    const int64_t w0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const double inf = __builtin_inf();
    for (int64_t x = w0; x < n; x += nw) {
        double m1 = inf, m2 = inf;
        int32_t a1 = 0x7fffffff;
        for (int64_t e = gp[x] + lane; e < gp[x + 1]; e += 64) {
            const int32_t y = gi[e];
            const double ve = gw[e] + (ma[y] == (int32_t)x ? mw[2 * y + 1] : mw[2 * y]);
            if (ve < m1 || (ve == m1 && y < a1)) {
                m2 = m1;
                m1 = ve;
                a1 = y;
            } else if (ve < m2) {
                m2 = ve;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double o1 = __shfl_xor(m1, off, 64), o2 = __shfl_xor(m2, off, 64);
            const int32_t oa = __shfl_xor(a1, off, 64);
            if (o1 < m1 || (o1 == m1 && oa < a1)) {
                m2 = m1 < o2 ? m1 : o2;
                m1 = o1;
                a1 = oa;
            } else {
                m2 = o1 < m2 ? o1 : m2;
            }
        }
        if (lane == 0) {
            aw[2 * x] = m1;
            aw[2 * x + 1] = m2;
            aa[x] = a1;
        }
    }
}

__global__ void k_bb_certify(const int64_t *__restrict__ src, const int64_t *__restrict__ dst,
                             const double *__restrict__ w, int64_t c0, int64_t c1,
                             const int64_t *__restrict__ gp, const int32_t *__restrict__ gi,
                             const double *__restrict__ gw, const double *__restrict__ D,
                             const int32_t *__restrict__ complete, int K, double eps, double m,
                             const double *__restrict__ mw, const int32_t *__restrict__ ma,
                             int part, int nparts, uint8_t *__restrict__ state,
                             uint8_t *__restrict__ why) {
    for (int64_t i = c0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < c1;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (state[i] != 0) continue;  // decided, or another part's column (3)
        const int64_t u = src[i], v = dst[i];
        // another part's column (pair form) and self-loops: k_bb_witness's
        if (u == v || (nparts > 1 && bb_col_part(u, v, nparts) != part)) continue;
        const double wi = w[i];
        const int64_t du = gp[u + 1] - gp[u], dv = gp[v + 1] - gp[v];
        if ((du == 1 && gi[gp[u]] == v) || (dv == 1 && gi[gp[v]] == u)) {
            const double wg = du == 1 && gi[gp[u]] == v ? gw[gp[u]] : gw[gp[v]];
            bb_set(state, why, i, (wi <= wg + eps) ? 1 : 2, kWhyDeg1);  // d = fl(0 + w_G) = w_G
            continue;
        }
        if (mw) {
            // w_G(u, v): v in the shorter of the two (sorted, symmetric) lists
            const bool us = du <= dv;
            int64_t lo = us ? gp[u] : gp[v], hi = us ? gp[u + 1] : gp[v + 1];
            const int32_t key = (int32_t)(us ? v : u);
            const int64_t end = hi;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (gi[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            const bool has = lo < end && gi[lo] == key;
            const double mu = ma[u] == (int32_t)v ? mw[2 * u + 1] : mw[2 * u];
            const double mv = ma[v] == (int32_t)u ? mw[2 * v + 1] : mw[2 * v];
            const double lb = (mu + mv) * (1.0 - 2.0 * m);  // +inf when either is missing
            if (has && wi > gw[lo] + eps) {
                bb_set(state, why, i, 2, kWhyDirect);
                continue;
            }
            if (wi <= lb) {
                bb_set(state, why, i, 1, kWhyLocal2);
                continue;
            }
        }
        uint8_t st = 0, cls = kWhyOpen;
        for (int l = 0; l < K && !st; ++l) {
            const double a = D[u * K + l], b = D[v * K + l];
            const bool fa = a != __builtin_inf(), fb = b != __builtin_inf();
            const bool exact = complete[l] != 0;  // else D holds upper bounds only
            if (fa != fb) {
                if (exact) {
                    st = 1;  // different components
                    cls = kWhyLmComp;
                }
            } else if (fa) {
                const double ub = (a + b) * (1.0 + m);
                if (wi > ub + eps) {
                    st = 2;
                    cls = kWhyLmPrune;
                } else if (exact) {
                    const double hi = a > b ? a : b, lo = a > b ? b : a;
                    const double lb = (hi - lo) - m * (hi + lo);
                    if (wi <= lb) {
                        st = 1;
                        cls = kWhyLmKeep;
                    }
                }
            }
        }
        state[i] = st;
        if (why && st) why[i] = cls;
    }
}

// witness + certificates of columns [E part / nparts, E (part + 1) / nparts)
void bb_certify(gs_ctx *c, int part, int nparts) {
    BbRun &R = bb_run(c);
    GS_CHECK(R.begun, GS_ESTATE, "gs_bb_begin first");
    GS_CHECK(nparts >= 1 && 0 <= part && part < nparts, GS_EINVAL, "bad part %d of %d", part, nparts);
    GS_HIP(hipSetDevice(c->device));
    const BbKnobs knobs = bb_knobs();
    hipStream_t s = c->stream;
    const int64_t E = R.E, c0 = E * part / nparts, c1 = E * (part + 1) / nparts;
    hipEvent_t tp = prof_begin(c);
    if (c1 > c0) {
        // the certificates first (landmarks, local bounds: O(K) / O(log d) per column), then
        // the 2-hop witnesses of the columns still open -- a merge of both endpoints'
        // lists, which the hub-hub columns the landmark labels decide made the dearest
        // local bounds (k_bb_certify; GSPARSE_BB_LOCALLB=0: off)
        const bool local = knobs.locallb;
        double *mw = nullptr, *aw = nullptr;
        int32_t *ma = nullptr, *aa = nullptr;
        if (local && R.n > 0) {
            mw = (double *)c->buf("bb_minw").ensure(16 * (size_t)R.n);
            ma = (int32_t *)c->buf("bb_mina").ensure(4 * (size_t)R.n);
            k_bb_minw<<<grid_for(R.n * 64, 256, 16384), 256, 0, s>>>(R.gp, R.gi, R.gw, R.n, mw, ma);
            aw = (double *)c->buf("bb_minw2").ensure(16 * (size_t)R.n);
            aa = (int32_t *)c->buf("bb_mina2").ensure(4 * (size_t)R.n);
            k_bb_minw2<<<grid_for(R.n * 64, 256, 16384), 256, 0, s>>>(R.gp, R.gi, R.gw, R.n, mw, ma, aw, aa);
        }
        if (R.K > 0 || local) {
            k_bb_certify<<<grid_for(c1 - c0, 256, 8192), 256, 0, s>>>(R.dsrc, R.ddst, R.dw, c0, c1, R.gp,
                                                                       R.gi, R.gw, R.D, R.lcomp, R.K,
                                                                       R.eps, R.mrg, mw, ma, R.pair_part,
                                                                       R.pair_nparts, R.state, R.why);
        }
        k_bb_witness<<<grid_for(c1 - c0, 256, 8192), 256, 0, s>>>(
            R.dsrc, R.ddst, R.dw, c0, c1, R.gp, R.gi, R.gw, R.eps, R.pair_part, R.pair_nparts, mw, ma,
            aw, aa, R.mrg, R.state, R.why);
        // the meet-in-the-middle certificate of the columns still open (k_bb_sssp_multi
        // PAIR: both ends searched to half the column's weight; GSPARSE_BB_MITM=1: on).
        // It needs the local bounds' direct-edge rule, so it runs only with them.  Off by
        // default: on R-MAT-18 it decides all but 202 of the 204 k open columns, but the
        // balls of radius ~9 around their (hub-adjacent) ends already hold ~0.28 E
        // relaxations each -- 1.2·10¹¹ for the 102 k pairs, 3.3 s against 0.38 s for the
        // searches it replaces (profiles/r05z10_*).
        if (knobs.mitm && local) bb_mitm(c, R, knobs, c0, c1, part, nparts);
        GS_HIP(hipGetLastError());
    }
    prof_end(c, tp, "bb_certify", 0.0);
    R.certified = true;
}

}  // namespace gs
