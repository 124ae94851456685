// gs_bb_multi.hpp -- k_bb_sssp_multi, the metric backbone's S-sources-per-workgroup
// search, and what only it uses.  Included by the units that instantiate it:
// gs_bb_search.hip (the 12 search forms) and gs_bb_mitm.hip (the PAIR form).
#pragma once

#include "gs_bb.hpp"

namespace gs {

// k_bb_sssp_multi's per-node mask: bits 0-7 the sources queued in the next frontier,
// 8-15 the sources for which the node waits in the far pile, 30 the node is in the
// far list, 31 in the reset list
static constexpr uint32_t kQMaskTouched = 0x80000000u;
static constexpr uint32_t kQMaskFarListed = 0x40000000u;
static constexpr uint32_t kQMaskSources = 0xffu;
static constexpr int kQMaskFarShift = 8;
// k_bb_sssp_multi: frontier nodes with more entries than this are expanded by the
// whole workgroup (at most kBbHeavyMax of them per round; the rest as usual)
#ifndef GS_BB_HEAVY
#define GS_BB_HEAVY 1024
#endif
static constexpr int64_t kBbHeavy = GS_BB_HEAVY;
static constexpr int kBbHeavyMax = 256;

// Lower a label whose prefetched value was above nb.  GS_BB_NORET: fire and forget
// (the wave does not wait for the atomic's return), and y counts as improved on the
// prefetched value alone -- when another lane got there first, y is queued for a
// source whose label it did not lower, an extra expansion that changes no fixpoint.
#ifndef GS_BB_NORET
#define GS_BB_NORET 1
#endif
__device__ __forceinline__ bool bb_min_improves(unsigned long long *p, unsigned long long nb) {
#if GS_BB_NORET
    atomicMin(p, nb);
    return true;
#else
    return nb < atomicMin(p, nb);
#endif
}

// Reverse columns (metric_backbone.py:97-111 decides column (v, u) from v's Dijkstra,
// column (u, v) from u's).  After u's search, D = u's label of v (the left fold of a
// real u-v path; m bounds the relative rounding of folds over simple paths, as in
// k_bb_certify):
//  * prune: d_fl(v, u) <= D (1 + m) (the same path folded from v), so a reverse
//    column with w > (D (1 + m) + eps)(1 + m) is pruned;
//  * exact: when u's search ran dry within bound bk >= D (frontier empty), labels
//    <= bk are exact and every other label exceeds bk, so A = min over v's other G
//    neighbours x of (label(x), or bk if beyond it) + w(x, v) bounds every u-v path
//    but the edge itself from below: real length >= A (1 - m).  A (1 - 3m) > D then
//    means the edge is the only shortest path from either end by more than any
//    rounding, so d_fl(v, u) = fl(0 + w_G) = D exactly, and the reverse column is
//    decided as the reference decides it: w <= D + eps.  (A v of more than
//    kBbCrossDeg neighbours -- a hub the search reached -- is scanned by the whole
//    workgroup after the classification, up to kBbCrossBig of them per batch.)
//  * keep, v unreached: d_fl(u, v) > bk, so w <= (bk (1 - m) + eps)(1 - m) keeps it.
// Whatever falls within the margins stays open for v's own search.
// skeys / sidx: every column's (row * n + col) key in ascending order and its column;
// rp: the first position of the reverse key (-1: none).
#ifndef GS_BB_CROSS_DEG
#define GS_BB_CROSS_DEG 128
#endif
static constexpr int64_t kBbCrossDeg = GS_BB_CROSS_DEG;
#ifndef GS_BB_CROSS_BIG
#define GS_BB_CROSS_BIG 1024
#endif
static constexpr int kBbCrossBig = GS_BB_CROSS_BIG;
template <int S>
__device__ __forceinline__ bool bb_cross_decide(const uint64_t *__restrict__ skeys,
                                                const int64_t *__restrict__ sidx, int64_t rp,
                                                int64_t u, int64_t v, int64_t n, int64_t E,
                                                int k, unsigned long long db, double bk, double m,
                                                double eps, const double *__restrict__ w,
                                                const int64_t *__restrict__ gp,
                                                const int32_t *__restrict__ gi,
                                                const double *__restrict__ gw,
                                                const unsigned long long *__restrict__ dist,
                                                uint8_t *__restrict__ state, uint8_t *__restrict__ why) {
    if (rp < 0) return false;
    const uint64_t rkey = (uint64_t)v * (uint64_t)n + (uint64_t)u;
    bool open = false;  // any reverse column still undecided
    for (int64_t p = rp; p < E && skeys[p] == rkey; ++p) open = open || state[sidx[p]] == 0;
    if (!open) return false;
    const bool reached = db != kInfBits;
    const double D = __longlong_as_double((long long)db);
    bool exact = false;
    const bool eligible = reached && bk >= 0.0 && D <= bk;
    if (eligible && gp[v + 1] - gp[v] <= kBbCrossDeg) {
        double A = __longlong_as_double((long long)kInfBits);
        for (int64_t e = gp[v]; e < gp[v + 1]; ++e) {
            const int32_t x = gi[e];
            if (x == u) continue;
            const unsigned long long bx = __hip_atomic_load(&dist[(int64_t)x * S + k], __ATOMIC_RELAXED,
                                                            __HIP_MEMORY_SCOPE_WORKGROUP);
            const double dx = __longlong_as_double((long long)bx);
            const double lb = (bx != kInfBits && dx <= bk) ? dx : bk;
            const double a = lb + gw[e];
            A = a < A ? a : A;
        }
        exact = A * (1.0 - 3.0 * m) > D;
    }
    const double hi = reached ? (D * (1.0 + m) + eps) * (1.0 + m) : 0.0;
    const bool keep_unreached = !reached && bk >= 0.0;
    const double lo = keep_unreached ? (bk * (1.0 - m) + eps) * (1.0 - m) : -1.0;
    bool left = false;
    for (int64_t p = rp; p < E && skeys[p] == rkey; ++p) {
        const int64_t r = sidx[p];
        if (state[r] != 0) continue;
        const double wr = w[r];
        if (exact) bb_set(state, why, r, wr <= D + eps ? 1 : 2, kWhyRevExact);
        else if (reached && wr > hi) bb_set(state, why, r, 2, kWhyRevPrune);
        else if (keep_unreached && wr <= lo) bb_set(state, why, r, 1, kWhyRevKeep);
        else left = true;
    }
    // a v of more than kBbCrossDeg neighbours: the caller's workgroup scans them
    return left && eligible && gp[v + 1] - gp[v] > kBbCrossDeg;
}

// order-preserving u64 key of a double (0 below every key: "no value")
__device__ __forceinline__ unsigned long long dkey(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double dkey_val(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// S per-source maxima at once: each thread's keys -> wave max -> one LDS atomicMax
// per wave and source into out[S] (0 on entry); ends with a barrier
template <int S>
__device__ __forceinline__ void bb_block_max_s(unsigned long long (&m)[S], unsigned long long *out) {
#pragma unroll
    for (int k = 0; k < S; ++k) {
        unsigned long long v = m[k];
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(v, off, 64);
            v = o > v ? o : v;
        }
        if ((threadIdx.x & 63) == 0 && v) atomicMax(&out[k], v);
    }
    __syncthreads();
}

// S sources per workgroup, searched together: dist[x*S + s] interleaved, so
// the random read of node x's labels is one 8S-byte segment shared by the S
// searches (the single-source kernel fetches a whole line per relaxation).
// The frontier is the union of the sources' frontiers; qmask[x] holds the
// sources whose label of x improved in the round (x is queued once).  Each
// source keeps its own bound s_wmax[s], lowered by its own targets exactly as
// in k_bb_sssp, so every source reaches the same fixpoint as alone.
// Near-far order (delta > 0): an improvement to a label >= the source's
// threshold s_thr[s] waits in the far pile instead of the next frontier; when
// a source has nothing near left its threshold moves to (least pending far
// label) + delta and the far labels below it join the frontier.  Labels are
// then mostly expanded once at their final value (a plain frontier search
// re-expands ~1.9x as many on RMAT-18's Jaccard costs; near-far ~1.05x at
// delta = median weight / 2, tools/bb_nearfar_sim.c) -- the fixpoint, and so
// every distance and decision, is the same in any order.
// PAIR (S = 2; the meet-in-the-middle certificate, bb_pair_certify): batch b searches
// both ends of the open column sources[b] = i (src[i], dst[i]) to the radius
// r = w_max (1 + 8m) / 2, w_max the larger of its and its reverse columns' weights, with
// no target pruning, then decides the column and its reverse columns where the balls
// prove it (see the evaluation below).
template <int NT, int S, bool PAIR = false>
__global__ void __launch_bounds__(NT) k_bb_sssp_multi(
    const int64_t *__restrict__ gp, const int32_t *__restrict__ gi, const double *__restrict__ gw,
    int64_t n, const int64_t *__restrict__ sources, int64_t nsrc, const int64_t *__restrict__ optr,
    const int64_t *__restrict__ order, const int64_t *__restrict__ src, const int64_t *__restrict__ dst,
    const double *__restrict__ w, double eps, uint8_t *__restrict__ state,
    unsigned long long *__restrict__ dist_all, uint32_t *__restrict__ qmask_all,
    int32_t *__restrict__ fr_all, uint32_t *__restrict__ fm_all, int32_t *__restrict__ touched_all,
    int32_t *__restrict__ far_all, double delta, int cross, const uint64_t *__restrict__ skeys,
    const int64_t *__restrict__ sidx, const int64_t *__restrict__ rpos, int64_t E, double mrg,
    int rev, int64_t b0, int64_t b1, int part, int nparts,
    unsigned long long *__restrict__ batch_next, unsigned long long *__restrict__ relax_total,
    unsigned long long *__restrict__ trace, uint8_t *__restrict__ why,
    const uint8_t *__restrict__ lmflag = nullptr, const double *__restrict__ LD = nullptr,
    const int32_t *__restrict__ lcomp = nullptr, int K = 0) {
    static_assert(S >= 1 && S <= 16, "1..16 sources per workgroup");
    static_assert(!PAIR || S == 2, "the pair form searches both ends of one column");
    // queue bits of the per-node mask; the near-far order needs S more bits for the
    // far pile (S <= 8 only: 16 sources fill the word)
    constexpr uint32_t QS = S <= 8 ? kQMaskSources : 0xffffu;
    constexpr bool NF = S <= 8;
    if (!NF) delta = 0.0;
    constexpr int NW = NT / 64;
    __shared__ int s_fcount, s_ncount, s_tcount, s_nfar, s_nfar2, s_farleft, s_nheavy, s_nbig;
    __shared__ int64_t s_big[kBbCrossBig];  // deferred reverse decisions: idx << 4 | source k
    __shared__ unsigned long long s_amin;
    __shared__ int32_t s_heavy[kBbHeavyMax];
    __shared__ uint32_t s_hmask[kBbHeavyMax];
    __shared__ uint32_t s_nearany;
    __shared__ double s_wmax[S], s_thr[S];
    __shared__ unsigned long long s_wkey[S], s_farmin[S];
    __shared__ int64_t s_src[S];
    __shared__ unsigned long long s_relax;
    __shared__ int32_t w_pre[NW][65];
    __shared__ int64_t w_beg[NW][64];
    __shared__ uint32_t w_m[NW][64];
    __shared__ double w_d[NW][64][S];
    unsigned long long *dist = dist_all + (int64_t)blockIdx.x * n * S;
    uint32_t *qmask = qmask_all + (int64_t)blockIdx.x * n;
    int32_t *fa = fr_all + (int64_t)blockIdx.x * 2 * n;
    int32_t *fb = fa + n;
    uint32_t *fm = fm_all + (int64_t)blockIdx.x * n;
    int32_t *touched = touched_all + (int64_t)blockIdx.x * n;
    int32_t *farA = far_all + (int64_t)blockIdx.x * 2 * n, *farB = farA + n;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double thr0 = delta > 0.0 ? delta : __longlong_as_double((long long)kInfBits);
    if (threadIdx.x == 0) s_relax = 0;
    unsigned long long relax = 0;
    const int64_t nbatch = PAIR ? nsrc : (nsrc + S - 1) / S;
    __shared__ int64_t s_pcol;
    // batches taken in order from a global counter as workgroups free up (batch_next;
    // null: static striding), so the long searches at the end of the order do not
    // leave workgroups idle behind a fixed share
    // batches [b0, b1) of the processing order (b1 <= nbatch), this part's every
    // nparts-th one: the j-th taken is b0 + part + j * nparts
    __shared__ long long s_bq;
    if (threadIdx.x == 0) s_bq = batch_next ? (long long)atomicAdd(batch_next, 1ull) : (long long)blockIdx.x;
    __syncthreads();
    for (int64_t bj = s_bq, bq = b0 + part + bj * nparts; bq < b1; bj = s_bq, bq = b0 + part + bj * nparts) {
        // rev: the batches from the last (the sources are in node order, i.e. by
        // descending column count after the relabeling)
        const int64_t bi = rev ? nbatch - 1 - bq : bq;
        // GSPARSE_BB_TRACE: the batch's start / end on the constant clock and workgroup
        const unsigned long long tb0 = trace ? (unsigned long long)wall_clock64() : 0ull;
        if (threadIdx.x < S) {
            if constexpr (PAIR) {
                const int64_t i = sources[bi];
                s_src[threadIdx.x] = threadIdx.x == 0 ? src[i] : dst[i];
                if (threadIdx.x == 0) s_pcol = i;
            } else {
                const int64_t si = bi * S + threadIdx.x;
                s_src[threadIdx.x] = si < nsrc ? sources[si] : -1;
            }
            s_wkey[threadIdx.x] = 0ull;
            s_thr[threadIdx.x] = thr0;
            s_farmin[threadIdx.x] = kInfBits;
        }
        __syncthreads();
        if constexpr (PAIR) {  // the radius: half the larger of the pair's open weights
            if (threadIdx.x == 0) {
                const int64_t i = s_pcol, u = s_src[0], v = s_src[1];
                double wm = w[i];
                const int64_t rp = rpos[i];
                if (rp >= 0) {
                    const uint64_t rkey = (uint64_t)v * (uint64_t)n + (uint64_t)u;
                    for (int64_t p = rp; p < E && skeys[p] == rkey; ++p)  // the open ones only
                        if (state[sidx[p]] == 0) wm = w[sidx[p]] > wm ? w[sidx[p]] : wm;
                }
                const double r = wm * (1.0 + 8.0 * mrg) * 0.5;
                // an end that is a (complete) landmark: its labels are exact already
                const bool skip = lmflag && (lmflag[u] || lmflag[v]);
                s_wkey[0] = s_wkey[1] = skip ? 0ull : dkey(r);
            }
            __syncthreads();
        } else
        // largest unresolved target weight of each source (none: nothing to decide)
        {
            unsigned long long lm[S];
#pragma unroll
            for (int k = 0; k < S; ++k) {
                lm[k] = 0ull;
                const int64_t u = s_src[k];
                if (u >= 0)
                    for (int64_t j = optr[u] + threadIdx.x; j < optr[u + 1]; j += NT) {
                        const int64_t idx = order[j];
                        if (state[idx] == 0) {
                            const unsigned long long kk = dkey(w[idx]);
                            lm[k] = kk > lm[k] ? kk : lm[k];
                        }
                    }
            }
            bb_block_max_s<S>(lm, s_wkey);
        }
        if (threadIdx.x < S)
            s_wmax[threadIdx.x] = s_wkey[threadIdx.x] ? dkey_val(s_wkey[threadIdx.x]) : -1.0;
        __syncthreads();
        if (trace && threadIdx.x == 0) {  // the batch's largest bound and its column count
            double bm = -1.0;
            long long nc = 0;
            for (int k = 0; k < S; ++k) {
                bm = s_wmax[k] > bm ? s_wmax[k] : bm;
                if (s_src[k] >= 0) nc += optr[s_src[k] + 1] - optr[s_src[k]];
            }
            trace[6 * bj + 3] = (unsigned long long)__double_as_longlong(bm);
            trace[6 * bj + 4] = (unsigned long long)nc;
        }
        const unsigned long long relax0 = relax;
        // seed: every live source at its own node (sources are distinct nodes)
        if (threadIdx.x == 0) {
            int f = 0;
            for (int k = 0; k < S; ++k) {
                if (s_src[k] < 0 || s_wmax[k] < 0.0) continue;
                const int32_t u = (int32_t)s_src[k];
                dist[(int64_t)u * S + k] = 0ull;
                qmask[u] = (1u << k) | kQMaskTouched;
                fa[f] = u;
                touched[f] = u;
                ++f;
            }
            s_fcount = f;
            s_ncount = 0;
            s_tcount = f;
            s_nfar = 0;
            s_farleft = 0;
            s_nearany = 0;
            s_nbig = 0;
            s_amin = kInfBits;
        }
        __syncthreads();
        int32_t *cur = fa, *nxt = fb;
        uint32_t nearacc = 0;  // sources this lane queued near in the round
        while (true) {
            const int fc = s_fcount;
            if (fc == 0 && !s_farleft) break;
            // the bounds in registers (8 sources or fewer), else read from LDS per relaxation
            constexpr int SW = S <= 8 ? S : 1;
            double wmax[SW];
#pragma unroll
            for (int k = 0; k < SW; ++k) wmax[k] = s_wmax[k];
            auto wmax_of = [&](int k) -> double {
                if constexpr (S <= 8) return wmax[k];
                else return s_wmax[k];
            };
            if (threadIdx.x == 0) s_nheavy = 0;
            __syncthreads();
            // heavy frontier nodes (more than kBbHeavy entries: the R-MAT hubs) are taken
            // out of the per-wave chunks and expanded by the whole workgroup below, so one
            // wave does not walk a hub's list while the others wait at the barrier
            for (int f = threadIdx.x; f < fc; f += NT) {
                const int32_t x = cur[f];
                uint32_t m = atomicAnd(&qmask[x], ~QS) & QS;
                if (m && gp[x + 1] - gp[x] > kBbHeavy) {
                    const int h = atomicAdd(&s_nheavy, 1);
                    if (h < kBbHeavyMax) {
                        s_heavy[h] = x;
                        s_hmask[h] = m;
                        m = 0;
                    }
                }
                fm[f] = m;
            }
            __syncthreads();
            for (int f0 = wv * 64; f0 < fc; f0 += NT) {
                const int f = f0 + lane;
                int deg = 0;
                int64_t b = 0;
                uint32_t m = 0;
                if (f < fc) {
                    const int32_t x = cur[f];
                    m = fm[f];
                    b = gp[x];
                    deg = m ? (int)(gp[x + 1] - b) : 0;
#pragma unroll
                    for (int k = 0; k < S; ++k)
                        w_d[wv][lane][k] = __longlong_as_double((long long)__hip_atomic_load(
                            &dist[(int64_t)x * S + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                }
                int incl = deg;
                for (int off = 1; off < 64; off <<= 1) {
                    const int t = __shfl_up(incl, off, 64);
                    if (lane >= off) incl += t;
                }
                const int total = __shfl(incl, 63, 64);
                w_pre[wv][lane + 1] = incl;
                if (lane == 0) w_pre[wv][0] = 0;
                w_beg[wv][lane] = b;
                w_m[wv][lane] = m;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                constexpr int U = S >= 16 ? 1 : S >= 8 ? 2 : 4;  // edges per lane per trip, all loads in flight
                for (int e0 = 0; e0 < total; e0 += 64 * U) {
                    int lo[U];
                    uint32_t mm[U];
                    double we[U];
                    int32_t y[U];
                    unsigned long long cd[U][S];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int e = e0 + u * 64 + lane;
                        const int ec = e < total ? e : 0;
                        int a = 0, z = 63;  // largest k with w_pre[k] <= ec
                        while (a < z) {
                            const int mid = (a + z + 1) >> 1;
                            if (w_pre[wv][mid] <= ec) a = mid;
                            else z = mid - 1;
                        }
                        lo[u] = a;
                        const int64_t ei = w_beg[wv][a] + (ec - w_pre[wv][a]);
                        mm[u] = e < total ? w_m[wv][a] : 0u;
                        we[u] = gw[ei];
                        y[u] = gi[ei];
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int k = 0; k < S; ++k)
                            cd[u][k] = ((mm[u] >> k) & 1u)
                                           ? __hip_atomic_load(&dist[(int64_t)y[u] * S + k],
                                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
                                           : 0ull;
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                    uint32_t imp = 0, fimp = 0;
                    bool btouch = false;  // PAIR: a label set beyond the radius
                    // PAIR: complete landmarks are reached, never expanded (their labels
                    // bound the paths through them, min_l D_l(u) + D_l(v))
                    const bool blk = PAIR && lmflag && mm[u] && lmflag[y[u]];
#pragma unroll
                    for (int k = 0; k < S; ++k) {
                        if (!((mm[u] >> k) & 1u)) continue;
                        ++relax;
                        const double nd = w_d[wv][lo[u]][k] + we[u];
                        if (!(nd <= wmax_of(k)) || blk) {
                            // PAIR: kept (a T label of the certificate), never expanded
                            if constexpr (PAIR) {
                                const unsigned long long nb = (unsigned long long)__double_as_longlong(nd);
                                if (nb < cd[u][k]) {
                                    atomicMin(&dist[(int64_t)y[u] * S + k], nb);
                                    btouch = true;
                                }
                            }
                            continue;
                        }
                        const unsigned long long nb = (unsigned long long)__double_as_longlong(nd);
                        if (nb >= cd[u][k]) continue;
                        if (bb_min_improves(&dist[(int64_t)y[u] * S + k], nb)) {
                            if (!NF || nd < s_thr[k]) {  // LDS: read on improvements only
                                imp |= 1u << k;
                            } else {
                                fimp |= 1u << (kQMaskFarShift + k);
                                atomicMin(&s_farmin[k], nb);
                            }
                        }
                    }
                    if (imp | fimp) {  // queue y once per round; far: list it once, reset list
                        const uint32_t add = fimp ? (imp | fimp | kQMaskFarListed | kQMaskTouched) : imp;
                        const uint32_t om = atomicOr(&qmask[y[u]], add);
                        if (imp && (om & QS) == 0) {
                            const int q = atomicAdd(&s_ncount, 1);
                            nxt[q] = y[u];
                        }
                        if (fimp && !(om & kQMaskFarListed)) farA[atomicAdd(&s_nfar, 1)] = y[u];
                        if (fimp && !(om & kQMaskTouched)) touched[atomicAdd(&s_tcount, 1)] = y[u];
                        nearacc |= imp;
                    }
                    if (PAIR && btouch && !(atomicOr(&qmask[y[u]], kQMaskTouched) & kQMaskTouched))
                        touched[atomicAdd(&s_tcount, 1)] = y[u];
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            {
                const int nh = s_nheavy < kBbHeavyMax ? s_nheavy : kBbHeavyMax;
                for (int h = 0; h < nh; ++h) {
                    const int32_t x = s_heavy[h];
                    const uint32_t m = s_hmask[h];
                    // the hub's labels: wave 0 stages them in its w_d row 0 (free after the
                    // light chunks), every wave reads them from there
                    if (wv == 0 && lane < S)
                        w_d[0][0][lane] = ((m >> lane) & 1u) ? __longlong_as_double((long long)__hip_atomic_load(
                                                                   &dist[(int64_t)x * S + lane], __ATOMIC_RELAXED,
                                                                   __HIP_MEMORY_SCOPE_WORKGROUP))
                                                             : 0.0;
                    __syncthreads();
                    const int64_t e1 = gp[x + 1];
                    for (int64_t e = gp[x] + threadIdx.x; e < e1; e += NT) {
                        const int32_t y = gi[e];
                        const double we = gw[e];
                        unsigned long long cd[S];
#pragma unroll
                        for (int k = 0; k < S; ++k)
                            cd[k] = ((m >> k) & 1u) ? __hip_atomic_load(&dist[(int64_t)y * S + k], __ATOMIC_RELAXED,
                                                                        __HIP_MEMORY_SCOPE_WORKGROUP)
                                                    : 0ull;
                        uint32_t imp = 0, fimp = 0;
                        bool btouch = false;
                        const bool blk = PAIR && lmflag && lmflag[y];
#pragma unroll
                        for (int k = 0; k < S; ++k) {
                            if (!((m >> k) & 1u)) continue;
                            ++relax;
                            const double nd = w_d[0][0][k] + we;
                            if (!(nd <= wmax_of(k)) || blk) {
                                if constexpr (PAIR) {
                                    const unsigned long long nb = (unsigned long long)__double_as_longlong(nd);
                                    if (nb < cd[k]) {
                                        atomicMin(&dist[(int64_t)y * S + k], nb);
                                        btouch = true;
                                    }
                                }
                                continue;
                            }
                            const unsigned long long nb = (unsigned long long)__double_as_longlong(nd);
                            if (nb >= cd[k]) continue;
                            if (bb_min_improves(&dist[(int64_t)y * S + k], nb)) {
                                if (!NF || nd < s_thr[k]) {
                                    imp |= 1u << k;
                                } else {
                                    fimp |= 1u << (kQMaskFarShift + k);
                                    atomicMin(&s_farmin[k], nb);
                                }
                            }
                        }
                        if (imp | fimp) {
                            const uint32_t add = fimp ? (imp | fimp | kQMaskFarListed | kQMaskTouched) : imp;
                            const uint32_t om = atomicOr(&qmask[y], add);
                            if (imp && (om & QS) == 0) nxt[atomicAdd(&s_ncount, 1)] = y;
                            if (fimp && !(om & kQMaskFarListed)) farA[atomicAdd(&s_nfar, 1)] = y;
                            if (fimp && !(om & kQMaskTouched)) touched[atomicAdd(&s_tcount, 1)] = y;
                            nearacc |= imp;
                        }
                        if (PAIR && btouch && !(atomicOr(&qmask[y], kQMaskTouched) & kQMaskTouched))
                            touched[atomicAdd(&s_tcount, 1)] = y;
                    }
                    __syncthreads();
                }
            }
            if (NF && delta > 0.0) {  // which sources queued anything near this round
                uint32_t v = nearacc;
                for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off, 64);
                if (lane == 0 && v) atomicOr(&s_nearany, v);
                nearacc = 0;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                s_fcount = s_ncount;
                s_ncount = 0;
            }
            int32_t *t = cur;
            cur = nxt;
            nxt = t;
            __syncthreads();
            // every node improved this round is in the new frontier: the first time one
            // appears there it joins the reset list
            {
                const int nf = s_fcount;
                for (int f = threadIdx.x; f < nf; f += NT) {
                    const int32_t y = cur[f];
                    const uint32_t om = atomicOr(&qmask[y], kQMaskTouched);
                    if (!(om & kQMaskTouched)) touched[atomicAdd(&s_tcount, 1)] = y;
                }
            }
            // hook: prune targets per source, lower its bound, end when all are done
            if (threadIdx.x < S) s_wkey[threadIdx.x] = 0ull;
            __syncthreads();
            if constexpr (PAIR) {
                if (threadIdx.x < S) s_wkey[threadIdx.x] = dkey(s_wmax[threadIdx.x]);  // the radius stays
                __syncthreads();
            } else {
                unsigned long long mx[S];
#pragma unroll
                for (int k = 0; k < S; ++k) {
                    mx[k] = 0ull;
                    const int64_t u = s_src[k];
                    if (u >= 0 && s_wmax[k] >= 0.0)
                        for (int64_t j = optr[u] + threadIdx.x; j < optr[u + 1]; j += NT) {
                            const int64_t idx = order[j];
                            if (state[idx] != 0) continue;
                            const unsigned long long db = __hip_atomic_load(
                                &dist[dst[idx] * S + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            if (db != kInfBits &&
                                w[idx] > __longlong_as_double((long long)db) + eps) {
                                bb_set(state, why, idx, 2, kWhySearchPrune);
                                continue;
                            }
                            const unsigned long long kk = dkey(w[idx]);
                            mx[k] = kk > mx[k] ? kk : mx[k];
                        }
                }
                bb_block_max_s<S>(mx, s_wkey);
            }
            __shared__ uint32_t s_refill;
            __shared__ double s_throld[S];
            if (threadIdx.x == 0) {
                bool any = false;
                for (int k = 0; k < S; ++k) {
                    s_wmax[k] = s_wkey[k] ? dkey_val(s_wkey[k]) : -1.0;
                    any = any || s_wkey[k] != 0ull;
                }
                if (!any) s_fcount = 0;
                // near-far: a source with nothing near queued and far labels pending
                // moves its threshold past the least of them
                uint32_t R = 0;
                if (NF && any && delta > 0.0)
                    for (int k = 0; k < S; ++k)
                        if (!((s_nearany >> k) & 1u) && s_farmin[k] != kInfBits) {
                            R |= 1u << k;
                            s_throld[k] = s_thr[k];
                            const double m = __longlong_as_double((long long)s_farmin[k]);
                            s_thr[k] = (m > s_thr[k] ? m : s_thr[k]) + delta;
                            s_farmin[k] = kInfBits;
                        }
                s_refill = R;
                s_nearany = 0;
                s_nfar2 = 0;
                s_farleft = any && s_nfar > 0 && (R || s_fcount > 0);
            }
            __syncthreads();
            const uint32_t R = NF ? s_refill : 0u;
            if (NF && R) {
                // far labels of the refilled sources: below the old threshold (expanded when
                // they improved) or beyond the bound -> dropped; below the new one -> the
                // frontier; the rest stay, and give the source's next least far label
                const int nf = s_nfar;
                for (int i = threadIdx.x; i < nf; i += NT) {
                    const int32_t y = farA[i];
                    const uint32_t om = __hip_atomic_load(&qmask[y], __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_WORKGROUP);
                    uint32_t clear = 0, set = 0;
#pragma unroll
                    for (int k = 0; k < S; ++k) {
                        if (!((R >> k) & 1u) || !((om >> (kQMaskFarShift + k)) & 1u)) continue;
                        const unsigned long long db = __hip_atomic_load(
                            &dist[(int64_t)y * S + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        const double d = __longlong_as_double((long long)db);
                        if (!(d <= s_wmax[k]) || d < s_throld[k]) {
                            clear |= 1u << (kQMaskFarShift + k);
                        } else if (d < s_thr[k]) {
                            clear |= 1u << (kQMaskFarShift + k);
                            set |= 1u << k;
                        } else {
                            atomicMin(&s_farmin[k], db);
                        }
                    }
                    uint32_t nm = (om & ~clear) | set;
                    if (!(nm & (QS << kQMaskFarShift))) nm &= ~kQMaskFarListed;
                    __hip_atomic_store(&qmask[y], nm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (set && !(om & QS)) cur[atomicAdd(&s_fcount, 1)] = y;
                    if (nm & kQMaskFarListed) farB[atomicAdd(&s_nfar2, 1)] = y;
                }
                __syncthreads();
                if (threadIdx.x == 0) {
                    s_nfar = s_nfar2;
                    s_farleft = s_nfar2 > 0;
                }
                int32_t *t = farA;
                farA = farB;
                farB = t;
                __syncthreads();
            }
        }
        if constexpr (PAIR) {
            // The balls of radius r around u and v (labels <= r exact, expanded; a label
            // beyond r is kept but never expanded: T_v(x) = min over v's ball nodes y of
            // d_v(y) + w_yx, the fold of a real v-x walk).  Every u-v path P but the edge
            // itself, of length L <= 2r (1 - 3m): x = its last node with
            // d_P(u, x) <= r (1 - 2m) and y the next lie in u's and v's balls (the labels
            // fold within m of the exact lengths; d_P(y, v) < r (1 - 4m)), so
            // d_u(x) + T_v(x) <= L (1 + 2m) (x = v: T_v(v) = 0).  x = u (P's first edge
            // leaves u's ball) is taken over u's other edges: w_uy + d_v(y), y in v's ball.
            // So M = min(min over x in u's ball but u of d_u(x) + T_v(x),
            //            min over (u, y), y != v, d_v(y) <= r of w_uy + d_v(y))
            // is at most (1 + 4m) times every such path's fold; every term is the length of
            // a real u-v walk (one through the edge itself is at least w_G: the prune below
            // then follows from d <= w_G; x = u, whose T_v may hold w_G, is excluded).  A
            // column (u, v) or (v, u) of weight w <= 2r (1 - 5m) (a longer path folds to
            // more than 2r (1 - 4m) > w):
            //  * w > fl(w_G + eps) (its own edge in G is shorter): prune (d <= w_G);
            //  * M (1 - 5m) >= w: every alternative path folds to >= w, and w <=
            //    fl(w_G + eps): keep (the reference's w <= fl(d + eps));
            //  * (M (1 + 4m) + eps)(1 + m) < w: a shorter path exists: prune.
            // Otherwise the column stays open for the searches.
            const int64_t u = s_src[0], v = s_src[1];
            const double r = s_wmax[0];
            double mloc = __longlong_as_double((long long)kInfBits);
            // paths through a blocked landmark l: at least D_l(u) + D_l(v) (its exact labels)
            if (lmflag)
                for (int l = threadIdx.x; l < K; l += NT)
                    if (lcomp[l]) {
                        const double t2 = (LD[u * K + l] + LD[v * K + l]) * (1.0 - 2.0 * mrg);
                        mloc = t2 < mloc ? t2 : mloc;
                    }
            const int tc = s_tcount;
            for (int t = threadIdx.x; t < tc; t += NT) {
                const int32_t x = touched[t];
                if (x == (int32_t)u) continue;  // u's first edges: below
                const double du = __longlong_as_double((long long)__hip_atomic_load(
                    &dist[(int64_t)x * 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                const unsigned long long bv = __hip_atomic_load(&dist[(int64_t)x * 2 + 1], __ATOMIC_RELAXED,
                                                                __HIP_MEMORY_SCOPE_WORKGROUP);
                if (du <= r && bv != kInfBits) {
                    const double t2 = du + __longlong_as_double((long long)bv);
                    mloc = t2 < mloc ? t2 : mloc;
                }
            }
            for (int64_t e = gp[u] + threadIdx.x; e < gp[u + 1]; e += NT) {
                const int32_t y = gi[e];
                if (y == (int32_t)v) continue;
                const double dv = __longlong_as_double((long long)__hip_atomic_load(
                    &dist[(int64_t)y * 2 + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                if (dv <= r) {
                    const double t2 = gw[e] + dv;
                    mloc = t2 < mloc ? t2 : mloc;
                }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const double o = __shfl_xor(mloc, off, 64);
                mloc = o < mloc ? o : mloc;
            }
            if ((threadIdx.x & 63) == 0)  // mloc >= 0: its bits order as the values
                atomicMin(&s_amin, (unsigned long long)__double_as_longlong(mloc));
            __syncthreads();
            if (threadIdx.x == 0 && r >= 0.0) {
                const double M = __longlong_as_double((long long)s_amin);
                // w_G(u, v): v in the shorter of the two sorted lists
                const int64_t du = gp[u + 1] - gp[u], dvv = gp[v + 1] - gp[v];
                const bool us = du <= dvv;
                int64_t lo = us ? gp[u] : gp[v], hi = us ? gp[u + 1] : gp[v + 1];
                const int64_t end = hi;
                const int32_t key = (int32_t)(us ? v : u);
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (gi[mid] < key) lo = mid + 1;
                    else hi = mid;
                }
                const bool has = lo < end && gi[lo] == key;
                const double wg = has ? gw[lo] : 0.0;
                auto decide = [&](int64_t c) {
                    if (state[c] != 0) return;
                    const double wc = w[c];
                    if (!(wc <= 2.0 * r * (1.0 - 5.0 * mrg))) return;
                    if (has && wc > wg + eps) bb_set(state, why, c, 2, kWhyMitm);
                    else if (M * (1.0 - 5.0 * mrg) >= wc) bb_set(state, why, c, 1, kWhyMitm);
                    else if ((M * (1.0 + 4.0 * mrg) + eps) * (1.0 + mrg) < wc) bb_set(state, why, c, 2, kWhyMitm);
                };
                decide(s_pcol);
                const int64_t rp = rpos[s_pcol];
                if (rp >= 0) {
                    const uint64_t rkey = (uint64_t)v * (uint64_t)n + (uint64_t)u;
                    for (int64_t p = rp; p < E && skeys[p] == rkey; ++p) decide(sidx[p]);
                }
            }
            if (threadIdx.x == 0) s_amin = kInfBits;
            __syncthreads();
        } else {
        // classify each source's unresolved targets; with cross != 0 also the reverse
        // columns (v, u) still open, from u's label of v (bb_cross_decide)
        for (int k = 0; k < S; ++k) {
            const int64_t u = s_src[k];
            if (u < 0) continue;
            const double bk = s_wmax[k];  // >= 0: u's search ran dry within this bound
            for (int64_t j = optr[u] + threadIdx.x; j < optr[u + 1]; j += NT) {
                const int64_t idx = order[j];
                const uint8_t st0 = state[idx];
                if (st0 != 0 && !cross) continue;
                const int64_t v = dst[idx];
                const unsigned long long db = __hip_atomic_load(
                    &dist[v * S + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                const double d = __longlong_as_double((long long)db);
                if (st0 == 0) {
                    const bool keep = (db == kInfBits) || (w[idx] <= d + eps);
                    bb_set(state, why, idx, keep ? 1 : 2, keep ? kWhySearchKeep : kWhySearchPrune);
                }
                if (cross &&
                    bb_cross_decide<S>(skeys, sidx, rpos[idx], u, v, n, E, k, db, bk, mrg, eps, w, gp, gi,
                                       gw, dist, state, why)) {
                    const int q = atomicAdd(&s_nbig, 1);
                    if (q < kBbCrossBig) s_big[q] = (idx << 4) | k;
                }
            }
        }
        __syncthreads();
        // deferred exact reverse decisions (targets of many neighbours): the workgroup
        // takes the lower bound A over v's neighbours together (bb_cross_decide's rule)
        {
            const int nbg = s_nbig < kBbCrossBig ? s_nbig : kBbCrossBig;
            for (int q = 0; q < nbg; ++q) {
                const int64_t idx = s_big[q] >> 4;
                const int k = (int)(s_big[q] & 15);
                const int64_t u = s_src[k], v = dst[idx];
                const double bk = s_wmax[k];
                double a = __longlong_as_double((long long)kInfBits);
                for (int64_t e = gp[v] + threadIdx.x; e < gp[v + 1]; e += NT) {
                    const int32_t x = gi[e];
                    if (x == u) continue;
                    const unsigned long long bx = __hip_atomic_load(&dist[(int64_t)x * S + k], __ATOMIC_RELAXED,
                                                                    __HIP_MEMORY_SCOPE_WORKGROUP);
                    const double dx = __longlong_as_double((long long)bx);
                    const double lb = ((bx != kInfBits && dx <= bk) ? dx : bk) + gw[e];
                    a = lb < a ? lb : a;
                }
                for (int off = 32; off > 0; off >>= 1) {
                    const double o = __shfl_xor(a, off, 64);
                    a = o < a ? o : a;
                }
                if ((threadIdx.x & 63) == 0)  // a >= 0: its bits order as the values
                    atomicMin(&s_amin, (unsigned long long)__double_as_longlong(a));
                __syncthreads();
                if (threadIdx.x == 0) {
                    const double A = __longlong_as_double((long long)s_amin);
                    const double D = __longlong_as_double((long long)__hip_atomic_load(
                        &dist[v * S + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                    if (A * (1.0 - 3.0 * mrg) > D) {
                        const uint64_t rkey = (uint64_t)v * (uint64_t)n + (uint64_t)u;
                        for (int64_t p = rpos[idx]; p < E && skeys[p] == rkey; ++p) {
                            const int64_t r = sidx[p];
                            if (state[r] == 0) bb_set(state, why, r, w[r] <= D + eps ? 1 : 2, kWhyRevExact);
                        }
                    }
                    s_amin = kInfBits;
                }
                __syncthreads();
            }
        }
        }  // !PAIR
        __syncthreads();
        if (trace && relax != relax0) atomicAdd(&trace[6 * bj + 5], relax - relax0);
        const int tc = s_tcount;
        for (int t = threadIdx.x; t < tc; t += NT) {
            const int32_t y = touched[t];
#pragma unroll
            for (int k = 0; k < S; ++k) dist[(int64_t)y * S + k] = kInfBits;
            qmask[y] = 0u;
        }
        if (threadIdx.x == 0) {
            if (trace) {
                trace[6 * bj] = tb0;
                trace[6 * bj + 1] = (unsigned long long)wall_clock64();
                trace[6 * bj + 2] = blockIdx.x;
            }
            s_bq = batch_next ? (long long)atomicAdd(batch_next, 1ull) : (long long)(bj + gridDim.x);
        }
        __syncthreads();
    }
    atomicAdd(&s_relax, relax);
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(relax_total, s_relax);
}

}  // namespace gs
