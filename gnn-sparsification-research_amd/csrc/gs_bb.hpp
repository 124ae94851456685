// gs_bb.hpp -- what the metric backbone's units share (gs_backbone.hip and
// gs_bb_*.hip): the run state of the staged form, the one reader of the
// GSPARSE_BB_* variables, the search geometry, the owner of the idle search
// slabs, the single-source search the landmark / pair / row kernels run, and the
// host functions the units call across.  No relocatable device code: a kernel
// launched from more than one unit is wrapped in a host function where it lives.
#pragma once

#include "gs_internal.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace gs {

static constexpr uint64_t kInfBits = 0x7ff0000000000000ull;
static constexpr int kBbLandmarkRounds = 256;  // frontier rounds per landmark search

// Which rule decided a column (gs_bb_classes / gs_bb_class_counts; include/gsparse.h
// GS_BB_WHY_*).  Recorded only when the caller asks (why != null): a diagnostic for the
// parity tests, which assert that every certificate class fires on their graphs.
enum : uint8_t {
    kWhyOpen = 0,      // not decided by this rank
    kWhySelf,          // self-loop: d(u, u) = 0
    kWhyIsolated,      // an endpoint without G edges: d = inf, keep
    kWhyDeg1,          // an endpoint of degree 1 whose only neighbour is the other: d = w_G
    kWhyDirect,        // w > fl(w_G + eps): prune
    kWhyLocal2,        // w <= fl(mu' + mv')(1 - 2m): keep
    kWhyLmComp,        // a complete landmark reaches one endpoint only: keep
    kWhyLmPrune,       // landmark upper bound: prune
    kWhyLmKeep,        // landmark lower bound: keep
    kWhyWitness,       // 2-hop path: prune
    kWhyLocal34,       // 2- / 3- / 4-edge local lower bound: keep
    kWhySearchPrune,   // the row's search: prune
    kWhySearchKeep,    // the row's search: keep
    kWhyRevExact,      // the reverse row's search, exact rule
    kWhyRevPrune,      // the reverse row's search, upper bound: prune
    kWhyRevKeep,       // the reverse row's search, v unreached within the bound: keep
    kWhyMitm,          // meet-in-the-middle certificate (GSPARSE_BB_MITM)
    kWhyClasses
};
__device__ __forceinline__ void bb_set(uint8_t *__restrict__ state, uint8_t *__restrict__ why, int64_t i,
                                       uint8_t st, uint8_t cls) {
    state[i] = st;
    if (why) why[i] = cls;
}

// Part of a column in the sharded form: both columns (u, v) and (v, u) of a pair go to
// the part of its lower-degree endpoint (the larger id after the relabeling, the
// caller's larger id without it), so one part decides both directions of a pair and
// a search's reverse-column decisions (bb_cross_decide) stay within the part.
__device__ __forceinline__ int bb_col_part(int64_t u, int64_t v, int nparts) {
    return (int)((u > v ? u : v) % nparts);
}

// per-source bounded label-correcting search; one workgroup per source.
struct BbSlab {
    unsigned long long *dist;  // n, +inf bits when idle
    int32_t *qflag;            // n, 0 when idle
    int32_t *fa, *fb;          // frontiers, n each
    int32_t *touched;          // n
};

// Bounded label-correcting search from u over G: dist[] (IEEE bits, +inf when
// idle) holds the least fixpoint of d(y) = min_x fl(d(x) + w(x,y)) restricted
// to values <= the bound s_wmax; touched[0 .. s_tcount) lists every node it
// wrote.  After every frontier round the whole workgroup runs hook(), which
// may lower s_wmax (never below a distance still needed) or end the search by
// zeroing s_fcount; a node whose true distance is <= the final bound gets its
// exact value, since no relaxation on its shortest path was ever cut.
template <class Hook>
__device__ void bb_search(const int64_t *__restrict__ gp, const int32_t *__restrict__ gi,
                          const double *__restrict__ gw, int32_t u, const double &s_wmax,
                          unsigned long long *__restrict__ dist, int32_t *__restrict__ qflag,
                          int32_t *__restrict__ fa, int32_t *__restrict__ fb,
                          int32_t *__restrict__ touched, int &s_fcount, int &s_ncount,
                          int &s_tcount, unsigned long long &relax, Hook hook) {
    if (threadIdx.x == 0) {
        dist[u] = 0ull;  // +0.0
        fa[0] = (int32_t)u;
        touched[0] = (int32_t)u;
    }
    __syncthreads();
    int32_t *cur = fa, *nxt = fb;
    while (true) {
        const int fc = s_fcount;
        if (fc == 0) break;
        const double wmax = s_wmax;
        for (int f = threadIdx.x; f < fc; f += blockDim.x) qflag[cur[f]] = 0;
        __syncthreads();
        // edge-parallel expansion: each wave takes 64 frontier nodes, scans their
        // degrees, and its lanes walk the concatenated edge lists 64 at a time
        // (coalesced, balanced across hubs and leaves); a relaxation only
        // issues the 64-bit atomicMin after a plain load shows it improves
        __shared__ int32_t w_pre[16][65];  // per wave (blocks of up to 1024 threads)
        __shared__ int64_t w_beg[16][64];
        __shared__ double w_d[16][64];
        const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
        for (int f0 = wv * 64; f0 < fc; f0 += (int)blockDim.x) {
            const int f = f0 + lane;
            int deg = 0;
            int64_t b = 0;
            double dx = 0.0;
            if (f < fc) {
                const int32_t x = cur[f];
                b = gp[x];
                deg = (int)(gp[x + 1] - b);
                dx = __longlong_as_double(
                    (long long)__hip_atomic_load(&dist[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
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
            w_d[wv][lane] = dx;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            constexpr int U = 4;  // edges per lane per trip, all loads in flight
            for (int e0 = 0; e0 < total; e0 += 64 * U) {
                int32_t y[U];
                unsigned long long nb[U], cur_d[U];
                bool go[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int e = e0 + u * 64 + lane;
                    go[u] = e < total;
                    const int ec = go[u] ? e : 0;
                    int lo = 0, hi = 63;  // largest k with w_pre[k] <= ec
                    while (lo < hi) {
                        const int mid = (lo + hi + 1) >> 1;
                        if (w_pre[wv][mid] <= ec) lo = mid;
                        else hi = mid - 1;
                    }
                    const int64_t ei = w_beg[wv][lo] + (ec - w_pre[wv][lo]);
                    relax += go[u] ? 1 : 0;
                    const double nd = w_d[wv][lo] + gw[ei];
                    go[u] = go[u] && (nd <= wmax);
                    y[u] = gi[ei];
                    nb[u] = (unsigned long long)__double_as_longlong(nd);
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    cur_d[u] = go[u] ? __hip_atomic_load(&dist[y[u]], __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_WORKGROUP)
                                     : 0ull;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (!go[u] || nb[u] >= cur_d[u]) continue;
                    const unsigned long long old = atomicMin(&dist[y[u]], nb[u]);
                    if (nb[u] < old) {
                        if (old == kInfBits) {
                            int t = atomicAdd(&s_tcount, 1);
                            touched[t] = y[u];
                        }
                        if (atomicExch(&qflag[y[u]], 1) == 0) {
                            int q = atomicAdd(&s_ncount, 1);
                            nxt[q] = y[u];
                        }
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
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
        hook();
    }
}

// block-wide max of v (values >= -1) into *out, which holds -1 on entry;
// ends with a barrier
__device__ void bb_block_max(double v, double *out) {
    for (int off = 32; off > 0; off >>= 1) {
        double o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *p = (unsigned long long *)out;
        unsigned long long old = *p;
        while (__longlong_as_double(old) < v) {
            unsigned long long prev = atomicCAS(p, old, (unsigned long long)__double_as_longlong(v));
            if (prev == old) break;
            old = prev;
        }
    }
    __syncthreads();
}

// The GSPARSE_BB_* variables as they are now.  bb_knobs() is the only reader of the
// environment in the backbone units; every stage calls it once on entry (the staged
// form therefore reads per stage, as the tests that set variables around whole runs
// expect).  A field holds the parsed value, not the text: the odd rules are bb_knobs's.
struct BbKnobs {
    bool relabel_set = false;  // RELABEL present: no gap test ...
    bool relabel = true;       // ... and relabel iff != 0
    int landmarks = -1;        // LANDMARKS: K (negative: 0); -1 = unset
    bool lmcoop = true;        // LMCOOP=0: one workgroup per landmark
    bool lmw_set = false;      // LMW: workgroups per landmark (clamped by the geometry)
    int lmw = 0;
    bool locallb = true;       // LOCALLB=0: no local lower bounds
    bool mitm = false;         // MITM != 0 (takes effect only with the local bounds)
    int64_t mitm_slabs = 0;    // MITM_SLABS, 0 = unset (ignored unless positive)
    bool mitm_lm = true;       // MITM_LM=0: complete landmarks expanded like any node
    int64_t slabs = 0;         // SLABS, 0 = unset (ignored unless positive)
    int multi = 0;             // MULTI rounded down to 1/2/4/8/16, 0 = unset
    int threads = 0;           // THREADS: 512 / 1024, anything else 256; 0 = unset
    bool refill = false;       // REFILL present: fill the slabs on every plan
    bool cross = true;         // CROSS=0: no reverse-column decisions
    bool order_rev = true;     // ORDER=desc: hubs first
    bool dynamic = true;       // DYNAMIC=0: static striding of the batches
    double nearfar = 2.0;      // NEARFAR: near-far step in median edge weights, 0 = plain
    const char *trace = nullptr;  // TRACE: file the per-batch records are appended to
    bool debug = false;        // DEBUG present
};
BbKnobs bb_knobs();

// The numbers bb_begin and bb_plan run with; pure host code (gs_bb_geometry exports it).
struct BbGeometry {
    int K = 0;             // landmarks
    bool lm_coop = false;  // their searches spread over the GPU (k_bb_lm_round)
    int lm_mine = 0;       // landmarks l = lpart (mod nranks)
    int lm_W = 0;          // workgroups per landmark of the spread form (lm_mine > 0 only)
    int S = 1;             // sources per workgroup
    int threads = 256;     // of a search workgroup
    int64_t nbatch = 0;    // ceil(nsrc / S)
    int64_t slabs = 0;     // workgroups, each with its label slab
};
BbGeometry bb_geometry(int64_t n, int64_t nsrc, int nranks, int lpart, const BbKnobs &k);

struct BbRun {
    bool begun = false, certified = false, planned = false;
    int64_t n = 0, E = 0;
    double eps = 0.0;
    // max(1e-8, 8 n 2^-53): bounds the relative rounding of folds over simple paths
    double mrg = 1e-8;
    int pair_part = 0, pair_nparts = 1;
    int nranks = 1;  // ranks of the staged form (the search geometry depends on it)
    int lpart = 0;   // this rank's landmarks l = lpart (mod nranks)
    const int64_t *dsrc = nullptr, *ddst = nullptr, *osrc = nullptr, *odst = nullptr;
    const double *dw = nullptr;
    int64_t *gp = nullptr;
    int32_t *gi = nullptr;
    double *gw = nullptr;
    double wmed = 0.0;
    int64_t *optr = nullptr, *order = nullptr;
    uint8_t *state = nullptr;
    // decision classes (gs_bb_classes): why[E] written beside state when why_on
    bool why_on = false;
    uint8_t *why = nullptr;
    int64_t why_E = 0;
    int K = 0;
    double *D = nullptr;
    int32_t *lcomp = nullptr;
    int64_t nsrc = 0, nbatch = 0, slabs = 0;
    int S = 1, bt = 256;
    int64_t *sources = nullptr;
    unsigned long long *dist = nullptr;
    int32_t *qflag = nullptr, *fr = nullptr, *touched = nullptr, *farl = nullptr;
    uint32_t *fm = nullptr;
    uint64_t *skeys = nullptr;
    int64_t *sidx = nullptr, *rpos = nullptr;
    int cross = 1, rev = 1;
    bool keys_ready = false;  // skeys / sidx / rpos built for this run
    bool dynamic = true;
    double delta = 0.0;
    // the search slabs hold +inf labels / zero masks between searches (every batch resets
    // what it touched): the leading bytes of bb_dist / bb_qflag known to be so (bb_slabs)
    size_t dist_clean = 0, q_clean = 0;
    unsigned long long *misc = nullptr;  // [0] unique edges, [1] relaxations, [2] batch
                                         // counter, [3] debug count; misc + 4: bad flag
    hipEvent_t tall = nullptr;           // the "metric_backbone" profile region
};

inline BbRun &bb_run(gs_ctx *c) {
    if (!c->bb) c->bb = std::make_shared<BbRun>();
    return *c->bb;
}

// The six per-slab arrays of `slabs` workgroups searching `width` sources each over n
// nodes (multi: the mask / far-pile arrays of k_bb_sssp_multi too).  The only code that
// sizes bb_dist, bb_qflag, bb_fr, bb_fmask, bb_touched and bb_far; dist and qflag come
// back idle (+inf / zero): what the run's record does not show idle is filled, all of
// it when `fill_all` (GSPARSE_BB_REFILL, and the callers that fill on every call).
struct BbSlabs {
    unsigned long long *dist;
    int32_t *qflag, *fr, *touched, *farl;
    uint32_t *fm;
};
BbSlabs bb_slabs(gs_ctx *c, int width, int64_t slabs, int64_t n, bool multi, bool fill_all);
void bb_fill_u64(gs_ctx *c, unsigned long long *p, int64_t n, unsigned long long v);

// gs_bb_graph.hip
void bb_build_graph(gs_ctx *c, int64_t n, int64_t E, const int64_t *dsrc, const int64_t *ddst,
                    const int64_t *osrc, const int64_t *odst, const double *dw,
                    unsigned long long *misc, int64_t *&gp, int32_t *&gi, double *&gw,
                    double *wmed = nullptr, int64_t *gnnz = nullptr);
// degree relabeling of the uploaded columns (where it pays): dsrc / ddst become the new ids
void bb_relabel(gs_ctx *c, const BbKnobs &k, int64_t n, int64_t E, const double *w, int loc,
                const int64_t *&dsrc, const int64_t *&ddst);
void bb_group_columns(gs_ctx *c, BbRun &R);  // R.order / R.optr: the columns by source row
void bb_top_degree(gs_ctx *c, const int64_t *gp, int64_t n, int K, int32_t *out);
void bb_keys(gs_ctx *c);
// gs_bb_landmarks.hip
void bb_landmarks(gs_ctx *c, BbRun &R, const BbGeometry &g, int lpart, int lparts, int64_t gnnz,
                  bool debug);
// gs_bb_certify.hip, gs_bb_mitm.hip
void bb_certify(gs_ctx *c, int part, int nparts);
void bb_mitm(gs_ctx *c, BbRun &R, const BbKnobs &k, int64_t c0, int64_t c1, int part, int nparts);
// gs_bb_search.hip
void bb_search_batches(gs_ctx *c, int64_t b0, int64_t b1, int part, int nparts);
// GSPARSE_BB_TRACE=file: each batch's start / end (constant clock, 100 MHz) and
// workgroup; bb_trace_begin zeroes nrec records for the launch to fill (null without a
// file), bb_trace_end waits for the launch and appends one JSON line, `prefix` first
struct BbTrace {
    const char *path;
    unsigned long long *rec;
    int64_t nrec;
};
BbTrace bb_trace_begin(gs_ctx *c, const char *path, int64_t nrec);
void bb_trace_end(gs_ctx *c, const BbTrace &t, const char *prefix, int part, int nparts, int64_t b0,
                  int64_t b1, int S, int64_t grid);

}  // namespace gs
