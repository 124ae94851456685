// gs_truss.hip -- the trussness of every edge of the resident (symmetric) graph, on the
// device (gs_trussness): t(e) = the largest k whose k-truss contains e, the k-truss being
// the largest subgraph in which every edge lies in at least k - 2 triangles of it.
//
// The level-synchronous peel of Kabir and Madduri's PKT ("Shared-memory graph truss
// decomposition", HiPC 2017), on the simple undirected graph of the CSR pattern (diagonal
// entries take no part, the multiplicities are ignored):
//   ids      entry (u, v), u < v, takes its rank among the upper entries (a prefix sum),
//            entry (v, u) the id of tpos; per undirected edge an int32 sup and a state byte
//            (alive, in the current frontier, processed)
//   support  the owner-side intersection kernels in count mode (gs_common_neighbors), less
//            the stored diagonal entries of the two ends, which that count includes
//   level s  the frontier is the alive edges with sup <= s (k_truss_min finds the smallest
//            alive sup, so empty levels cost nothing; k_truss_scan lists the frontier);
//            every frontier edge has trussness s + 2
//   sub-round (k_truss_peel) one wave per frontier edge e1 = (u, v) -- 4 or 16 waves, each
//            with every 4th or 16th step, while the frontier is short: its lanes stride the
//            shorter of the two sorted neighbour lists and binary-search the longer
//            (gs_tri.hpp's common_pos, shared with the Simmelian backbone); for every
//            common neighbour w, e2 = (u, w), e3 = (v, w):
//              e2 or e3 processed               the triangle is gone already
//              e2 and e3 in the frontier        nothing is left to decrement
//              one of them in the frontier      the lower id of the two frontier edges
//                                               decrements the third edge
//              neither                          e1 decrements both
//            so every alive edge loses exactly one per triangle that dies.  A decrement is
//            one int32 atomicSub; the one that returns s + 1 appends its edge to the next
//            frontier (once per edge: sup only falls), one append atomic per wave step
//            (gs_wave.hpp's wave_reserve, for the appends of e2 and e3 together).
//   between  (k_truss_flip) the current frontier becomes processed, the next one current.
// The state bytes change only between launches; inside a launch other workgroups change
// sup and the append cursor only, both by atomics, so no kernel reads plain memory that
// another workgroup writes in the same launch (the XCD L2s are not coherent for plain
// loads).  Integer atomics only: the trussness, the levels and the sub-rounds are
// properties of the graph, the same on every run; only the order inside a frontier list
// varies, and nothing depends on it.
//
// The tail (k_truss_tail): a sub-round whose frontier has at most GSPARSE_TRUSS_TAIL
// edges, and at most twice as many 64-entry steps over their shorter lists (a hub's edge
// is no work for one CU), is run by one workgroup, which goes on with the sub-rounds of
// the level by itself -- workgroup barriers between the peel and the flip -- until the
// frontier is empty or outgrows either bound, at most `alive` times.  The layering is the
// same; only the host waits differ (a triangular lattice peels one ring per sub-round: one
// wait instead of one each).
#include <climits>
#include <cstdlib>

#include "gs_tri.hpp"
#include "gs_wave.hpp"

namespace gs {

static constexpr uint8_t kTrussAlive = 0, kTrussFrontier = 1, kTrussDone = 2;
static constexpr int kTrussTailThreads = 1024;
static constexpr int64_t kTrussTailDefault = 16;  // the measured table
static constexpr int64_t kTrussTailMax = 1 << 20;

// what the host reads back once per wait: written with vector stores and atomics only
struct TrussCtl {
    unsigned int inv;     // INT_MAX - the smallest alive sup (k_truss_min), so that 0 is "none"
    unsigned int ncur;    // edges of the listed frontier (k_truss_scan, k_truss_tail)
    unsigned int nn[2];   // edges appended to the next frontier (k_truss_peel); sub-rounds
                          // alternate between the two, k_truss_flip zeroes the other one
    unsigned int steps;   // wave-steps (truss_steps) of every frontier listed so far in the
                          // level: the host takes differences (k_truss_scan, k_truss_flip,
                          // k_truss_tail)
    unsigned int rounds;  // sub-rounds the tail ran (odd: the frontier it left is in its
                          // second list) ...
    unsigned int done;    // ... and the edges they processed
    unsigned int pad;
};

// the 64-entry steps a wave takes over the shorter list of edge e: what a sub-round costs
__device__ __forceinline__ unsigned int truss_steps(int32_t e, const int32_t *__restrict__ eu,
                                                    const int32_t *__restrict__ ev,
                                                    const int64_t *__restrict__ ip) {
    const int32_t u = eu[e], v = ev[e];
    const int64_t d = min(ip[u + 1] - ip[u], ip[v + 1] - ip[v]);
    return (unsigned int)((d + 63) >> 6);
}

// GSPARSE_TRUSS_TAIL as it is now: the largest frontier the tail takes, 0 = no tail
static int64_t truss_tail_cap() {
    const char *e = getenv("GSPARSE_TRUSS_TAIL");
    if (!e || !*e) return kTrussTailDefault;
    const long long v = atoll(e);
    return v < 0 ? 0 : v > kTrussTailMax ? kTrussTailMax : (int64_t)v;
}

// GSPARSE_TRUSS_WAVES = 1 / 4 / 16 (an A/B hook): that many waves per frontier edge in every
// sub-round; returns -1 / 2 / 4, or 0 (unset): 16 waves up to kTrussWide16 frontier edges,
// 4 up to kTrussWide4, one above
static constexpr int64_t kTrussWide16 = 4096, kTrussWide4 = 32768;
static int truss_waves() {
    const char *e = getenv("GSPARSE_TRUSS_WAVES");
    const int v = e ? atoi(e) : 0;
    return v == 1 ? -1 : v == 4 ? 2 : v == 16 ? 4 : 0;
}

// flag[e] = entry e is an upper one (flag[nnz] = 0: the scan's last value is the edge
// count); diag[u] = (u, u) is stored
__global__ void k_truss_flags(const int32_t *__restrict__ rows, const int32_t *__restrict__ idx,
                              int64_t nnz, int64_t *__restrict__ flag, uint8_t *__restrict__ diag) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e <= nnz;
         e += (int64_t)gridDim.x * blockDim.x) {
        if (e == nnz) {
            flag[e] = 0;
            continue;
        }
        const int32_t r = rows[e], c = idx[e];
        flag[e] = c > r ? 1 : 0;
        if (c == r) diag[r] = 1;
    }
}

// ids of both entries of a pair, its ends and its support; cnt counts u (v) itself as a
// common neighbour of (u, v) when (u, u) ((v, v)) is stored
__global__ void k_truss_init(const int32_t *__restrict__ rows, const int32_t *__restrict__ idx,
                             const int64_t *__restrict__ tpos, const int64_t *__restrict__ rank,
                             const double *__restrict__ cnt, const uint8_t *__restrict__ diag,
                             int64_t nnz, int32_t *__restrict__ eid, int32_t *__restrict__ eu,
                             int32_t *__restrict__ ev, int *__restrict__ sup) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t r = rows[e], c = idx[e];
        if (c == r) eid[e] = -1;
        if (c <= r) continue;
        const int32_t id = (int32_t)rank[e];
        eu[id] = r;
        ev[id] = c;
        sup[id] = support_less_diag(cnt[e], diag[r], diag[c]);
        eid[e] = id;
        eid[tpos[e]] = id;
    }
}

__global__ void __launch_bounds__(256)
k_truss_min(const uint8_t *__restrict__ state, const int *__restrict__ sup, int64_t m,
            TrussCtl *__restrict__ ctl) {
    int lo = INT_MAX;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m;
         e += (int64_t)gridDim.x * blockDim.x)
        if (state[e] == kTrussAlive) lo = min(lo, sup[e]);
    lo = wave_min(lo);
    if ((threadIdx.x & 63) == 0 && lo != INT_MAX) atomicMax(&ctl->inv, (unsigned int)(INT_MAX - lo));
}

// the frontier of level s = INT_MAX - ctl->inv (written by the launch before): listed in
// cur, marked; one append atomic per wave and step
__global__ void __launch_bounds__(256)
k_truss_scan(uint8_t *__restrict__ state, const int *__restrict__ sup, int64_t m,
             const int32_t *__restrict__ eu, const int32_t *__restrict__ ev,
             const int64_t *__restrict__ ip, int32_t *__restrict__ cur, TrussCtl *__restrict__ ctl) {
    const int s = INT_MAX - (int)ctl->inv;
    const int lane = threadIdx.x & 63;
    for (int64_t b = blockIdx.x * (int64_t)blockDim.x; b < m; b += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = b + threadIdx.x;
        const bool in = e < m && state[e] == kTrussAlive && sup[e] <= s;
        if (!__ballot(in)) continue;  // most trips: nothing to list, no steps to add
        const unsigned int at = wave_append(in, &ctl->ncur);
        unsigned int w = 0;
        if (in) {
            cur[at] = (int32_t)e;
            state[e] = kTrussFrontier;
            w = truss_steps((int32_t)e, eu, ev, ip);
        }
        w = wave_sum(w);
        if (lane == 0) atomicAdd(&ctl->steps, w);
    }
}

// What the tail reads again after it changed it in the same launch -- the state bytes
// and the frontier lists -- it stores and loads with agent-scope atomics (they pass the
// CU's L1, which an atomic by the same workgroup does not refresh), a workgroup barrier
// between the store and the load.  sup is only ever touched by atomicSub.  The grid
// kernel reads what earlier launches wrote: plain loads.
template <bool TAIL, class T>
__device__ __forceinline__ T truss_load(const T *p) {
    if (TAIL) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}
template <bool TAIL, class T>
__device__ __forceinline__ void truss_store(T *p, T v) {
    if (TAIL)
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        *p = v;
}

// The tail's barrier between a store and its load by another wave: s_barrier waits for no
// counter, so every wave first waits until its own stores and atomics are acknowledged
// (vmcnt(0) alone).
__device__ __forceinline__ void truss_tail_sync() {
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
}

// One wave, one frontier edge f of level s, the steps sub, sub + nsub, ... of the shorter
// list (64 entries a step).  nnext: the append cursor (global for the grid kernel, LDS for
// the tail).
template <bool TAIL>
__device__ __forceinline__ void truss_edge(int32_t f, int s, const int64_t *__restrict__ ip,
                                           const int32_t *__restrict__ ix,
                                           const int32_t *__restrict__ eid,
                                           const int32_t *__restrict__ eu,
                                           const int32_t *__restrict__ ev, const uint8_t *state,
                                           int *sup, int32_t *next, unsigned int *nnext, int lane,
                                           int32_t sub, int32_t nsub) {
    const int32_t u = eu[f], v = ev[f];
    const TriRows l(ip, u, v);
    for (int32_t i0 = sub * 64; i0 < l.da; i0 += nsub * 64) {  // wave-uniform trips: the ballots are whole
        const int32_t i = i0 + lane;
        int32_t d2 = -1, d3 = -1;  // the edges this lane decrements
        const int32_t at = i < l.da ? common_pos(ix, l, u, v, i) : -1;
        if (at >= 0) {
            const int32_t e2 = eid[l.pa + i], e3 = eid[l.pb + at];
            const uint8_t s2 = truss_load<TAIL>(state + e2), s3 = truss_load<TAIL>(state + e3);
            if (s2 != kTrussDone && s3 != kTrussDone) {
                const bool f2 = s2 == kTrussFrontier, f3 = s3 == kTrussFrontier;
                if (!f2 && !f3) {
                    d2 = e2;
                    d3 = e3;
                } else if (f2 && !f3) {
                    if (f < e2) d3 = e3;
                } else if (f3 && !f2) {
                    if (f < e3) d2 = e2;
                }
            }
        }
        const bool a2 = d2 >= 0 && atomicSub(sup + d2, 1) == s + 1;
        const bool a3 = d3 >= 0 && atomicSub(sup + d3, 1) == s + 1;
        const unsigned long long m2 = __ballot(a2), m3 = __ballot(a3);
        const unsigned int c2 = (unsigned int)__popcll(m2), c3 = (unsigned int)__popcll(m3);
        if (c2 + c3 == 0) continue;
        const unsigned int base = wave_reserve(c2 + c3, nnext);
        if (a2) truss_store<TAIL>(next + base + lanes_below(m2), d2);
        if (a3) truss_store<TAIL>(next + base + c2 + lanes_below(m3), d3);
    }
}

// 2^lw waves per frontier edge (the host's choice by the frontier's length: a short
// frontier leaves most of the chip idle while one wave walks a hub's list), each with its
// own ballots and its own append atomic; gridDim.x * 4 is a multiple of 2^lw
__global__ void __launch_bounds__(256)
k_truss_peel(const int32_t *__restrict__ cur, unsigned int ncur, int s, int lw,
             const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
             const int32_t *__restrict__ eid, const int32_t *__restrict__ eu,
             const int32_t *__restrict__ ev, const uint8_t *__restrict__ state, int *sup,
             int32_t *__restrict__ truss, int32_t *__restrict__ next, unsigned int *nnext) {
    const int lane = threadIdx.x & 63;
    const unsigned int gw = blockIdx.x * 4u + (threadIdx.x >> 6);
    const int32_t sub = (int32_t)(gw & ((1u << lw) - 1u));
    const unsigned int ne = (gridDim.x * 4u) >> lw;
    for (unsigned int k = gw >> lw; k < ncur; k += ne) {
        const int32_t f = cur[k];
        if (lane == 0 && sub == 0) truss[f] = s + 2;
        truss_edge<false>(f, s, ip, ix, eid, eu, ev, state, sup, next, nnext, lane, sub, 1 << lw);
    }
}

// par: which of ctl->nn counted this sub-round's appends; the other one is zeroed for the next
__global__ void k_truss_flip(const int32_t *__restrict__ cur, unsigned int ncur,
                             const int32_t *__restrict__ next, TrussCtl *__restrict__ ctl, int par,
                             const int32_t *__restrict__ eu, const int32_t *__restrict__ ev,
                             const int64_t *__restrict__ ip, uint8_t *__restrict__ state) {
    const unsigned int nn = ctl->nn[par];
    const unsigned int stride = gridDim.x * blockDim.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->nn[par ^ 1] = 0;
    unsigned int w = 0;
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < ncur; i += stride)
        state[cur[i]] = kTrussDone;
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < nn; i += stride) {
        const int32_t e = next[i];
        state[e] = kTrussFrontier;
        w += truss_steps(e, eu, ev, ip);
    }
    w = wave_sum(w);
    if ((threadIdx.x & 63) == 0 && w) atomicAdd(&ctl->steps, w);
}

// One workgroup: the sub-rounds of level s from the frontier la[0, ncur) of `steps`
// wave-steps on, while the frontier is neither empty nor above cap edges or 2 cap steps; at
// most `bound` (the alive edges) of them.  base: ctl->steps as the host last read it.
__global__ void __launch_bounds__(kTrussTailThreads)
k_truss_tail(int32_t *la, int32_t *lb, unsigned int ncur, unsigned int steps, unsigned int base, int s,
             unsigned int cap, unsigned int bound, const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
             const int32_t *__restrict__ eid, const int32_t *__restrict__ eu,
             const int32_t *__restrict__ ev, uint8_t *state, int *sup,
             int32_t *__restrict__ truss, TrussCtl *ctl) {
    __shared__ unsigned int n_next, n_steps[2];  // sub-rounds alternate between the two sums
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned int rounds = 0, done = 0;
    for (unsigned int it = 0; it < bound && ncur > 0 && ncur <= cap && steps <= 2u * cap; ++it) {
        if (tid == 0) n_next = n_steps[it & 1u] = 0;
        truss_tail_sync();
        for (unsigned int k = wave; k < ncur; k += kTrussTailThreads / 64) {
            const int32_t f = truss_load<true>(la + k);
            if (lane == 0) truss[f] = s + 2;
            truss_edge<true>(f, s, ip, ix, eid, eu, ev, state, sup, lb, &n_next, lane, 0, 1);
        }
        truss_tail_sync();  // every decrement of the sub-round is done, lb and n_next are whole
        const unsigned int nn = n_next;
        for (unsigned int i = tid; i < ncur; i += kTrussTailThreads)
            truss_store<true>(state + truss_load<true>(la + i), kTrussDone);
        unsigned int w = 0;
        for (unsigned int i = tid; i < nn; i += kTrussTailThreads) {
            const int32_t e = truss_load<true>(lb + i);
            truss_store<true>(state + e, kTrussFrontier);
            w += truss_steps(e, eu, ev, ip);
        }
        w = wave_sum(w);
        if (lane == 0 && w) atomicAdd(&n_steps[it & 1u], w);
        ++rounds;
        done += ncur;
        ncur = nn;
        int32_t *t = la;
        la = lb;
        lb = t;
        truss_tail_sync();  // the states are in place before the next sub-round loads them
        steps = n_steps[it & 1u];
    }
    if (tid == 0) {
        ctl->ncur = ncur;
        ctl->steps = base + steps;
        ctl->rounds = rounds;
        ctl->done = done;
    }
}

__global__ void k_truss_out(const int32_t *__restrict__ eid, const int32_t *__restrict__ truss,
                            int64_t nnz, double *__restrict__ out) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t id = eid[e];
        out[e] = id < 0 ? 0.0 : (double)truss[id];
    }
}

struct TrussOut {
    int64_t max_truss = 0, rounds = 0, waits = 0;
    int32_t levels = 0;
};

// one host wait: `bytes` (<= sizeof(TrussCtl)) at src into the context's pinned copy
static const void *truss_wait(gs_ctx *c, const void *src, size_t bytes, TrussOut &o) {
    if (!c->truss_host) GS_HIP(hipHostMalloc(&c->truss_host, sizeof(TrussCtl), hipHostMallocDefault));
    GS_HIP(hipMemcpyAsync(c->truss_host, src, bytes, hipMemcpyDeviceToHost, c->stream));
    GS_HIP(hipStreamSynchronize(c->stream));
    ++o.waits;
    return c->truss_host;
}

static TrussCtl truss_read(gs_ctx *c, const TrussCtl *ctl, TrussOut &o) {
    return *(const TrussCtl *)truss_wait(c, ctl, sizeof(TrussCtl), o);
}

// dout: the supports of gs_common_neighbors on entry, the trussness on return
static TrussOut truss_run(gs_ctx *c, double *dout) {
    Graph &g = c->g;
    hipStream_t st = c->stream;
    const int64_t n = g.n, nnz = g.nnz;
    const int64_t cap = truss_tail_cap();
    const int waves = truss_waves();
    TrussOut o;
    const unsigned gz = grid_for(nnz + 1, 256, 8192);
    // the scan's input and output: dead after k_truss_init, when they hold the two lists
    int64_t *flag = (int64_t *)c->buf("truss_flag").ensure(sizeof(int64_t) * 2 * (nnz + 1));
    int64_t *rank = flag + (nnz + 1);
    uint8_t *diag = (uint8_t *)c->buf("truss_diag").ensure((size_t)n);
    TrussCtl *ctl = (TrussCtl *)c->buf("truss_ctl").ensure(sizeof(TrussCtl));
    GS_HIP(hipMemsetAsync(diag, 0, (size_t)n, st));
    k_truss_flags<<<gz, 256, 0, st>>>(g.rows.as<int32_t>(), g.indices.as<int32_t>(), nnz, flag, diag);
    GS_HIP(hipGetLastError());
    exclusive_scan_i64(c, flag, rank, nnz + 1);
    static_assert(sizeof(TrussCtl) >= sizeof(int64_t), "the edge count is read through the same copy");
    const int64_t m = *(const int64_t *)truss_wait(c, rank + nnz, sizeof(int64_t), o);
    if (m == 0) {  // diagonal entries only
        GS_HIP(hipMemsetAsync(dout, 0, sizeof(double) * nnz, st));
        return o;
    }
    int32_t *eid = (int32_t *)c->buf("truss_eid").ensure(sizeof(int32_t) * nnz);
    int32_t *eu = (int32_t *)c->buf("truss_eu").ensure(sizeof(int32_t) * m);
    int32_t *ev = (int32_t *)c->buf("truss_ev").ensure(sizeof(int32_t) * m);
    int *sup = (int *)c->buf("truss_sup").ensure(sizeof(int) * m);
    int32_t *truss = (int32_t *)c->buf("truss_t").ensure(sizeof(int32_t) * m);
    uint8_t *state = (uint8_t *)c->buf("truss_state").ensure((size_t)m);
    GS_HIP(hipMemsetAsync(state, kTrussAlive, (size_t)m, st));
    k_truss_init<<<gz, 256, 0, st>>>(g.rows.as<int32_t>(), g.indices.as<int32_t>(),
                                     g.tpos.as<int64_t>(), rank, dout, diag, nnz, eid, eu, ev, sup);
    GS_HIP(hipGetLastError());
    int32_t *cur = (int32_t *)flag, *nxt = cur + m;  // 2 m int32 <= 2 (nnz + 1) int64

    const int64_t *ip = g.indptr.as<int64_t>();
    const int32_t *ix = g.indices.as<int32_t>();
    const unsigned gm = grid_for(m, 256, 8192);
    int64_t alive = m;
    int s = 0, par = 0;
    while (alive > 0) {
        GS_HIP(hipMemsetAsync(ctl, 0, sizeof(TrussCtl), st));
        k_truss_min<<<gm, 256, 0, st>>>(state, sup, m, ctl);
        k_truss_scan<<<gm, 256, 0, st>>>(state, sup, m, eu, ev, ip, cur, ctl);
        GS_HIP(hipGetLastError());
        TrussCtl h = truss_read(c, ctl, o);
        int64_t ncur = h.ncur;
        const int smin = INT_MAX - (int)h.inv;
        GS_CHECK(ncur > 0 && ncur <= alive && smin >= s, GS_ESTATE,
                 "trussness: level %d lists %lld of %lld alive edges", smin, (long long)ncur,
                 (long long)alive);
        s = smin;
        ++o.levels;
        unsigned int base = h.steps, steps = h.steps;  // ctl->steps as last read; the frontier's share
        while (ncur > 0) {
            if (cap > 0 && ncur <= cap && steps <= 2u * (unsigned)cap) {
                k_truss_tail<<<1, kTrussTailThreads, 0, st>>>(cur, nxt, (unsigned)ncur, steps, base, s,
                                                              (unsigned)cap, (unsigned)alive, ip, ix, eid,
                                                              eu, ev, state, sup, truss, ctl);
                GS_HIP(hipGetLastError());
                h = truss_read(c, ctl, o);
                GS_CHECK(h.rounds > 0 && (int64_t)h.done <= alive, GS_ESTATE,
                         "trussness: the tail ran %u sub-rounds over %u edges", h.rounds, h.done);
                o.rounds += h.rounds;
                alive -= h.done;
                ncur = h.ncur;
                if (h.rounds & 1u) std::swap(cur, nxt);
            } else {
                const int lw = waves < 0 ? 0 : waves > 0 ? waves : ncur <= kTrussWide16 ? 4 : ncur <= kTrussWide4 ? 2 : 0;
                const unsigned blocks = 4u * grid_for(ncur << lw, 16, 1 << 14);
                k_truss_peel<<<blocks, 256, 0, st>>>(cur, (unsigned)ncur, s, lw, ip, ix, eid, eu, ev, state,
                                                     sup, truss, nxt, &ctl->nn[par]);
                k_truss_flip<<<grid_for(ncur, 256, 1024), 256, 0, st>>>(cur, (unsigned)ncur, nxt, ctl, par,
                                                                        eu, ev, ip, state);
                GS_HIP(hipGetLastError());
                h = truss_read(c, ctl, o);
                ++o.rounds;
                alive -= ncur;
                ncur = h.nn[par];
                par ^= 1;
                std::swap(cur, nxt);
            }
            steps = h.steps - base;
            base = h.steps;
            GS_CHECK(ncur <= alive, GS_ESTATE, "trussness: a frontier of %lld with %lld edges alive",
                     (long long)ncur, (long long)alive);
        }
    }
    o.max_truss = s + 2;
    k_truss_out<<<gz, 256, 0, st>>>(eid, truss, nnz, dout);
    GS_HIP(hipGetLastError());
    return o;
}

}  // namespace gs

using namespace gs;

extern "C" int gs_trussness(gs_ctx *c, double *out, int loc, int64_t *max_truss, int32_t *levels,
                            int64_t *rounds, int64_t *host_waits) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        Graph &g = c->g;
        ensure_transpose(c);
        GS_CHECK(g.symmetric, GS_EUNSUPPORTED, "trussness needs a symmetric graph");
        GS_CHECK(g.nnz < (int64_t(1) << 31) - 1, GS_EUNSUPPORTED, "nnz = %lld: edge ids are 32-bit",
                 (long long)g.nnz);
        GS_HIP(hipSetDevice(c->device));
        double *dout = (double *)out_device(c, c->outbuf, out, sizeof(double) * (g.nnz ? g.nnz : 1), loc);
        TrussOut o;
        if (g.nnz) {
            support_pass(c, dout);
            o = truss_run(c, dout);
        }
        finish_out(c, out, dout, sizeof(double) * g.nnz, loc);
        if (max_truss) *max_truss = o.max_truss;
        if (levels) *levels = o.levels;
        if (rounds) *rounds = o.rounds;
        if (host_waits) *host_waits = o.waits;
    });
}
