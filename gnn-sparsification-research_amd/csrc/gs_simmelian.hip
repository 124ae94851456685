// gs_simmelian.hip -- the Simmelian backbone score of every edge of the resident
// (symmetric) graph, on the device (gs_simmelian; Nick, Lee, Cunningham, Brandes, ASONAM
// 2013): an edge scores by how far its two ends agree on who their strongest ties are.
//
// On the simple undirected graph of the CSR pattern (diagonal entries take no part, the
// multiplicities are ignored): t(u, w) = the triangles through {u, w}.  For an edge
// {u, v} the ego u ranks N(u) \ {v} by t, ties sharing the best rank (0-based), and
// P_k(u|v) holds the neighbours of rank < k -- a tie group enters whole.
//   max_rank = 0   s(u, v) = max over k >= 1 of |P_k(u|v) ∩ P_k(v|u)| / |P_k(u|v) ∪ P_k(v|u)|
//   max_rank = k0  o(u, v) = |P_k0(u|v) ∩ P_k0(v|u)|
// The intersection only grows at k = m_w + 1, m_w the larger of a common neighbour's two
// ranks, and the union never shrinks in between: with j = the common neighbours of
// m <= m_w, candidate m_w is j / (|P_{m_w+1}(u|v)| + |P_{m_w+1}(v|u)| - j), and s is the
// largest candidate -- compared exactly by cross-multiplication in int64, then ONE IEEE
// division.  Integer atomics only: the same bytes on every run.
//
// Stages:
//   counts   t per entry: the support pass of the trussness (support_pass, less the stored
//            diagonals); a diagonal entry gets -1, which ranks last
//   tables   every row ordered by t descending -- gs_segment_rank with the CSR's own row
//            ids, its strict order only sorts -- and scattered: st[ip[u] + rank] = t, the
//            row's sorted counts; rf[e] = the entries of e's row with a larger t (one
//            binary search), the tie-aware rank in the whole row.  With the alter v
//            removed: rank(w) = rf(u, w) - [t(u, v) > t(u, w)], and |P_k(u|v)| is read off
//            the sorted row with one copy of t(u, v) skipped (sim_size)
//   pairs    one unit of work per upper entry u < v, both directions written through
//            tpos: the lanes stride the shorter sorted neighbour list and binary-search the
//            longer (gs_tri.hpp's common_pos, as k_truss_peel); a hit's two entry positions
//            give m_w; lists and keys are appended with gs_wave.hpp's wave_append.  By the
//            shorter list's length, an upper bound on the common neighbours:
//              WAVE   <= 64    one m per lane; j and "the last of equal m" by cross-lane
//                              counts; no LDS
//              MID    <= 512   one wave per pair, the m compacted into the wave's LDS
//                              slice, the same counts over the slice
//              LDS    <= 8192  one workgroup per pair, the m compacted into LDS, a bitonic
//                              sort: position p holds candidate j = p + 1
//              STREAM beyond   the hubs' (pair, m) gathered and radix-sorted (rocPRIM), one
//                              workgroup per pair over its run
//            In overlap mode nothing is ordered: the hits with m < k0 are counted.
// GSPARSE_SIM_WAVE_MAX / _MID_MAX / _LDS_MAX lower the class bounds (gs_sim.hpp); the
// scores do not depend on them.  No kernel reads plain memory that another workgroup
// writes in the same launch: every stage is its own launch.
#include "gs_sim.hpp"
#include "gs_sort.hpp"
#include "gs_tri.hpp"
#include "gs_wave.hpp"

namespace gs {

static constexpr int kSimLdsThreads = 1024;

// what the host reads back: written by atomics only
struct SimHdr {
    unsigned long long cls[SIM_CLASSES];   // pairs per class
    unsigned long long fill[SIM_CLASSES];  // list cursors
    unsigned long long sbound;             // the STREAM pairs' shorter lists, summed
    unsigned long long scur;               // their hits gathered so far
    unsigned long long nonzero;            // pairs with a common neighbour
    unsigned int maxc, pad;                // the most common neighbours of a pair
};

struct SimG {
    const int64_t *ip;
    const int32_t *ix, *rows;
    const int64_t *tpos;
    const uint8_t *diag;
    const int32_t *tt, *st, *rf;  // t per entry; per row sorted descending; larger counts in the row
};

struct SimPair {
    int64_t e, er;  // the entry (u, v) and its reverse
    int32_t u, v, tuv;
    TriRows l;      // the shorter and the longer of the two rows
};

__device__ __forceinline__ SimPair sim_pair(const SimG &g, int64_t e) {
    const int32_t u = g.rows[e], v = g.ix[e];
    return SimPair{e, g.tpos[e], u, v, g.tt[e], TriRows(g.ip, u, v)};
}

// entry i < l.da of the shorter row: m_w when it is a common neighbour w, else -1
__device__ __forceinline__ int32_t sim_probe(const SimG &g, const SimPair &p, int32_t i) {
    const int32_t at = common_pos(g.ix, p.l, p.u, p.v, i);
    if (at < 0) return -1;
    const int64_t ea = p.l.pa + i, eb = p.l.pb + at;
    const int32_t ma = g.rf[ea] - (p.tuv > g.tt[ea]), mb = g.rf[eb] - (p.tuv > g.tt[eb]);
    return ma > mb ? ma : mb;
}

// |P_k(x|y)|, exy the entry (x, y) and txy its count: the row's sorted counts with one
// copy of txy taken out at its first position rf[exy]; below the row's length the size
// is the end of the tie group that holds position k - 1
__device__ __forceinline__ int64_t sim_size(const SimG &g, int32_t x, int64_t exy, int32_t k, int32_t txy) {
    const int64_t base = g.ip[x];
    const int32_t d = (int32_t)(g.ip[x + 1] - base);
    const int32_t L = d - (int32_t)g.diag[x] - 1;
    if (k >= L) return L;
    const int32_t pos = g.rf[exy], j = k - 1;
    const int32_t val = g.st[base + (j < pos ? j : j + 1)];  // j + 1 <= L - 1 < d
    // the first position with a count < val (the diagonal's -1 included)
    const int32_t *__restrict__ row = g.st + base;
    const int32_t lo = partition_point(d, [=](int32_t q) { return row[q] >= val; });
    return (int64_t)lo - (txy >= val);
}

// candidate m with j common neighbours of rank <= m
__device__ __forceinline__ int64_t sim_den(const SimG &g, const SimPair &p, int32_t m, int64_t j) {
    return sim_size(g, p.u, p.e, m + 1, p.tuv) + sim_size(g, p.v, p.er, m + 1, p.tuv) - j;
}

// a / b > c / d, exactly (all four below 2^32)
__device__ __forceinline__ bool sim_better(int64_t a, int64_t b, int64_t c, int64_t d) { return a * d > c * b; }

__device__ __forceinline__ void sim_wave_best(int64_t &num, int64_t &den) {
    for (int off = 32; off > 0; off >>= 1) {
        const int64_t on = __shfl_down((long long)num, off, 64), od = __shfl_down((long long)den, off, 64);
        if (sim_better(on, od, num, den)) {
            num = on;
            den = od;
        }
    }
}

__device__ __forceinline__ void sim_put(const SimPair &p, double *__restrict__ out, int64_t num, int64_t den) {
    const double val = num ? (double)num / (double)den : 0.0;
    out[p.e] = val;
    out[p.er] = val;
}

// a wave's share of the two counters, once per kernel
__device__ __forceinline__ void sim_note(SimHdr *hdr, unsigned int maxc, unsigned long long nz) {
    if (maxc) atomicMax(&hdr->maxc, maxc);
    if (nz) atomicAdd(&hdr->nonzero, nz);
}

__global__ void __launch_bounds__(256) k_sim_diag(const int32_t *__restrict__ rows, const int32_t *__restrict__ idx,
                                                  int64_t nnz, uint8_t *__restrict__ diag) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz;
         e += (int64_t)gridDim.x * blockDim.x)
        if (rows[e] == idx[e]) diag[rows[e]] = 1;
}

// cnt (the support pass's counts) becomes the score gs_segment_rank orders the rows by
__global__ void __launch_bounds__(256) k_sim_counts(const int32_t *__restrict__ rows, const int32_t *__restrict__ idx,
                                                    const uint8_t *__restrict__ diag, int64_t nnz,
                                                    double *__restrict__ cnt, int32_t *__restrict__ tt,
                                                    int64_t *__restrict__ rows64) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t r = rows[e], c = idx[e];
        const int32_t t = r == c ? -1 : support_less_diag(cnt[e], diag[r], diag[c]);
        tt[e] = t;
        cnt[e] = (double)t;
        rows64[e] = r;
    }
}

__global__ void __launch_bounds__(256) k_sim_scatter(const int32_t *__restrict__ rows, const int64_t *__restrict__ ip,
                                                     const int32_t *__restrict__ rank,
                                                     const int32_t *__restrict__ tt, int64_t nnz,
                                                     int32_t *__restrict__ st) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t base = ip[rows[e]];
        const int64_t d = ip[rows[e] + 1] - base;
        const int64_t r = rank[e];
        if (r >= 0 && r < d) st[base + r] = tt[e];  // always: a rank is a position in its row
    }
}

__global__ void __launch_bounds__(256) k_sim_rf(const int32_t *__restrict__ rows, const int64_t *__restrict__ ip,
                                                const int32_t *__restrict__ st, const int32_t *__restrict__ tt,
                                                int64_t nnz, int32_t *__restrict__ rf) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t base = ip[rows[e]];
        const int32_t t = tt[e];
        // the first position with a count <= t
        rf[e] = partition_point((int32_t)(ip[rows[e] + 1] - base), [=](int32_t q) { return st[base + q] > t; });
    }
}

__device__ __forceinline__ int sim_entry_class(const int32_t *__restrict__ rows, const int32_t *__restrict__ idx,
                                               const int64_t *__restrict__ ip, int64_t e, const SimBounds &b,
                                               int64_t &shorter) {
    const int32_t r = rows[e], c = idx[e];
    if (c <= r) return -1;
    shorter = min(ip[r + 1] - ip[r], ip[c + 1] - ip[c]);
    return sim_class(shorter, b);
}

__global__ void __launch_bounds__(256) k_sim_classify(const int32_t *__restrict__ rows, const int32_t *__restrict__ idx,
                                                      const int64_t *__restrict__ ip, int64_t nnz, SimBounds b,
                                                      SimHdr *__restrict__ hdr) {
    __shared__ unsigned int sc[SIM_CLASSES];
    __shared__ unsigned long long ssb;
    if (threadIdx.x < SIM_CLASSES) sc[threadIdx.x] = 0;
    if (threadIdx.x == 0) ssb = 0;
    __syncthreads();
    unsigned long long sb = 0;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz;
         e += (int64_t)gridDim.x * blockDim.x) {
        int64_t shorter = 0;
        const int k = sim_entry_class(rows, idx, ip, e, b, shorter);
        if (k < 0) continue;
        atomicAdd(&sc[k], 1u);
        if (k == SIM_STREAM) sb += (unsigned long long)shorter;
    }
    if (sb) atomicAdd(&ssb, sb);
    __syncthreads();
    if (threadIdx.x < SIM_CLASSES && sc[threadIdx.x])
        atomicAdd(&hdr->cls[threadIdx.x], (unsigned long long)sc[threadIdx.x]);
    if (threadIdx.x == 0 && ssb) atomicAdd(&hdr->sbound, ssb);
}

// the pairs of class k at list[base[k], base[k + 1]): one cursor atomic per wave, step and class
struct SimBases {
    int64_t at[SIM_CLASSES + 1];
};
__global__ void __launch_bounds__(256) k_sim_lists(const int32_t *__restrict__ rows, const int32_t *__restrict__ idx,
                                                   const int64_t *__restrict__ ip, int64_t nnz, SimBounds b,
                                                   SimBases bs, SimHdr *__restrict__ hdr,
                                                   int32_t *__restrict__ list) {
    const int lane = threadIdx.x & 63;
    // e0 is the same in every lane of the wave: the ballots are whole
    for (int64_t e0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x - lane; e0 < nnz;
         e0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = e0 + lane;
        int64_t shorter = 0;
        const int k = e < nnz ? sim_entry_class(rows, idx, ip, e, b, shorter) : -1;
        for (int q = 0; q < SIM_CLASSES; ++q) {
            const int64_t p = bs.at[q] + (int64_t)wave_append(k == q, &hdr->fill[q]);
            if (k == q && p < bs.at[q + 1]) list[p] = (int32_t)e;  // always: the counts are the classify pass's
        }
    }
}

// WAVE: one wave per pair of at most 64 entries in its shorter list
__global__ void __launch_bounds__(256) k_sim_wave(SimG g, const int32_t *__restrict__ list, int64_t total, int32_t k0,
                                                  double *__restrict__ out, SimHdr *__restrict__ hdr) {
    const int lane = threadIdx.x & 63;
    const int64_t gw = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    unsigned int maxc = 0;
    unsigned long long nz = 0;
    for (int64_t it = gw; it < total; it += nw) {  // wave-uniform trips
        const SimPair p = sim_pair(g, list[it]);
        const int32_t m = lane < p.l.da ? sim_probe(g, p, lane) : -1;
        const unsigned int c = (unsigned int)__popcll(__ballot(m >= 0));
        if (!c) continue;  // out is zeroed
        maxc = c > maxc ? c : maxc;
        ++nz;
        if (k0 > 0) {
            const int64_t o = __popcll(__ballot(m >= 0 && m < k0));
            if (lane == 0) sim_put(p, out, o, 1);
            continue;
        }
        int32_t j = 0, later = 0;  // hits of rank <= m; hits of the same rank in a higher lane
        for (int r = 0; r < p.l.da && r < 64; ++r) {
            const int32_t om = __shfl(m, r, 64);
            j += om >= 0 && om <= m;
            later += om == m && r > lane;
        }
        int64_t num = 0, den = 1;
        if (m >= 0 && !later) {
            num = j;
            den = sim_den(g, p, m, j);
        }
        sim_wave_best(num, den);
        if (lane == 0) sim_put(p, out, num, den);
    }
    if (lane == 0) sim_note(hdr, maxc, nz);
}

// MID: one wave per pair of at most kSimMidMax entries in its shorter list, four per
// workgroup; the m compacted into the wave's LDS slice
__global__ void __launch_bounds__(256) k_sim_mid(SimG g, const int32_t *__restrict__ list, int64_t total, int32_t k0,
                                                 double *__restrict__ out, SimHdr *__restrict__ hdr) {
    __shared__ int32_t ms[4][kSimMidMax];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned int maxc = 0;
    unsigned long long nz = 0;
    // g0 is the same in every thread of the workgroup: the barriers are whole
    for (int64_t g0 = blockIdx.x * (int64_t)4; g0 < total; g0 += (int64_t)gridDim.x * 4) {
        const int64_t it = g0 + w;
        const bool have = it < total;
        SimPair p = sim_pair(g, list[have ? it : total - 1]);
        if (!have || p.l.da > kSimMidMax) p.l.da = 0;
        int32_t c = 0, o = 0;
        for (int32_t i0 = 0; i0 < p.l.da; i0 += 64) {  // wave-uniform trips
            const int32_t i = i0 + lane;
            const int32_t m = i < p.l.da ? sim_probe(g, p, i) : -1;
            const unsigned long long mk = __ballot(m >= 0);
            if (m >= 0 && k0 == 0) ms[w][c + lanes_below(mk)] = m;  // c + 63 < da
            c += __popcll(mk);
            o += __popcll(__ballot(m >= 0 && m < k0));
        }
        if (c) {
            maxc = (unsigned int)c > maxc ? (unsigned int)c : maxc;
            ++nz;
        }
        if (k0 > 0) {  // the same in every thread: no barrier is skipped by some
            if (c && lane == 0) sim_put(p, out, o, 1);
            continue;
        }
        __syncthreads();
        int64_t num = 0, den = 1;
        for (int32_t i = lane; i < c; i += 64) {
            const int32_t m = ms[w][i];
            int32_t j = 0, later = 0;
            for (int32_t r = 0; r < c; ++r) {  // every lane reads the same word: a broadcast
                const int32_t om = ms[w][r];
                j += om <= m;
                later += om == m && r > i;
            }
            if (later) continue;
            const int64_t d = sim_den(g, p, m, j);
            if (sim_better(j, d, num, den)) {
                num = j;
                den = d;
            }
        }
        sim_wave_best(num, den);
        if (c && lane == 0) sim_put(p, out, num, den);
        __syncthreads();  // the slices are reused by the next pairs
    }
    if (lane == 0) sim_note(hdr, maxc, nz);
}

// LDS: one workgroup per pair of at most kSimLdsMax entries in its shorter list; in overlap
// mode (k0 > 0: nothing is staged) of any length
__global__ void __launch_bounds__(kSimLdsThreads) k_sim_lds(SimG g, const int32_t *__restrict__ list, int64_t total,
                                                            int32_t k0, double *__restrict__ out,
                                                            SimHdr *__restrict__ hdr) {
    __shared__ uint32_t ms[kSimLdsMax];
    __shared__ unsigned int n_hit, n_low;
    __shared__ int64_t bn[kSimLdsThreads / 64], bd[kSimLdsThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned int maxc = 0;
    unsigned long long nz = 0;
    for (int64_t it = blockIdx.x; it < total; it += gridDim.x) {  // the same in every thread
        const SimPair p = sim_pair(g, list[it]);
        if (k0 == 0 && p.l.da > kSimLdsMax) continue;  // never: the class bound
        if (tid == 0) n_hit = n_low = 0;
        __syncthreads();
        for (int32_t i0 = 0; i0 < p.l.da; i0 += kSimLdsThreads) {  // workgroup-uniform trips
            const int32_t i = i0 + tid;
            const int32_t m = i < p.l.da ? sim_probe(g, p, i) : -1;
            const unsigned long long mk = __ballot(m >= 0), lk = __ballot(m >= 0 && m < k0);
            if (!mk) continue;
            const unsigned int at = wave_reserve((unsigned int)__popcll(mk), &n_hit);
            if (lk) wave_reserve((unsigned int)__popcll(lk), &n_low);
            if (m >= 0 && k0 == 0) ms[at + lanes_below(mk)] = (uint32_t)m;  // < da
        }
        __syncthreads();
        const int32_t c = (int32_t)n_hit;
        if (tid == 0 && c) {
            maxc = (unsigned int)c > maxc ? (unsigned int)c : maxc;
            ++nz;
        }
        if (k0 > 0 || c == 0) {
            if (tid == 0 && c) sim_put(p, out, n_low, 1);
            __syncthreads();  // the counters are zeroed for the next pair
            continue;
        }
        int32_t N = 2;
        while (N < c) N <<= 1;  // <= kSimLdsMax, a power of two
        for (int32_t i = c + tid; i < N; i += kSimLdsThreads) ms[i] = 0xFFFFFFFFu;
        __syncthreads();
        for (int32_t k = 2; k <= N; k <<= 1)
            for (int32_t j = k >> 1; j > 0; j >>= 1) {
                for (int32_t t = tid; t < (N >> 1); t += kSimLdsThreads) {
                    const int32_t ix = ((t & ~(j - 1)) << 1) | (t & (j - 1)), lx = ix | j;
                    const uint32_t a = ms[ix], b = ms[lx];
                    if ((a > b) == ((ix & k) == 0)) {  // ascending where (ix & k) == 0
                        ms[ix] = b;
                        ms[lx] = a;
                    }
                }
                __syncthreads();
            }
        int64_t num = 0, den = 1;
        for (int32_t q = tid; q < c; q += kSimLdsThreads) {
            const uint32_t m = ms[q];
            if (q + 1 < c && ms[q + 1] == m) continue;  // not the last of its rank
            const int64_t d = sim_den(g, p, (int32_t)m, q + 1);
            if (sim_better(q + 1, d, num, den)) {
                num = q + 1;
                den = d;
            }
        }
        sim_wave_best(num, den);
        if (lane == 0) {
            bn[w] = num;
            bd[w] = den;
        }
        __syncthreads();
        if (w == 0) {
            num = lane < kSimLdsThreads / 64 ? bn[lane] : 0;
            den = lane < kSimLdsThreads / 64 ? bd[lane] : 1;
            sim_wave_best(num, den);
            if (lane == 0) sim_put(p, out, num, den);
        }
        __syncthreads();  // ms, the counters and bn / bd are reused by the next pair
    }
    if (tid == 0) sim_note(hdr, maxc, nz);
}

// STREAM: the hits of slot s (the s-th pair of the class) as keys s << 32 | m, appended at
// a cursor: one atomic per wave and step.  The unused keys stay all ones and sort last.
__global__ void __launch_bounds__(256) k_sim_gather(SimG g, const int32_t *__restrict__ list, int64_t total, int64_t S,
                                                    SimHdr *__restrict__ hdr, uint64_t *__restrict__ keys) {
    for (int64_t s = blockIdx.x; s < total; s += gridDim.x) {
        const SimPair p = sim_pair(g, list[s]);
        for (int32_t i0 = 0; i0 < p.l.da; i0 += 256) {  // workgroup-uniform trips
            const int32_t i = i0 + (int32_t)threadIdx.x;
            const int32_t m = i < p.l.da ? sim_probe(g, p, i) : -1;
            const int64_t q = (int64_t)wave_append(m >= 0, &hdr->scur);
            if (m >= 0 && q < S) keys[q] = ((uint64_t)s << 32) | (uint32_t)m;  // always: S sums the lists
        }
    }
}

// the run of slot s in the sorted keys: position q - lo holds candidate j = q - lo + 1
__global__ void __launch_bounds__(256) k_sim_stream(SimG g, const int32_t *__restrict__ list, int64_t total, int64_t S,
                                                    const uint64_t *__restrict__ keys, double *__restrict__ out,
                                                    SimHdr *__restrict__ hdr) {
    __shared__ int64_t bn[4], bd[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned int maxc = 0;
    unsigned long long nz = 0;
    for (int64_t s = blockIdx.x; s < total; s += gridDim.x) {  // the same in every thread
        const SimPair p = sim_pair(g, list[s]);
        int64_t b[2];
        for (int h = 0; h < 2; ++h) b[h] = lower_bound(keys, S, (uint64_t)(s + h) << 32);  // the first key >= (s + h) << 32
        const int64_t c = b[1] - b[0];
        if (c == 0) continue;
        if (tid == 0) {
            maxc = (unsigned int)c > maxc ? (unsigned int)c : maxc;
            ++nz;
        }
        int64_t num = 0, den = 1;
        for (int64_t q = b[0] + tid; q < b[1]; q += 256) {
            if (q + 1 < b[1] && keys[q + 1] == keys[q]) continue;  // not the last of its rank
            const int64_t j = q - b[0] + 1;
            const int64_t d = sim_den(g, p, (int32_t)(uint32_t)keys[q], j);
            if (sim_better(j, d, num, den)) {
                num = j;
                den = d;
            }
        }
        sim_wave_best(num, den);
        if (lane == 0) {
            bn[w] = num;
            bd[w] = den;
        }
        __syncthreads();
        if (tid == 0) {
            for (int q = 1; q < 4; ++q)
                if (sim_better(bn[q], bd[q], num, den)) {
                    num = bn[q];
                    den = bd[q];
                }
            sim_put(p, out, num, den);
        }
        __syncthreads();  // bn / bd are reused by the next pair
    }
    if (tid == 0) sim_note(hdr, maxc, nz);
}

struct SimOut {
    int64_t max_common = 0, nonzero = 0;
    int64_t cls[SIM_CLASSES] = {};
};

static SimHdr sim_read(gs_ctx *c, const SimHdr *hdr) {
    SimHdr h;
    GS_HIP(hipMemcpyAsync(&h, hdr, sizeof(SimHdr), hipMemcpyDeviceToHost, c->stream));
    GS_HIP(hipStreamSynchronize(c->stream));
    return h;
}

// dout [nnz]: scratch for the counts first, the scores on return
static SimOut sim_run(gs_ctx *c, double *dout, int32_t k0) {
    Graph &g = c->g;
    hipStream_t st = c->stream;
    const int64_t n = g.n, nnz = g.nnz;
    const SimBounds b = sim_bounds();
    SimOut o;
    const int32_t *rows = g.rows.as<int32_t>(), *ix = g.indices.as<int32_t>();
    const int64_t *ip = g.indptr.as<int64_t>();
    const unsigned gz = grid_for(nnz, 256, 8192);

    // t per entry, and every row's counts in descending order
    hipEvent_t t0 = prof_begin(c);
    support_pass(c, dout);
    uint8_t *diag = (uint8_t *)c->buf("sim_diag").ensure((size_t)n);
    int32_t *tt = (int32_t *)c->buf("sim_t").ensure(sizeof(int32_t) * nnz);
    int32_t *sorted = (int32_t *)c->buf("sim_sorted").ensure(sizeof(int32_t) * nnz);
    int32_t *rf = (int32_t *)c->buf("sim_rf").ensure(sizeof(int32_t) * nnz);
    int32_t *rank = (int32_t *)c->buf("sim_rank").ensure(sizeof(int32_t) * nnz);
    int64_t *rows64 = (int64_t *)c->buf("sim_rows").ensure(sizeof(int64_t) * nnz);
    GS_HIP(hipMemsetAsync(diag, 0, (size_t)n, st));
    k_sim_diag<<<gz, 256, 0, st>>>(rows, ix, nnz, diag);
    k_sim_counts<<<gz, 256, 0, st>>>(rows, ix, diag, nnz, dout, tt, rows64);
    GS_HIP(hipGetLastError());
    prof_end(c, t0, "simmelian_counts", (4.0 + 4.0 + 8.0 + 8.0 + 4.0 + 8.0) * (double)nnz);
    const int rc = gs_segment_rank(c, dout, GS_DEVICE, nnz, rows64, GS_DEVICE, nnz, n, 0, rank, GS_DEVICE,
                                   nullptr, GS_DEVICE, nullptr, nullptr, 0);
    if (rc != GS_OK) throw GsError{rc};
    t0 = prof_begin(c);
    k_sim_scatter<<<gz, 256, 0, st>>>(rows, ip, rank, tt, nnz, sorted);
    k_sim_rf<<<gz, 256, 0, st>>>(rows, ip, sorted, tt, nnz, rf);

    // the pairs by class
    SimHdr *hdr = (SimHdr *)c->buf("sim_hdr").ensure(sizeof(SimHdr));
    int32_t *list = (int32_t *)c->buf("sim_list").ensure(sizeof(int32_t) * nnz);
    GS_HIP(hipMemsetAsync(hdr, 0, sizeof(SimHdr), st));
    GS_HIP(hipMemsetAsync(dout, 0, sizeof(double) * nnz, st));
    k_sim_classify<<<gz, 256, 0, st>>>(rows, ix, ip, nnz, b, hdr);
    GS_HIP(hipGetLastError());
    // rows, sorted counts and ranks of the two table kernels; rows and both degrees of the
    // two class passes, the list written
    prof_end(c, t0, "simmelian_tables", (4.0 * 6 + 8.0 + 2.0 * (8.0 + 32.0) + 4.0) * (double)nnz);
    SimHdr h = sim_read(c, hdr);
    SimBases bs;
    sim_bases(h.cls, bs.at);
    const int64_t pairs = bs.at[SIM_CLASSES];
    GS_CHECK(pairs <= nnz / 2, GS_ESTATE, "simmelian: %lld pairs of %lld entries", (long long)pairs,
             (long long)nnz);
    for (int k = 0; k < SIM_CLASSES; ++k) o.cls[k] = (int64_t)h.cls[k];
    if (pairs == 0) return o;  // diagonal entries only
    k_sim_lists<<<gz, 256, 0, st>>>(rows, ix, ip, nnz, b, bs, hdr, list);
    GS_HIP(hipGetLastError());

    const SimG sg{ip, ix, rows, g.tpos.as<int64_t>(), diag, tt, sorted, rf};
    const int64_t nwave = o.cls[SIM_WAVE], nmid = o.cls[SIM_MID], nlds = o.cls[SIM_LDS], nstr = o.cls[SIM_STREAM];
    t0 = prof_begin(c);
    if (nwave) k_sim_wave<<<grid_for(nwave, 4, 1 << 15), 256, 0, st>>>(sg, list + bs.at[SIM_WAVE], nwave, k0, dout, hdr);
    GS_HIP(hipGetLastError());
    // per pair its two entries, four row bounds and both outputs; per hit two ranks and two counts
    prof_end(c, t0, "simmelian_wave", (8.0 + 16.0 + 32.0 + 16.0) * (double)nwave);
    t0 = prof_begin(c);
    if (nmid) k_sim_mid<<<grid_for(nmid, 4, 1 << 14), 256, 0, st>>>(sg, list + bs.at[SIM_MID], nmid, k0, dout, hdr);
    GS_HIP(hipGetLastError());
    prof_end(c, t0, "simmelian_mid", (8.0 + 16.0 + 32.0 + 16.0) * (double)nmid);
    // overlap mode orders nothing: the workgroup kernel counts the hubs' pairs too
    const int64_t nwg = k0 > 0 ? nlds + nstr : nlds;
    t0 = prof_begin(c);
    if (nwg)
        k_sim_lds<<<grid_for(nwg, 1, 4096), kSimLdsThreads, 0, st>>>(sg, list + bs.at[SIM_LDS], nwg, k0, dout, hdr);
    GS_HIP(hipGetLastError());
    prof_end(c, t0, "simmelian_lds", (8.0 + 16.0 + 32.0 + 16.0) * (double)nwg);
    if (k0 == 0 && nstr) {
        const int64_t S = (int64_t)h.sbound;
        t0 = prof_begin(c);
        uint64_t *key = (uint64_t *)c->buf("sim_key0").ensure(sizeof(uint64_t) * S);
        uint64_t *key2 = (uint64_t *)c->buf("sim_key1").ensure(sizeof(uint64_t) * S);
        GS_HIP(hipMemsetAsync(key, 0xFF, sizeof(uint64_t) * S, st));
        k_sim_gather<<<grid_for(nstr, 1, 4096), 256, 0, st>>>(sg, list + bs.at[SIM_STREAM], nstr, S, hdr, key);
        GS_HIP(hipGetLastError());
        key = radix_sort_keys(c, c->buf("sim_tmp"), key, key2, S, 0, 64, st);
        k_sim_stream<<<grid_for(nstr, 1, 4096), 256, 0, st>>>(sg, list + bs.at[SIM_STREAM], nstr, S, key, dout, hdr);
        GS_HIP(hipGetLastError());
        // the keys filled, written, sorted in eight digit passes and read; per hit two ranks and two counts
        prof_end(c, t0, "simmelian_stream", (8.0 + 8.0 + 8.0 * 16.0 + 8.0 + 16.0) * (double)S);
    }
    h = sim_read(c, hdr);
    o.max_common = h.maxc;
    o.nonzero = (int64_t)h.nonzero;
    return o;
}

}  // namespace gs

using namespace gs;

extern "C" int gs_simmelian(gs_ctx *c, double *out, int loc, int64_t max_rank, int64_t *max_common,
                            int64_t *nonzero_pairs, int64_t *class_counts, int ncounts) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        GS_CHECK(sim_rank_ok(max_rank), GS_EINVAL, "max_rank must be in [0, 2^31), got %lld", (long long)max_rank);
        GS_CHECK(ncounts >= 0 && (ncounts == 0 || class_counts), GS_EINVAL, "class_counts is null");
        Graph &g = c->g;
        ensure_transpose(c);
        GS_CHECK(g.symmetric, GS_EUNSUPPORTED, "the Simmelian backbone needs a symmetric graph");
        GS_CHECK(g.nnz < (int64_t(1) << 31) - 1, GS_EUNSUPPORTED, "nnz = %lld: entry ids are 32-bit",
                 (long long)g.nnz);
        GS_HIP(hipSetDevice(c->device));
        double *dout = (double *)out_device(c, c->outbuf, out, sizeof(double) * (g.nnz ? g.nnz : 1), loc);
        SimOut o;
        if (g.nnz) o = sim_run(c, dout, (int32_t)max_rank);
        finish_out(c, out, dout, sizeof(double) * g.nnz, loc);
        if (max_common) *max_common = o.max_common;
        if (nonzero_pairs) *nonzero_pairs = o.nonzero;
        for (int i = 0; i < ncounts; ++i) class_counts[i] = i < SIM_CLASSES ? o.cls[i] : 0;
    });
}
