// gs_segrank.hip -- the rank of every edge_index column inside its source node's segment
// (gs_segment_rank), and the local-filter score built on it (gs_local_scores): what the
// local sparsifiers (L-Spar, Local Degree, NetworKit's local filter) need, sparsify_local.
//
// Column i is better than column j when (order_key(score), column id) is lexicographically
// larger -- keep_lowest: smaller -- a strict total order (gs_topk_mask's keys: -0.0 == +0.0,
// NaN the largest).  rank[i] = the better columns among those with src == src[i].  The
// kernels compare the pair (k, c) = (key, column id), both complemented for keep_lowest, so
// that better is always "larger".  The tie is broken by the column id itself, never by the
// position in the grouped list: the scatter of an unsorted src places columns in atomic
// order, the ranks are the same bytes on every run all the same.
//
// Segments and node lists: seg_build (gs_seg.hpp, shared with gs_segment_topk).  Ranks by length:
//   d <= 64      SHORT     sub-wave groups of 8 / 16 / 64 lanes, one (k, c) per lane; the
//                          rank is a count over the group of the pairs that are larger:
//                          each key is read once, each rank written once.  The count is
//                          quadratic, d^2 <= 4096 compares of register operands per
//                          segment, below what staging and ordering 64 pairs would cost
//   d <= LDS max LDS       up to 512 columns (MID) one wave per segment: (k, c) staged
//                          once in the wave's LDS slice and the same count, every lane
//                          reading the same staged pair per step: d steps of ceil(d / 64)
//                          compares a lane and two workgroup barriers, where the sort
//                          below costs such a segment 36 to 45 (DESIGN.md 4k has the
//                          measured times of both and why the bound is 512).  Above, one
//                          workgroup per segment; (k, c) staged once in LDS (12 bytes a
//                          column) and a bitonic sort of 16-bit positions that compares the
//                          staged pairs: O(d log^2 d) compare-exchanges of 2-byte elements,
//                          position r of the sorted list is rank r.  8192 columns: 96 KiB
//                          of pairs + 16 KiB of positions, one workgroup of 1024 per CU;
//                          up to 2048 columns 28 KiB and 256 threads, five per CU
//   beyond       STREAM    hubs are rare: their column ids are gathered, sorted by column
//                          (the gather's order is the atomic one), stably by order_key and
//                          stably by source with rocPRIM's radix sort; position p of d in
//                          its source's run is rank d - 1 - p (keep_lowest: p)
// GSPARSE_SEGR_MODE=sort takes every segment through the STREAM formulation (all columns
// are already in column order: two sorts), the A/B baseline of DESIGN.md §4k.
// GSPARSE_SEGR_SHORT_MAX / GSPARSE_SEGR_LDS_MAX lower the class limits.
// The host waits once, for the header; the sorts of the STREAM class follow that wait.
//
// gs_local_scores: x = T[rank + 1] / T[deg] (0 for rank 0) per column, one IEEE divide on
// a table the host computed; y = the minimum of x over the columns of an unordered pair
// (gs_undirected_ids), an integer atomicMin on the bit pattern of the non-negative doubles
// -- order-preserving, exact, independent of the arrival order; out = 1 - y.
#include <cstring>

#include "gs_keys.hpp"
#include "gs_seg.hpp"
#include "gs_sort.hpp"
#include "gs_wave.hpp"

namespace gs {

static constexpr int kSegrLdsMax = 8192;  // 12 + 2 bytes a column: 112 KiB of the CU's 160

__device__ __forceinline__ uint64_t segr_key(double s, int lowest) {
    const uint64_t k = order_key(s);
    return lowest ? ~k : k;
}
__device__ __forceinline__ uint32_t segr_col(int64_t col, int lowest) {
    return lowest ? ~(uint32_t)col : (uint32_t)col;
}

__global__ void __launch_bounds__(256) k_segr_deg(int64_t n, const int64_t *__restrict__ off,
                                                  const SegkHdr *__restrict__ hdr, int64_t *__restrict__ deg) {
    if (hdr->bad) return;
    for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < n;
         u += (int64_t)gridDim.x * blockDim.x)
        deg[u] = off[u + 1] - off[u];
}

// SHORT: W lanes per segment, one pair per lane.  LISTED: the segments of list L (their
// lengths in (W / 2 or 8, W]); else every node of <= min(8, smax) columns.
template <int W, bool LISTED>
__global__ void __launch_bounds__(256) k_segr_short(const double *__restrict__ s, const int64_t *__restrict__ off,
                                                    const int64_t *__restrict__ cols,
                                                    const SegkHdr *__restrict__ hdr,
                                                    const int64_t *__restrict__ list, int L, int64_t n, int smax,
                                                    int lowest, int32_t *__restrict__ rank) {
    if (hdr->bad) return;
    const int64_t *cl = hdr->unsorted ? cols : nullptr;
    const int64_t total = LISTED ? (int64_t)hdr->nlist[L] : n;
    const int64_t lbase = LISTED ? (int64_t)hdr->base[L] : 0;
    constexpr int GPW = 64 / W;  // segments per wave and trip
    const int lane = threadIdx.x & 63, g = lane / W, sl = lane % W;
    const int64_t wv = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    // g0 is the same in every lane of the wave: whole waves run every trip
    for (int64_t g0 = wv * GPW; g0 < total; g0 += nw * GPW) {
        const int64_t idx = g0 + g;
        int64_t lo = 0;
        int d = 0;
        if (idx < total) {
            const int64_t u = LISTED ? list[lbase + idx] : idx;
            lo = off[u];
            const int64_t dd = off[u + 1] - lo;
            d = LISTED ? (dd <= W ? (int)dd : 0) : (dd <= 8 && dd <= smax) ? (int)dd : 0;
        }
        const bool have = sl < d;
        const int64_t col = have ? (cl ? cl[lo + sl] : lo + sl) : 0;
        const uint64_t key = have ? segr_key(s[col], lowest) : 0ull;
        const uint32_t ck = segr_col(col, lowest);
        int better = 0;
#pragma unroll 8
        for (int r = 0; r < W; ++r) {
            const uint64_t ok = __shfl((unsigned long long)key, r, W);
            const uint32_t oc = __shfl(ck, r, W);
            better += r < d && (ok > key || (ok == key && oc > ck));
        }
        if (have) rank[col] = better;
    }
}

// MID: the segments of list L with d <= kSegrMidMax, one wave per segment, four per
// workgroup.  The pairs are staged in the wave's LDS slice; lane j counts, for the columns
// j, j + 64, ..., the staged pairs that are larger (every lane reads the same LDS word: a
// broadcast).  d steps of ceil(d / 64) compares a lane -- 2, 4 or 8 by the segment's length
// -- and two workgroup barriers a segment, where the bitonic sort takes 36 to 45 stages
// with a barrier each.
static constexpr int kSegrMidMax = 512;
static constexpr int kSegrMidQ = kSegrMidMax / 64;

template <int Q>
__device__ __forceinline__ void segr_count(const uint64_t *keys, const uint32_t *cks, int d,
                                           const uint64_t (&k)[kSegrMidQ], const uint32_t (&c)[kSegrMidQ],
                                           int (&better)[kSegrMidQ]) {
    for (int r = 0; r < d; ++r) {
        const uint64_t ok = keys[r];
        const uint32_t oc = cks[r];
#pragma unroll
        for (int q = 0; q < Q; ++q) better[q] += ok > k[q] || (ok == k[q] && oc > c[q]);
    }
}

__global__ void __launch_bounds__(256) k_segr_mid(const double *__restrict__ s, const int64_t *__restrict__ off,
                                                  const int64_t *__restrict__ cols,
                                                  const SegkHdr *__restrict__ hdr,
                                                  const int64_t *__restrict__ list, int L, int lowest,
                                                  int32_t *__restrict__ rank) {
    if (hdr->bad) return;
    constexpr int Q = kSegrMidQ;
    __shared__ uint64_t keys[4][kSegrMidMax];
    __shared__ uint32_t cks[4][kSegrMidMax];
    const int64_t *cl = hdr->unsorted ? cols : nullptr;
    const int64_t total = (int64_t)hdr->nlist[L];
    const int64_t lbase = (int64_t)hdr->base[L];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // g0 is the same in every thread of the workgroup: the barriers are whole
    for (int64_t g0 = blockIdx.x * (int64_t)4; g0 < total; g0 += (int64_t)gridDim.x * 4) {
        const int64_t idx = g0 + w;
        int64_t lo = 0;
        int d = 0;
        if (idx < total) {
            const int64_t u = list[lbase + idx];
            lo = off[u];
            const int64_t dd = off[u + 1] - lo;
            d = dd <= kSegrMidMax ? (int)dd : 0;  // longer ones are k_segr_lds'
        }
        uint64_t k[Q];
        uint32_t c[Q];
        int better[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int i = lane + 64 * q;
            k[q] = 0;
            c[q] = 0;
            better[q] = 0;
            if (i < d) {
                const int64_t col = cl ? cl[lo + i] : lo + i;
                k[q] = keys[w][i] = segr_key(s[col], lowest);
                c[q] = cks[w][i] = segr_col(col, lowest);
            }
        }
        __syncthreads();
        if (d <= 128)  // the same in every lane of the wave
            segr_count<2>(keys[w], cks[w], d, k, c, better);
        else if (d <= 256)
            segr_count<4>(keys[w], cks[w], d, k, c, better);
        else
            segr_count<Q>(keys[w], cks[w], d, k, c, better);
#pragma unroll
        for (int q = 0; q < Q; ++q)
            if (lane + 64 * q < d) rank[lowest ? ~c[q] : c[q]] = better[q];
        __syncthreads();  // the slices are reused by the next segments
    }
}

// LDS: one workgroup of NT threads per segment of list L with more than SKIP columns
// (d <= CAP by the list's definition).  pos[0, N), N = d rounded up to a power of two: positions >= d are the
// padding, worse than every column.
template <int CAP, int NT, int SKIP>
__global__ void __launch_bounds__(NT) k_segr_lds(const double *__restrict__ s, const int64_t *__restrict__ off,
                                                 const int64_t *__restrict__ cols,
                                                 const SegkHdr *__restrict__ hdr,
                                                 const int64_t *__restrict__ list, int L, int lowest,
                                                 int32_t *__restrict__ rank) {
    if (hdr->bad) return;
    __shared__ uint64_t keys[CAP];
    __shared__ uint32_t cks[CAP];
    __shared__ uint16_t pos[CAP];
    static_assert(CAP <= 65536, "16-bit positions");
    const int64_t *cl = hdr->unsorted ? cols : nullptr;
    const int64_t total = (int64_t)hdr->nlist[L];
    const int64_t lbase = (int64_t)hdr->base[L];
    const int tid = threadIdx.x;
    for (int64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const int64_t u = list[lbase + it];
        const int64_t lo = off[u];
        const int64_t dd = off[u + 1] - lo;
        if (dd <= SKIP || dd > CAP) continue;  // the same in every thread
        const int d = (int)dd;
        int N = 2;
        while (N < d) N <<= 1;
        for (int i = tid; i < N; i += NT) {
            pos[i] = (uint16_t)i;
            if (i < d) {
                const int64_t col = cl ? cl[lo + i] : lo + i;
                keys[i] = segr_key(s[col], lowest);
                cks[i] = segr_col(col, lowest);
            }
        }
        __syncthreads();
        for (int k = 2; k <= N; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                // four compare-exchanges a thread at a time (their pairs are disjoint): the
                // positions, then the staged pairs, then the swaps, each as one batch of LDS
                // accesses in flight.  Positions are < N <= CAP, so the padding's (unstaged)
                // pairs are read too and ignored.
                for (int t0 = tid; t0 < (N >> 1); t0 += NT * 4) {
                    int ix[4], lx[4], a[4], b[4];
                    bool sw[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int t = t0 + q * NT;
                        sw[q] = t < (N >> 1);
                        ix[q] = sw[q] ? ((t & ~(j - 1)) << 1) | (t & (j - 1)) : 0;
                        lx[q] = ix[q] | j;
                        a[q] = pos[ix[q]];
                        b[q] = pos[lx[q]];
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        // best first where (i & k) == 0, worst first elsewhere; the last merge
                        // (k == N) is best first throughout: swap when hi is better than lw
                        const int hi = (ix[q] & k) ? a[q] : b[q], lw = (ix[q] & k) ? b[q] : a[q];
                        const uint64_t kh = keys[hi], kl = keys[lw];
                        const uint32_t ch = cks[hi], cw = cks[lw];
                        sw[q] = sw[q] && hi < d && (lw >= d || kh > kl || (kh == kl && ch > cw));
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (sw[q]) {
                            pos[ix[q]] = (uint16_t)b[q];
                            pos[lx[q]] = (uint16_t)a[q];
                        }
                }
                __syncthreads();
            }
        }
        for (int r = tid; r < d; r += NT) {
            const uint32_t ck = cks[pos[r]];
            rank[lowest ? ~ck : ck] = r;
        }
        __syncthreads();  // the staged pairs are reused by the next segment
    }
}

// STREAM: the column ids of the segments of list L, each segment at a cursor's place
__global__ void __launch_bounds__(256) k_segr_gather(const int64_t *__restrict__ off,
                                                     const int64_t *__restrict__ cols,
                                                     const SegkHdr *__restrict__ hdr,
                                                     const int64_t *__restrict__ list, int L, int64_t S,
                                                     unsigned long long *__restrict__ cursor,
                                                     uint32_t *__restrict__ sub) {
    __shared__ unsigned long long sbase;
    const int64_t *cl = hdr->unsorted ? cols : nullptr;
    const int64_t total = (int64_t)hdr->nlist[L];
    const int64_t lbase = (int64_t)hdr->base[L];
    for (int64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const int64_t u = list[lbase + it];
        const int64_t lo = off[u], d = off[u + 1] - lo;
        if (threadIdx.x == 0) sbase = atomicAdd(cursor, (unsigned long long)d);
        __syncthreads();
        const int64_t base = (int64_t)sbase;
        if (base + d <= S)  // always: S is the sum of these lengths
            for (int64_t i = threadIdx.x; i < d; i += blockDim.x)
                sub[base + i] = (uint32_t)(cl ? cl[lo + i] : lo + i);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_segr_iota(int64_t S, uint32_t *__restrict__ sub) {
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < S;
         j += (int64_t)gridDim.x * blockDim.x)
        sub[j] = (uint32_t)j;
}

// SRC: the source of the column; else its score's key
template <bool SRC>
__global__ void __launch_bounds__(256) k_segr_sortkey(const double *__restrict__ s,
                                                      const int64_t *__restrict__ src,
                                                      const uint32_t *__restrict__ sub, int64_t S,
                                                      uint64_t *__restrict__ key) {
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < S;
         j += (int64_t)gridDim.x * blockDim.x)
        key[j] = SRC ? (uint64_t)src[sub[j]] : order_key(s[sub[j]]);
}

// the first position of every source's run
__global__ void __launch_bounds__(256) k_segr_heads(const uint64_t *__restrict__ skey, int64_t S,
                                                    int64_t *__restrict__ start) {
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < S;
         j += (int64_t)gridDim.x * blockDim.x)
        if (j == 0 || skey[j - 1] != skey[j]) start[skey[j]] = j;
}

// runs are ascending in (key, column): the best column is the last (keep_lowest: the first)
__global__ void __launch_bounds__(256) k_segr_assign(const uint64_t *__restrict__ skey,
                                                     const uint32_t *__restrict__ sub, int64_t S,
                                                     const int64_t *__restrict__ start,
                                                     const int64_t *__restrict__ off, int lowest,
                                                     int32_t *__restrict__ rank) {
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < S;
         j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t u = (int64_t)skey[j];
        const int64_t p = j - start[u], d = off[u + 1] - off[u];
        rank[sub[j]] = (int32_t)(lowest ? p : d - 1 - p);
    }
}

static int segr_bits(uint64_t v) {
    int b = 0;
    while (b < 64 && (v >> b)) ++b;
    return b < 1 ? 1 : b;
}

// (key, column) pairs sorted stably by the low `bits` of the key; both point at the
// sorted copies afterwards
static void segr_sort_pairs(gs_ctx *c, uint64_t *&key, uint64_t *&key2, uint32_t *&val, uint32_t *&val2,
                            int64_t S, int bits) {
    const auto r = radix_sort_pairs(c, c->buf("segr_tmp"), key, key2, val, val2, S, 0, bits, c->stream);
    if (r.keys != key) std::swap(key, key2);
    if (r.vals != val) std::swap(val, val2);
}

// The ranks of the S columns of the STREAM list's segments; all: these are all E columns.
static void segr_stream(gs_ctx *c, const double *ds, const int64_t *dsrc, const SegBufs &sb, int64_t E,
                        int64_t n, int64_t S, bool all, int lowest, int32_t *dr) {
    hipStream_t st = c->stream;
    const unsigned g = grid_for(S, 256, 8192);
    uint64_t *key = (uint64_t *)c->buf("segr_key0").ensure(sizeof(uint64_t) * S);
    uint64_t *key2 = (uint64_t *)c->buf("segr_key1").ensure(sizeof(uint64_t) * S);
    uint32_t *val = (uint32_t *)c->buf("segr_val0").ensure(sizeof(uint32_t) * S);
    uint32_t *val2 = (uint32_t *)c->buf("segr_val1").ensure(sizeof(uint32_t) * S);
    hipEvent_t t0 = prof_begin(c);
    int digits = 8 + (segr_bits((uint64_t)(n - 1)) + 7) / 8;
    if (all) {
        k_segr_iota<<<g, 256, 0, st>>>(S, val);
    } else {
        auto *cursor = (unsigned long long *)c->buf("segr_cur").ensure(sizeof(unsigned long long));
        GS_HIP(hipMemsetAsync(cursor, 0, sizeof(unsigned long long), st));
        k_segr_gather<<<grid_for(n, 1, 1024), 256, 0, st>>>(sb.off, sb.cols, sb.hdr, sb.list, SL_STREAM, S,
                                                            cursor, val);
        // into column order
        if (radix_sort_keys(c, c->buf("segr_tmp"), val, val2, S, 0, segr_bits((uint64_t)(E - 1)), st) != val)
            std::swap(val, val2);
    }
    k_segr_sortkey<false><<<g, 256, 0, st>>>(ds, dsrc, val, S, key);
    segr_sort_pairs(c, key, key2, val, val2, S, 64);
    k_segr_sortkey<true><<<g, 256, 0, st>>>(ds, dsrc, val, S, key);
    segr_sort_pairs(c, key, key2, val, val2, S, segr_bits((uint64_t)(n - 1)));
    k_segr_heads<<<g, 256, 0, st>>>(key, S, sb.cnt);  // the scatter cursors are dead
    k_segr_assign<<<g, 256, 0, st>>>(key, val, S, sb.cnt, sb.off, lowest, dr);
    GS_HIP(hipGetLastError());
    // the two key passes (a score or a source gathered, a key written), every 8-bit digit
    // pass reading and writing the (key, column) pairs, one histogram read per sort, the
    // heads, and the ranks (pair read, two node reads, rank written)
    prof_end(c, t0, "segment_rank_sort",
             (2.0 * (4.0 + 8.0 + 8.0) + digits * 2.0 * 12.0 + 2.0 * 8.0 + 8.0 + (12.0 + 24.0 + 4.0)) * (double)S);
}

// what the host reads back from gs_local_scores
struct LocalHdr {
    int bad_rank, small_table;
    unsigned long long n_top;
};

__global__ void __launch_bounds__(256) k_local_fill(int64_t m, unsigned long long *__restrict__ y) {
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < m;
         p += (int64_t)gridDim.x * blockDim.x)
        y[p] = 0x7ff0000000000000ull;  // +inf
}

__global__ void __launch_bounds__(256) k_local_x(const int32_t *__restrict__ rank, const int64_t *__restrict__ src,
                                                 const int64_t *__restrict__ deg,
                                                 const double *__restrict__ table, int64_t ntable,
                                                 const int64_t *__restrict__ pair, int64_t E,
                                                 unsigned long long *__restrict__ y, LocalHdr *__restrict__ hdr) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t d = deg[src[i]];
        const int64_t r = rank[i];
        if (d >= ntable) {
            atomicOr(&hdr->small_table, 1);
            continue;
        }
        if (r < 0 || r >= d) {
            atomicOr(&hdr->bad_rank, 1);
            continue;
        }
        const double x = r == 0 ? 0.0 : table[r + 1] / table[d];  // r + 1 <= d < ntable
        atomicMin(&y[pair[i]], (unsigned long long)__builtin_bit_cast(uint64_t, x));
    }
}

__global__ void __launch_bounds__(256) k_local_out(const int64_t *__restrict__ pair, int64_t E,
                                                   const unsigned long long *__restrict__ y,
                                                   double *__restrict__ out, LocalHdr *__restrict__ hdr) {
    if (hdr->bad_rank || hdr->small_table) return;
    unsigned long long top = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        const double v = 1.0 - __builtin_bit_cast(double, (uint64_t)y[pair[i]]);
        out[i] = v;
        top += v == 1.0;
    }
    top = wave_sum(top);
    if ((threadIdx.x & 63) == 0 && top) atomicAdd(&hdr->n_top, top);
}

}  // namespace gs

using namespace gs;

extern "C" int gs_segment_rank(gs_ctx *c, const double *scores, int s_loc, int64_t nscores,
                               const int64_t *src, int src_loc, int64_t E, int64_t n, int keep_lowest,
                               int32_t *rank, int rank_loc, int64_t *deg, int deg_loc, int64_t *max_deg,
                               int64_t *class_counts, int ncounts) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        GS_CHECK(n >= 1 && E >= 0, GS_EINVAL, "need n >= 1 and E >= 0 (n=%lld, E=%lld)", (long long)n,
                 (long long)E);
        GS_CHECK(nscores >= E, GS_EINVAL,
                 "%lld scores for %lld columns: one score per edge_index column is needed (scores of "
                 "the canonical CSR, which merges duplicates, do not index the columns)",
                 (long long)nscores, (long long)E);
        GS_CHECK(E < (int64_t(1) << 31), GS_EUNSUPPORTED, "E = %lld: ranks and column ids are 32-bit",
                 (long long)E);
        GS_CHECK(E == 0 || (scores && src && rank), GS_EINVAL, "null scores/src/rank");
        GS_CHECK(ncounts >= 0 && (ncounts == 0 || class_counts), GS_EINVAL, "class_counts is null");
        GS_HIP(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        const char *mode = getenv("GSPARSE_SEGR_MODE");
        const bool sort_all = mode && !strcmp(mode, "sort");
        const int lowest = keep_lowest ? 1 : 0;
        // sort mode: no segment is SHORT or LDS
        const int smax = sort_all ? 0 : knob_limit(getenv("GSPARSE_SEGR_SHORT_MAX"), kSegkShortMax);
        const int lmax = sort_all ? 0 : knob_limit(getenv("GSPARSE_SEGR_LDS_MAX"), kSegrLdsMax);
        const int64_t E1 = E ? E : 1;
        const double *ds = (const double *)to_device(c, c->buf("segr_s"), scores, sizeof(double) * E, s_loc);
        const int64_t *dsrc = (const int64_t *)to_device(c, c->buf("segr_src"), src, sizeof(int64_t) * E,
                                                         src_loc);
        int32_t *dr = (int32_t *)out_device(c, c->buf("segr_rank"), rank, sizeof(int32_t) * E1, rank_loc);
        int64_t *dd = deg ? (int64_t *)out_device(c, c->buf("segr_deg"), deg, sizeof(int64_t) * n, deg_loc)
                          : nullptr;
        hipEvent_t t0 = prof_begin(c);
        const SegBufs sb = seg_build(c, dsrc, E, n, 0, smax, lmax);  // k = 0: no segment is "all"
        const unsigned gn = grid_for(n, 256, 8192);
        if (dd) k_segr_deg<<<gn, 256, 0, st>>>(n, sb.off, sb.hdr, dd);
        // the list lengths stay on the device: fixed grids, workgroups without work leave
        if (!sort_all && E) {
            k_segr_short<8, false><<<grid_for(n, 32, 8192), 256, 0, st>>>(ds, sb.off, sb.cols, sb.hdr, sb.list, 0,
                                                                          n, smax, lowest, dr);
            k_segr_short<16, true><<<grid_for(n, 16, 2048), 256, 0, st>>>(ds, sb.off, sb.cols, sb.hdr, sb.list,
                                                                          SL_16, n, smax, lowest, dr);
            k_segr_short<64, true><<<grid_for(n, 4, 2048), 256, 0, st>>>(ds, sb.off, sb.cols, sb.hdr, sb.list,
                                                                         SL_64, n, smax, lowest, dr);
            k_segr_mid<<<grid_for(n, 4, 2048), 256, 0, st>>>(ds, sb.off, sb.cols, sb.hdr, sb.list, SL_LDS1, lowest,
                                                             dr);
            k_segr_lds<kSegkLdsSmall, 256, kSegrMidMax><<<grid_for(n, 1, 2048), 256, 0, st>>>(
                ds, sb.off, sb.cols, sb.hdr, sb.list, SL_LDS1, lowest, dr);
            k_segr_lds<kSegrLdsMax, 1024, 0><<<grid_for(n, 1, 256), 1024, 0, st>>>(ds, sb.off, sb.cols, sb.hdr,
                                                                                   sb.list, SL_LDS2, lowest, dr);
        }
        GS_HIP(hipGetLastError());
        hipEvent_t t1 = prof_begin(c);  // the end of the class kernels: the wait is not theirs
        SegkHdr hh;
        GS_HIP(hipMemcpyAsync(&hh, sb.hdr, sizeof(SegkHdr), hipMemcpyDeviceToHost, st));
        GS_HIP(hipStreamSynchronize(st));
        if (t0 && t1) {
            // src and the scores once, the ranks once, the counts and offsets (scan, two
            // classify passes, the rank kernels), the degrees; an unsorted src is read again
            // and its column ids written and read; the STREAM class has its own entry
            double bytes = 8.0 * 2 * (double)E + 4.0 * (double)E + 8.0 * 6 * (double)n + (dd ? 16.0 * n : 0.0);
            if (hh.unsorted) bytes += 8.0 * 3 * (double)E;
            c->pending.push_back(ProfPending{"segment_rank", t0, t1, bytes});
        }
        GS_CHECK(!hh.bad, GS_EINVAL, "edge_index source out of range [0, %lld)", (long long)n);
        const int64_t S = (int64_t)hh.scols;
        GS_CHECK(S <= E, GS_ESTATE, "segment ranks: %lld columns in hub segments of %lld", (long long)S,
                 (long long)E);
        if (S > 0) segr_stream(c, ds, dsrc, sb, E, n, S, S == E, lowest, dr);
        finish_out(c, rank, dr, sizeof(int32_t) * E, rank_loc);
        if (deg) finish_out(c, deg, dd, sizeof(int64_t) * n, deg_loc);
        if (max_deg) *max_deg = (int64_t)hh.maxdeg;
        const int from[GS_SEGR_CLASSES] = {GS_SEGK_EMPTY, GS_SEGK_SHORT, GS_SEGK_LDS, GS_SEGK_STREAM};
        for (int i = 0; i < ncounts; ++i) class_counts[i] = i < GS_SEGR_CLASSES ? (int64_t)hh.cls[from[i]] : 0;
    });
}

extern "C" int gs_local_scores(gs_ctx *c, const int32_t *rank, int r_loc, const int64_t *src,
                               const int64_t *dst, int e_loc, int64_t E, int64_t n, const int64_t *deg,
                               int d_loc, const double *table, int t_loc, int64_t ntable, double *out,
                               int out_loc, int64_t *n_top) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        GS_CHECK(n >= 1 && E >= 0, GS_EINVAL, "need n >= 1 and E >= 0 (n=%lld, E=%lld)", (long long)n,
                 (long long)E);
        GS_CHECK(n < (int64_t(1) << 31), GS_EUNSUPPORTED, "n = %lld: pair keys are 62-bit", (long long)n);
        GS_CHECK(ntable >= 1 && table, GS_EINVAL, "the table needs an entry per degree 0..max (ntable=%lld)",
                 (long long)ntable);
        if (n_top) *n_top = 0;
        if (E == 0) return;
        GS_CHECK(rank && src && dst && deg && out, GS_EINVAL, "null rank/src/dst/deg/out");
        GS_HIP(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        const int32_t *dr = (const int32_t *)to_device(c, c->buf("lsc_rank"), rank, sizeof(int32_t) * E, r_loc);
        const int64_t *dsrc = (const int64_t *)to_device(c, c->buf("lsc_src"), src, sizeof(int64_t) * E, e_loc);
        const int64_t *ddst = (const int64_t *)to_device(c, c->buf("lsc_dst"), dst, sizeof(int64_t) * E, e_loc);
        const int64_t *ddeg = (const int64_t *)to_device(c, c->buf("lsc_deg"), deg, sizeof(int64_t) * n, d_loc);
        const double *dt = (const double *)to_device(c, c->buf("lsc_table"), table, sizeof(double) * ntable,
                                                     t_loc);
        double *dout = (double *)out_device(c, c->buf("lsc_out"), out, sizeof(double) * E, out_loc);
        int64_t *pair = (int64_t *)c->buf("lsc_pair").ensure(sizeof(int64_t) * E);
        // np.unique's inverse of the undirected keys: equal ids <=> the same unordered pair
        int32_t status = 1;
        int64_t m = 0;
        const int rc = gs_undirected_ids(c, n, E, dsrc, ddst, GS_DEVICE, pair, GS_DEVICE, &m, &status);
        if (rc != GS_OK) throw GsError{rc};
        GS_CHECK(status == 0, GS_EINVAL, "edge_index id out of range [0, %lld)", (long long)n);
        auto *y = (unsigned long long *)c->buf("lsc_y").ensure(sizeof(unsigned long long) * m);
        LocalHdr *hdr = (LocalHdr *)c->buf("lsc_hdr").ensure(sizeof(LocalHdr));
        hipEvent_t t0 = prof_begin(c);
        GS_HIP(hipMemsetAsync(hdr, 0, sizeof(LocalHdr), st));
        const unsigned g = grid_for(E, 256, 8192);
        k_local_fill<<<grid_for(m, 256, 8192), 256, 0, st>>>(m, y);
        k_local_x<<<g, 256, 0, st>>>(dr, dsrc, ddeg, dt, ntable, pair, E, y, hdr);
        k_local_out<<<g, 256, 0, st>>>(pair, E, y, dout, hdr);
        GS_HIP(hipGetLastError());
        // per column: the rank, the source, its degree, two table entries, the pair id (twice),
        // the pair's minimum (one atomic, one read), the score; per pair the fill
        prof_end(c, t0, "local_scores", (4.0 + 8.0 + 8.0 + 16.0 + 16.0 + 16.0 + 8.0) * (double)E + 8.0 * (double)m);
        LocalHdr h;
        GS_HIP(hipMemcpyAsync(&h, hdr, sizeof(LocalHdr), hipMemcpyDeviceToHost, st));
        GS_HIP(hipStreamSynchronize(st));
        GS_CHECK(!h.small_table, GS_EINVAL,
                 "the table holds %lld entries: one per degree 0..max degree is needed", (long long)ntable);
        GS_CHECK(!h.bad_rank, GS_EINVAL, "a rank outside [0, degree of its source)");
        finish_out(c, out, dout, sizeof(double) * E, out_loc);
        if (n_top) *n_top = (int64_t)h.n_top;
    });
}
