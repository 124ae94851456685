// gs_seg.hip -- the segments of an edge_index by source node, as the segmented top-k
// (gs_segtopk.hip) and the segment ranks (gs_segrank.hip) use them (seg_build): columns per
// node (in the range-check pass, which also detects a sorted src), exclusive scan, and --
// only for an unsorted src -- a scatter of the column ids (a sorted src is its own grouping:
// column id = position); then the nodes classified by segment length into one list per
// kernel.  Nothing here waits for the host.
#include "gs_seg.hpp"

namespace gs {

// range check, sortedness, columns per node -- one read of src.  A wave's 64 consecutive
// columns are cut into runs of one source and the head of a run adds its length: one
// atomic per run (a sorted src: per node and wave), not per column.
__global__ void __launch_bounds__(256) k_segk_check(const int64_t *__restrict__ src, int64_t E, int64_t n,
                                                           SegkHdr *__restrict__ hdr, int64_t *__restrict__ cnt) {
    int bad = 0, uns = 0;
    const int lane = threadIdx.x & 63;
    // b0 is the same in every lane of the wave: whole waves run every trip
    for (int64_t b0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x - lane; b0 < E;
         b0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = b0 + lane;
        const bool in = i < E;
        const int64_t u = in ? src[i] : -1;
        const bool ok = in && u >= 0 && u < n;
        bad |= in && !ok;
        const int64_t up = __shfl_up((long long)u, 1, 64);
        const int64_t prev = lane ? up : (ok && i > 0 ? src[i - 1] : u);
        uns |= ok && prev > u;
        const bool head = ok && (lane == 0 || up != u);
        // a run ends at the next head, or at a lane without a valid source
        const unsigned long long ends = __ballot(head) | ~__ballot(ok);
        if (head) {
            const unsigned long long above = ends & ~((2ull << lane) - 1ull);
            const int end = above ? __builtin_ctzll(above) : 64;
            atomicAdd((unsigned long long *)&cnt[u], (unsigned long long)(end - lane));
        }
    }
    if (bad) atomicOr(&hdr->bad, 1);
    if (uns) atomicOr(&hdr->unsorted, 1);
}

// unsorted src only: column ids grouped by source (any order inside a segment)
__global__ void __launch_bounds__(256) k_segk_scatter(const int64_t *__restrict__ src, int64_t E,
                                                             const SegkHdr *__restrict__ hdr,
                                                             const int64_t *__restrict__ off,
                                                             int64_t *__restrict__ cur, int64_t *__restrict__ cols) {
    if (hdr->bad || !hdr->unsorted) return;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t u = src[i];
        const int64_t p = off[u] + (int64_t)atomicAdd((unsigned long long *)&cur[u], 1ull);
        cols[p] = i;
    }
}

// nodes per class and per list, the longest segment, the STREAM list's columns
__global__ void __launch_bounds__(256) k_segk_classify(int64_t n, int64_t k, const int64_t *__restrict__ off,
                                                              SegkHdr *__restrict__ hdr, int smax, int lmax) {
    if (hdr->bad) return;
    __shared__ unsigned int sc[GS_SEGK_CLASSES + SL_COUNT];
    __shared__ unsigned long long smx, ssc;
    if (threadIdx.x < GS_SEGK_CLASSES + SL_COUNT) sc[threadIdx.x] = 0;
    if (threadIdx.x == 0) smx = ssc = 0;
    __syncthreads();
    unsigned long long mx = 0, scn = 0;
    for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < n;
         u += (int64_t)gridDim.x * blockDim.x) {
        const int64_t d = off[u + 1] - off[u];
        const int l = segk_list(d, smax, lmax);
        atomicAdd(&sc[segk_class(d, k, smax, lmax)], 1u);
        if (l >= 0) atomicAdd(&sc[GS_SEGK_CLASSES + l], 1u);
        mx = (unsigned long long)d > mx ? (unsigned long long)d : mx;
        if (l == SL_STREAM) scn += (unsigned long long)d;
    }
    if (mx) atomicMax(&smx, mx);
    if (scn) atomicAdd(&ssc, scn);
    __syncthreads();
    if (threadIdx.x < GS_SEGK_CLASSES + SL_COUNT && sc[threadIdx.x]) {
        unsigned long long *dst = threadIdx.x < GS_SEGK_CLASSES ? &hdr->cls[threadIdx.x]
                                                                : &hdr->nlist[threadIdx.x - GS_SEGK_CLASSES];
        atomicAdd(dst, (unsigned long long)sc[threadIdx.x]);
    }
    if (threadIdx.x == 0) {
        if (smx) atomicMax(&hdr->maxdeg, smx);
        if (ssc) atomicAdd(&hdr->scols, ssc);
    }
}

// The lists.  A workgroup counts the nodes of its trips per list, takes its places with one
// cursor atomic per list (the cursors are five addresses: an atomic per node, or per wave,
// is what this pass would cost), and walks its nodes again to write them.
__global__ void __launch_bounds__(256) k_segk_lists(int64_t n, const int64_t *__restrict__ off,
                                                           SegkHdr *__restrict__ hdr, int smax, int lmax,
                                                           int64_t *__restrict__ list) {
    if (hdr->bad) return;
    __shared__ unsigned int cnt[SL_COUNT], cur[SL_COUNT];
    __shared__ unsigned long long at[SL_COUNT];
    if (threadIdx.x < SL_COUNT) cnt[threadIdx.x] = cur[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < n;
         u += (int64_t)gridDim.x * blockDim.x) {
        const int l = segk_list(off[u + 1] - off[u], smax, lmax);
        if (l >= 0) atomicAdd(&cnt[l], 1u);
    }
    __syncthreads();
    if (threadIdx.x < SL_COUNT && cnt[threadIdx.x])
        at[threadIdx.x] = hdr->base[threadIdx.x] +
                          atomicAdd(&hdr->fill[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
    __syncthreads();
    for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < n;
         u += (int64_t)gridDim.x * blockDim.x) {
        const int l = segk_list(off[u + 1] - off[u], smax, lmax);
        if (l >= 0) list[at[l] + atomicAdd(&cur[l], 1u)] = u;
    }
}

__global__ void k_segk_bases(SegkHdr *hdr) {
    unsigned long long acc = 0;
    for (int l = 0; l < SL_COUNT; ++l) {
        hdr->base[l] = acc;
        acc += hdr->nlist[l];
    }
}

SegBufs seg_build(gs_ctx *c, const int64_t *dsrc, int64_t E, int64_t n, int64_t k, int smax, int lmax) {
    hipStream_t st = c->stream;
    const int64_t E1 = E ? E : 1, n1 = n ? n : 1;
    SegBufs b;
    b.hdr = (SegkHdr *)c->buf("segk_hdr").ensure(sizeof(SegkHdr));
    b.cnt = (int64_t *)c->buf("segk_cnt").ensure(sizeof(int64_t) * (n + 1));
    b.off = (int64_t *)c->buf("segk_off").ensure(sizeof(int64_t) * (n + 1));
    b.cols = (int64_t *)c->buf("segk_cols").ensure(sizeof(int64_t) * E1);
    b.list = (int64_t *)c->buf("segk_list").ensure(sizeof(int64_t) * n1);
    GS_HIP(hipMemsetAsync(b.hdr, 0, sizeof(SegkHdr), st));
    GS_HIP(hipMemsetAsync(b.cnt, 0, sizeof(int64_t) * (n + 1), st));
    const unsigned ge = grid_for(E, 256, 8192), gn = grid_for(n, 256, 8192);
    k_segk_check<<<ge, 256, 0, st>>>(dsrc, E, n, b.hdr, b.cnt);
    exclusive_scan_i64(c, b.cnt, b.off, n + 1);
    GS_HIP(hipMemsetAsync(b.cnt, 0, sizeof(int64_t) * (n + 1), st));  // now the scatter cursors
    k_segk_scatter<<<ge, 256, 0, st>>>(dsrc, E, b.hdr, b.off, b.cnt, b.cols);
    k_segk_classify<<<gn, 256, 0, st>>>(n, k, b.off, b.hdr, smax, lmax);
    k_segk_bases<<<1, 1, 0, st>>>(b.hdr);
    k_segk_lists<<<grid_for(n, 256, 1024), 256, 0, st>>>(n, b.off, b.hdr, smax, lmax, b.list);
    return b;
}

}  // namespace gs
