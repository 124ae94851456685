// gs_bb_graph.hip -- the metric backbone's graph stage: G of metric_backbone.py:70-79
// as a symmetric CSR, the degree relabeling, the columns grouped by source row, the
// highest-degree nodes (the landmarks) and the sorted column keys of the reverse-column
// lookup.
#include "gs_bb.hpp"

namespace gs {

static int bits_for_bb(uint64_t v) {
    int b = 0;
    while (b < 64 && (v >> b)) ++b;
    return b < 1 ? 1 : b;
}

// osrc/odst: the caller's ids (which columns are s < d: metric_backbone.py:70-79
// builds G from those); src/dst: the (possibly relabeled) ids G is built in
__global__ void k_bb_keys(const int64_t *__restrict__ src, const int64_t *__restrict__ dst,
                          const int64_t *__restrict__ osrc, const int64_t *__restrict__ odst,
                          const double *__restrict__ w, int64_t E, int64_t n,
                          uint64_t *__restrict__ keys, int64_t *__restrict__ idx,
                          int *__restrict__ bad) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t os = osrc[i], od = odst[i];
        if (os < 0 || os >= n || od < 0 || od >= n) {
            atomicOr(bad, 1);
            keys[i] = (uint64_t)n * (uint64_t)n;
            idx[i] = i;
            continue;
        }
        const int64_t s = src[i], d = dst[i];
        double x = w[i];
        if (!(x >= 0.0)) atomicOr(bad, 2);  // negative or NaN weight
        // undirected edges from s<d columns (caller's ids); others sort to the end
        const uint64_t lo = (uint64_t)(s < d ? s : d), hi = (uint64_t)(s < d ? d : s);
        keys[i] = os < od ? lo * (uint64_t)n + hi : (uint64_t)n * (uint64_t)n;
        idx[i] = i;
    }
}

// runs of equal keys -> unique undirected edges with min weight
__global__ void k_bb_unique(const uint64_t *__restrict__ keys, const int64_t *__restrict__ idx,
                            const double *__restrict__ w, int64_t E, int64_t n,
                            unsigned long long *__restrict__ ucount, uint64_t *__restrict__ ukeys,
                            double *__restrict__ uw) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t k = keys[i];
        if (k >= (uint64_t)n * (uint64_t)n) continue;
        if (i > 0 && keys[i - 1] == k) continue;
        double m = w[idx[i]];
        for (int64_t j = i + 1; j < E && keys[j] == k; ++j) {
            double x = w[idx[j]];
            if (x < m) m = x;
        }
        if (m == 0.0) m = 0.0;
        unsigned long long p = atomicAdd(ucount, 1ull);
        uint64_t u = k / (uint64_t)n, v = k % (uint64_t)n;
        ukeys[2 * p] = u * (uint64_t)n + v;
        ukeys[2 * p + 1] = v * (uint64_t)n + u;
        uw[p] = m;
    }
}

__global__ void k_bb_sym_payload(int64_t cnt2, int64_t *__restrict__ pay) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cnt2;
         i += (int64_t)gridDim.x * blockDim.x)
        pay[i] = i >> 1;
}

__global__ void k_bb_gfill(const uint64_t *__restrict__ skeys, const int64_t *__restrict__ pay,
                           const double *__restrict__ uw, int64_t cnt2, int64_t n,
                           int32_t *__restrict__ gi, double *__restrict__ gw) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cnt2;
         i += (int64_t)gridDim.x * blockDim.x) {
        gi[i] = (int32_t)(skeys[i] % (uint64_t)n);
        gw[i] = uw[pay[i]];
    }
}

// row pointers of keys sorted by row = key / div (rows < n): ptr[r] = the first entry whose
// key is >= r * div, one binary search per row (no atomics: an R-MAT hub's degree counted
// by atomics on one address serialises -- the G fill and the columns-by-row pass took
// 1.6 + 1.2 ms of RMAT-18's begin, round 5; and no per-entry loop over the empty rows
// between entries: the degree relabeling puts ~40 % of the rows, all empty, last)
__global__ void k_bb_rowptr(const uint64_t *__restrict__ keys, int64_t cnt, uint64_t div, int64_t n,
                            int64_t *__restrict__ ptr) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r <= n;
         r += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t t = (uint64_t)r * div;
        int64_t lo = 0, hi = cnt;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (keys[mid] < t) lo = mid + 1;
            else hi = mid;
        }
        ptr[r] = lo;
    }
}

__global__ void k_bb_srckeys(const int64_t *__restrict__ src, int64_t E, uint64_t *__restrict__ keys,
                             int64_t *__restrict__ idx) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        keys[i] = (uint64_t)src[i];
        idx[i] = i;
    }
}

// (row * n + col) key of every column, for the reverse-column lookup
__global__ void k_bb_pairkeys(const int64_t *__restrict__ src, const int64_t *__restrict__ dst,
                              int64_t E, int64_t n, uint64_t *__restrict__ keys,
                              int64_t *__restrict__ idx) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        keys[i] = (uint64_t)src[i] * (uint64_t)n + (uint64_t)dst[i];
        idx[i] = i;
    }
}

// first position of column i's reverse key (col * n + row) in the sorted keys, -1 if
// absent or a self-loop
__global__ void k_bb_revpos(const int64_t *__restrict__ src, const int64_t *__restrict__ dst,
                            int64_t E, int64_t n, const uint64_t *__restrict__ skeys,
                            int64_t *__restrict__ rpos) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t u = src[i], v = dst[i];
        const uint64_t key = (uint64_t)v * (uint64_t)n + (uint64_t)u;
        int64_t lo = 0, hi = E;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (skeys[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        rpos[i] = (u != v && lo < E && skeys[lo] == key) ? lo : -1;
    }
}

// Node relabeling for the searches' locality: node ids ordered by descending
// column count (hubs first, ties by id), so the labels a search touches most
// often share cache lines.  Distances, sums and decisions do not depend on the
// labels (every fold runs along the path from the source), only where the
// searches' distance slabs are read.
__global__ void k_bb_count(const int64_t *__restrict__ src, const int64_t *__restrict__ dst,
                           int64_t E, unsigned long long *__restrict__ cnt) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        atomicAdd(&cnt[src[i]], 1ull);
        atomicAdd(&cnt[dst[i]], 1ull);
    }
}

// sum over columns of |src - dst| (the ids' existing locality), per-wave partials
__global__ void k_bb_gap(const int64_t *__restrict__ src, const int64_t *__restrict__ dst,
                         int64_t E, unsigned long long *__restrict__ sum) {
    unsigned long long acc = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = src[i] - dst[i];
        acc += (unsigned long long)(g < 0 ? -g : g);
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(sum, acc);
}

__global__ void k_bb_relabel_keys(const unsigned long long *__restrict__ cnt, int64_t n,
                                  uint64_t *__restrict__ keys, int64_t *__restrict__ ids) {
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < n;
         x += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t c = cnt[x] < 0xffffffffull ? cnt[x] : 0xffffffffull;
        keys[x] = ((0xffffffffull - c) << 32) | (uint64_t)x;
        ids[x] = x;
    }
}

// landmark order: ascending ((2^32 - 1 - degree in G) << 32 | id) = by degree, high first,
// ties by id (round 5's host partial_sort over a copy of G's row pointers)
__global__ void k_bb_degkeys(const int64_t *__restrict__ gp, int64_t n, uint64_t *__restrict__ keys,
                             int64_t *__restrict__ ids) {
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < n;
         x += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t d = (uint64_t)(gp[x + 1] - gp[x]);
        keys[x] = ((0xffffffffull - (d < 0xffffffffull ? d : 0xffffffffull)) << 32) | (uint64_t)x;
        ids[x] = x;
    }
}

__global__ void k_bb_first_ids(const int64_t *__restrict__ ids, int K, int32_t *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < K) out[i] = (int32_t)ids[i];
}

__global__ void k_bb_perm(const int64_t *__restrict__ ids, int64_t n, int64_t *__restrict__ perm) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        perm[ids[i]] = i;
}

__global__ void k_bb_map(const int64_t *__restrict__ perm, const int64_t *__restrict__ a,
                         const int64_t *__restrict__ b, int64_t E, int64_t *__restrict__ ma,
                         int64_t *__restrict__ mb) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        ma[i] = perm[a[i]];
        mb[i] = perm[b[i]];
    }
}

// G of metric_backbone.py:70-79 as a symmetric CSR: the columns with s < d in
// the caller's ids (osrc/odst), keyed by the ids G is built in (src/dst), weight
// the minimum over duplicates.  misc[0] is used as the unique-edge counter,
// misc + 4 as the bad-input flag.
void bb_build_graph(gs_ctx *c, int64_t n, int64_t E, const int64_t *dsrc, const int64_t *ddst,
                    const int64_t *osrc, const int64_t *odst, const double *dw,
                    unsigned long long *misc, int64_t *&gp, int32_t *&gi, double *&gw, double *wmed,
                    int64_t *gnnz) {
    hipStream_t s = c->stream;
    int *bad = (int *)(misc + 4);
    uint64_t *keys = (uint64_t *)c->buf("bb_keys").ensure(8 * E);
    int64_t *idx = (int64_t *)c->buf("bb_idx").ensure(8 * E);
    k_bb_keys<<<grid_for(E, 256, 8192), 256, 0, s>>>(dsrc, ddst, osrc, odst, dw, E, n, keys, idx,
                                                     bad);
    int hbad = 0;
    GS_HIP(hipMemcpyAsync(&hbad, bad, 4, hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));
    GS_CHECK(!(hbad & 1), GS_EINVAL, "edge_index entry out of range [0, %lld)", (long long)n);
    GS_CHECK(!(hbad & 2), GS_EUNSUPPORTED,
             "edge weights must be non-negative and not NaN (Dijkstra contract)");
    sort_pairs_u64_i64(c, keys, idx, E, bits_for_bb((uint64_t)n * (uint64_t)n));
    uint64_t *ukeys = (uint64_t *)c->buf("bb_ukeys").ensure(16 * E);
    double *uw = (double *)c->buf("bb_uw").ensure(8 * E);
    k_bb_unique<<<grid_for(E, 256, 8192), 256, 0, s>>>(keys, idx, dw, E, n, misc, ukeys, uw);
    unsigned long long ucnt = 0;
    GS_HIP(hipMemcpyAsync(&ucnt, misc, 8, hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));
    int64_t cnt2 = 2 * (int64_t)ucnt;
    if (gnnz) *gnnz = cnt2;
    if (wmed) {  // median of <= 1023 evenly spaced unique-edge weights
        *wmed = 0.0;
        if (ucnt) {
            const int64_t m = ucnt < 1023 ? (int64_t)ucnt : 1023, stride = (int64_t)ucnt / m;
            std::vector<double> smp(m);
            GS_HIP(hipMemcpy2DAsync(smp.data(), 8, uw, 8 * stride, 8, m, hipMemcpyDeviceToHost, s));
            GS_HIP(hipStreamSynchronize(s));
            std::nth_element(smp.begin(), smp.begin() + m / 2, smp.end());
            *wmed = smp[m / 2];
        }
    }
    // G as symmetric CSR sorted by (row, col): unique keys -> no ties in order
    int64_t *pay = (int64_t *)c->buf("bb_pay").ensure(8 * (cnt2 + 1));
    k_bb_sym_payload<<<grid_for(cnt2 + 1, 256, 8192), 256, 0, s>>>(cnt2, pay);
    sort_pairs_u64_i64(c, ukeys, pay, cnt2, bits_for_bb((uint64_t)n * (uint64_t)n));
    gp = (int64_t *)c->buf("bb_gp").ensure(8 * (n + 1));
    gi = (int32_t *)c->buf("bb_gi").ensure(4 * (cnt2 + 1));
    gw = (double *)c->buf("bb_gw").ensure(8 * (cnt2 + 1));
    if (cnt2) k_bb_gfill<<<grid_for(cnt2, 256, 8192), 256, 0, s>>>(ukeys, pay, uw, cnt2, n, gi, gw);
    k_bb_rowptr<<<grid_for(n + 1, 256, 8192), 256, 0, s>>>(ukeys, cnt2, (uint64_t)n, n, gp);
}

void bb_relabel(gs_ctx *c, const BbKnobs &k, int64_t n, int64_t E, const double *w, int loc,
                const int64_t *&dsrc, const int64_t *&ddst) {
    hipStream_t s = c->stream;
    bool relabel = E > 0 && n > 1;
    if (k.relabel_set) relabel = relabel && k.relabel;
    // only graphs whose ids carry no locality of their own (mean |u - v| above n / 64:
    // R-MAT 0.33 n; a word chain with short chords ~2) -- relabeling a chain-ordered
    // graph by degree would scatter it (Roman-like: 2.2 -> 3.2 ms)
    if (relabel && !k.relabel_set) {
        unsigned long long *gs = (unsigned long long *)c->buf("bb_gap").ensure(8);
        GS_HIP(hipMemsetAsync(gs, 0, 8, s));
        k_bb_gap<<<grid_for(E, 256, 2048), 256, 0, s>>>(dsrc, ddst, E, gs);
        unsigned long long hg = 0;
        GS_HIP(hipMemcpyAsync(&hg, gs, 8, hipMemcpyDeviceToHost, s));
        GS_HIP(hipStreamSynchronize(s));
        relabel = (double)hg / (double)E > (double)n / 64.0;
    }
    if (!relabel) return;
    // validate before indexing the counters with the raw ids
    int *bad0 = (int *)c->buf("bb_bad0").ensure(sizeof(int));
    GS_HIP(hipMemsetAsync(bad0, 0, sizeof(int), s));
    uint64_t *k0 = (uint64_t *)c->buf("bb_keys").ensure(8 * E);
    int64_t *i0 = (int64_t *)c->buf("bb_idx").ensure(8 * E);
    k_bb_keys<<<grid_for(E, 256, 8192), 256, 0, s>>>(dsrc, ddst, dsrc, ddst, (const double *)to_device(
        c, c->buf("bb_w"), w, sizeof(double) * E, loc), E, n, k0, i0, bad0);
    int hb = 0;
    GS_HIP(hipMemcpyAsync(&hb, bad0, 4, hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));
    GS_CHECK(!(hb & 1), GS_EINVAL, "edge_index entry out of range [0, %lld)", (long long)n);
    auto *cnt = (unsigned long long *)c->buf("bb_flag").ensure(8 * (n + 1));
    GS_HIP(hipMemsetAsync(cnt, 0, 8 * (n + 1), s));
    k_bb_count<<<grid_for(E, 256, 8192), 256, 0, s>>>(dsrc, ddst, E, cnt);
    uint64_t *nk = (uint64_t *)c->buf("bb_okeys").ensure(8 * (n > E ? n : E));
    int64_t *ids = (int64_t *)c->buf("bb_order").ensure(8 * (n > E ? n : E));
    k_bb_relabel_keys<<<grid_for(n, 256, 8192), 256, 0, s>>>(cnt, n, nk, ids);
    sort_pairs_u64_i64(c, nk, ids, n, 64);
    int64_t *perm = (int64_t *)c->buf("bb_perm").ensure(8 * n);
    k_bb_perm<<<grid_for(n, 256, 8192), 256, 0, s>>>(ids, n, perm);
    int64_t *ms = (int64_t *)c->buf("bb_msrc").ensure(8 * E), *md = (int64_t *)c->buf("bb_mdst").ensure(8 * E);
    k_bb_map<<<grid_for(E, 256, 8192), 256, 0, s>>>(perm, dsrc, ddst, E, ms, md);
    GS_HIP(hipGetLastError());
    dsrc = ms;
    ddst = md;
}

// columns grouped by source row (stable: radix sort is stable)
void bb_group_columns(gs_ctx *c, BbRun &R) {
    hipStream_t s = c->stream;
    const int64_t n = R.n, E = R.E;
    uint64_t *okeys = (uint64_t *)c->buf("bb_okeys").ensure(8 * E);
    R.order = (int64_t *)c->buf("bb_order").ensure(8 * E);
    R.optr = (int64_t *)c->buf("bb_optr").ensure(8 * (n + 1));
    k_bb_srckeys<<<grid_for(E, 256, 8192), 256, 0, s>>>(R.dsrc, E, okeys, R.order);
    sort_pairs_u64_i64(c, okeys, R.order, E, bits_for_bb((uint64_t)n));
    k_bb_rowptr<<<grid_for(n + 1, 256, 8192), 256, 0, s>>>(okeys, E, 1, n, R.optr);
}

// the K highest-degree nodes of G (ties: the lower id), on the device
void bb_top_degree(gs_ctx *c, const int64_t *gp, int64_t n, int K, int32_t *out) {
    hipStream_t s = c->stream;
    uint64_t *dk = (uint64_t *)c->buf("bb_lmkeys").ensure(8 * n);
    int64_t *di = (int64_t *)c->buf("bb_lmord").ensure(8 * n);
    k_bb_degkeys<<<grid_for(n, 256, 8192), 256, 0, s>>>(gp, n, dk, di);
    sort_pairs_u64_i64(c, dk, di, n, 64);
    k_bb_first_ids<<<(unsigned)((K + 255) / 256), 256, 0, s>>>(di, K, out);
}

// every column's (row * n + col) key sorted, its column, and the position of its reverse
// key (the reverse-column decisions of the searches and the pair certificate); once per run
void bb_keys(gs_ctx *c) {
    BbRun &R = bb_run(c);
    if (R.keys_ready) return;
    hipStream_t s = c->stream;
    const int64_t E = R.E, n = R.n;
    R.skeys = (uint64_t *)c->buf("bb_skeys").ensure(8 * E);
    R.sidx = (int64_t *)c->buf("bb_sidx").ensure(8 * E);
    R.rpos = (int64_t *)c->buf("bb_rpos").ensure(8 * E);
    k_bb_pairkeys<<<grid_for(E, 256, 8192), 256, 0, s>>>(R.dsrc, R.ddst, E, n, R.skeys, R.sidx);
    sort_pairs_u64_i64(c, R.skeys, R.sidx, E, bits_for_bb((uint64_t)n * (uint64_t)n));
    k_bb_revpos<<<grid_for(E, 256, 8192), 256, 0, s>>>(R.dsrc, R.ddst, E, n, R.skeys, R.rpos);
    GS_HIP(hipGetLastError());
    R.keys_ready = true;
}

}  // namespace gs
