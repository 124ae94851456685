// gs_backbone.hip -- metric backbone prune (compute_metric_backbone,
// metric_backbone.py:28-141) on the device.
//
// Reference: G = undirected graph of the src<dst edge_index columns with
// weight min over duplicates (:70-79); APSP by Dijkstra (:86); column
// idx=(u,v) kept iff d_G(u,v) == inf or w[idx] <= d + eps (:97-111).
// Any exact SSSP whose path sums are left-folded from the source reproduces
// Dijkstra's distances bit for bit (fl(a+w) is monotone in a, so the least
// fixpoint of d(y) = min_x fl(d(x) + w(x,y)) is unique); here:
//   1. exact 2-hop witness: prune (u,v) when some common neighbour x gives
//      w_uv > fl(fl(w_ux + w_xv) + eps)  (d <= that path, so w > fl(d+eps));
//   2. for every source row u with unresolved targets: a label-correcting
//      frontier search (one workgroup per source, distances as 64-bit
//      atomicMin on the IEEE bits -- valid for non-negative doubles) pruned
//      at the largest unresolved target weight: a target beyond it has
//      d > w and is kept whatever its exact distance.
//
// This unit: the staged host driver (begin / plan / finish; the stages between are
// the units' -- gs_bb_graph.hip, gs_bb_landmarks.hip, gs_bb_certify.hip, gs_bb_mitm.hip,
// gs_bb_search.hip), the knob reader, the search geometry, the owner of the idle search
// slabs, every C entry point, and gs_pair_distances.
#include "gs_bb.hpp"

namespace gs {

// Full searches for sampled node pairs (verify_geodesic_preservation,
// compute_geodesic_preservation): one workgroup per distinct source, then the
// exact distance of each of its targets (+inf when unreachable).
__global__ void __launch_bounds__(256) k_bb_pairs(
    const int64_t *__restrict__ gp, const int32_t *__restrict__ gi, const double *__restrict__ gw,
    int64_t n, const int64_t *__restrict__ srcs, const int64_t *__restrict__ qptr,
    const int64_t *__restrict__ qt, int64_t nsrc, double *__restrict__ out,
    unsigned long long *__restrict__ dist_all, int32_t *__restrict__ qflag_all,
    int32_t *__restrict__ fr_all, int32_t *__restrict__ touched_all) {
    __shared__ int s_fcount, s_ncount, s_tcount;
    __shared__ double s_inf;
    unsigned long long *dist = dist_all + (int64_t)blockIdx.x * n;
    int32_t *qflag = qflag_all + (int64_t)blockIdx.x * n;
    int32_t *fa = fr_all + (int64_t)blockIdx.x * 2 * n;
    int32_t *fb = fa + n;
    int32_t *touched = touched_all + (int64_t)blockIdx.x * n;
    unsigned long long relax = 0;
    for (int64_t si = blockIdx.x; si < nsrc; si += gridDim.x) {
        if (threadIdx.x == 0) {
            s_fcount = 1;
            s_ncount = 0;
            s_tcount = 1;
            s_inf = __builtin_inf();
        }
        __syncthreads();
        bb_search(gp, gi, gw, (int32_t)srcs[si], s_inf, dist, qflag, fa, fb, touched, s_fcount,
                  s_ncount, s_tcount, relax, [&] { __syncthreads(); });
        for (int64_t q = qptr[si] + threadIdx.x; q < qptr[si + 1]; q += blockDim.x)
            out[q] = __longlong_as_double((long long)dist[qt[q]]);
        __syncthreads();
        const int tc = s_tcount;
        for (int t = threadIdx.x; t < tc; t += blockDim.x) {
            const int32_t y = touched[t];
            dist[y] = kInfBits;
            qflag[y] = 0;
        }
        __syncthreads();
    }
}

__global__ void k_bb_count0(const uint8_t *__restrict__ state, int64_t E,
                            unsigned long long *__restrict__ cnt) {
    unsigned long long c = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x)
        c += state[i] == 0;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(cnt, c);
}

__global__ void k_bb_fill_u64(unsigned long long *p, int64_t n, unsigned long long v) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        p[i] = v;
}

// sources: rows with an unresolved target (other parts' columns are marked 3)
// flag[u] = 1 for every row with an open column (flag zeroed before); one thread per
// column (a thread per row walked a hub's 10^4-10^5 columns alone: 3.3 ms on RMAT-18)
__global__ void k_bb_need(const int64_t *__restrict__ src, const uint8_t *__restrict__ state,
                          int64_t E, int64_t *__restrict__ flag) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x)
        if (state[i] == 0) flag[src[i]] = 1;
}

__global__ void k_bb_compact(const int64_t *__restrict__ flag, const int64_t *__restrict__ pos,
                             int64_t n, int64_t *__restrict__ sources) {
    for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < n;
         u += (int64_t)gridDim.x * blockDim.x)
        if (flag[u]) sources[pos[u]] = u;
}

// keep bytes of this part's columns (bb_col_part), 0 elsewhere
__global__ void k_bb_keep(const uint8_t *__restrict__ state, const int64_t *__restrict__ src,
                          const int64_t *__restrict__ dst, int64_t E, int part, int nparts,
                          uint8_t *__restrict__ keep) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x)
        keep[i] = state[i] == 1 && bb_col_part(src[i], dst[i], nparts) == part;
}

__global__ void k_bb_why_hist(const uint8_t *__restrict__ why, int64_t E,
                              unsigned long long *__restrict__ cnt) {
    __shared__ unsigned int h[kWhyClasses];
    for (int k = threadIdx.x; k < kWhyClasses; k += blockDim.x) h[k] = 0;
    __syncthreads();
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t k = why[i];
        atomicAdd(&h[k < kWhyClasses ? k : 0], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kWhyClasses; k += blockDim.x)
        if (h[k]) atomicAdd(&cnt[k], (unsigned long long)h[k]);
}

// ---------------------------------------------------------------------------
// Host side, in stages (the prune over N ranks).  One call of
// gs_metric_backbone runs them back to back; the multi-rank form
// (gsparse.distributed.sharded_backbone) runs them on every rank with one exchange
// between stages:
//   begin     relabel, G, columns by row, this rank's landmark searches (l = part mod N)
//             -> exchange D (min) and the completeness flags (max)
//   certify   2-hop witness + degree-1 / landmark certificates of this rank's column
//             range -> exchange the column states (max: 0 open < 1 keep < 2 prune; two
//             ranks that decide a column decide it the same way, every rule is exact)
//   plan      the sources with open columns (the same list on every rank)
//   search    batches [b0, b1) of the ascending-count order, this rank's every N-th
//             -> exchange the states; the next range starts from every rank's decisions
//             (the short searches' reverse-column decisions close most hub columns
//             before the hubs search)
//   finish    keep bytes of every column
// The legacy one-exchange form (gs_metric_backbone_part: pairs max(u, v) % N, keep
// bytes summed) runs the same stages with the pair flags.

// The one reader of the environment (gs_bb.hpp).
BbKnobs bb_knobs() {
    BbKnobs k;
    if (const char *e = getenv("GSPARSE_BB_RELABEL")) {
        k.relabel_set = true;
        k.relabel = atoi(e) != 0;
    }
    if (const char *e = getenv("GSPARSE_BB_LANDMARKS")) k.landmarks = atoi(e) < 0 ? 0 : atoi(e);
    if (const char *e = getenv("GSPARSE_BB_LMCOOP")) k.lmcoop = atoi(e) != 0;
    if (const char *e = getenv("GSPARSE_BB_LMW")) {
        k.lmw_set = true;
        k.lmw = atoi(e);
    }
    if (const char *e = getenv("GSPARSE_BB_LOCALLB")) k.locallb = atoi(e) != 0;
    if (const char *e = getenv("GSPARSE_BB_MITM")) k.mitm = atoi(e) != 0;
    if (const char *e = getenv("GSPARSE_BB_MITM_SLABS")) k.mitm_slabs = atoi(e) > 0 ? atoi(e) : 0;
    if (const char *e = getenv("GSPARSE_BB_MITM_LM")) k.mitm_lm = atoi(e) != 0;
    if (const char *e = getenv("GSPARSE_BB_SLABS")) k.slabs = atoi(e) > 0 ? atoi(e) : 0;
    if (const char *e = getenv("GSPARSE_BB_MULTI")) {
        const int v = atoi(e);
        k.multi = v >= 16 ? 16 : v >= 8 ? 8 : v >= 4 ? 4 : v >= 2 ? 2 : 1;
    }
    if (const char *e = getenv("GSPARSE_BB_THREADS")) k.threads = atoi(e) == 1024 ? 1024 : atoi(e) == 512 ? 512 : 256;
    k.refill = getenv("GSPARSE_BB_REFILL") != nullptr;
    if (const char *e = getenv("GSPARSE_BB_CROSS")) k.cross = atoi(e) != 0;
    if (const char *e = getenv("GSPARSE_BB_ORDER")) k.order_rev = strcmp(e, "desc") != 0;
    if (const char *e = getenv("GSPARSE_BB_DYNAMIC")) k.dynamic = atoi(e) != 0;
    if (const char *e = getenv("GSPARSE_BB_NEARFAR")) k.nearfar = atof(e);
    k.trace = getenv("GSPARSE_BB_TRACE");
    k.debug = getenv("GSPARSE_BB_DEBUG") != nullptr;
    return k;
}

BbGeometry bb_geometry(int64_t n, int64_t nsrc, int nranks, int lpart, const BbKnobs &k) {
    BbGeometry g;
    // landmarks: 48 on large graphs, 16 on small ones (GSPARSE_BB_LANDMARKS = K, 0 = off)
    int K = n > 65536 ? 48 : 16;
    if (k.landmarks >= 0) K = k.landmarks;
    if (K > n) K = (int)n;
    g.K = K;
    // large graphs: their searches spread over the GPU (GSPARSE_BB_LMCOOP=0: one
    // workgroup per landmark)
    g.lm_coop = n > 65536 && n < ((int64_t)1 << 31) && k.lmcoop;
    g.lm_mine = (K - lpart + nranks - 1) / nranks;  // landmarks l = lpart (mod nranks)
    if (g.lm_mine > 0) {
        // workgroups per landmark: about two 512-thread workgroups per CU in all
        int W = (512 + g.lm_mine - 1) / g.lm_mine;
        if (k.lmw_set) W = k.lmw;
        g.lm_W = std::max(1, std::min(W, 256));
    }
    // large graphs (big search balls): 512 workgroups of 512 threads, two per CU
    // (RMAT-18 with the final search: 650 vs 692 ms for 256 x 1,024; round 1's
    // plain search preferred 256 x 1,024); small ones (many short searches):
    // 1,024 workgroups of 256 (Roman: 2.2 vs 3.0 ms)
    const bool big = n > 65536;
    // a rank of 8 or more (staged form) has few batches per workgroup and waits on
    // single searches: 2 sources per workgroup of 1,024 threads, 256 workgroups
    // (RMAT-18 at N = 8: 120.5 ms per rank vs 131.5 ms with 8 sources x 512
    // threads; at N = 4 the latter wins, 188.8 vs 204.9 ms; tools/bb_stage_probe.py,
    // profiles/r05t_*)
    const bool wide = big && nranks >= 8;
    int64_t maxslabs = big ? (wide ? 256 : 512) : 1024;
    if (k.slabs > 0) maxslabs = k.slabs;
    // sources searched together per workgroup (k_bb_sssp_multi), 1 = alone: on
    // large graphs 16 on one GPU (RMAT-18 with the local-bound certificates: 455.9
    // vs 475.8 ms with 8, which keep the near-far order), 8 per rank of 2 to 7 (N = 4:
    // 188.8 ms; 16: 219.7); alone on small ones (Roman: 2.30 ms vs 2.45 ms with 8)
    int S = big ? (wide ? 2 : nranks == 1 ? 16 : 8) : 1;
    if (k.multi) S = k.multi;
    g.S = S;
    g.nbatch = (nsrc + S - 1) / S;
    int64_t slabs = g.nbatch < maxslabs ? g.nbatch : maxslabs;
    // keep the working set of all slabs under ~48 GB (of 288)
    const double per = S == 1 ? 24.0 : 8.0 * S + 28.0;
    int64_t cap = (int64_t)(48e9 / (per * (double)(n ? n : 1)));
    if (cap < 1) cap = 1;
    if (slabs > cap) slabs = cap;
    g.slabs = slabs;
    g.threads = big ? (wide ? 1024 : 512) : 256;
    if (k.threads) g.threads = k.threads;
    return g;
}

void bb_fill_u64(gs_ctx *c, unsigned long long *p, int64_t n, unsigned long long v) {
    k_bb_fill_u64<<<grid_for(n, 256, 65536), 256, 0, c->stream>>>(p, n, v);
}

BbSlabs bb_slabs(gs_ctx *c, int width, int64_t slabs, int64_t n, bool multi, bool fill_all) {
    BbRun &R = bb_run(c);
    hipStream_t s = c->stream;
    const size_t dbytes = 8 * (size_t)width * slabs * n, qbytes = 4 * (size_t)slabs * n;
    DevBuf &bd = c->buf("bb_dist"), &bq = c->buf("bb_qflag");
    // a buffer that has to grow is a new allocation (DevBuf::ensure frees first):
    // nothing of it is known idle, wherever it lands
    if (dbytes > bd.bytes) R.dist_clean = 0;
    if (qbytes > bq.bytes) R.q_clean = 0;
    BbSlabs sl{};
    sl.dist = (unsigned long long *)bd.ensure(dbytes);
    sl.qflag = (int32_t *)bq.ensure(qbytes);
    sl.fr = (int32_t *)c->buf("bb_fr").ensure(8 * (size_t)slabs * n);
    sl.touched = (int32_t *)c->buf("bb_touched").ensure(4 * (size_t)slabs * n);
    if (multi) {
        sl.fm = (uint32_t *)c->buf("bb_fmask").ensure(4 * (size_t)slabs * n);
        sl.farl = (int32_t *)c->buf("bb_far").ensure(8 * (size_t)slabs * n);
    }
    // (RMAT-18, 16 sources x 512 slabs: 17 GB, 3.2 ms per prune when filled each time)
    const size_t d0 = fill_all ? 0 : std::min(R.dist_clean, dbytes);
    if (d0 < dbytes) bb_fill_u64(c, sl.dist + d0 / 8, (int64_t)((dbytes - d0) / 8), kInfBits);
    R.dist_clean = std::max(R.dist_clean, dbytes);
    const size_t q0 = fill_all ? 0 : std::min(R.q_clean, qbytes);
    if (q0 < qbytes) GS_HIP(hipMemsetAsync((char *)sl.qflag + q0, 0, qbytes - q0, s));
    R.q_clean = std::max(R.q_clean, qbytes);
    return sl;
}

static void bb_begin(gs_ctx *c, int64_t n, int64_t E, const int64_t *src, const int64_t *dst,
                     const double *w, int64_t nw, int loc, double eps, int lpart, int lparts,
                     int pair_part, int pair_nparts) {
    GS_CHECK(c, GS_EINVAL, "null context");
    // the reference indexes edge_weights[idx] for every column (metric_backbone.py:73-74)
    GS_CHECK(nw >= E, GS_EINDEX, "index %lld is out of bounds for axis 0 with size %lld",
             (long long)nw, (long long)nw);
    GS_CHECK(E == 0 || (src && dst && w), GS_EINVAL, "null column/weight array");
    GS_CHECK(lparts >= 1 && 0 <= lpart && lpart < lparts, GS_EINVAL, "bad part %d of %d", lpart, lparts);
    GS_CHECK(pair_nparts >= 1 && 0 <= pair_part && pair_part < pair_nparts, GS_EINVAL,
             "bad part %d of %d", pair_part, pair_nparts);
    GS_CHECK(n >= 0 && E >= 0, GS_EINVAL, "negative n/E");
    GS_CHECK(n < (int64_t(1) << 31), GS_EUNSUPPORTED, "n >= 2^31");
    GS_HIP(hipSetDevice(c->device));
    const BbKnobs knobs = bb_knobs();
    BbRun &R = bb_run(c);
    R.begun = R.certified = R.planned = false;
    R.keys_ready = false;
    R.n = n;
    R.E = E;
    R.eps = eps;
    R.mrg = std::max(1e-8, 8.0 * (double)n * 0x1p-53);
    R.pair_part = pair_part;
    R.pair_nparts = pair_nparts;
    R.nranks = lparts;
    R.lpart = lpart;
    R.K = 0;
    R.nsrc = R.nbatch = 0;
    hipStream_t s = c->stream;
    // own buffers (the scorer scratch slots stay untouched)
    const int64_t *dsrc = (const int64_t *)to_device(c, c->buf("bb_src"), src, sizeof(int64_t) * E, loc);
    const int64_t *ddst = (const int64_t *)to_device(c, c->buf("bb_dst"), dst, sizeof(int64_t) * E, loc);
    R.osrc = dsrc;  // the caller's ids
    R.odst = ddst;
    bb_relabel(c, knobs, n, E, w, loc, dsrc, ddst);
    R.dsrc = dsrc;
    R.ddst = ddst;
    R.dw = (const double *)to_device(c, c->buf("bb_w"), w, sizeof(double) * E, loc);
    R.misc = (unsigned long long *)c->buf("bb_misc").ensure(64);
    GS_HIP(hipMemsetAsync(R.misc, 0, 64, s));
    R.state = (uint8_t *)c->buf("bb_state").ensure(E ? E : 1);
    if (E) GS_HIP(hipMemsetAsync(R.state, 0, E, s));
    R.why = nullptr;
    R.why_E = 0;
    if (R.why_on) {
        R.why = (uint8_t *)c->buf("bb_why").ensure(E ? E : 1);
        if (E) GS_HIP(hipMemsetAsync(R.why, 0, E, s));
        R.why_E = E;
    }
    R.tall = prof_begin(c);
    if (E > 0) {
        hipEvent_t t0 = prof_begin(c);  // ended as "bb_build" below (no leak at E = 0)
        int64_t gnnz = 0;
        bb_build_graph(c, n, E, R.dsrc, R.ddst, R.osrc, R.odst, R.dw, R.misc, R.gp, R.gi, R.gw, &R.wmed, &gnnz);
        bb_group_columns(c, R);
        prof_end(c, t0, "bb_build", 0.0);
        hipEvent_t tp = prof_begin(c);
        bb_landmarks(c, R, bb_geometry(n, 0, lparts, lpart, knobs), lpart, lparts, gnnz, knobs.debug);
        prof_end(c, tp, "bb_landmarks", 0.0);
    }
    R.begun = true;
}

// the sources with open columns, in node order (the same list on every rank), and the
// search geometry
static void bb_plan(gs_ctx *c) {
    BbRun &R = bb_run(c);
    GS_CHECK(R.certified, GS_ESTATE, "gs_bb_certify first");
    GS_HIP(hipSetDevice(c->device));
    const BbKnobs knobs = bb_knobs();
    hipStream_t s = c->stream;
    const int64_t n = R.n, E = R.E;
    R.nsrc = R.nbatch = 0;
    hipEvent_t tp = prof_begin(c);
    if (E > 0) {
        int64_t *flag = (int64_t *)c->buf("bb_flag").ensure(8 * (n + 1));
        int64_t *pos = (int64_t *)c->buf("bb_pos").ensure(8 * (n + 1));
        hipEvent_t tq = prof_begin(c);
        GS_HIP(hipMemsetAsync(flag, 0, 8 * (n + 1), s));
        k_bb_need<<<grid_for(E, 256, 8192), 256, 0, s>>>(R.dsrc, R.state, E, flag);
        exclusive_scan_i64(c, flag, pos, n);
        int64_t lastp = 0, lastf = 0;
        if (n) {
            GS_HIP(hipMemcpyAsync(&lastp, pos + n - 1, 8, hipMemcpyDeviceToHost, s));
            GS_HIP(hipMemcpyAsync(&lastf, flag + n - 1, 8, hipMemcpyDeviceToHost, s));
        }
        GS_HIP(hipStreamSynchronize(s));
        prof_end(c, tq, "bb_plan_need", 0.0);
        R.nsrc = lastp + lastf;
        if (knobs.debug) {
            GS_HIP(hipMemsetAsync(R.misc + 3, 0, 8, s));
            k_bb_count0<<<grid_for(E, 256, 4096), 256, 0, s>>>(R.state, E, R.misc + 3);
            unsigned long long open = 0;
            GS_HIP(hipMemcpyAsync(&open, R.misc + 3, 8, hipMemcpyDeviceToHost, s));
            GS_HIP(hipStreamSynchronize(s));
            fprintf(stderr, "[backbone] open before searches=%llu sources=%lld\n", open,
                    (long long)R.nsrc);
        }
        if (R.nsrc > 0) {
            R.sources = (int64_t *)c->buf("bb_sources").ensure(8 * R.nsrc);
            k_bb_compact<<<grid_for(n, 256, 8192), 256, 0, s>>>(flag, pos, n, R.sources);
            const BbGeometry g = bb_geometry(n, R.nsrc, R.nranks, R.lpart, knobs);
            const int S = R.S = g.S;
            R.nbatch = g.nbatch;
            R.slabs = g.slabs;
            R.bt = g.threads;
            hipEvent_t tf = prof_begin(c);
            const BbSlabs sl = bb_slabs(c, S, g.slabs, n, S > 1, knobs.refill);
            R.dist = sl.dist;
            R.qflag = sl.qflag;
            R.fr = sl.fr;
            R.touched = sl.touched;
            prof_end(c, tf, "bb_plan_fill", 0.0);
            if (S > 1) {
                R.fm = sl.fm;
                R.farl = sl.farl;
                // reverse-column decisions after every search (GSPARSE_BB_CROSS=0: off)
                R.cross = knobs.cross;
                hipEvent_t tc = prof_begin(c);
                if (R.cross) bb_keys(c);
                prof_end(c, tc, "bb_plan_cross", 0.0);
                // sources by ascending column count (the batches from the last): the
                // short searches first, so their reverse-column decisions close most of
                // the hubs' targets before the hubs search (RMAT-18 1.63 -> 0.83 s;
                // GSPARSE_BB_ORDER=desc: hubs first)
                R.rev = knobs.order_rev;
                // batches from a global counter (misc + 2); GSPARSE_BB_DYNAMIC=0: static striding
                R.dynamic = knobs.dynamic;
                // near-far step: twice the median edge weight (GSPARSE_BB_NEARFAR = the
                // factor, 0 = plain frontier order; RMAT-18: 1 / 2 / 4 -> 687 / 692 / 700 ms
                // at 256 x 1,024 threads, 0 -> 723 ms)
                R.delta = knobs.nearfar > 0.0 && R.wmed > 0.0 ? knobs.nearfar * R.wmed : 0.0;
            }
            GS_HIP(hipGetLastError());
        }
    }
    prof_end(c, tp, "bb_plan", 0.0);
    R.planned = true;
}

static void bb_finish(gs_ctx *c, uint8_t *keep, int keep_loc, int64_t *n_relax) {
    BbRun &R = bb_run(c);
    GS_CHECK(R.certified, GS_ESTATE, "gs_bb_certify first");
    GS_CHECK(R.E == 0 || keep, GS_EINVAL, "null keep array");
    GS_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t E = R.E;
    uint8_t *dkeep = (uint8_t *)out_device(c, c->buf("bb_keep"), keep, E ? E : 1, keep_loc);
    int64_t relax = 0;
    if (E > 0) {
        k_bb_keep<<<grid_for(E, 256, 8192), 256, 0, s>>>(R.state, R.dsrc, R.ddst, E, R.pair_part,
                                                       R.pair_nparts, dkeep);
        GS_HIP(hipGetLastError());
        unsigned long long hr = 0;
        GS_HIP(hipMemcpyAsync(&hr, R.misc + 1, 8, hipMemcpyDeviceToHost, s));
        GS_HIP(hipStreamSynchronize(s));
        relax = (int64_t)hr;
    }
    prof_end(c, R.tall, "metric_backbone", 12.0 * (double)relax + 9.0 * (double)E);
    R.tall = nullptr;
    finish_out(c, keep, dkeep, E, keep_loc);
    if (n_relax) *n_relax = relax;
    R.begun = R.certified = R.planned = false;
}

extern "C" int gs_metric_backbone_part(gs_ctx *c, int64_t n, int64_t E, const int64_t *src,
                                       const int64_t *dst, const double *w, int64_t nw, int loc,
                                       double eps, int part, int nparts, uint8_t *keep,
                                       int keep_loc, int64_t *n_relax) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        GS_CHECK(E == 0 || keep, GS_EINVAL, "null column/weight/keep array");
        bb_begin(c, n, E, src, dst, w, nw, loc, eps, 0, 1, part, nparts);
        bb_certify(c, 0, 1);
        bb_plan(c);
        bb_search_batches(c, 0, bb_run(c).nbatch, 0, 1);
        bb_finish(c, keep, keep_loc, n_relax);
    });
}

extern "C" int gs_metric_backbone(gs_ctx *c, int64_t n, int64_t E, const int64_t *src,
                                  const int64_t *dst, const double *w, int64_t nw, int loc,
                                  double eps, uint8_t *keep, int keep_loc, int64_t *n_relax) {
    return gs_metric_backbone_part(c, n, E, src, dst, w, nw, loc, eps, 0, 1, keep, keep_loc,
                                   n_relax);
}

extern "C" int gs_bb_begin(gs_ctx *c, int64_t n, int64_t E, const int64_t *src, const int64_t *dst,
                           const double *w, int64_t nw, int loc, double eps, int part, int nparts,
                           int32_t *n_landmarks) {
    return guard([&] {
        bb_begin(c, n, E, src, dst, w, nw, loc, eps, part, nparts, 0, 1);
        if (n_landmarks) *n_landmarks = bb_run(c).K;
    });
}

extern "C" int gs_bb_geometry(int64_t n, int64_t nsrc, int32_t nranks, int32_t lpart, int64_t out[7]) {
    return guard([&] {
        GS_CHECK(n >= 0 && nsrc >= 0, GS_EINVAL, "negative n/nsrc");
        GS_CHECK(nranks >= 1 && 0 <= lpart && lpart < nranks, GS_EINVAL, "bad part %d of %d", lpart, nranks);
        GS_CHECK(out, GS_EINVAL, "null output");
        const BbGeometry g = bb_geometry(n, nsrc, nranks, lpart, bb_knobs());
        const int64_t o[7] = {g.K, g.lm_coop, g.lm_W, g.S, g.threads, g.nbatch, g.slabs};
        std::copy(o, o + 7, out);
    });
}

extern "C" int gs_bb_landmarks_io(gs_ctx *c, double *D, int32_t *complete, int loc, int dir) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        BbRun &R = bb_run(c);
        GS_CHECK(R.begun, GS_ESTATE, "gs_bb_begin first");
        GS_CHECK(dir == 0 || dir == 1, GS_EINVAL, "dir must be 0 (out) or 1 (in)");
        if (R.K == 0 || R.E == 0) return;
        GS_CHECK(D && complete, GS_EINVAL, "null landmark buffers");
        GS_HIP(hipSetDevice(c->device));
        const size_t nd = 8 * (size_t)R.K * R.n, nc = 4 * (size_t)R.K;
        const hipMemcpyKind k = loc == GS_DEVICE ? hipMemcpyDeviceToDevice
                                : dir == 0 ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
        if (dir == 0) {
            GS_HIP(hipMemcpyAsync(D, R.D, nd, k, c->stream));
            GS_HIP(hipMemcpyAsync(complete, R.lcomp, nc, k, c->stream));
        } else {
            GS_HIP(hipMemcpyAsync(R.D, D, nd, k, c->stream));
            GS_HIP(hipMemcpyAsync(R.lcomp, complete, nc, k, c->stream));
        }
        GS_HIP(hipStreamSynchronize(c->stream));
    });
}

extern "C" int gs_bb_certify(gs_ctx *c, int part, int nparts) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        bb_certify(c, part, nparts);
    });
}

extern "C" int gs_bb_state_io(gs_ctx *c, uint8_t *state, int loc, int dir) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        BbRun &R = bb_run(c);
        GS_CHECK(R.begun, GS_ESTATE, "gs_bb_begin first");
        GS_CHECK(dir == 0 || dir == 1, GS_EINVAL, "dir must be 0 (out) or 1 (in)");
        if (R.E == 0) return;
        GS_CHECK(state, GS_EINVAL, "null state buffer");
        GS_HIP(hipSetDevice(c->device));
        const hipMemcpyKind k = loc == GS_DEVICE ? hipMemcpyDeviceToDevice
                                : dir == 0 ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
        if (dir == 0) GS_HIP(hipMemcpyAsync(state, R.state, R.E, k, c->stream));
        else GS_HIP(hipMemcpyAsync(R.state, state, R.E, k, c->stream));
        GS_HIP(hipStreamSynchronize(c->stream));
    });
}

extern "C" int gs_bb_plan(gs_ctx *c, int64_t *nbatch) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        bb_plan(c);
        if (nbatch) *nbatch = bb_run(c).nbatch;
    });
}

extern "C" int gs_bb_search(gs_ctx *c, int64_t b0, int64_t b1, int part, int nparts) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        bb_search_batches(c, b0, b1, part, nparts);
    });
}

extern "C" int gs_bb_finish(gs_ctx *c, uint8_t *keep, int keep_loc, int64_t *n_relax) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        bb_finish(c, keep, keep_loc, n_relax);
    });
}

extern "C" int gs_bb_classes(gs_ctx *c, int on) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        bb_run(c).why_on = on != 0;
    });
}

extern "C" int gs_bb_class_counts(gs_ctx *c, int64_t *counts, int ncounts, uint8_t *why, int64_t nwhy,
                                  int why_loc, int64_t *n_columns) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        GS_CHECK(counts && ncounts >= (int)kWhyClasses, GS_EINVAL, "counts needs %d entries", (int)kWhyClasses);
        BbRun &R = bb_run(c);
        GS_CHECK(R.why_on && R.why, GS_ESTATE, "gs_bb_classes(ctx, 1) before the backbone run");
        GS_CHECK(!why || nwhy >= R.why_E, GS_EINDEX, "why holds %lld bytes, the run has %lld columns",
                 (long long)nwhy, (long long)R.why_E);
        if (n_columns) *n_columns = R.why_E;
        GS_HIP(hipSetDevice(c->device));
        hipStream_t s = c->stream;
        auto *d = (unsigned long long *)c->buf("bb_whycnt").ensure(8 * kWhyClasses);
        GS_HIP(hipMemsetAsync(d, 0, 8 * kWhyClasses, s));
        if (R.why_E > 0) k_bb_why_hist<<<grid_for(R.why_E, 256, 2048), 256, 0, s>>>(R.why, R.why_E, d);
        GS_HIP(hipGetLastError());
        unsigned long long h[kWhyClasses];
        GS_HIP(hipMemcpyAsync(h, d, 8 * kWhyClasses, hipMemcpyDeviceToHost, s));
        if (why && R.why_E > 0)
            GS_HIP(hipMemcpyAsync(why, R.why, R.why_E,
                                  why_loc == GS_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        GS_HIP(hipStreamSynchronize(s));
        for (int k = 0; k < ncounts; ++k) counts[k] = k < (int)kWhyClasses ? (int64_t)h[k] : 0;
    });
}

extern "C" int gs_pair_distances(gs_ctx *c, int64_t n, int64_t E, const int64_t *src,
                                 const int64_t *dst, const double *w, int64_t nw, int loc,
                                 int64_t nq, const int64_t *qs, const int64_t *qt, double *out) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        GS_CHECK(!w || nw >= E, GS_EINDEX, "index %lld is out of bounds for axis 0 with size %lld",
                 (long long)nw, (long long)nw);
        GS_CHECK(n >= 0 && E >= 0 && nq >= 0, GS_EINVAL, "negative n/E/nq");
        GS_CHECK(n < (int64_t(1) << 31), GS_EUNSUPPORTED, "n >= 2^31");
        GS_CHECK(nq == 0 || (qs && qt && out), GS_EINVAL, "null query arrays");
        GS_HIP(hipSetDevice(c->device));
        hipStream_t s = c->stream;
        if (nq == 0) return;
        // queries (host) grouped by source, in a stable order
        std::vector<int64_t> ord((size_t)nq);
        for (int64_t q = 0; q < nq; ++q) {
            GS_CHECK(qs[q] >= 0 && qs[q] < n && qt[q] >= 0 && qt[q] < n, GS_EINVAL,
                     "query %lld out of range [0, %lld)", (long long)q, (long long)n);
            ord[(size_t)q] = q;
        }
        std::stable_sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return qs[a] < qs[b]; });
        std::vector<int64_t> srcs, qptr, tq((size_t)nq);
        for (int64_t i = 0; i < nq; ++i) {
            const int64_t q = ord[(size_t)i];
            if (srcs.empty() || srcs.back() != qs[q]) {
                srcs.push_back(qs[q]);
                qptr.push_back(i);
            }
            tq[(size_t)i] = qt[q];
        }
        qptr.push_back(nq);
        const int64_t nsrc = (int64_t)srcs.size();
        std::vector<double> res((size_t)nq, __builtin_inf());
        if (E > 0) {
            const int64_t *dsrc = (const int64_t *)to_device(c, c->buf("bp_src"), src, 8 * E, loc);
            const int64_t *ddst = (const int64_t *)to_device(c, c->buf("bp_dst"), dst, 8 * E, loc);
            const double *dw;
            if (w) {
                dw = (const double *)to_device(c, c->buf("bp_w"), w, 8 * E, loc);
            } else {  // unweighted: hop counts (sums of 1.0 are exact)
                double *d1 = (double *)c->buf("bp_w").ensure(8 * E);
                k_bb_fill_u64<<<grid_for(E, 256, 8192), 256, 0, s>>>(
                    (unsigned long long *)d1, E, 0x3ff0000000000000ull);  // 1.0
                dw = d1;
            }
            auto *misc = (unsigned long long *)c->buf("bp_misc").ensure(64);
            GS_HIP(hipMemsetAsync(misc, 0, 64, s));
            int64_t *gp;
            int32_t *gi;
            double *gw;
            bb_build_graph(c, n, E, dsrc, ddst, dsrc, ddst, dw, misc, gp, gi, gw);
            int64_t *d_src = (int64_t *)c->buf("bp_srcs").ensure(8 * nsrc);
            int64_t *d_ptr = (int64_t *)c->buf("bp_qptr").ensure(8 * (nsrc + 1));
            int64_t *d_tq = (int64_t *)c->buf("bp_tq").ensure(8 * nq);
            double *d_out = (double *)c->buf("bp_out").ensure(8 * nq);
            GS_HIP(hipMemcpyAsync(d_src, srcs.data(), 8 * nsrc, hipMemcpyHostToDevice, s));
            GS_HIP(hipMemcpyAsync(d_ptr, qptr.data(), 8 * (nsrc + 1), hipMemcpyHostToDevice, s));
            GS_HIP(hipMemcpyAsync(d_tq, tq.data(), 8 * nq, hipMemcpyHostToDevice, s));
            const int64_t slabs = nsrc < 256 ? nsrc : 256;
            // the backbone's slabs, filled on every call (the record is kept right all the same)
            const BbSlabs sl = bb_slabs(c, 1, slabs, n, false, true);
            k_bb_pairs<<<(unsigned)slabs, 256, 0, s>>>(gp, gi, gw, n, d_src, d_ptr, d_tq, nsrc, d_out,
                                                       sl.dist, sl.qflag, sl.fr, sl.touched);
            GS_HIP(hipGetLastError());
            std::vector<double> hout((size_t)nq);
            GS_HIP(hipMemcpyAsync(hout.data(), d_out, 8 * nq, hipMemcpyDeviceToHost, s));
            GS_HIP(hipStreamSynchronize(s));
            for (int64_t i = 0; i < nq; ++i) res[(size_t)ord[(size_t)i]] = hout[(size_t)i];
        }
        for (int64_t q = 0; q < nq; ++q) out[q] = qs[q] == qt[q] ? 0.0 : res[(size_t)q];
    });
}

}  // namespace gs
