// gs_bb_search.hip -- the metric backbone's search stage: one source per workgroup
// (k_bb_sssp) or S together (k_bb_sssp_multi, gs_bb_multi.hpp), and the batch trace.
#include "gs_bb.hpp"
#include "gs_bb_multi.hpp"

namespace gs {

template <int NT>
__global__ void __launch_bounds__(NT) k_bb_sssp(
    const int64_t *__restrict__ gp, const int32_t *__restrict__ gi, const double *__restrict__ gw,
    int64_t n, const int64_t *__restrict__ sources, int64_t nsrc, const int64_t *__restrict__ optr,
    const int64_t *__restrict__ order, const int64_t *__restrict__ dst,
    const double *__restrict__ w, double eps, uint8_t *__restrict__ state,
    unsigned long long *__restrict__ dist_all, int32_t *__restrict__ qflag_all,
    int32_t *__restrict__ fr_all, int32_t *__restrict__ touched_all, int64_t b0, int64_t b1,
    int part, int nparts, unsigned long long *__restrict__ relax_total, uint8_t *__restrict__ why) {
    __shared__ int s_fcount, s_ncount, s_tcount;
    __shared__ double s_wmax, s_wnext;
    __shared__ unsigned long long s_relax;
    unsigned long long *dist = dist_all + (int64_t)blockIdx.x * n;
    int32_t *qflag = qflag_all + (int64_t)blockIdx.x * n;
    int32_t *fa = fr_all + (int64_t)blockIdx.x * 2 * n;
    int32_t *fb = fa + n;
    int32_t *touched = touched_all + (int64_t)blockIdx.x * n;
    if (threadIdx.x == 0) s_relax = 0;
    unsigned long long relax = 0;
    // sources [b0, b1) of the list (b1 <= nsrc), this part's every nparts-th one
    for (int64_t j = blockIdx.x;; j += gridDim.x) {
        const int64_t si = b0 + part + j * nparts;
        if (si >= b1) break;
        const int64_t u = sources[si];
        const int64_t c0 = optr[u], c1 = optr[u + 1];
        if (threadIdx.x == 0) {
            s_wmax = -1.0;
            s_fcount = 1;
            s_ncount = 0;
            s_tcount = 1;
        }
        __syncthreads();
        // largest unresolved target weight
        double lm = -1.0;
        for (int64_t j = c0 + threadIdx.x; j < c1; j += blockDim.x) {
            int64_t idx = order[j];
            if (state[idx] == 0 && w[idx] > lm) lm = w[idx];
        }
        bb_block_max(lm, &s_wmax);
        if (s_wmax < 0.0) {
            __syncthreads();
            continue;  // nothing unresolved for this source
        }
        // after each round: a target whose current (upper-bound) distance
        // already proves w > fl(d + eps) is pruned for good; the bound drops to
        // the largest weight still undecided, and the search ends when none is
        auto hook = [&]() {
            if (threadIdx.x == 0) s_wnext = -1.0;
            __syncthreads();
            double m = -1.0;
            for (int64_t j = c0 + threadIdx.x; j < c1; j += blockDim.x) {
                const int64_t idx = order[j];
                if (state[idx] != 0) continue;
                const unsigned long long db =
                    __hip_atomic_load(&dist[dst[idx]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (db != kInfBits && w[idx] > __longlong_as_double((long long)db) + eps) {
                    bb_set(state, why, idx, 2, kWhySearchPrune);
                    continue;
                }
                m = w[idx] > m ? w[idx] : m;
            }
            bb_block_max(m, &s_wnext);
            if (threadIdx.x == 0) {
                s_wmax = s_wnext;
                if (s_wnext < 0.0) s_fcount = 0;
            }
            __syncthreads();
        };
        bb_search(gp, gi, gw, (int32_t)u, s_wmax, dist, qflag, fa, fb, touched, s_fcount,
                  s_ncount, s_tcount, relax, hook);
        // classify unresolved targets
        for (int64_t j = c0 + threadIdx.x; j < c1; j += blockDim.x) {
            int64_t idx = order[j];
            if (state[idx] != 0) continue;
            int64_t v = dst[idx];
            unsigned long long db =
                __hip_atomic_load(&dist[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            double d = __longlong_as_double((long long)db);
            bool keep = (db == kInfBits) || (w[idx] <= d + eps);
            bb_set(state, why, idx, keep ? 1 : 2, keep ? kWhySearchKeep : kWhySearchPrune);
        }
        __syncthreads();
        const int tc = s_tcount;
        for (int t = threadIdx.x; t < tc; t += blockDim.x) {
            int32_t y = touched[t];
            dist[y] = kInfBits;
            qflag[y] = 0;
        }
        __syncthreads();
    }
    atomicAdd(&s_relax, relax);
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(relax_total, s_relax);
}

BbTrace bb_trace_begin(gs_ctx *c, const char *path, int64_t nrec) {
    BbTrace t{path, nullptr, nrec};
    if (path) {
        t.rec = (unsigned long long *)c->buf("bb_trace").ensure(48 * (size_t)nrec);
        GS_HIP(hipMemsetAsync(t.rec, 0, 48 * (size_t)nrec, c->stream));
    }
    return t;
}

void bb_trace_end(gs_ctx *c, const BbTrace &t, const char *prefix, int part, int nparts, int64_t b0,
                  int64_t b1, int S, int64_t grid) {
    if (!t.path) return;
    std::vector<unsigned long long> h(6 * (size_t)t.nrec);
    GS_HIP(hipMemcpyAsync(h.data(), t.rec, 48 * (size_t)t.nrec, hipMemcpyDeviceToHost, c->stream));
    GS_HIP(hipStreamSynchronize(c->stream));
    if (FILE *f = fopen(t.path, "a")) {
        fprintf(f, "{%s\"part\": %d, \"nparts\": %d, \"b0\": %lld, \"b1\": %lld, \"S\": %d, \"grid\": %lld, \"rec\": [",
                prefix, part, nparts, (long long)b0, (long long)b1, S, (long long)grid);
        for (int64_t i = 0; i < t.nrec; ++i) {
            double bm;
            memcpy(&bm, &h[6 * i + 3], 8);
            fprintf(f, "%s[%llu, %llu, %llu, %.9g, %llu, %llu]", i ? ", " : "", h[6 * i], h[6 * i + 1],
                    h[6 * i + 2], bm, h[6 * i + 4], h[6 * i + 5]);
        }
        fprintf(f, "]}\n");
        fclose(f);
    }
}

// the 12 search forms of k_bb_sssp_multi: S outside 2 / 4 / 8 takes 16, threads outside
// 512 / 1024 take 256
template <int NT, int S>
static void bb_multi_launch(const BbRun &R, unsigned grid, hipStream_t s, int64_t b0, int64_t b1, int part,
                            int nparts, unsigned long long *bnext, unsigned long long *trace) {
    k_bb_sssp_multi<NT, S><<<grid, NT, 0, s>>>(
        R.gp, R.gi, R.gw, R.n, R.sources, R.nsrc, R.optr, R.order, R.dsrc, R.ddst, R.dw, R.eps, R.state,
        R.dist, (uint32_t *)R.qflag, R.fr, R.fm, R.touched, R.farl, R.delta, R.cross, R.skeys, R.sidx,
        R.rpos, R.E, R.mrg, R.rev, b0, b1, part, nparts, bnext, R.misc + 1, trace, R.why);
}

template <int NT>
static void bb_multi_by_s(const BbRun &R, unsigned grid, hipStream_t s, int64_t b0, int64_t b1, int part,
                            int nparts, unsigned long long *bnext, unsigned long long *trace) {
    switch (R.S) {
    case 2: bb_multi_launch<NT, 2>(R, grid, s, b0, b1, part, nparts, bnext, trace); break;
    case 4: bb_multi_launch<NT, 4>(R, grid, s, b0, b1, part, nparts, bnext, trace); break;
    case 8: bb_multi_launch<NT, 8>(R, grid, s, b0, b1, part, nparts, bnext, trace); break;
    default: bb_multi_launch<NT, 16>(R, grid, s, b0, b1, part, nparts, bnext, trace); break;
    }
}

static void bb_launch_multi(const BbRun &R, unsigned grid, hipStream_t s, int64_t b0, int64_t b1, int part,
                            int nparts, unsigned long long *bnext, unsigned long long *trace) {
    switch (R.bt) {
    case 1024: bb_multi_by_s<1024>(R, grid, s, b0, b1, part, nparts, bnext, trace); break;
    case 512: bb_multi_by_s<512>(R, grid, s, b0, b1, part, nparts, bnext, trace); break;
    default: bb_multi_by_s<256>(R, grid, s, b0, b1, part, nparts, bnext, trace); break;
    }
}

// search batches [b0, b1) of the processing order, this part's every nparts-th one
void bb_search_batches(gs_ctx *c, int64_t b0, int64_t b1, int part, int nparts) {
    BbRun &R = bb_run(c);
    GS_CHECK(R.planned, GS_ESTATE, "gs_bb_plan first");
    GS_CHECK(nparts >= 1 && 0 <= part && part < nparts, GS_EINVAL, "bad part %d of %d", part, nparts);
    GS_CHECK(0 <= b0 && b0 <= b1 && b1 <= R.nbatch, GS_EINVAL, "batches [%lld, %lld) outside [0, %lld)",
             (long long)b0, (long long)b1, (long long)R.nbatch);
    GS_HIP(hipSetDevice(c->device));
    if (b1 - b0 <= part) return;  // none of this part's
    const BbKnobs knobs = bb_knobs();
    hipStream_t s = c->stream;
    const int64_t mine = (b1 - b0 - part + nparts - 1) / nparts;
    const unsigned grid = (unsigned)std::min<int64_t>(R.slabs, mine);
    hipEvent_t tp = prof_begin(c);
    if (R.S == 1) {
        auto kfn = R.bt == 1024 ? k_bb_sssp<1024> : R.bt == 512 ? k_bb_sssp<512> : k_bb_sssp<256>;
        kfn<<<grid, R.bt, 0, s>>>(R.gp, R.gi, R.gw, R.n, R.sources, R.nsrc, R.optr, R.order, R.ddst,
                                  R.dw, R.eps, R.state, R.dist, R.qflag, R.fr, R.touched, b0, b1, part,
                                  nparts, R.misc + 1, R.why);
    } else {
        unsigned long long *bnext = R.dynamic ? R.misc + 2 : nullptr;
        if (bnext) GS_HIP(hipMemsetAsync(bnext, 0, 8, s));
        // one trace line per launch (waits for the launch)
        const BbTrace tr = bb_trace_begin(c, knobs.trace, mine);
        bb_launch_multi(R, grid, s, b0, b1, part, nparts, bnext, tr.rec);
        bb_trace_end(c, tr, "", part, nparts, b0, b1, R.S, grid);
    }
    GS_HIP(hipGetLastError());
    prof_end(c, tp, "bb_search", 0.0);
}

}  // namespace gs
