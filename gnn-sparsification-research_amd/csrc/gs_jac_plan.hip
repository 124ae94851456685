// gs_jac_plan.hip -- the symmetric Jaccard's plan (gs_jac.hpp JacPlan): the class and
// task count of every row of a range, the per-class task lists in row order, and the
// bitmap rows cut into batches.  jac_plan() returns the kept plan when the graph and the
// rows are the ones it was built for.
#include "gs_jac.hpp"
#include "gs_wave.hpp"

namespace gs {

// per row of [r0, r1) (one wave each): class, task count (work = sum of d_v over
// owned entries); tot[0..4] = per-class task totals of the range, tot[5] = its rows
// with bitmap tasks.  A part of the sharded form plans only its own rows.
__global__ void __launch_bounds__(256) k_jac_plan(const int64_t *__restrict__ ip,
                                                  const int32_t *__restrict__ ix, int64_t r0,
                                                  int64_t r1, int8_t *__restrict__ cls,
                                                  int32_t *__restrict__ ntask,
                                                  unsigned long long *__restrict__ tot) {
    const int lane = threadIdx.x & 63;
    const int64_t w0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    unsigned long long mine[kJacClasses + 1] = {};  // lane 0: this wave's task totals
    for (int64_t u = r0 + w0; u < r1; u += nw) {
        const int64_t a = ip[u], du = ip[u + 1] - a;
        const int k = jac_class(du);
        int64_t w = 0;
        if (k >= 0) {
            for (int64_t e = a + lane; e < a + du; e += 64) {
                const int32_t v = ix[e];
                const int64_t dv = ip[v + 1] - ip[v];
                if (jac_owns(du, dv, (int32_t)u, v)) w += dv;
            }
            w = wave_sum(w);
        }
        if (lane == 0) {
            const int64_t nt = jac_row_tasks(k, du, w);
            cls[u] = (int8_t)k;
            ntask[u] = (int32_t)nt;
            if (nt) {
#pragma unroll
                for (int q = 0; q < kJacClasses; ++q) mine[q] += q == k ? (unsigned long long)nt : 0ull;
                mine[kJacClasses] += k == kJacBitmap ? 1ull : 0ull;
            }
        }
    }
    __shared__ unsigned long long red[kJacClasses + 1];
    if (threadIdx.x < kJacClasses + 1) red[threadIdx.x] = 0;
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int q = 0; q <= kJacClasses; ++q)
            if (mine[q]) atomicAdd(&red[q], mine[q]);
    __syncthreads();
    if (threadIdx.x < kJacClasses + 1 && red[threadIdx.x]) atomicAdd(&tot[threadIdx.x], red[threadIdx.x]);
}

// rows [r0, r1): cnt / gflag indexed u - r0
__global__ void k_jac_mask(const int8_t *__restrict__ cls, const int32_t *__restrict__ ntask,
                           int64_t r0, int64_t r1, int k, int64_t *__restrict__ cnt,
                           int64_t *__restrict__ gflag) {
    for (int64_t u = r0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < r1;
         u += (int64_t)gridDim.x * blockDim.x) {
        const bool in = cls[u] == k;
        cnt[u - r0] = in ? ntask[u] : 0;
        if (gflag) gflag[u - r0] = (in && ntask[u] > 0) ? 1 : 0;
    }
}

// tasks of class k in row order; giant rows also get their bitmap slot
__global__ void k_jac_emit(const int8_t *__restrict__ cls, const int32_t *__restrict__ ntask,
                           const int64_t *__restrict__ off, const int64_t *__restrict__ goff,
                           int64_t r0, int64_t r1, int k, int32_t *__restrict__ trow,
                           int32_t *__restrict__ ti, int32_t *__restrict__ tslot,
                           int32_t *__restrict__ grow) {
    for (int64_t u = r0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < r1;
         u += (int64_t)gridDim.x * blockDim.x) {
        if (cls[u] != k) continue;
        const int32_t nt = ntask[u];
        if (!nt) continue;
        const int64_t o = off[u - r0];
        const int32_t g = goff ? (int32_t)goff[u - r0] : 0;
        if (goff) grow[g] = (int32_t)u;
        for (int32_t i = 0; i < nt; ++i) {
            trow[o + i] = (int32_t)u;
            ti[o + i] = i;
            if (tslot) tslot[o + i] = g;
        }
    }
}

// B_J for a symmetric graph: 8 * sum_u d_u^2 + 12 * nnz
__global__ void k_jac_bytes(const int64_t *__restrict__ ip, int64_t n,
                            unsigned long long *__restrict__ acc) {
    unsigned long long s = 0;
    for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < n;
         u += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long d = (unsigned long long)(ip[u + 1] - ip[u]);
        s += d * d;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(acc, s);
}

// sum of squared degrees, once per graph (the profile's byte count)
double jac_deg2(gs_ctx *c) {
    JacState &J = jac_state(c);
    Graph &g = c->g;
    if (J.deg2_epoch != g.epoch) {
        hipStream_t st = c->stream;
        auto *acc = (unsigned long long *)c->buf("jac_bytes").ensure(8);
        GS_HIP(hipMemsetAsync(acc, 0, 8, st));
        k_jac_bytes<<<grid_for(g.n, 256, 4096), 256, 0, st>>>(g.indptr.as<int64_t>(), g.n, acc);
        unsigned long long s = 0;
        GS_HIP(hipMemcpyAsync(&s, acc, 8, hipMemcpyDeviceToHost, st));
        GS_HIP(hipStreamSynchronize(st));
        J.deg2 = (double)s;
        J.deg2_epoch = g.epoch;
    }
    return J.deg2;
}

// bitmaps in batches of rows (<= 1 GiB of bits at a time): each batch's task range.
// Tasks are in row order, so batch [g0, g1) holds the tasks from the first of row
// grow[g0] to the first of row grow[g1]; off = the task offsets by row - r0.
static void plan_batches(gs_ctx *c, const JacKnobs &k, JacPlan &p, const int64_t *off) {
    hipStream_t st = c->stream;
    const int64_t words = (p.n + 31) / 32;
    int64_t per = ((int64_t)1 << 30) / (4 * words);
    if (per < 1) per = 1;
    if (k.bmrows >= 1 && k.bmrows < per) per = k.bmrows;
    std::vector<int32_t> hrow(p.ngiant);
    GS_HIP(hipMemcpyAsync(hrow.data(), p.grow, sizeof(int32_t) * p.ngiant, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    for (int64_t g0 = 0; g0 < p.ngiant; g0 += per) {
        const int64_t g1 = g0 + per < p.ngiant ? g0 + per : p.ngiant;
        int64_t tb[2] = {0, p.tot[kJacBitmap]};
        GS_HIP(hipMemcpyAsync(&tb[0], off + (hrow[g0] - p.r0), 8, hipMemcpyDeviceToHost, st));
        if (g1 < p.ngiant)
            GS_HIP(hipMemcpyAsync(&tb[1], off + (hrow[g1] - p.r0), 8, hipMemcpyDeviceToHost, st));
        GS_HIP(hipStreamSynchronize(st));
        p.batches.push_back({g0, g1, tb[0], tb[1]});
    }
}

const JacPlan &jac_plan(gs_ctx *c, const JacKnobs &k, int64_t r0, int64_t r1) {
    Graph &g = c->g;
    JacPlan &p = jac_state(c).plan;
    if (p.has(g.epoch, r0, r1, g.n, g.nnz, k.bmrows)) return p;
    p.valid = false;  // until everything below is in place
    p.epoch = g.epoch, p.r0 = r0, p.r1 = r1, p.n = g.n, p.nnz = g.nnz, p.bmrows = k.bmrows;
    p.batches.clear();
    hipStream_t st = c->stream;
    const int64_t n = g.n, nr = r1 - r0;  // this part's rows: planned, task lists emitted
    const int64_t *ip = g.indptr.as<int64_t>();
    const int32_t *ix = g.indices.as<int32_t>();
    p.cls = (int8_t *)c->buf("jac_cls").ensure(n);
    p.ntask = (int32_t *)c->buf("jac_ntask").ensure(sizeof(int32_t) * n);
    auto *cnt = (int64_t *)c->buf("jac_cnt").ensure(sizeof(int64_t) * (n + 1));
    auto *off = (int64_t *)c->buf("jac_off").ensure(sizeof(int64_t) * (n + 1));
    auto *gfl = (int64_t *)c->buf("jac_gflag").ensure(sizeof(int64_t) * (n + 1));
    auto *goff = (int64_t *)c->buf("jac_goff").ensure(sizeof(int64_t) * (n + 1));
    constexpr int kTot = kJacClasses + 1;
    auto *dtot = (unsigned long long *)c->buf("jac_tot").ensure(8 * kTot);
    GS_HIP(hipMemsetAsync(dtot, 0, 8 * kTot, st));
    if (nr) k_jac_plan<<<grid_for(nr, 4, 4096), 256, 0, st>>>(ip, ix, r0, r1, p.cls, p.ntask, dtot);
    GS_HIP(hipGetLastError());
    unsigned long long htot[kTot];
    GS_HIP(hipMemcpyAsync(htot, dtot, 8 * kTot, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));  // the only sync unless bitmap rows exist
    p.ngiant = (int64_t)htot[kJacClasses];
    for (int q = 0; q < kJacClasses; ++q) {
        static const char *const kTrow[kJacClasses] = {"jac_trow0", "jac_trow1", "jac_trow2",
                                                      "jac_trow3", "jac_trow4"};
        static const char *const kTi[kJacClasses] = {"jac_ti0", "jac_ti1", "jac_ti2", "jac_ti3",
                                                    "jac_ti4"};
        const int64_t ntot = p.tot[q] = (int64_t)htot[q];
        GS_CHECK(ntot <= INT32_MAX, GS_EUNSUPPORTED, "too many Jaccard tasks (%lld)", (long long)ntot);
        if (!ntot) continue;
        const bool giant = q == kJacBitmap;
        p.trow[q] = (int32_t *)c->buf(kTrow[q]).ensure(sizeof(int32_t) * ntot);
        p.ti[q] = (int32_t *)c->buf(kTi[q]).ensure(sizeof(int32_t) * ntot);
        if (giant) {
            p.tslot = (int32_t *)c->buf("jac_tslot").ensure(sizeof(int32_t) * ntot);
            p.grow = (int32_t *)c->buf("jac_grow").ensure(sizeof(int32_t) * p.ngiant);
        }
        GS_HIP(hipMemsetAsync(cnt + nr, 0, sizeof(int64_t), st));
        GS_HIP(hipMemsetAsync(gfl + nr, 0, sizeof(int64_t), st));
        k_jac_mask<<<grid_for(nr, 256, 16384), 256, 0, st>>>(p.cls, p.ntask, r0, r1, q, cnt,
                                                             giant ? gfl : nullptr);
        exclusive_scan_i64(c, cnt, off, nr + 1);
        if (giant) exclusive_scan_i64(c, gfl, goff, nr + 1);
        k_jac_emit<<<grid_for(nr, 256, 16384), 256, 0, st>>>(p.cls, p.ntask, off, giant ? goff : nullptr,
                                                             r0, r1, q, p.trow[q], p.ti[q],
                                                             giant ? p.tslot : nullptr,
                                                             giant ? p.grow : nullptr);
        GS_HIP(hipGetLastError());
        if (giant) plan_batches(c, k, p, off);
    }
    p.valid = true;
    return p;
}

}  // namespace gs
