// gs_jac_bitmap.hip -- the symmetric Jaccard's giant rows (d > 16384): an n-bit bitmap
// of each row in global memory, built and probed a batch of rows at a time.
#include "gs_jac_probe.hpp"

namespace gs {

__global__ void k_jac_bitmap_build(const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
                                   const int32_t *__restrict__ grow, int32_t g0, int64_t words,
                                   uint32_t *__restrict__ bm) {
    const int32_t u = grow[g0 + blockIdx.y];
    uint32_t *m = bm + (int64_t)blockIdx.y * words;
    for (int64_t e = ip[u] + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < ip[u + 1];
         e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t x = ix[e];
        atomicOr(&m[x >> 5], 1u << (x & 31));
    }
}

__global__ void __launch_bounds__(1024) k_jac_bitmap(const int64_t *__restrict__ ip,
                                                     const int32_t *__restrict__ ix,
                                                     const int32_t *__restrict__ ntask,
                                                     const int32_t *__restrict__ trow,
                                                     const int32_t *__restrict__ ti,
                                                     const int32_t *__restrict__ tslot,
                                                     int64_t t0, int32_t g0, int64_t words,
                                                     const uint32_t *__restrict__ bm, JacSink sk) {
    const int64_t t = t0 + blockIdx.x;
    const int32_t u = trow[t];
    int64_t a, du, lo, hi;
    jac_task_range(ip, ntask, u, ti[t], a, du, lo, hi);
    const uint32_t *m = bm + (int64_t)(tslot[t] - g0) * words;
    __shared__ JacStage st;
    if (threadIdx.x == 0) st.nbig = st.nsmall = 0;
    __syncthreads();
    jac_stage(ip, ix, u, du, lo, hi, st);
    __syncthreads();
    jac_probe_staged(ix, du, lo, st, sk, JacBitProbe{m});
}

// each batch of the plan in turn: clear and build its rows' bitmaps, probe its tasks
void jac_launch_bitmap(gs_ctx *c, const JacPlan &p, const JacSink &sk) {
    Graph &g = c->g;
    hipStream_t st = c->stream;
    const int64_t *ip = g.indptr.as<int64_t>();
    const int32_t *ix = g.indices.as<int32_t>();
    const int64_t words = (p.n + 31) / 32;
    DevBuf &buf = c->buf("jac_bitmap");
    for (const JacPlan::Batch &b : p.batches) {
        if (b.t1 <= b.t0) continue;
        const int64_t rows = b.g1 - b.g0;
        auto *bm = (uint32_t *)buf.ensure(sizeof(uint32_t) * words * rows);
        GS_HIP(hipMemsetAsync(bm, 0, sizeof(uint32_t) * words * rows, st));
        k_jac_bitmap_build<<<dim3(64, (unsigned)rows), 256, 0, st>>>(ip, ix, p.grow, (int32_t)b.g0,
                                                                    words, bm);
        k_jac_bitmap<<<(unsigned)(b.t1 - b.t0), 1024, 0, st>>>(ip, ix, p.ntask, p.trow[kJacBitmap],
                                                               p.ti[kJacBitmap], p.tslot, b.t0,
                                                               (int32_t)b.g0, words, bm, sk);
        GS_HIP(hipGetLastError());
    }
}

}  // namespace gs
