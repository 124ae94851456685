// gs_bb_mitm.hip -- the meet-in-the-middle certificate of the metric backbone
// (GSPARSE_BB_MITM=1; off by default, see bb_certify): the PAIR form of
// k_bb_sssp_multi and its driver.
#include "gs_bb.hpp"
#include "gs_bb_multi.hpp"

namespace gs {

// the pair certificate's columns in [c0, c1): open, not a self-loop, one of each
// (u, v) / (v, u) pair (the u < v one when both are open)
__global__ void k_bb_pairflag(const int64_t *__restrict__ src, const int64_t *__restrict__ dst,
                              const uint8_t *__restrict__ state, const int64_t *__restrict__ rpos,
                              const int64_t *__restrict__ sidx, int64_t c0, int64_t c1,
                              int64_t *__restrict__ flag) {
    for (int64_t i = c0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < c1;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t u = src[i], v = dst[i];
        int64_t f = 0;
        if (state[i] == 0 && u != v) {
            const int64_t rp = rpos[i];
            f = (u < v || rp < 0 || state[sidx[rp]] != 0) ? 1 : 0;
        }
        flag[i - c0] = f;
    }
}

// lmflag[x] = 1 for the complete landmarks (k_bb_sssp_multi PAIR does not expand them)
__global__ void k_bb_lmflag(const int32_t *__restrict__ lm, const int32_t *__restrict__ lcomp, int K,
                            uint8_t *__restrict__ lmflag) {
    for (int l = threadIdx.x; l < K; l += blockDim.x)
        if (lcomp[l]) lmflag[lm[l]] = 1;
}

__global__ void k_bb_pcompact(const int64_t *__restrict__ flag, const int64_t *__restrict__ pos,
                              int64_t c0, int64_t cnt, int64_t *__restrict__ out) {
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < cnt;
         j += (int64_t)gridDim.x * blockDim.x)
        if (flag[j]) out[pos[j]] = c0 + j;
}

// the open columns of [c0, c1), one of each pair, searched from both ends (bb_certify)
void bb_mitm(gs_ctx *c, BbRun &R, const BbKnobs &k, int64_t c0, int64_t c1, int part, int nparts) {
    hipStream_t s = c->stream;
    hipEvent_t tq = prof_begin(c);
    bb_keys(c);
    const int64_t nc = c1 - c0;
    int64_t *pf = (int64_t *)c->buf("bb_pflag").ensure(8 * (nc + 1));
    int64_t *pp = (int64_t *)c->buf("bb_ppos").ensure(8 * (nc + 1));
    k_bb_pairflag<<<grid_for(nc, 256, 8192), 256, 0, s>>>(R.dsrc, R.ddst, R.state, R.rpos, R.sidx, c0,
                                                           c1, pf);
    exclusive_scan_i64(c, pf, pp, nc);
    int64_t lastp = 0, lastf = 0;
    GS_HIP(hipMemcpyAsync(&lastp, pp + nc - 1, 8, hipMemcpyDeviceToHost, s));
    GS_HIP(hipMemcpyAsync(&lastf, pf + nc - 1, 8, hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));
    const int64_t np = lastp + lastf;
    if (k.debug) fprintf(stderr, "[backbone] pair certificate: %lld open pairs\n", (long long)np);
    if (np > 0) {
        int64_t *plist = (int64_t *)c->buf("bb_plist").ensure(8 * np);
        k_bb_pcompact<<<grid_for(nc, 256, 8192), 256, 0, s>>>(pf, pp, c0, nc, plist);
        int64_t P = 512;
        if (k.mitm_slabs > 0) P = k.mitm_slabs;
        P = std::min<int64_t>(P, np);
        const int64_t cap = (int64_t)(48e9 / (44.0 * (double)R.n));  // slab bytes per node: 2 x 8 + 28
        if (P > cap) P = std::max<int64_t>(cap, 1);
        const BbSlabs sl = bb_slabs(c, 2, P, R.n, true, false);
        const double delta = k.nearfar > 0.0 && R.wmed > 0.0 ? k.nearfar * R.wmed : 0.0;
        unsigned long long *bnext = R.misc + 2;
        GS_HIP(hipMemsetAsync(bnext, 0, 8, s));
        // complete landmarks blocked (GSPARSE_BB_MITM_LM=0: expanded like any node)
        uint8_t *lmf = nullptr;
        if (R.K > 0 && k.mitm_lm) {
            lmf = (uint8_t *)c->buf("bb_lmflag").ensure((size_t)R.n);
            GS_HIP(hipMemsetAsync(lmf, 0, (size_t)R.n, s));
            k_bb_lmflag<<<1, 64, 0, s>>>((const int32_t *)c->buf("bb_lm").ptr, R.lcomp, R.K, lmf);
        }
        // GSPARSE_BB_TRACE: as the searches', one line per launch ("pairs": true)
        const BbTrace tr = bb_trace_begin(c, k.trace, np);
        k_bb_sssp_multi<512, 2, true><<<(unsigned)P, 512, 0, s>>>(
            R.gp, R.gi, R.gw, R.n, plist, np, R.optr, R.order, R.dsrc, R.ddst, R.dw, R.eps, R.state,
            sl.dist, (uint32_t *)sl.qflag, sl.fr, sl.fm, sl.touched, sl.farl, delta, 0, R.skeys, R.sidx,
            R.rpos, R.E, R.mrg, 0, 0, np, 0, 1, bnext, R.misc + 1, tr.rec, R.why, lmf, R.D, R.lcomp, R.K);
        GS_HIP(hipGetLastError());
        bb_trace_end(c, tr, "\"pairs\": true, ", part, nparts, 0, np, 2, P);
    }
    prof_end(c, tq, "bb_pairs", 0.0);
}

}  // namespace gs
