// gs_jac_hash.hip -- the symmetric Jaccard's light rows (sorted-list merge) and hash
// classes (the owner row's neighbour set in an LDS table, int32 slots or 16-bit
// quotient slots), with their launchers.
#include "gs_jac_probe.hpp"

namespace gs {

// light rows: one thread per owned entry, merge of two <= 32-long sorted lists
__global__ void __launch_bounds__(256) k_jac_light(const int64_t *__restrict__ ip,
                                                   const int32_t *__restrict__ ix,
                                                   const int32_t *__restrict__ rows,
                                                   int64_t e0, int64_t e1, JacSink sk) {
    for (int64_t e = e0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < e1;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t u = rows[e];
        const int64_t a = ip[u], du = ip[u + 1] - a;
        if (du > kJacLight) continue;
        const int32_t v = ix[e];
        const int64_t b = ip[v], dv = ip[v + 1] - b;
        if (!jac_owns(du, dv, u, v)) continue;
        int64_t i = 0, j = 0, cnt = 0;
        while (i < du && j < dv) {
            const int32_t x = ix[a + i], y = ix[b + j];
            cnt += (x == y);
            i += (x <= y);
            j += (y <= x);
        }
        sk.put(e, cnt, du, dv);
    }
}

// one task per workgroup; table of C int32 slots in LDS (empty = -1)
template <int C>
__global__ void __launch_bounds__(1024) k_jac_hash(const int64_t *__restrict__ ip,
                                                   const int32_t *__restrict__ ix,
                                                   const int32_t *__restrict__ ntask,
                                                   const int32_t *__restrict__ trow,
                                                   const int32_t *__restrict__ ti, int64_t t0,
                                                   JacSink sk) {
    // 4-slot buckets (one 16-B LDS read per probe step); a bucket fills from
    // slot 0 up, so a bucket with a free slot 3 ends an unsuccessful search
    __shared__ int4 tab[C / 4];
    __shared__ JacStage st;
    const int64_t t = t0 + blockIdx.x;
    const int32_t u = trow[t];
    int64_t a, du, lo, hi;
    jac_task_range(ip, ntask, u, ti[t], a, du, lo, hi);
    if (threadIdx.x == 0) st.nbig = st.nsmall = 0;
    for (int s = threadIdx.x; s < C / 4; s += blockDim.x) tab[s] = make_int4(-1, -1, -1, -1);
    __syncthreads();
    jac_stage(ip, ix, u, du, lo, hi, st);
    constexpr uint32_t shift = 32 - __builtin_ctz(C / 4);
    constexpr uint32_t mask = C / 4 - 1;
    int32_t *slots = reinterpret_cast<int32_t *>(tab);
    for (int64_t e = a + threadIdx.x; e < a + du; e += blockDim.x) {
        const int32_t x = ix[e];
        uint32_t h = jac_hash(x) >> shift;
        bool done = false;
        while (!done) {
#pragma unroll
            for (int q = 0; q < 4 && !done; ++q) {
                const int32_t prev = atomicCAS(&slots[h * 4 + q], -1, x);
                done = prev == -1 || prev == x;
            }
            h = (h + 1) & mask;
        }
    }
    __syncthreads();
    constexpr int U = C >= 16384 ? GS_JAC_UNROLL_BIG : kJacUnrollDef;
    jac_probe_staged<JacHashProbe, U>(ix, du, lo, st, sk, JacHashProbe{tab, shift, mask});
}

// one task per workgroup; C 16-bit quotient slots in LDS (gs_jac.hpp); MINW waves per SIMD
template <int C, int NT, int MINW>
__global__ void __launch_bounds__(NT, MINW) k_jac_hashq(const int64_t *__restrict__ ip,
                                                        const int32_t *__restrict__ ix,
                                                        const int32_t *__restrict__ ntask,
                                                        const int32_t *__restrict__ trow,
                                                        const int32_t *__restrict__ ti, int64_t t0,
                                                        JacQParams qp, JacSink sk) {
    constexpr int NB = C / 8;
    __shared__ uint4 tab[NB];
    __shared__ JacStage st;
    __shared__ int ovf;
    const int64_t t = t0 + blockIdx.x;
    const int32_t u = trow[t];
    int64_t a, du, lo, hi;
    jac_task_range(ip, ntask, u, ti[t], a, du, lo, hi);
    if (threadIdx.x == 0) st.nbig = st.nsmall = ovf = 0;
    for (int s = threadIdx.x; s < NB; s += blockDim.x) tab[s] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    jac_stage(ip, ix, u, du, lo, hi, st);
    uint32_t *words = reinterpret_cast<uint32_t *>(tab);
    for (int64_t e = a + threadIdx.x; e < a + du; e += blockDim.x) {
        const uint32_t h = jac_mul((uint32_t)ix[e]) & qp.hmask;
        const uint32_t home = h >> qp.qb, rem = h & qp.rmask;
        bool in = false;
        for (uint32_t d = 0; d <= qp.dmax && !in; ++d) {
            const uint32_t ent = jac_qslot(qp.qb, d, rem);
            uint32_t *w = words + ((home + d) & (NB - 1)) * 4;
            for (int q = 0; q < 8 && !in; ++q) {
                const int sh = (q & 1) * 16;
                uint32_t cur = 0;  // guess: the word is empty
                while (true) {
                    if ((cur >> sh) & 0xFFFFu) break;  // slot taken: the next one
                    const uint32_t prev = atomicCAS(&w[q >> 1], cur, cur | (ent << sh));
                    if (prev == cur) {
                        in = true;
                        break;
                    }
                    cur = prev;
                }
            }
        }
        if (!in) ovf = 1;
    }
    __syncthreads();
    if (ovf)
        jac_probe_staged<JacSortedProbe, 1>(ix, du, lo, st, sk, JacSortedProbe{ix + a, du});
    else
        jac_probe_staged<JacQProbe, (MINW >= 8 ? GS_JAC_LOADS_Q8 : GS_JAC_UNROLL_BIG),
                         (MINW >= 8 ? GS_JAC_UNROLL_Q8 : GS_JAC_UNROLL_BIG)>(ix, du, lo, st, sk,
                                                                             JacQProbe{tab, qp, NB - 1});
}

void jac_launch_light(gs_ctx *c, int64_t e0, int64_t e1, const JacSink &sk) {
    Graph &g = c->g;
    if (e1 > e0)
        k_jac_light<<<grid_for(e1 - e0, 256, 65536), 256, 0, c->stream>>>(
            g.indptr.as<int64_t>(), g.indices.as<int32_t>(), g.rows.as<int32_t>(), e0, e1, sk);
    GS_HIP(hipGetLastError());
}

// Class k's tasks, one workgroup each: the table size and form by class -- int32 slots
// (2K / 8K / 16K / 32K), or for the classes in GS_JAC_Q16 whose ids fit 16-bit quotient
// slots (16K for class 1, 32K for classes 2 and 3)
void jac_launch_class(gs_ctx *c, int k, const JacPlan &p, const JacKnobs &kn, const JacSink &sk,
                      hipStream_t s) {
    const unsigned nb = (unsigned)p.tot[k];
    if (!nb) return;
    Graph &g = c->g;
    const int64_t *ip = g.indptr.as<int64_t>();
    const int32_t *ix = g.indices.as<int32_t>();
    const int32_t *ntask = p.ntask, *trow = p.trow[k], *ti = p.ti[k];
    JacQParams qp{};
    const bool q16 = k >= 1 && k <= 3 && ((GS_JAC_Q16 >> k) & 1) &&
                     jac_qparams(p.n, k == 1 ? 16384 : 32768, qp);
    // test hook: a smaller largest distance, so the overflow path runs
    if (q16 && kn.qdmax >= 0 && kn.qdmax < (int64_t)qp.dmax) qp.dmax = (uint32_t)kn.qdmax;
    if (k == 0) {
        k_jac_hash<2048><<<nb, 256, 0, s>>>(ip, ix, ntask, trow, ti, 0, sk);
    } else if (q16 && k == 1) {
        k_jac_hashq<16384, 512, 4><<<nb, 512, 0, s>>>(ip, ix, ntask, trow, ti, 0, qp, sk);
    } else if (q16) {
        k_jac_hashq<32768, 1024, 8><<<nb, 1024, 0, s>>>(ip, ix, ntask, trow, ti, 0, qp, sk);
    } else if (k == 1) {
        k_jac_hash<8192><<<nb, 512, 0, s>>>(ip, ix, ntask, trow, ti, 0, sk);
    } else if (k == 2) {
        k_jac_hash<16384><<<nb, 1024, 0, s>>>(ip, ix, ntask, trow, ti, 0, sk);
    } else {
        k_jac_hash<32768><<<nb, 1024, 0, s>>>(ip, ix, ntask, trow, ti, 0, sk);
    }
    GS_HIP(hipGetLastError());
}

}  // namespace gs
