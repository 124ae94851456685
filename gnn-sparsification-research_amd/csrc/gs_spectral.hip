// gs_spectral.hip -- spectral sparsification by effective-resistance sampling on the
// device (Spielman-Srivastava; selection.spectral_sample is the definition,
// gs_spectral.hpp has the per-element rules): q draws with replacement over the
// undirected pairs with probability proportional to their score, a kept pair's weight
// count / (q p), bit for bit what NumPy computes.
//
//   pairs          gs_undirected_ids names every column's unordered pair
//   pair reduce    an integer atomicMin of the column index and an integer atomicAdd of
//                  the column count per pair (32-bit while E < 2^32)
//   gather         r[j] = the score of pair j's lowest column, 0 for loops and scores
//                  that are NaN, +-inf or <= 0; the non-loop pairs without exactly two
//                  columns are counted (n_irregular)
//   total, norm    gs_sample.hip's blocked pairwise np.sum, then p = r / total
//   multinomial    gs_sample.hip's ordered cumsum and divide; draw j is stream position
//                  j (runs of 8 per thread), searched in the cdf and counted with an
//                  integer atomicAdd on uint32 cnt[i] (a two-level search through a
//                  coarse table in LDS was measured and not kept)
//   independent    one fused pass: the uniform of pair j is stream position j, compared
//                  with min(1, q p_j); no array of uniforms is stored
//   weights        per column: c = cnt[inverse[col]], mask = c > 0, weight = c / (q p)
//                  (1 / min(1, q p) for the independent method)
// Integer adds and minima commute and there are no float atomics, so every output is
// the same bytes on every run.  The host reads the status words only.
#include "gs_sample_dev.hpp"
#include "gs_spectral.hpp"

namespace gs {

// what the host reads back: written with vector stores and atomics only
struct SpcState {
    unsigned long long n_irregular;  // non-loop pairs without exactly two columns
    unsigned long long n_kept;       // pairs with a count > 0
    unsigned int max_count;
    unsigned int pad;
};

template <class P>
__global__ void k_spc_first(const int64_t *__restrict__ inv, int64_t E, P *__restrict__ first,
                            P *__restrict__ ncol) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = inv[i];
        atomicMin(&first[j], (P)i);
        atomicAdd(&ncol[j], (P)1);
    }
}

template <class P>
__global__ void k_spc_gather(const double *__restrict__ scores, const int64_t *__restrict__ src,
                             const int64_t *__restrict__ dst, const P *__restrict__ first,
                             const P *__restrict__ ncol, int64_t m, double *__restrict__ r,
                             SpcState *__restrict__ st) {
    unsigned long long irr = 0;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m;
         j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = (int64_t)first[j];  // every pair has a column: f < E
        const bool loop = src[f] == dst[f];
        r[j] = spectral_rate(scores[f], loop);
        irr += spectral_irregular((uint64_t)ncol[j], loop);
    }
    for (int off = 32; off > 0; off >>= 1) irr += __shfl_down(irr, off, 64);
    if ((threadIdx.x & 63) == 0 && irr) atomicAdd(&st->n_irregular, irr);
}

__global__ void k_spc_norm(double *__restrict__ p, int64_t m, const SmpState *__restrict__ st) {
    const double tot = st->total;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m;
         j += (int64_t)gridDim.x * blockDim.x)
        p[j] = p[j] / tot;
}

// thread t: draws [t kSampleRun, (t + 1) kSampleRun), s0 = the stream state before draw 0
__global__ void __launch_bounds__(256) k_spc_draw(const double *__restrict__ cdf, int64_t m, u128 s0,
                                                  u128 inc, int64_t q, unsigned int *__restrict__ cnt) {
    const int64_t j0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) * kSampleRun;
    if (j0 >= q) return;
    Pcg64 g{pcg_advance(s0, inc, (uint64_t)j0), inc};
    const int64_t j1 = j0 + kSampleRun < q ? j0 + kSampleRun : q;
    for (int64_t j = j0; j < j1; ++j) {
        const double x = sample_double(g.next());
        const int64_t i = sample_search(cdf, m, x);
        if (i < m) atomicAdd(&cnt[i], 1u);  // cdf[m - 1] == 1 > x: always
    }
}

// thread t: pairs [t kSampleRun, (t + 1) kSampleRun); the uniform of pair j is stream position j
__global__ void __launch_bounds__(256) k_spc_indep(const double *__restrict__ p, int64_t m, double q,
                                                   u128 s0, u128 inc, unsigned int *__restrict__ cnt) {
    const int64_t j0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) * kSampleRun;
    if (j0 >= m) return;
    Pcg64 g{pcg_advance(s0, inc, (uint64_t)j0), inc};
    const int64_t j1 = j0 + kSampleRun < m ? j0 + kSampleRun : m;
    for (int64_t j = j0; j < j1; ++j) {
        const double x = sample_double(g.next());
        cnt[j] = x < spectral_keep_prob(q, p[j]) ? 1u : 0u;
    }
}

// the kept pairs, the largest count and (optional) the counts as int64
__global__ void k_spc_stats(const unsigned int *__restrict__ cnt, int64_t m, int64_t *__restrict__ counts,
                            SpcState *__restrict__ st) {
    unsigned long long kept = 0;
    unsigned int mx = 0;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m;
         j += (int64_t)gridDim.x * blockDim.x) {
        const unsigned int c = cnt[j];
        if (counts) counts[j] = (int64_t)c;
        kept += c > 0;
        mx = c > mx ? c : mx;
    }
    for (int off = 32; off > 0; off >>= 1) {
        kept += __shfl_down(kept, off, 64);
        const unsigned int o = __shfl_down(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0) {
        if (kept) atomicAdd(&st->n_kept, kept);
        if (mx) atomicMax(&st->max_count, mx);
    }
}

__global__ void k_spc_weights(const unsigned int *__restrict__ cnt, const double *__restrict__ p,
                              const int64_t *__restrict__ inv, int64_t E, double q, int method,
                              uint8_t *__restrict__ mask, double *__restrict__ weight,
                              int64_t *__restrict__ inv_out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = inv[i];
        const unsigned int c = cnt[j];
        mask[i] = c > 0;
        weight[i] = spectral_weight(c, q, p[j], method);
        if (inv_out) inv_out[i] = j;
    }
}

template <class P>
static void pair_rates(gs_ctx *c, const double *ds, const int64_t *dsrc, const int64_t *ddst,
                       const int64_t *inv, int64_t E, int64_t m, double *r, SpcState *st) {
    hipStream_t s = c->stream;
    P *first = (P *)c->buf("spc_first").ensure(sizeof(P) * m);
    P *ncol = (P *)c->buf("spc_ncol").ensure(sizeof(P) * m);
    hipEvent_t t0 = prof_begin(c);
    GS_HIP(hipMemsetAsync(first, 0xff, sizeof(P) * m, s));
    GS_HIP(hipMemsetAsync(ncol, 0, sizeof(P) * m, s));
    k_spc_first<P><<<grid_for(E, 256, 8192), 256, 0, s>>>(inv, E, first, ncol);
    GS_HIP(hipGetLastError());
    prof_end(c, t0, "spectral_pair_reduce", (8.0 + 4.0 * sizeof(P)) * E);
    t0 = prof_begin(c);
    k_spc_gather<P><<<grid_for(m, 256, 8192), 256, 0, s>>>(ds, dsrc, ddst, first, ncol, m, r, st);
    GS_HIP(hipGetLastError());
    prof_end(c, t0, "spectral_gather", (2.0 * sizeof(P) + 8.0 * 4) * m);
}

}  // namespace gs

using namespace gs;

extern "C" int gs_spectral_sample(gs_ctx *c, const double *scores, int s_loc, int64_t nscores,
                                  const int64_t *src, const int64_t *dst, int loc, int64_t E, int64_t n,
                                  int64_t q, int method, uint64_t state_hi, uint64_t state_lo,
                                  uint64_t inc_hi, uint64_t inc_lo, uint8_t *mask, int m_loc,
                                  double *weight, int w_loc, int64_t *counts, int c_loc,
                                  int64_t *inverse, int i_loc, int64_t *m_out, int64_t *n_kept_pairs,
                                  int64_t *max_count, int64_t *n_irregular, int64_t *draws,
                                  int32_t *status) {
    return guard([&] {
        GS_CHECK(c && status, GS_EINVAL, "null context/status");
        *status = 1;
        GS_CHECK(method == kSpectralMultinomial || method == kSpectralIndependent, GS_EINVAL,
                 "method must be 0 (multinomial) or 1 (independent), got %d", method);
        // outside the device contract: the caller evaluates the specification on the host
        if (E < 1 || n < 1 || n >= (int64_t(1) << 31) || nscores < E || q < 1 || q >= (int64_t(1) << 31))
            return;
        GS_CHECK(scores && src && dst && mask && weight, GS_EINVAL, "null scores/src/dst/mask/weight");
        GS_HIP(hipSetDevice(c->device));
        hipStream_t s = c->stream;
        const double *ds = (const double *)to_device(c, c->buf("spc_s"), scores, sizeof(double) * E, s_loc);
        const int64_t *dsrc = (const int64_t *)to_device(c, c->buf("spc_src"), src, sizeof(int64_t) * E, loc);
        const int64_t *ddst = (const int64_t *)to_device(c, c->buf("spc_dst"), dst, sizeof(int64_t) * E, loc);
        // the ids go to scratch first: nothing of the caller's is written before the gates
        int64_t *inv = (int64_t *)c->buf("spc_inv").ensure(sizeof(int64_t) * E);
        int32_t id_status = 1;
        int64_t m = 0;
        const int rc = gs_undirected_ids(c, n, E, dsrc, ddst, GS_DEVICE, inv, GS_DEVICE, &m, &id_status);
        if (rc != GS_OK) throw GsError{rc};
        if (id_status != 0) return;
        GS_CHECK(m >= 1 && m <= E, GS_EHIP, "gs_undirected_ids gave %lld pairs for %lld columns",
                 (long long)m, (long long)E);

        double *p = (double *)c->buf("spc_p").ensure(sizeof(double) * m);
        SpcState *st = (SpcState *)c->buf("spc_st").ensure(sizeof(SpcState));
        SmpState *sst = (SmpState *)c->buf("smp_st").ensure(sizeof(SmpState));
        GS_HIP(hipMemsetAsync(st, 0, sizeof(SpcState), s));
        if (E < (int64_t(1) << 32)) pair_rates<unsigned int>(c, ds, dsrc, ddst, inv, E, m, p, st);
        else pair_rates<unsigned long long>(c, ds, dsrc, ddst, inv, E, m, p, st);
        SmpState h{};
        hipEvent_t t0 = prof_begin(c);
        sample_total_device(c, p, m, sst, &h);
        prof_end(c, t0, "spectral_total", 8.0 * (double)m);
        if (h.bad) return;  // a total that is not finite and positive
        t0 = prof_begin(c);
        k_spc_norm<<<grid_for(m, 256, 8192), 256, 0, s>>>(p, m, sst);
        GS_HIP(hipGetLastError());
        prof_end(c, t0, "spectral_norm", 8.0 * 2 * (double)m);

        unsigned int *cnt = (unsigned int *)c->buf("spc_cnt").ensure(sizeof(unsigned int) * m);
        const u128 inc = make_u128(inc_hi, inc_lo);
        const u128 s0 = make_u128(state_hi, state_lo);
        const double qd = (double)q;
        if (method == kSpectralMultinomial) {
            double *cdf = (double *)c->buf("spc_cdf").ensure(sizeof(double) * m);
            cumsum_ordered(c, p, m, cdf, sst);
            cdf_divide(c, cdf, m, sst);
            GS_HIP(hipMemsetAsync(cnt, 0, sizeof(unsigned int) * m, s));
            t0 = prof_begin(c);
            k_spc_draw<<<sample_run_grid(q), 256, 0, s>>>(cdf, m, s0, inc, q, cnt);
            GS_HIP(hipGetLastError());
            prof_end(c, t0, "spectral_draw", (8.0 + 4.0) * (double)q);
        } else {
            t0 = prof_begin(c);
            k_spc_indep<<<sample_run_grid(m), 256, 0, s>>>(p, m, qd, s0, inc, cnt);
            GS_HIP(hipGetLastError());
            prof_end(c, t0, "spectral_independent", (8.0 + 4.0) * (double)m);
        }

        uint8_t *dm = (uint8_t *)out_device(c, c->buf("spc_mask"), mask, (size_t)E, m_loc);
        double *dw = (double *)out_device(c, c->buf("spc_w"), weight, sizeof(double) * E, w_loc);
        int64_t *dc = counts ? (int64_t *)out_device(c, c->buf("spc_cnt64"), counts, sizeof(int64_t) * m, c_loc)
                             : nullptr;
        int64_t *di = inverse && i_loc == GS_DEVICE ? inverse : nullptr;
        t0 = prof_begin(c);
        k_spc_stats<<<grid_for(m, 256, 8192), 256, 0, s>>>(cnt, m, dc, st);
        k_spc_weights<<<grid_for(E, 256, 8192), 256, 0, s>>>(cnt, p, inv, E, qd, method, dm, dw, di);
        GS_HIP(hipGetLastError());
        prof_end(c, t0, "spectral_weights", (4.0 + 8.0) * m + (8.0 + 4.0 + 8.0 + 1.0 + 8.0) * E);
        SpcState hs{};
        GS_HIP(hipMemcpyAsync(&hs, st, sizeof(SpcState), hipMemcpyDeviceToHost, s));
        GS_HIP(hipStreamSynchronize(s));
        if (counts) finish_out(c, counts, dc, sizeof(int64_t) * m, c_loc);
        if (inverse && i_loc != GS_DEVICE) finish_out(c, inverse, inv, sizeof(int64_t) * E, i_loc);
        finish_out(c, weight, dw, sizeof(double) * E, w_loc);
        finish_out(c, mask, dm, (size_t)E, m_loc);
        if (m_out) *m_out = m;
        if (n_kept_pairs) *n_kept_pairs = (int64_t)hs.n_kept;
        if (max_count) *max_count = (int64_t)hs.max_count;
        if (n_irregular) *n_irregular = (int64_t)hs.n_irregular;
        if (draws) *draws = method == kSpectralMultinomial ? q : m;
        *status = 0;
    });
}
