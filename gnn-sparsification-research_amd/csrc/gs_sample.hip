// gs_sample.hip -- score-proportional sampling without replacement on the device
// (GraphSparsifier.sparsify_sampled, core.py:333-350): the rejection rounds of NumPy's
// Generator.choice(replace=False, p=...), bit for bit (gs_sample.hpp has the definition
// and the per-element logic).
//
//   prep + total   p = max(nan_to_num(s), 1e-8); np.sum(p) in parallel: the pairwise tree of
//                  every 8192-element block is cut into subtrees of <= GS_SAMPLE_SUBTREE
//                  terms, one thread each; the nodes above them are combined in post-order
//                  and the blocks folded in order by one thread (the shape depends on E alone)
//   normalise      p /= total; a total that is not finite or a p that became 0 is the
//                  degenerate case (status 1: NumPy raises there)
//   per round      cdf = the ordered cumsum of p (one workgroup: the add chain is
//                  sequential by definition, a parallel scan rounds differently), divided
//                  by its last value; draw j is stream position base + j: its double is
//                  searched in cdf and the index claimed in a bitmap with an atomic OR;
//                  a fresh claim zeroes p[i] (cdf is a separate buffer) and is counted
//   driver         rounds until num_keep indices are claimed; the host reads one count
//                  per round.  A draw never lands on a zeroed index (the cdf is flat there
//                  and the search is side='right'), so the order of a round's claims does
//                  not matter and the atomics leave the result deterministic.
#include "gs_sample_dev.hpp"

namespace gs {

static constexpr int kTile = GS_SAMPLE_TILE;
static_assert(kTile % 128 == 0, "the cumsum's staging waves take 128 and 64 elements per step");
static constexpr int64_t kSub = GS_SAMPLE_SUBTREE;
static constexpr int kRun = kSampleRun;

__global__ void k_smp_prep(const double *__restrict__ s, int64_t n, double *__restrict__ p) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        p[i] = sample_prep(s[i]);
}

// task t: the pairwise sum of the subtree p[offs[t], offs[t + 1])
__global__ void __launch_bounds__(64) k_smp_partial(const double *__restrict__ p,
                                                    const int64_t *__restrict__ offs, int64_t ntask,
                                                    double *__restrict__ part) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= ntask) return;
    part[t] = sample_subtree_sum(p, offs[t], offs[t + 1] - offs[t]);
}

// the nodes above the subtrees in post-order, the blocks in order (the subtrees come in
// ascending offset)
__global__ void k_smp_total(const double *__restrict__ part, int64_t n, int64_t ntask,
                            SmpState *__restrict__ st) {
    int64_t k = 0;
    const double tot = sample_total(n, kSub, [&](int64_t, int64_t) {
        const double v = k < ntask ? part[k] : 0.0;
        ++k;
        return v;
    });
    st->total = tot;
    st->last = 0.0;
    st->count = 0ull;
    st->bad = sample_total_ok(tot) ? 0 : 1;
}

__global__ void k_smp_norm(double *__restrict__ p, int64_t n, SmpState *__restrict__ st) {
    const double tot = st->total;
    int bad = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const double v = p[i] / tot;
        p[i] = v;
        bad |= !(v > 0.0);
    }
    if (bad) atomicOr(&st->bad, 1);
}

// cdf[0] = p[0], cdf[i] = fl(cdf[i - 1] + p[i]).  One workgroup: lane 0 of wave 0 carries
// the dependent add chain over the tile in LDS (the next eight values already in registers),
// two waves load the next tile of p and one writes the previous tile of cdf back,
// coalesced, in the meantime.
__global__ void __launch_bounds__(256) k_smp_cumsum(const double *__restrict__ p, int64_t n,
                                                    double *__restrict__ cdf,
                                                    SmpState *__restrict__ st) {
    __shared__ __align__(16) double in[2][kTile], out[2][kTile];
    const int tid = threadIdx.x;
    const int64_t nt = (n + kTile - 1) / kTile;
    for (int i = tid; i < kTile; i += 256)
        if (i < n) in[0][i] = p[i];
    __syncthreads();
    double carry = 0.0;
    for (int64_t t = 0; t < nt; ++t) {
        const int b = (int)(t & 1);
        if (tid < 64) {
            if (tid == 0) {
                const int64_t left = n - t * kTile;
                const int m = left < kTile ? (int)left : kTile;
                const double *src = in[b];
                double *dst = out[b];
                int i = 0;
                if (t == 0) {  // the chain starts from p[0] itself (keeps a -0.0)
                    carry = src[0];
                    dst[0] = carry;
                    for (i = 1; i < 8 && i < m; ++i) {
                        carry = carry + src[i];
                        dst[i] = carry;
                    }
                }
                // groups of eight from a multiple of 8 (16-byte LDS accesses); the next
                // group is read before the adds of this one, so the chain never waits on LDS
                double2 a0, a1, a2, a3;
                if (i + 8 <= m) {
                    const double2 *q = (const double2 *)(src + i);
                    a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3];
                }
                while (i + 8 <= m) {
                    double2 b0 = a0, b1 = a1, b2 = a2, b3 = a3;
                    if (i + 16 <= m) {
                        const double2 *q = (const double2 *)(src + i + 8);
                        b0 = q[0], b1 = q[1], b2 = q[2], b3 = q[3];
                    }
                    const double c0 = carry + a0.x, c1 = c0 + a0.y, c2 = c1 + a1.x, c3 = c2 + a1.y;
                    const double c4 = c3 + a2.x, c5 = c4 + a2.y, c6 = c5 + a3.x, c7 = c6 + a3.y;
                    double2 *o = (double2 *)(dst + i);
                    o[0] = make_double2(c0, c1), o[1] = make_double2(c2, c3);
                    o[2] = make_double2(c4, c5), o[3] = make_double2(c6, c7);
                    carry = c7;
                    a0 = b0, a1 = b1, a2 = b2, a3 = b3;
                    i += 8;
                }
                for (; i < m; ++i) {
                    carry = carry + src[i];
                    dst[i] = carry;
                }
            }
        } else if (tid < 192) {
            // waves 1 and 2: the next tile of p, every thread's loads in flight at once
            // (indices past the end are clamped: the chain never reads those slots)
            if (t + 1 < nt) {
                const int64_t base = (t + 1) * kTile;
                const int s = tid - 64;
                double v[kTile / 128];
#pragma unroll
                for (int k = 0; k < kTile / 128; ++k) {
                    const int64_t g = base + s + 128 * k;
                    v[k] = p[g < n ? g : n - 1];
                }
#pragma unroll
                for (int k = 0; k < kTile / 128; ++k) in[b ^ 1][s + 128 * k] = v[k];
            }
        } else if (t > 0) {
            // wave 3: the previous tile of cdf (a whole tile)
            const int64_t base = (t - 1) * kTile;
            const int s = tid - 192;
#pragma unroll
            for (int k = 0; k < kTile / 64; ++k) cdf[base + s + 64 * k] = out[b ^ 1][s + 64 * k];
        }
        __syncthreads();
    }
    const int64_t base = (nt - 1) * kTile;
    const int m = (int)(n - base);
    for (int i = tid; i < m; i += 256) cdf[base + i] = out[(nt - 1) & 1][i];
    if (tid == 0) st->last = carry;
}

__global__ void k_smp_div(double *__restrict__ cdf, int64_t n, const SmpState *__restrict__ st) {
    const double last = st->last;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        cdf[i] = cdf[i] / last;
}

// thread t: draws [t kRun, (t + 1) kRun) of the round, s0 = the stream state before draw 0
__global__ void __launch_bounds__(256) k_smp_draw(const double *__restrict__ cdf, int64_t n, u128 s0,
                                                  u128 inc, int64_t nd, unsigned int *__restrict__ bits,
                                                  double *__restrict__ p, SmpState *__restrict__ st) {
    const int64_t j0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) * kRun;
    unsigned long long fresh = 0;
    if (j0 < nd) {
        Pcg64 g{pcg_advance(s0, inc, (uint64_t)j0), inc};
        const int64_t j1 = j0 + kRun < nd ? j0 + kRun : nd;
        for (int64_t j = j0; j < j1; ++j) {
            const double x = sample_double(g.next());
            const int64_t i = sample_search(cdf, n, x);
            if (i < n) {  // cdf[n - 1] == 1 > x: always
                const unsigned int bit = 1u << (i & 31);
                const unsigned int old = atomicOr(&bits[i >> 5], bit);
                if (!(old & bit)) {
                    p[i] = 0.0;
                    ++fresh;
                }
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) fresh += __shfl_down(fresh, off, 64);
    if ((threadIdx.x & 63) == 0 && fresh) atomicAdd(&st->count, fresh);
}

__global__ void k_smp_expand(const unsigned int *__restrict__ bits, int64_t n,
                             uint8_t *__restrict__ mask) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        mask[i] = (bits[i >> 5] >> (i & 31)) & 1u;
}

__global__ void __launch_bounds__(256) k_smp_doubles(u128 s0, u128 inc, int64_t n,
                                                     double *__restrict__ out) {
    const int64_t j0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) * kRun;
    if (j0 >= n) return;
    Pcg64 g{pcg_advance(s0, inc, (uint64_t)j0), inc};
    const int64_t j1 = j0 + kRun < n ? j0 + kRun : n;
    for (int64_t j = j0; j < j1; ++j) out[j] = sample_double(g.next());
}

static unsigned run_grid(int64_t n) { return sample_run_grid(n); }

void sample_total_device(gs_ctx *c, const double *p, int64_t n, SmpState *st, SmpState *host) {
    hipStream_t s = c->stream;
    std::vector<int64_t> offs;
    sample_total(n, kSub, [&](int64_t off, int64_t) {
        offs.push_back(off);
        return 0.0;
    });
    const int64_t ntask = (int64_t)offs.size();
    offs.push_back(n);
    int64_t *doffs = (int64_t *)c->buf("smp_offs").ensure(sizeof(int64_t) * offs.size());
    double *part = (double *)c->buf("smp_part").ensure(sizeof(double) * ntask);
    GS_HIP(hipMemcpyAsync(doffs, offs.data(), sizeof(int64_t) * offs.size(), hipMemcpyHostToDevice, s));
    k_smp_partial<<<grid_for(ntask, 64), 64, 0, s>>>(p, doffs, ntask, part);
    k_smp_total<<<1, 1, 0, s>>>(part, n, ntask, st);
    GS_HIP(hipGetLastError());
    if (host) GS_HIP(hipMemcpyAsync(host, st, sizeof(SmpState), hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));  // offs is a host temporary
}

// p = max(nan_to_num(s), 1e-8) / total into p[n]; st->total, st->bad set
static void sample_probs(gs_ctx *c, const double *ds, int64_t n, double *p, SmpState *st) {
    hipStream_t s = c->stream;
    hipEvent_t t0 = prof_begin(c);
    k_smp_prep<<<grid_for(n, 256, 8192), 256, 0, s>>>(ds, n, p);
    sample_total_device(c, p, n, st);
    k_smp_norm<<<grid_for(n, 256, 8192), 256, 0, s>>>(p, n, st);
    GS_HIP(hipGetLastError());
    prof_end(c, t0, "sample_probs", 8.0 * 4 * (double)n);
}

void cumsum_ordered(gs_ctx *c, const double *p, int64_t n, double *cdf, SmpState *st) {
    hipEvent_t t0 = prof_begin(c);
    k_smp_cumsum<<<1, 256, 0, c->stream>>>(p, n, cdf, st);
    GS_HIP(hipGetLastError());
    prof_end(c, t0, "sample_cumsum", 8.0 * 2 * (double)n);
}

void cdf_divide(gs_ctx *c, double *cdf, int64_t n, const SmpState *st) {
    hipEvent_t t0 = prof_begin(c);
    k_smp_div<<<grid_for(n, 256, 8192), 256, 0, c->stream>>>(cdf, n, st);
    GS_HIP(hipGetLastError());
    prof_end(c, t0, "sample_divide", 8.0 * 2 * (double)n);
}

}  // namespace gs

using namespace gs;

extern "C" int gs_sample_mask(gs_ctx *c, const double *scores, int s_loc, int64_t nscores, int64_t E,
                              int64_t num_keep, uint64_t state_hi, uint64_t state_lo,
                              uint64_t inc_hi, uint64_t inc_lo, uint8_t *mask, int m_loc,
                              int32_t *status, int64_t *rounds, int64_t *draws) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        GS_CHECK(status, GS_EINVAL, "status must not be NULL");
        *status = 1;
        if (rounds) *rounds = 0;
        if (draws) *draws = 0;
        // NumPy raises on these (a and p differ in size, a keep count outside [0, E])
        if (E < 1 || nscores != E || num_keep < 0 || num_keep > E) return;
        GS_HIP(hipSetDevice(c->device));
        hipStream_t s = c->stream;
        const double *ds = (const double *)to_device(c, c->buf("smp_s"), scores, sizeof(double) * E, s_loc);
        double *p = (double *)c->buf("smp_p").ensure(sizeof(double) * E);
        double *cdf = (double *)c->buf("smp_cdf").ensure(sizeof(double) * E);
        const int64_t nwords = (E + 31) / 32;
        unsigned int *bits = (unsigned int *)c->buf("smp_bits").ensure(sizeof(unsigned int) * nwords);
        SmpState *st = (SmpState *)c->buf("smp_st").ensure(sizeof(SmpState));
        sample_probs(c, ds, E, p, st);
        SmpState h{};
        GS_HIP(hipMemcpyAsync(&h, st, sizeof(SmpState), hipMemcpyDeviceToHost, s));
        GS_HIP(hipStreamSynchronize(s));
        if (h.bad) return;  // the mask is untouched
        uint8_t *dm = (uint8_t *)out_device(c, c->outbuf, mask, E, m_loc);
        GS_HIP(hipMemsetAsync(bits, 0, sizeof(unsigned int) * nwords, s));
        const u128 inc = make_u128(inc_hi, inc_lo);
        u128 state = make_u128(state_hi, state_lo);
        int64_t n_uniq = 0, nrounds = 0, ndraws = 0;
        while (n_uniq < num_keep) {
            const int64_t nd = num_keep - n_uniq;
            cumsum_ordered(c, p, E, cdf, st);
            cdf_divide(c, cdf, E, st);
            hipEvent_t t0 = prof_begin(c);
            k_smp_draw<<<run_grid(nd), 256, 0, s>>>(cdf, E, state, inc, nd, bits, p, st);
            GS_HIP(hipGetLastError());
            prof_end(c, t0, "sample_draw", 8.0 * (double)nd);
            unsigned long long cnt = 0;
            GS_HIP(hipMemcpyAsync(&cnt, &st->count, 8, hipMemcpyDeviceToHost, s));
            GS_HIP(hipStreamSynchronize(s));
            // every round claims at least its first draw's index
            GS_CHECK((int64_t)cnt > n_uniq && (int64_t)cnt <= num_keep, GS_EHIP,
                     "sampling round %lld claimed %lld indices after %lld (keep %lld)",
                     (long long)nrounds, (long long)cnt, (long long)n_uniq, (long long)num_keep);
            n_uniq = (int64_t)cnt;
            state = pcg_advance(state, inc, (uint64_t)nd);
            ++nrounds;
            ndraws += nd;
        }
        k_smp_expand<<<grid_for(E, 256, 8192), 256, 0, s>>>(bits, E, dm);
        GS_HIP(hipGetLastError());
        finish_out(c, mask, dm, E, m_loc);
        *status = 0;
        if (rounds) *rounds = nrounds;
        if (draws) *draws = ndraws;
    });
}

extern "C" int gs_pcg64_doubles(gs_ctx *c, uint64_t state_hi, uint64_t state_lo, uint64_t inc_hi,
                                uint64_t inc_lo, uint64_t offset, int64_t n, double *out, int loc) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        GS_CHECK(n >= 0, GS_EINVAL, "negative n");
        if (n == 0) return;
        GS_HIP(hipSetDevice(c->device));
        double *d = (double *)out_device(c, c->buf("smp_cdf"), out, sizeof(double) * n, loc);
        const u128 inc = make_u128(inc_hi, inc_lo);
        const u128 s0 = pcg_advance(make_u128(state_hi, state_lo), inc, offset);
        k_smp_doubles<<<run_grid(n), 256, 0, c->stream>>>(s0, inc, n, d);
        GS_HIP(hipGetLastError());
        finish_out(c, out, d, sizeof(double) * n, loc);
    });
}

extern "C" int gs_sample_probs(gs_ctx *c, const double *scores, int s_loc, int64_t n, double *p_out,
                               int loc, double *total_out) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        GS_CHECK(n >= 1, GS_EINVAL, "need n >= 1 (n=%lld)", (long long)n);
        GS_HIP(hipSetDevice(c->device));
        const double *ds = (const double *)to_device(c, c->buf("smp_s"), scores, sizeof(double) * n, s_loc);
        double *p = (double *)out_device(c, c->buf("smp_p"), p_out, sizeof(double) * n, loc);
        SmpState *st = (SmpState *)c->buf("smp_st").ensure(sizeof(SmpState));
        sample_probs(c, ds, n, p, st);
        if (total_out) {
            GS_HIP(hipMemcpyAsync(total_out, &st->total, 8, hipMemcpyDeviceToHost, c->stream));
            GS_HIP(hipStreamSynchronize(c->stream));
        }
        finish_out(c, p_out, p, sizeof(double) * n, loc);
    });
}

extern "C" int gs_cumsum_ordered(gs_ctx *c, const double *p, int p_loc, int64_t n, double *out, int loc) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        GS_CHECK(n >= 0, GS_EINVAL, "negative n");
        if (n == 0) return;
        GS_HIP(hipSetDevice(c->device));
        const double *dp = (const double *)to_device(c, c->buf("smp_p"), p, sizeof(double) * n, p_loc);
        double *d = (double *)out_device(c, c->buf("smp_cdf"), out, sizeof(double) * n, loc);
        GS_CHECK(dp != d, GS_EINVAL, "gs_cumsum_ordered does not work in place");
        SmpState *st = (SmpState *)c->buf("smp_st").ensure(sizeof(SmpState));
        cumsum_ordered(c, dp, n, d, st);
        finish_out(c, out, d, sizeof(double) * n, loc);
    });
}
