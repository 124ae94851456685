// gs_random.hip -- the symmetric random baseline on the device
// (precompute_random_scores / random_sparsify, random.py:14-52).
//
// gs_undirected_ids replaces np.unique(keys, return_inverse=True) (random.py:23-30):
// a range-check and key pass, a rocPRIM radix sort of (key, column) pairs over
// bits_for((n + 1)^2) bits (32-bit columns while E < 2^32), head flags, a scan, and
// the scatter inverse[column] = rank.  One host wait, for the status and the count.
// gs_random_mask is random.py:45-49: gs_topk_mask's select of the n_keep highest
// undirected scores into context scratch, then mask[i] = keep_undir[inverse[i]].
// The per-element logic is gs_random.hpp's.
#include "gs_random.hpp"
#include "gs_sort.hpp"
#include "gs_wave.hpp"

namespace gs {

static int bits_for(uint64_t v) {
    int b = 0;
    while (b < 64 && (v >> b)) ++b;
    return b < 1 ? 1 : b;
}

// what the host reads back: written with vector stores and atomics only
struct RandState {
    int bad;                    // an id outside [0, n)
    int pad;
    long long count;            // distinct keys
    unsigned long long n_bad;   // inverse entries outside [-m, m)
};

template <class P>
__global__ void k_und_keys(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, int64_t E,
                           int64_t n, uint64_t *__restrict__ keys, P *__restrict__ pos,
                           RandState *__restrict__ st) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        int64_t s = src[i], d = dst[i];
        if (!undirected_in_range(s, d, n)) {
            atomicOr(&st->bad, 1);
            s = d = 0;
        }
        keys[i] = undirected_key(s, d, n);
        pos[i] = (P)i;
    }
}

__global__ void k_und_flags(const uint64_t *__restrict__ keys, int64_t E, int64_t *__restrict__ flag) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x)
        flag[i] = undirected_head(keys, i);
}

// nothing is written for an input outside the contract (st->bad)
template <class P>
__global__ void k_und_scatter(const int64_t *__restrict__ flag, const int64_t *__restrict__ before,
                              const P *__restrict__ pos, int64_t E, RandState *__restrict__ st,
                              int64_t *__restrict__ inverse) {
    if (st->bad) return;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = undirected_rank(before[i], flag[i]);
        inverse[(int64_t)pos[i]] = r;
        if (i == E - 1) st->count = r + 1;
    }
}

__global__ void k_rand_gather(const uint8_t *__restrict__ keep, int64_t m, const int64_t *__restrict__ inverse,
                              int64_t E, uint8_t *__restrict__ mask, RandState *__restrict__ st) {
    unsigned long long bad = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t w = wrap_index(inverse[i], m);
        mask[i] = w < 0 ? (uint8_t)0 : keep[w];
        bad += w < 0;
    }
    bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&st->n_bad, bad);
}

// (key, column) pairs sorted by key; keys / vals then point at the sorted copies
// (the caller's buffers or scratch[4] / scratch[3]: no copy back)
template <class P>
static void sort_pairs(gs_ctx *c, uint64_t *&keys, P *&vals, int64_t n, int end_bit) {
    if (n <= 1) return;  // nothing to sort: no alternates either
    uint64_t *k2 = (uint64_t *)c->scratch[4].ensure(sizeof(uint64_t) * n);
    P *v2 = (P *)c->scratch[3].ensure(sizeof(P) * n);
    const auto r = radix_sort_pairs(c, c->scratch[5], keys, k2, vals, v2, n, 0, end_bit, c->stream);
    keys = r.keys;
    vals = r.vals;
}

template <class P>
static void undirected_ids(gs_ctx *c, int64_t n, int64_t E, const int64_t *dsrc, const int64_t *ddst,
                           RandState *st, int64_t *dinv) {
    hipStream_t s = c->stream;
    const unsigned g = grid_for(E, 256, 8192);
    const int bits = bits_for((uint64_t)(n + 1) * (uint64_t)(n + 1));
    uint64_t *keys = (uint64_t *)c->scratch[2].ensure(sizeof(uint64_t) * E);
    P *pos = (P *)c->buf("rand_pos").ensure(sizeof(P) * E);
    int64_t *flag = (int64_t *)c->scratch[0].ensure(sizeof(int64_t) * E);
    int64_t *before = (int64_t *)c->scratch[1].ensure(sizeof(int64_t) * E);
    hipEvent_t t0 = prof_begin(c);
    k_und_keys<P><<<g, 256, 0, s>>>(dsrc, ddst, E, n, keys, pos, st);
    prof_end(c, t0, "undirected_keys", (16.0 + 8.0 + sizeof(P)) * E);
    t0 = prof_begin(c);
    sort_pairs<P>(c, keys, pos, E, bits);
    // every 8-bit digit pass reads and writes the pairs; one histogram read of the keys
    prof_end(c, t0, "undirected_sort", ((bits + 7) / 8) * 2.0 * (8.0 + sizeof(P)) * E + 8.0 * E);
    t0 = prof_begin(c);
    k_und_flags<<<g, 256, 0, s>>>(keys, E, flag);
    exclusive_scan_i64(c, flag, before, E);
    prof_end(c, t0, "undirected_scan", (8.0 + 8.0 + 8.0 + 8.0) * E);
    t0 = prof_begin(c);
    k_und_scatter<P><<<g, 256, 0, s>>>(flag, before, pos, E, st, dinv);
    GS_HIP(hipGetLastError());
    prof_end(c, t0, "undirected_scatter", (8.0 + 8.0 + sizeof(P) + 8.0) * E);
}

}  // namespace gs

using namespace gs;

extern "C" int gs_undirected_ids(gs_ctx *c, int64_t n, int64_t E, const int64_t *src, const int64_t *dst,
                                 int loc, int64_t *inverse, int inv_loc, int64_t *n_undirected,
                                 int32_t *status) {
    return guard([&] {
        GS_CHECK(c && status, GS_EINVAL, "null context/status");
        *status = 1;
        // outside the device contract: the caller makes the reference's own calls
        if (E < 1 || n < 1 || n >= (int64_t(1) << 31)) return;
        GS_CHECK(src && dst && inverse, GS_EINVAL, "null src/dst/inverse");
        GS_HIP(hipSetDevice(c->device));
        const int64_t *dsrc = (const int64_t *)to_device(c, c->inbuf, src, sizeof(int64_t) * E, loc);
        const int64_t *ddst = (const int64_t *)to_device(c, c->inbuf2, dst, sizeof(int64_t) * E, loc);
        int64_t *dinv = (int64_t *)out_device(c, c->outbuf, inverse, sizeof(int64_t) * E, inv_loc);
        RandState *st = (RandState *)c->buf("rand_st").ensure(sizeof(RandState));
        GS_HIP(hipMemsetAsync(st, 0, sizeof(RandState), c->stream));
        if (E < (int64_t(1) << 32)) undirected_ids<uint32_t>(c, n, E, dsrc, ddst, st, dinv);
        else undirected_ids<int64_t>(c, n, E, dsrc, ddst, st, dinv);
        RandState h;
        GS_HIP(hipMemcpyAsync(&h, st, sizeof(RandState), hipMemcpyDeviceToHost, c->stream));
        GS_HIP(hipStreamSynchronize(c->stream));
        if (h.bad) return;
        if (inv_loc != GS_DEVICE) {
            GS_HIP(hipMemcpyAsync(inverse, dinv, sizeof(int64_t) * E, hipMemcpyDeviceToHost, c->stream));
            GS_HIP(hipStreamSynchronize(c->stream));
        }
        if (n_undirected) *n_undirected = (int64_t)h.count;
        *status = 0;
    });
}

extern "C" int gs_random_mask(gs_ctx *c, const double *scores, int s_loc, int64_t m, int64_t n_keep,
                              const int64_t *inverse, int i_loc, int64_t E, uint8_t *mask, int m_loc,
                              double *cut, int64_t *n_beyond, int64_t *n_tied, int64_t *n_bad) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        GS_CHECK(m >= 1 && E >= 0, GS_EINVAL, "need m >= 1 scores and E >= 0 (m=%lld, E=%lld)",
                 (long long)m, (long long)E);
        GS_CHECK(n_keep >= 1, GS_EINVAL, "need n_keep >= 1 (n_keep=%lld)", (long long)n_keep);
        GS_CHECK(scores && (E == 0 || (inverse && mask)), GS_EINVAL, "null scores/inverse/mask");
        GS_HIP(hipSetDevice(c->device));
        // keep_undir: argsort(scores)[-n_keep:] keeps everything once n_keep >= m
        uint8_t *keep = (uint8_t *)c->buf("rand_keep").ensure((size_t)m);
        const int rc = gs_topk_mask(c, scores, s_loc, m, m, n_keep < m ? n_keep : m, 0, keep, GS_DEVICE,
                                    cut, n_beyond, n_tied);
        if (rc != GS_OK) throw GsError{rc};
        RandState h{};
        if (E > 0) {
            const int64_t *dinv =
                (const int64_t *)to_device(c, c->inbuf2, inverse, sizeof(int64_t) * E, i_loc);
            uint8_t *dm = (uint8_t *)out_device(c, c->outbuf, mask, (size_t)E, m_loc);
            RandState *st = (RandState *)c->buf("rand_st").ensure(sizeof(RandState));
            GS_HIP(hipMemsetAsync(st, 0, sizeof(RandState), c->stream));
            hipEvent_t t0 = prof_begin(c);
            k_rand_gather<<<grid_for(E, 256, 8192), 256, 0, c->stream>>>(keep, m, dinv, E, dm, st);
            GS_HIP(hipGetLastError());
            prof_end(c, t0, "random_gather", (8.0 + 1.0 + 1.0) * E);
            GS_HIP(hipMemcpyAsync(&h, st, sizeof(RandState), hipMemcpyDeviceToHost, c->stream));
            GS_HIP(hipStreamSynchronize(c->stream));
            finish_out(c, mask, dm, (size_t)E, m_loc);
        }
        if (n_bad) *n_bad = (int64_t)h.n_bad;
    });
}
