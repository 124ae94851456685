// gs_sample_dev.hpp -- the device stages of gs_sample.hip that other units share
// (gs_spectral.hip): the blocked pairwise total of np.sum, the ordered cumsum and its
// divide.  The kernels are gs_sample.hip's; the per-element logic is gs_sample.hpp's.
#pragma once
#include "gs_internal.hpp"
#include "gs_sample.hpp"

namespace gs {

static constexpr int kSampleRun = 8;  // consecutive draws per thread (one pcg_advance each)

struct SmpState {
    double total;              // p.sum()
    double last;               // cumsum(p)[-1] of the round
    unsigned long long count;  // indices claimed so far
    int bad;                   // the degenerate gate
    int pad;
};

// workgroups of 256 threads for n draws in runs of kSampleRun
inline unsigned sample_run_grid(int64_t n) {
    return (unsigned)((n + 256 * (int64_t)kSampleRun - 1) / (256 * (int64_t)kSampleRun));
}

inline u128 make_u128(uint64_t hi, uint64_t lo) { return ((u128)hi << 64) | lo; }

// st->total = np.sum(p[0, n)) (k_smp_partial / k_smp_total), st->bad = the total is not
// finite and positive, st->last = 0, st->count = 0; the stream is synchronised (the
// subtree offsets are a host temporary).  host (optional) receives *st before that wait.
void sample_total_device(gs_ctx *c, const double *p, int64_t n, SmpState *st, SmpState *host = nullptr);
// cdf = np.cumsum(p) (k_smp_cumsum; cdf must not be p), st->last = cdf[n - 1]
void cumsum_ordered(gs_ctx *c, const double *p, int64_t n, double *cdf, SmpState *st);
// cdf /= st->last (k_smp_div)
void cdf_divide(gs_ctx *c, double *cdf, int64_t n, const SmpState *st);

}  // namespace gs
