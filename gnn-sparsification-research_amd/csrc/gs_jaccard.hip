// gs_jaccard.hip -- the symmetric Jaccard's knob reader and driver (gs_jac.hpp has the
// method and the units).
#include "gs_jac.hpp"

#include <cstdlib>
#include <cstring>

namespace gs {

JacKnobs jac_knobs() {
    JacKnobs k;
    if (const char *e = getenv("GSPARSE_JACCARD")) k.merge_only = strcmp(e, "merge") == 0;
    if (const char *e = getenv("GSPARSE_JAC_CONCURRENT")) k.concurrent = atoi(e) != 0;
    if (const char *e = getenv("GSPARSE_JAC_QDMAX")) k.qdmax = atoi(e) >= 0 ? atoi(e) : -1;
    if (const char *e = getenv("GSPARSE_JAC_BMROWS")) k.bmrows = atoi(e) >= 1 ? atoi(e) : -1;
    return k;
}

// Whole-graph Jaccard of a symmetric graph into device out[nnz], or part
// `part` of `nparts` of it: the owner entries of that part's rows (jaccard_shares),
// both CSR entries of each pair written into out (every other entry 0.0, so the
// nparts outputs sum to the whole) -- or, with cc, the raw counts into the part's
// compact owner-entry array (gs_jaccard_part_counts).
void jaccard_symmetric(gs_ctx *c, const JacKnobs &kn, double *out, int part, int nparts, int counts,
                       uint32_t *cc) {
    Graph &g = c->g;
    const int64_t n = g.n, nnz = g.nnz;
    if (!nnz) return;
    hipStream_t st = c->stream;
    int64_t r0 = 0, r1 = n, e0 = 0, e1 = nnz, obase = 0;
    if (nparts > 1) {
        const JacShares &sh = jaccard_shares(c, nparts);
        r0 = sh.R(part), r1 = sh.R(part + 1);
        e0 = sh.E(part), e1 = sh.E(part + 1);
        obase = sh.O(part);
    }
    if (nparts > 1 && !cc) GS_HIP(hipMemsetAsync(out, 0, sizeof(double) * nnz, st));
    const JacSink sk{out, g.tpos.as<int64_t>(), counts, cc, cc ? jac_owners(c).opre : nullptr, obase};
    const double algo = c->profiling ? (8.0 * jac_deg2(c) + 12.0 * (double)nnz) * ((double)(e1 - e0) / (double)nnz)
                                     : 0.0;
    hipEvent_t t0 = prof_begin(c);
    const JacPlan &p = jac_plan(c, kn, r0, r1);
    jac_launch_light(c, e0, e1, sk);
    // the hash classes run concurrently on side streams (a class of big LDS tables
    // fills one or two workgroups per CU; the others use the rest); the bitmap class
    // stays on the context stream.  GSPARSE_JAC_CONCURRENT=0: all on the context stream
    JacState &J = jac_state(c);
    int forked = 0;
    for (int k = 0; k < kJacBitmap; ++k) {
        if (!p.tot[k]) continue;
        hipStream_t hs = st;
        if (kn.concurrent) {
            if (!J.aux[k]) GS_HIP(hipStreamCreateWithFlags(&J.aux[k], hipStreamNonBlocking));
            if (!J.aux_ev[k]) GS_HIP(hipEventCreateWithFlags(&J.aux_ev[k], hipEventDisableTiming));
            GS_HIP(hipEventRecord(J.aux_ev[k], st));
            GS_HIP(hipStreamWaitEvent(J.aux[k], J.aux_ev[k], 0));
            hs = J.aux[k];
            forked |= 1 << k;
        }
        jac_launch_class(c, k, p, kn, sk, hs);
    }
    jac_launch_bitmap(c, p, sk);
    // join the side streams back into the context stream
    for (int k = 0; k < kJacBitmap; ++k)
        if (forked & (1 << k)) {
            GS_HIP(hipEventRecord(J.aux_ev[k], J.aux[k]));
            GS_HIP(hipStreamWaitEvent(st, J.aux_ev[k], 0));
        }
    prof_end(c, t0, counts ? "common_neighbors" : "jaccard", algo);
}

}  // namespace gs
