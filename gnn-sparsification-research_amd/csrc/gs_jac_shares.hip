// gs_jac_shares.hip -- the sharded form of the symmetric Jaccard: the rows cut into
// contiguous ranges of equal intersection work, the owner entries listed in CSR order
// (so a part's counts travel as a compact array), and the parts' counts scattered back
// into the score of every entry.  gs_jaccard_shares, gs_jaccard_part_counts,
// gs_jaccard_from_counts.
#include "gs_jac.hpp"
#include "gs_wave.hpp"

namespace gs {

// per-row intersection work of the owner entries -- light rows d_u + d_v per owned
// entry (the merge), other rows d_v per owned entry (the probes) plus d_u per task (the
// table build) -- for cutting the rows into contiguous ranges of equal work
__global__ void __launch_bounds__(256) k_jac_rowwork(const int64_t *__restrict__ ip,
                                                     const int32_t *__restrict__ ix, int64_t n,
                                                     int64_t *__restrict__ work) {
    const int lane = threadIdx.x & 63;
    const int64_t w0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t u = w0; u < n; u += nw) {
        const int64_t a = ip[u], du = ip[u + 1] - a;
        const int k = jac_class(du);
        int64_t w = 0;
        for (int64_t e = a + lane; e < a + du; e += 64) {
            const int32_t v = ix[e];
            const int64_t dv = ip[v + 1] - ip[v];
            if (jac_owns(du, dv, (int32_t)u, v)) w += k < 0 ? du + dv : dv;
        }
        w = wave_sum(w);
        if (lane == 0) work[u] = w + jac_row_tasks(k, du, w) * du;
    }
}

// owner flag of every CSR entry (1: the entry (u, v) is its pair's owner entry)
__global__ void k_jac_owner_flags(const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
                                  const int32_t *__restrict__ rows, int64_t nnz,
                                  int64_t *__restrict__ flag) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t u = rows[e], v = ix[e];
        flag[e] = jac_owns(ip[u + 1] - ip[u], ip[v + 1] - ip[v], u, v) ? 1 : 0;
    }
}

// owner list: for owner entry i (CSR order) its CSR position, its reverse entry and
// d_u + d_v, so the scatter streams them instead of reading both endpoints' indptr at
// random
__global__ void k_jac_owner_list(const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
                                 const int32_t *__restrict__ rows, const int64_t *__restrict__ rev,
                                 const int64_t *__restrict__ opre, int64_t nnz,
                                 int32_t *__restrict__ opos, int32_t *__restrict__ orev,
                                 int32_t *__restrict__ osum) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = opre[e];
        if (opre[e + 1] == i) continue;  // not an owner entry
        const int32_t u = rows[e], v = ix[e];
        opos[i] = (int32_t)e;
        orev[i] = (int32_t)rev[e];
        osum[i] = (int32_t)((ip[u + 1] - ip[u]) + (ip[v + 1] - ip[v]));
    }
}

// cut rows: R[r] = first row u with S[u] >= total * r / P (S: exclusive prefix of the
// row work, S[n] = total), R[0] = 0, R[P] = n; then E[r] = ip[R[r]] and
// O[r] = opre[E[r]].  One thread per cut (P + 1 of them, any P: the grid covers
// them all).  out = [R | E | O], 3 (P + 1) values.
__global__ void k_jac_cuts(const int64_t *__restrict__ S, const int64_t *__restrict__ ip,
                           const int64_t *__restrict__ opre, int64_t n, int P,
                           int64_t *__restrict__ out) {
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r > P) return;
    const int64_t total = S[n];
    // first u in [0, n] with S[u] >= total * r / P
    const int64_t R = r == 0 ? 0 : r == P ? n : lower_bound(S, n, total * r / P);
    out[r] = R;
    out[P + 1 + r] = ip[R];
    out[2 * (P + 1) + r] = opre[ip[R]];
}

// every part's counts -> both CSR entries of each pair, one thread per owner pair i;
// O[0..P] = cuts[2 (P + 1) ..].  fl(d_u + d_v) == d_u + d_v exactly, so the value is
// jac_value's bit for bit.
__global__ void k_jac_scatter_owners(const int32_t *__restrict__ opos, const int32_t *__restrict__ orev,
                                     const int32_t *__restrict__ osum, const int64_t *__restrict__ cuts,
                                     int P, const uint32_t *__restrict__ cc, int64_t stride,
                                     int64_t nown, double *__restrict__ out) {
    const int64_t *O = cuts + 2 * (P + 1);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nown;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int lo = jac_part_of(O, P, i);
        const int64_t cnt = cc[lo * stride + (i - O[lo])];
        const double uni = (double)osum[i] - (double)cnt;
        const double val = uni > 0.0 ? (double)cnt / uni : 0.0;
        out[opos[i]] = val;
        out[orev[i]] = val;
    }
}

// graphs past int32 positions: every part's counts -> both CSR entries
__global__ void k_jac_from_counts(const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
                                  const int32_t *__restrict__ rows, const int64_t *__restrict__ rev,
                                  const int64_t *__restrict__ opre, const int64_t *__restrict__ cuts,
                                  int P, const uint32_t *__restrict__ cc, int64_t stride,
                                  int64_t nnz, double *__restrict__ out) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t u = rows[e], v = ix[e];
        const int64_t du = ip[u + 1] - ip[u], dv = ip[v + 1] - ip[v];
        if (!jac_owns(du, dv, u, v)) continue;
        int r = 0;  // part whose row range holds u: cuts[0..P] = R
        while (r + 1 < P && u >= cuts[r + 1]) ++r;
        const int64_t cnt = cc[r * stride + (opre[e] - cuts[2 * (P + 1) + r])];
        const double val = jac_value(cnt, du, dv);
        out[e] = val;
        out[rev[e]] = val;
    }
}

// the owner prefix and lists of this graph (the same for every part count)
static void build_owners(gs_ctx *c, JacOwners &own) {
    Graph &g = c->g;
    const int64_t nnz = g.nnz;
    hipStream_t st = c->stream;
    const int64_t *ip = g.indptr.as<int64_t>();
    const int32_t *ix = g.indices.as<int32_t>();
    own = JacOwners{};
    auto *opre = (int64_t *)c->buf("jac_opre").ensure(sizeof(int64_t) * (nnz + 1));
    own.opre = opre;
    DevBuf &flags = c->buf("jac_oflag");
    auto *fl = (int64_t *)flags.ensure(sizeof(int64_t) * (nnz + 1));
    GS_HIP(hipMemsetAsync(fl + nnz, 0, sizeof(int64_t), st));
    if (nnz)
        k_jac_owner_flags<<<grid_for(nnz, 256, 65536), 256, 0, st>>>(ip, ix, g.rows.as<int32_t>(), nnz, fl);
    exclusive_scan_i64(c, fl, opre, nnz + 1);
    flags.release();
    if (nnz >= (int64_t)INT32_MAX) return;
    GS_HIP(hipMemcpyAsync(&own.nown, opre + nnz, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    const size_t b = sizeof(int32_t) * (size_t)(own.nown ? own.nown : 1);
    auto *opos = (int32_t *)c->buf("jac_opos").ensure(b);
    auto *orev = (int32_t *)c->buf("jac_orev").ensure(b);
    auto *osum = (int32_t *)c->buf("jac_osum").ensure(b);
    if (nnz)
        k_jac_owner_list<<<grid_for(nnz, 256, 65536), 256, 0, st>>>(
            ip, ix, g.rows.as<int32_t>(), g.tpos.as<int64_t>(), opre, nnz, opos, orev, osum);
    GS_HIP(hipGetLastError());
    own.opos = opos, own.orev = orev, own.osum = osum;
}

// Row ranges of the sharded form (kept per graph and part count): R[0..P] cut rows,
// E[r] = ip[R[r]], O[r] = owner entries before E[r]
const JacShares &jaccard_shares(gs_ctx *c, int P) {
    Graph &g = c->g;
    JacState &J = jac_state(c);
    if (J.shares_epoch != g.epoch) {
        J.shares.clear();
        J.shares_epoch = g.epoch;
    }
    auto it = J.shares.find(P);
    if (it != J.shares.end()) return it->second;
    const int64_t n = g.n;
    hipStream_t st = c->stream;
    const int64_t *ip = g.indptr.as<int64_t>();
    if (J.shares.empty()) build_owners(c, J.own);
    DevBuf &wb = c->buf("jac_work"), &sb = c->buf("jac_wpre");
    auto *work = (int64_t *)wb.ensure(sizeof(int64_t) * (n + 1));
    auto *S = (int64_t *)sb.ensure(sizeof(int64_t) * (n + 1));
    GS_HIP(hipMemsetAsync(work + n, 0, sizeof(int64_t), st));
    if (n) k_jac_rowwork<<<grid_for(n, 4, 4096), 256, 0, st>>>(ip, g.indices.as<int32_t>(), n, work);
    exclusive_scan_i64(c, work, S, n + 1);
    auto *dcut = (int64_t *)c->buf("jac_cutbuf").ensure(sizeof(int64_t) * 3 * (P + 1));
    k_jac_cuts<<<(unsigned)((P + 1 + 127) / 128), 128, 0, st>>>(S, ip, J.own.opre, n, P, dcut);
    GS_HIP(hipGetLastError());
    JacShares sh;
    sh.cuts.resize(3 * (P + 1));
    GS_HIP(hipMemcpyAsync(sh.cuts.data(), dcut, sizeof(int64_t) * 3 * (P + 1), hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    wb.release();
    sb.release();
    return J.shares.emplace(P, std::move(sh)).first->second;
}

const JacOwners &jac_owners(gs_ctx *c) { return jac_state(c).own; }

// gs_jaccard_from_counts: every part's counts -> the Jaccard score of every entry
void jaccard_from_counts(gs_ctx *c, int P, const uint32_t *cc, int64_t stride, double *out) {
    Graph &g = c->g;
    const int64_t nnz = g.nnz;
    if (!nnz) return;
    const JacShares &sh = jaccard_shares(c, P);
    const JacOwners &own = jac_owners(c);
    for (int r = 0; r < P; ++r)
        GS_CHECK(sh.O(r + 1) - sh.O(r) <= stride, GS_EINDEX,
                 "part %d holds %lld owner pairs, more than the stride %lld", r,
                 (long long)(sh.O(r + 1) - sh.O(r)), (long long)stride);
    auto *dcut = (int64_t *)c->buf("jac_cutdev").ensure(sizeof(int64_t) * sh.cuts.size());
    GS_HIP(hipMemcpyAsync(dcut, sh.cuts.data(), sizeof(int64_t) * sh.cuts.size(),
                          hipMemcpyHostToDevice, c->stream));
    hipEvent_t t0 = prof_begin(c);
    const int64_t nown = sh.O(P);
    if (nnz < (int64_t)INT32_MAX) {
        // per owner pair: position, reverse position, d_u + d_v, the count (4 B each) in;
        // both entries (8 B each) out
        k_jac_scatter_owners<<<grid_for(nown, 256, 65536), 256, 0, c->stream>>>(
            own.opos, own.orev, own.osum, dcut, P, cc, stride, nown, out);
        GS_HIP(hipGetLastError());
        prof_end(c, t0, "jaccard_scatter", 32.0 * (double)nown);
    } else {
        k_jac_from_counts<<<grid_for(nnz, 256, 65536), 256, 0, c->stream>>>(
            g.indptr.as<int64_t>(), g.indices.as<int32_t>(), g.rows.as<int32_t>(), g.tpos.as<int64_t>(),
            own.opre, dcut, P, cc, stride, nnz, out);
        GS_HIP(hipGetLastError());
        prof_end(c, t0, "jaccard_scatter", 48.0 * (double)nnz + 8.0 * (double)nown);
    }
    // the host copy of cuts must outlive the async H2D copy: it lives in the kept shares
}

static void check_sharded_jaccard(gs_ctx *c, int nparts) {
    GS_CHECK(c, GS_EINVAL, "null context");
    GS_CHECK(nparts >= 1 && nparts <= 4096, GS_EINVAL, "bad part count %d", nparts);
    GS_CHECK(c->g.has_transpose, GS_ESTATE, "no graph set");
    GS_CHECK(c->g.symmetric, GS_EUNSUPPORTED,
             "owner-pair shares need a symmetric graph (use edge ranges on a directed one)");
}

}  // namespace gs

using namespace gs;

extern "C" {

int gs_jaccard_shares(gs_ctx *c, int nparts, int64_t *row_cut, int64_t *owner_off) {
    return guard([&] {
        check_sharded_jaccard(c, nparts);
        GS_HIP(hipSetDevice(c->device));
        const JacShares &sh = jaccard_shares(c, nparts);
        for (int r = 0; r <= nparts; ++r) {
            if (row_cut) row_cut[r] = sh.R(r);
            if (owner_off) owner_off[r] = sh.O(r);
        }
    });
}

int gs_jaccard_part_counts(gs_ctx *c, int part, int nparts, uint32_t *counts, int loc) {
    return guard([&] {
        check_sharded_jaccard(c, nparts);
        GS_CHECK(0 <= part && part < nparts, GS_EINVAL, "bad part %d of %d", part, nparts);
        GS_HIP(hipSetDevice(c->device));
        const JacShares &sh = jaccard_shares(c, nparts);
        const int64_t cnt = sh.O(part + 1) - sh.O(part);
        auto *d = (uint32_t *)out_device(c, c->outbuf, counts, sizeof(uint32_t) * cnt, loc);
        if (cnt) jaccard_symmetric(c, jac_knobs(), nullptr, part, nparts, 0, d);
        finish_out(c, counts, d, sizeof(uint32_t) * cnt, loc);
    });
}

int gs_jaccard_from_counts(gs_ctx *c, int nparts, const uint32_t *counts, int64_t stride,
                           int c_loc, double *out, int loc) {
    return guard([&] {
        check_sharded_jaccard(c, nparts);
        GS_CHECK(stride >= 0, GS_EINVAL, "negative stride");
        GS_HIP(hipSetDevice(c->device));
        const int64_t nnz = c->g.nnz;
        const uint32_t *dc = (const uint32_t *)to_device(c, c->inbuf, counts,
                                                         sizeof(uint32_t) * stride * nparts, c_loc);
        double *dout = (double *)out_device(c, c->outbuf, out, sizeof(double) * nnz, loc);
        jaccard_from_counts(c, nparts, dc, stride, dout);
        finish_out(c, out, dout, sizeof(double) * nnz, loc);
    });
}

}  // extern "C"
