// gs_tri.hpp -- what the trussness (gs_truss.hip) and the Simmelian backbone
// (gs_simmelian.hip) share: the triangle counts both start from, and the step both walk the
// triangles of a pair {u, v} with -- the lanes stride the shorter of the two sorted
// neighbour lists and binary-search the longer.
#pragma once

#include "gs_jac.hpp"
#include "gs_util.hpp"

namespace gs {

// The triangle counts of the simple undirected graph of the pattern: the owner-side
// intersection kernels in count mode (gs_common_neighbors) into device out[nnz] ...
inline void support_pass(gs_ctx *c, double *out) { jaccard_symmetric(c, jac_knobs(), out, 0, 1, 1); }
// ... less the stored diagonal entries of the two ends of an off-diagonal entry (r, c),
// which that count includes: u (v) itself is a "common neighbour" of (u, v) when (u, u)
// ((v, v)) is stored
__host__ __device__ __forceinline__ int support_less_diag(double cnt, uint8_t diag_r, uint8_t diag_c) {
    return (int)cnt - (int)diag_r - (int)diag_c;
}

// the rows of u and v, the shorter one first (u's when they are equally long): where they
// start in the column indices and how long they are
struct TriRows {
    int64_t pa, pb;
    int32_t da, db;
    __device__ __forceinline__ TriRows(const int64_t *__restrict__ ip, int32_t u, int32_t v) {
        const int64_t pu = ip[u], pv = ip[v];
        const int32_t du = (int32_t)(ip[u + 1] - pu), dv = (int32_t)(ip[v + 1] - pv);
        const bool ufirst = du <= dv;
        pa = ufirst ? pu : pv;
        pb = ufirst ? pv : pu;
        da = ufirst ? du : dv;
        db = ufirst ? dv : du;
    }
};

// entry i < da of the shorter row: its position in the longer row when it is a common
// neighbour other than u and v, else -1
__device__ __forceinline__ int32_t common_pos(const int32_t *__restrict__ ix, const TriRows &l, int32_t u,
                                              int32_t v, int32_t i) {
    const int32_t w = ix[l.pa + i];
    if (w == u || w == v) return -1;
    const int32_t *__restrict__ lb = ix + l.pb;
    const int32_t lo = lower_bound(lb, l.db, w);
    return lo < l.db && lb[lo] == w ? lo : -1;
}

}  // namespace gs
