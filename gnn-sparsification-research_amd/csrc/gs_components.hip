// gs_components.hip -- connected components of the resident graph on the device:
// min-label propagation with pointer jumping (label = smallest node id of the
// component), and the component count and largest size read off the labels.
#include "gs_dense.hpp"

namespace gs {

__global__ void k_cc_init(int64_t n, int32_t *__restrict__ lab) {
    for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < n;
         u += (int64_t)gridDim.x * blockDim.x)
        lab[u] = (int32_t)u;
}

__global__ void k_cc_hook(const int32_t *__restrict__ rows, const int32_t *__restrict__ ix,
                          int64_t nnz, int32_t *__restrict__ lab, int *__restrict__ changed) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t a = lab[rows[e]], b = lab[ix[e]];
        if (a < b) {
            atomicMin(&lab[b], a);
            *changed = 1;
        } else if (b < a) {
            atomicMin(&lab[a], b);
            *changed = 1;
        }
    }
}

__global__ void k_cc_jump(int64_t n, int32_t *__restrict__ lab) {
    for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < n;
         u += (int64_t)gridDim.x * blockDim.x) {
        int32_t l = lab[u];
        while (lab[l] != l) l = lab[l];
        lab[u] = l;
    }
}

__global__ void k_comp_sizes(const int32_t *__restrict__ lab, int64_t n,
                             unsigned long long *__restrict__ size) {
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < n;
         v += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(&size[lab[v]], 1ull);
}

__global__ void k_comp_stats(const int32_t *__restrict__ lab,
                             const unsigned long long *__restrict__ size, int64_t n,
                             unsigned long long *__restrict__ stats) {
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < n;
         v += (int64_t)gridDim.x * blockDim.x)
        if (lab[v] == v) {
            atomicAdd(&stats[0], 1ull);
            atomicMax(&stats[1], size[v]);
        }
}

int32_t *components(gs_ctx *c) {
    Graph &g = c->g;
    hipStream_t st = c->stream;
    const int64_t n = g.n, nnz = g.nnz;
    auto *flags = (int *)c->buf("cc_flags").ensure(64);
    auto *lab = (int32_t *)c->buf("xer_lab").ensure(4 * (n ? n : 1));
    if (!n) return lab;
    k_cc_init<<<grid_for(n, 256, 8192), 256, 0, st>>>(n, lab);
    for (int round = 0; round < 4096; ++round) {
        GS_HIP(hipMemsetAsync(flags, 0, 4, st));
        if (nnz)
            k_cc_hook<<<grid_for(nnz, 256, 8192), 256, 0, st>>>(g.rows.as<int32_t>(),
                                                                g.indices.as<int32_t>(), nnz, lab,
                                                                flags);
        k_cc_jump<<<grid_for(n, 256, 8192), 256, 0, st>>>(n, lab);
        int ch = 0;
        GS_HIP(hipMemcpyAsync(&ch, flags, 4, hipMemcpyDeviceToHost, st));
        GS_HIP(hipStreamSynchronize(st));
        if (!ch) break;
    }
    return lab;
}

void component_stats(gs_ctx *c, const int32_t *lab, int64_t *count, int64_t *largest) {
    hipStream_t st = c->stream;
    const int64_t n = c->g.n;
    auto *size = (unsigned long long *)c->buf("topo_size").ensure(8 * (n ? n : 1));
    auto *stats = (unsigned long long *)c->buf("topo_stats").ensure(16);
    GS_HIP(hipMemsetAsync(stats, 0, 16, st));
    if (n) {
        GS_HIP(hipMemsetAsync(size, 0, 8 * n, st));
        k_comp_sizes<<<grid_for(n, 256, 8192), 256, 0, st>>>(lab, n, size);
        k_comp_stats<<<grid_for(n, 256, 8192), 256, 0, st>>>(lab, size, n, stats);
    }
    unsigned long long h[2] = {0, 0};
    GS_HIP(hipMemcpyAsync(h, stats, 16, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    if (count) *count = (int64_t)h[0];
    if (largest) *largest = (int64_t)h[1];
}

}  // namespace gs
