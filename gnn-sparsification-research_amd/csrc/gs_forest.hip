// gs_forest.hip -- the maximum spanning forest of an edge list under per-column scores,
// on the device (gs_spanning_forest): the columns Kruskal's walk, best first, adds.
//
// One stable rocPRIM radix sort of (order_key(score), column) gives every column its
// rank in the strict total order (key, index) -- 0 is the best -- and the ends of the
// columns are gathered once into rank order (int32).  Boruvka rounds then run over a
// work list of ranks:
//   k_forest_best   every listed column whose ends carry different labels takes an
//                   integer atomicMin of its rank on both components' roots, and is
//                   written to the next round's list; columns that have become internal
//                   (and self-loops, in the first round) are dropped there
//   k_forest_hook   every root with a pick marks the column and records the root on the
//                   far side; of two roots that picked the same column the smaller hooks
//   k_forest_apply  the hooks become labels, the picks are reset
//   k_forest_jump   labels are flattened by pointer jumping: a bounded walk per node,
//                   repeated (with one more host wait) only while a walk hit its bound
// and the host waits once per round, for the hook count, the next list's length and the
// "not flat" flag.  No float atomics: ranks are distinct integers, so the forest, the
// labels and the counts are the same bytes on every run.
// With expand, gs_undirected_ids names every column's unordered pair first, the rounds
// mark pairs instead of columns, and one last pass writes mask[i] = marked[pair[i]].
// The per-element rules are gs_forest.hpp's.
#include "gs_forest.hpp"
#include "gs_sort.hpp"
#include "gs_wave.hpp"

namespace gs {

// what the host reads back once per round: written with vector stores and atomics only
struct ForestState {
    int bad;                     // an id outside [0, n)
    int notflat;                 // a pointer-jumping walk stopped at its bound
    unsigned long long hooked;   // roots hooked this round = columns added
    unsigned long long wcount;   // columns on the next round's list
    unsigned long long marked;   // mask bytes set by the expansion
};

static constexpr int kForestItems = 8;    // columns per thread and list pass
static constexpr int kForestWalk = 64;    // parent steps per node and jump pass

template <class P>
__global__ void k_forest_keys(const double *__restrict__ s, const int64_t *__restrict__ src,
                              const int64_t *__restrict__ dst, int64_t E, int64_t n,
                              uint64_t *__restrict__ keys, P *__restrict__ pos, ForestState *__restrict__ st) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (!forest_in_range(src[i], dst[i], n)) atomicOr(&st->bad, 1);
        keys[i] = order_key(s[i]);
        pos[i] = (P)i;
    }
}

// the ends of the column of rank r (only run once every id is known to be in range)
template <class P>
__global__ void k_forest_ends(const int64_t *__restrict__ src, const int64_t *__restrict__ dst,
                              const P *__restrict__ pos, int64_t E, int keep_lowest,
                              int32_t *__restrict__ eu, int32_t *__restrict__ ev) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < E;
         r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t col = (int64_t)pos[forest_flip(r, E, keep_lowest)];
        eu[r] = (int32_t)src[col];
        ev[r] = (int32_t)dst[col];
    }
}

template <class P>
__global__ void k_forest_init(int64_t n, int32_t *__restrict__ lab, P *__restrict__ best) {
    for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < n;
         u += (int64_t)gridDim.x * blockDim.x) {
        lab[u] = (int32_t)u;
        best[u] = (P)~(P)0;
    }
}

// best[a] only ever falls, so a plain (possibly stale) read of it is an upper bound:
// a column that is not below it cannot win and sends no atomic.  The list is in rank
// order, best first, so at a star's hub all but the first few columns stop here.
template <class P>
__device__ __forceinline__ void forest_offer(P *best, P r) {
    if (r < *best) atomicMin(best, r);
}

// one workgroup: kForestItems x 256 consecutive list entries (win == nullptr: the ranks
// themselves, the first round).  The survivors keep their order inside the workgroup
// and take one global atomic per workgroup for their place in the next list.
template <class P>
__global__ void __launch_bounds__(256)
k_forest_best(const P *__restrict__ win, int64_t W, const int32_t *__restrict__ eu,
              const int32_t *__restrict__ ev, const int32_t *__restrict__ lab, P *__restrict__ best,
              P *__restrict__ wout, ForestState *__restrict__ st) {
    __shared__ unsigned int cnt[kForestItems * 4];
    __shared__ unsigned long long base;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t b0 = (int64_t)blockIdx.x * (256 * kForestItems);
    P r[kForestItems];
    unsigned int before[kForestItems];
    bool keep[kForestItems];
#pragma unroll
    for (int k = 0; k < kForestItems; ++k) {
        const int64_t i = b0 + k * 256 + t;
        keep[k] = false;
        r[k] = 0;
        if (i < W) {
            r[k] = win ? win[i] : (P)i;
            const int32_t a = lab[eu[r[k]]], b = lab[ev[r[k]]];
            if (forest_crossing(a, b)) {
                keep[k] = true;
                forest_offer(best + a, r[k]);
                forest_offer(best + b, r[k]);
            }
        }
        const unsigned long long m = __ballot(keep[k]);
        before[k] = lanes_below(m);
        if (lane == 0) cnt[k * 4 + wave] = (unsigned int)__popcll(m);
    }
    __syncthreads();
    if (t == 0) {
        unsigned int total = 0;
        for (int j = 0; j < kForestItems * 4; ++j) {
            const unsigned int c = cnt[j];
            cnt[j] = total;
            total += c;
        }
        base = total ? atomicAdd(&st->wcount, (unsigned long long)total) : 0ull;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kForestItems; ++k)
        if (keep[k]) wout[base + cnt[k * 4 + wave] + before[k]] = r[k];
}

// mark: the mask itself (pair == nullptr) or the marks of the unordered pairs
template <class P>
__global__ void k_forest_hook(int64_t n, const int32_t *__restrict__ lab, const P *__restrict__ best,
                              const int32_t *__restrict__ eu, const int32_t *__restrict__ ev,
                              const P *__restrict__ pos, int64_t E, int keep_lowest,
                              const int64_t *__restrict__ pair, uint8_t *__restrict__ mark,
                              int32_t *__restrict__ hook, ForestState *__restrict__ st) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t trips = (n + stride - 1) / stride;
    unsigned long long mine = 0;
    for (int64_t tr = 0, a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; tr < trips; ++tr, a += stride) {
        if (a >= n || lab[a] != (int32_t)a) continue;
        const P r = best[a];
        int32_t to = (int32_t)a;
        if (r != (P)~(P)0) {
            const int32_t other = forest_other((int32_t)a, lab[eu[r]], lab[ev[r]]);
            if (forest_hooks((int32_t)a, other, best[other] == r)) {
                to = other;
                const int64_t col = (int64_t)pos[forest_flip((int64_t)r, E, keep_lowest)];
                mark[pair ? pair[col] : col] = 1;
                ++mine;
            }
        }
        hook[a] = to;
    }
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&st->hooked, mine);
}

template <class P>
__global__ void k_forest_apply(int64_t n, int32_t *__restrict__ lab, const int32_t *__restrict__ hook,
                               P *__restrict__ best) {
    for (int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; a < n;
         a += (int64_t)gridDim.x * blockDim.x)
        if (lab[a] == (int32_t)a) {
            lab[a] = hook[a];
            best[a] = (P)~(P)0;
        }
}

// Every value a pass stores in lab[u] is an ancestor of u, and a root's own label never
// changes, so a walk that reads labels other threads are rewriting still climbs its own
// tree.  A pass in which no walk hit the bound left every label a root.
__global__ void k_forest_jump(int64_t n, int32_t *__restrict__ lab, ForestState *__restrict__ st) {
    for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < n;
         u += (int64_t)gridDim.x * blockDim.x) {
        int32_t l = lab[u], up = lab[l];
        for (int step = 0; up != l && step < kForestWalk; ++step) {
            l = up;
            up = lab[l];
        }
        if (up != l) st->notflat = 1;
        lab[u] = l;
    }
}

__global__ void k_forest_expand(const int64_t *__restrict__ pair, const uint8_t *__restrict__ mark,
                                int64_t E, uint8_t *__restrict__ mask, ForestState *__restrict__ st) {
    unsigned long long mine = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t m = mark[pair[i]];
        mask[i] = m;
        mine += m;
    }
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&st->marked, mine);
}

struct ForestOut {
    int64_t n_forest = 0, n_marked = 0;
    int32_t rounds = 0;
};

static ForestState forest_read(gs_ctx *c, const ForestState *st) {
    ForestState h;
    GS_HIP(hipMemcpyAsync(&h, st, sizeof(ForestState), hipMemcpyDeviceToHost, c->stream));
    GS_HIP(hipStreamSynchronize(c->stream));
    return h;
}

// dm: E zeroed bytes; lab: n labels out; pair: the columns' unordered ids, or nullptr
template <class P>
static ForestOut forest_run(gs_ctx *c, const double *ds, const int64_t *dsrc, const int64_t *ddst,
                            int64_t E, int64_t n, int keep_lowest, const int64_t *pair, uint8_t *dm,
                            int32_t *lab) {
    hipStream_t s = c->stream;
    ForestOut out;
    const unsigned gE = grid_for(E, 256, 8192), gn = grid_for(n, 256, 8192);
    ForestState *st = (ForestState *)c->buf("forest_st").ensure(sizeof(ForestState));
    P *best = (P *)c->buf("forest_best").ensure(sizeof(P) * n);
    int32_t *hook = (int32_t *)c->buf("forest_hook").ensure(sizeof(int32_t) * n);
    GS_HIP(hipMemsetAsync(st, 0, sizeof(ForestState), s));
    k_forest_init<P><<<gn, 256, 0, s>>>(n, lab, best);
    if (E == 0) {
        GS_HIP(hipGetLastError());
        return out;
    }
    uint64_t *key0 = (uint64_t *)c->buf("forest_key0").ensure(sizeof(uint64_t) * E);
    uint64_t *key1 = (uint64_t *)c->buf("forest_key1").ensure(sizeof(uint64_t) * E);
    P *pos0 = (P *)c->buf("forest_pos0").ensure(sizeof(P) * E);
    P *pos1 = (P *)c->buf("forest_pos1").ensure(sizeof(P) * E);
    int32_t *eu = (int32_t *)c->buf("forest_eu").ensure(sizeof(int32_t) * E);
    int32_t *ev = (int32_t *)c->buf("forest_ev").ensure(sizeof(int32_t) * E);
    uint8_t *mark = dm;
    if (pair) {
        mark = (uint8_t *)c->buf("forest_mark").ensure((size_t)E);
        GS_HIP(hipMemsetAsync(mark, 0, (size_t)E, s));
    }

    hipEvent_t t0 = prof_begin(c);
    k_forest_keys<P><<<gE, 256, 0, s>>>(ds, dsrc, ddst, E, n, key0, pos0, st);
    GS_HIP(hipGetLastError());
    const ForestState h0 = forest_read(c, st);
    GS_CHECK(!h0.bad, GS_EINVAL, "edge_index id out of range [0, %lld)", (long long)n);
    const P *pos = radix_sort_pairs(c, c->buf("forest_tmp"), key0, key1, pos0, pos1, E, 0, 64, s).vals;
    k_forest_ends<P><<<gE, 256, 0, s>>>(dsrc, ddst, pos, E, keep_lowest, eu, ev);
    GS_HIP(hipGetLastError());
    // keys and ids read and written; eight 8-bit digit passes over the pairs and one
    // histogram read of the keys; the gather of the ends
    prof_end(c, t0, "forest_rank", (24.0 + 8.0 + sizeof(P)) * E + 8 * 2.0 * (8.0 + sizeof(P)) * E +
                                       8.0 * E + (sizeof(P) + 16.0 + 8.0) * E);

    // the sorted keys are dead: their buffers hold the two work lists
    P *wl[2] = {(P *)key0, (P *)key1};
    const P *win = nullptr;
    int64_t W = E;
    const bool debug = getenv("GSPARSE_FOREST_DEBUG") != nullptr;
    for (int round = 0; round < 64 && W > 0; ++round) {
        t0 = prof_begin(c);
        GS_HIP(hipMemsetAsync(st, 0, sizeof(ForestState), s));
        P *wout = wl[round & 1];
        const int64_t per = 256 * kForestItems;
        k_forest_best<P><<<(unsigned)((W + per - 1) / per), 256, 0, s>>>(win, W, eu, ev, lab, best, wout, st);
        k_forest_hook<P><<<gn, 256, 0, s>>>(n, lab, best, eu, ev, pos, E, keep_lowest, pair, mark, hook, st);
        k_forest_apply<P><<<gn, 256, 0, s>>>(n, lab, hook, best);
        k_forest_jump<<<gn, 256, 0, s>>>(n, lab, st);
        GS_HIP(hipGetLastError());
        // the list, its ends and their labels, the survivors; per node the label, the
        // pick, the hook and the jump
        prof_end(c, t0, "forest_round", (sizeof(P) + 8.0 + 8.0) * W + (12.0 + 2.0 * sizeof(P) + 8.0 + 12.0) * n);
        ForestState h = forest_read(c, st);
        const int64_t hooked = (int64_t)h.hooked, Wnext = (int64_t)h.wcount;
        int passes = 1;
        while (h.notflat) {
            GS_CHECK(passes < 64, GS_ESTATE, "spanning forest: labels not flat after %d passes", passes);
            GS_HIP(hipMemsetAsync(&st->notflat, 0, sizeof(int), s));
            k_forest_jump<<<gn, 256, 0, s>>>(n, lab, st);
            GS_HIP(hipGetLastError());
            h = forest_read(c, st);
            ++passes;
        }
        if (debug)
            fprintf(stderr, "[forest] round=%d list=%lld crossing=%lld hooked=%lld jump_passes=%d\n", round,
                    (long long)W, (long long)Wnext, (long long)hooked, passes);
        if (!hooked) break;
        out.n_forest += hooked;
        ++out.rounds;
        if (out.n_forest >= n - 1) break;  // one component: nothing crosses any more
        win = wout;
        W = Wnext;
    }
    out.n_marked = out.n_forest;
    if (pair) {
        t0 = prof_begin(c);
        GS_HIP(hipMemsetAsync(st, 0, sizeof(ForestState), s));
        k_forest_expand<<<gE, 256, 0, s>>>(pair, mark, E, dm, st);
        GS_HIP(hipGetLastError());
        prof_end(c, t0, "forest_expand", (8.0 + 1.0 + 1.0) * E);
        out.n_marked = (int64_t)forest_read(c, st).marked;
    }
    return out;
}

}  // namespace gs

using namespace gs;

extern "C" int gs_spanning_forest(gs_ctx *c, const double *scores, int s_loc, int64_t nscores,
                                  const int64_t *src, const int64_t *dst, int e_loc, int64_t E, int64_t n,
                                  int keep_lowest, int expand, uint8_t *mask, int m_loc, int32_t *labels,
                                  int l_loc, int64_t *n_forest, int64_t *n_marked, int32_t *rounds) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        GS_CHECK(n >= 1 && E >= 0, GS_EINVAL, "need n >= 1 and E >= 0 (n=%lld, E=%lld)", (long long)n,
                 (long long)E);
        GS_CHECK(nscores >= E, GS_EINVAL,
                 "%lld scores for %lld columns: one score per edge_index column is needed (scores of "
                 "the canonical CSR, which merges duplicates, do not index the columns)",
                 (long long)nscores, (long long)E);
        GS_CHECK(n < (int64_t(1) << 31), GS_EUNSUPPORTED, "n = %lld: node labels are 32-bit", (long long)n);
        GS_CHECK(E == 0 || (scores && src && dst && mask), GS_EINVAL, "null scores/src/dst/mask");
        GS_HIP(hipSetDevice(c->device));
        hipStream_t s = c->stream;
        const double *ds = (const double *)to_device(c, c->buf("forest_s"), scores, sizeof(double) * E, s_loc);
        const int64_t *dsrc = (const int64_t *)to_device(c, c->buf("forest_src"), src, sizeof(int64_t) * E, e_loc);
        const int64_t *ddst = (const int64_t *)to_device(c, c->buf("forest_dst"), dst, sizeof(int64_t) * E, e_loc);
        uint8_t *dm = (uint8_t *)out_device(c, c->buf("forest_mask"), mask, E ? (size_t)E : 1, m_loc);
        int32_t *lab = (int32_t *)out_device(c, c->buf("forest_lab"), labels, sizeof(int32_t) * n,
                                             labels ? l_loc : GS_HOST);
        if (E) GS_HIP(hipMemsetAsync(dm, 0, (size_t)E, s));
        const int64_t *pair = nullptr;
        if (expand && E) {
            // np.unique's inverse of the undirected keys: equal ids <=> the same unordered pair
            int64_t *inv = (int64_t *)c->buf("forest_pair").ensure(sizeof(int64_t) * E);
            int32_t status = 1;
            const int rc = gs_undirected_ids(c, n, E, dsrc, ddst, GS_DEVICE, inv, GS_DEVICE, nullptr, &status);
            if (rc != GS_OK) throw GsError{rc};
            GS_CHECK(status == 0, GS_EINVAL, "edge_index id out of range [0, %lld)", (long long)n);
            pair = inv;
        }
        const ForestOut out = E < (int64_t(1) << 32)
                                  ? forest_run<uint32_t>(c, ds, dsrc, ddst, E, n, keep_lowest, pair, dm, lab)
                                  : forest_run<unsigned long long>(c, ds, dsrc, ddst, E, n, keep_lowest, pair, dm, lab);
        if (labels) finish_out(c, labels, lab, sizeof(int32_t) * n, l_loc);
        finish_out(c, mask, dm, (size_t)E, m_loc);
        if (n_forest) *n_forest = out.n_forest;
        if (n_marked) *n_marked = out.n_marked;
        if (rounds) *rounds = out.rounds;
    });
}
