// gs_segtopk.hip -- segmented top-k (sparsify_degree_aware phase 1, core.py:415-428,
// any min_edges_per_node): for every node the set of its min(k, d) highest-scoring
// edge_index columns, d = columns with src == node.  Exact, on the order_key keys.
//
// Per node with d > k: t = its k-th largest key, gt = keys above t, eq = keys equal
// to t.  gt + eq == k: the set {key >= t} is unique and its mask bytes are set.
// Otherwise (or with a NaN in the segment) np.argsort's order decides inside the tie
// block: status 2, no byte set, the caller makes the reference's own call.
//
// Segments and node lists: seg_build (gs_seg.hpp).  Selection by length:
//   d <= k                 every column (handled by the kernel of its length)
//   d <= 64      SHORT     sub-wave groups of 8 / 16 / 64 lanes, one key per lane; the
//                          rank is a count of greater / equal keys over the group
//   d <= LDS max LDS       one workgroup per segment, keys staged once in LDS, MSB-first
//                          radix select with an 8-bit LDS histogram per digit
//   beyond       STREAM    the same select re-reading the keys from HBM per digit
// Nothing waits for the host before the one copy that returns the counts.
#include "gs_keys.hpp"
#include "gs_seg.hpp"
#include "gs_wave.hpp"

namespace gs {

// SHORT: W lanes per segment, one key per lane.  LISTED: the segments of list L (their
// lengths in (W / 2 or 8, W]); else every node of <= min(8, smax) columns.
template <int W, bool LISTED>
__global__ void __launch_bounds__(256) k_segk_short(const double *__restrict__ s, const int64_t *__restrict__ off,
                                                    const int64_t *__restrict__ cols,
                                                    const SegkHdr *__restrict__ hdr,
                                                    const int64_t *__restrict__ list, int L, int64_t n, int64_t k,
                                                    int smax, uint8_t *__restrict__ mask,
                                                    uint8_t *__restrict__ status) {
    if (hdr->bad) return;
    const int64_t *cl = hdr->unsorted ? cols : nullptr;
    const int64_t total = LISTED ? (int64_t)hdr->nlist[L] : n;
    const int64_t lbase = LISTED ? (int64_t)hdr->base[L] : 0;
    constexpr int GPW = 64 / W;  // segments per wave and trip
    const int lane = threadIdx.x & 63, g = lane / W, sl = lane % W;
    const int64_t wv = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int kq = k > W ? W + 1 : (int)k;
    // g0 is the same in every lane of the wave: whole waves run every trip
    for (int64_t g0 = wv * GPW; g0 < total; g0 += nw * GPW) {
        const int64_t idx = g0 + g;
        int64_t u = 0, lo = 0;
        int d = 0;
        if (idx < total) {
            u = LISTED ? list[lbase + idx] : idx;
            lo = off[u];
            const int64_t dd = off[u + 1] - lo;
            d = (LISTED || (dd <= 8 && dd <= smax)) ? (int)dd : 0;
        }
        const bool have = sl < d;
        const int64_t col = have ? (cl ? cl[lo + sl] : lo + sl) : 0;
        const uint64_t key = have ? order_key(s[col]) : 0ull;
        int gt = 0, eq = 0;
#pragma unroll 8
        for (int r = 0; r < W; ++r) {
            const uint64_t o = __shfl((unsigned long long)key, r, W);
            const bool v = r < d;
            gt += v && o > key;
            eq += v && o == key;
        }
        bool keep = have, ambl = false;
        if (d > kq) {
            keep = have && gt < kq;
            ambl = have && ((gt < kq && gt + eq > kq) || key == ~0ull);
        }
        const unsigned long long b = __ballot(ambl);
        const bool amb = W == 64 ? b != 0 : ((b >> (g * W)) & ((1ull << (W & 63)) - 1ull)) != 0;
        if (keep && !amb) mask[col] = 1;
        if (sl == 0 && d > 0) status[u] = amb ? 2 : 1;
    }
}

// LDS / STREAM: one workgroup of NT threads per segment of list L.  STAGED: the keys
// are read once into LDS (d <= CAP by the list's definition); else every digit pass
// re-reads them through the column ids.
template <bool STAGED, int CAP, int NT>
__global__ void __launch_bounds__(NT) k_segk_block(const double *__restrict__ s, const int64_t *__restrict__ off,
                                                   const int64_t *__restrict__ cols,
                                                   const SegkHdr *__restrict__ hdr,
                                                   const int64_t *__restrict__ list, int L, int64_t k,
                                                   uint8_t *__restrict__ mask, uint8_t *__restrict__ status) {
    if (hdr->bad) return;
    __shared__ uint64_t keys[STAGED ? CAP : 1];
    __shared__ unsigned long long h[256];
    __shared__ unsigned long long wsum[4];
    __shared__ unsigned long long sel_excl, sel_cnt;
    __shared__ int sel_digit, snan;
    const int64_t *cl = hdr->unsorted ? cols : nullptr;
    const int64_t total = (int64_t)hdr->nlist[L];
    const int64_t lbase = (int64_t)hdr->base[L];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const int64_t u = list[lbase + it];
        const int64_t lo = off[u];
        const int64_t d = off[u + 1] - lo;
        if (d <= k) {  // every column
            for (int64_t i = tid; i < d; i += NT) mask[cl ? cl[lo + i] : lo + i] = 1;
            if (tid == 0) status[u] = 1;
            continue;
        }
        if (tid == 0) snan = 0;
        __syncthreads();
        if (STAGED) {
            for (int64_t i = tid; i < d; i += NT) {
                const uint64_t key = order_key(s[cl ? cl[lo + i] : lo + i]);
                keys[i] = key;
                if (key == ~0ull) snan = 1;
            }
        }
        uint64_t prefix = 0;
        unsigned long long rank = (unsigned long long)(d - k);  // ascending position of the k-th largest
        unsigned long long lt = 0, eq = 0;                      // keys below / equal to the cut
        for (int shift = 56; shift >= 0; shift -= 8) {
            if (tid < 256) h[tid] = 0;
            __syncthreads();  // also: the staged keys are written
            for (int64_t i0 = 0; i0 < d; i0 += NT) {  // whole waves run every trip
                const int64_t i = i0 + tid;
                const bool valid = i < d;
                uint64_t key = 0;
                if (valid) key = STAGED ? keys[i] : order_key(s[cl ? cl[lo + i] : lo + i]);
                if (!STAGED && shift == 56 && valid && key == ~0ull) snan = 1;
                const bool m = valid && (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8)));
                const unsigned dg = (unsigned)(key >> shift) & 0xffu;
                // scores of one node share their high digits: one LDS atomic per wave then
                const unsigned long long bm = __ballot(m);
                if (bm) {
                    const int leader = __builtin_ctzll(bm);
                    const unsigned d0 = __shfl(dg, leader, 64);
                    if (__all(!m || dg == d0)) {
                        if (lane == leader) atomicAdd(&h[d0], (unsigned long long)__popcll(bm));
                    } else if (m) {
                        atomicAdd(&h[dg], 1ull);
                    }
                }
            }
            __syncthreads();
            // the digit holding `rank`: an exclusive scan of the 256 bins over waves 0..3
            const unsigned long long cnt = tid < 256 ? h[tid] : 0ull;
            unsigned long long v = cnt;
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long t = __shfl_up(v, o, 64);
                if (lane >= o) v += t;
            }
            if (lane == 63 && w < 4) wsum[w] = v;
            __syncthreads();
            if (tid < 256) {
                unsigned long long base = 0;
                for (int j = 0; j < w; ++j) base += wsum[j];
                const unsigned long long excl = base + v - cnt;
                if (cnt && excl <= rank && rank < excl + cnt) {
                    sel_digit = tid;
                    sel_excl = excl;
                    sel_cnt = cnt;
                }
            }
            __syncthreads();
            prefix |= (uint64_t)sel_digit << shift;
            rank -= sel_excl;
            lt += sel_excl;
            eq = sel_cnt;
        }
        const unsigned long long gt = (unsigned long long)d - lt - eq;
        const bool amb = snan || gt + eq != (unsigned long long)k;
        if (!amb) {
            for (int64_t i = tid; i < d; i += NT) {
                const int64_t col = cl ? cl[lo + i] : lo + i;
                const uint64_t key = STAGED ? keys[i] : order_key(s[col]);
                if (key >= prefix) mask[col] = 1;
            }
        }
        if (tid == 0) status[u] = amb ? 2 : 1;
        __syncthreads();  // keys / snan are reused by the next segment
    }
}

// guaranteed columns (= mask bytes set) and ambiguous nodes
__global__ void __launch_bounds__(256) k_segk_tally(int64_t n, int64_t k, const int64_t *__restrict__ off,
                                                    const uint8_t *__restrict__ status,
                                                    SegkHdr *__restrict__ hdr) {
    if (hdr->bad) return;
    unsigned long long g = 0, a = 0;
    for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < n;
         u += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t st = status[u];
        const int64_t d = off[u + 1] - off[u];
        if (st == 1) g += (unsigned long long)(d < k ? d : k);
        a += st == 2;
    }
    g = wave_sum(g);
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) {
        if (g) atomicAdd(&hdr->nguar, g);
        if (a) atomicAdd(&hdr->namb, a);
    }
}

}  // namespace gs

using namespace gs;

extern "C" int gs_segment_topk(gs_ctx *c, const double *scores, int s_loc, int64_t nscores,
                               const int64_t *src, int src_loc, int64_t E, int64_t n, int64_t k,
                               uint8_t *mask, int mask_loc, uint8_t *status, int status_loc,
                               int64_t *n_guaranteed, int64_t *n_ambiguous, int64_t *class_counts,
                               int ncounts) {
    return guard([&] {
        GS_CHECK(c, GS_EINVAL, "null context");
        GS_CHECK(n >= 0 && E >= 0, GS_EINVAL, "negative n/E");
        GS_CHECK(k >= 1, GS_EINVAL, "k must be >= 1 (k=%lld)", (long long)k);
        GS_CHECK(E <= nscores, GS_EINVAL,
                 "index %lld is out of bounds for axis 0 with size %lld (scores are per CSR "
                 "entry, columns per edge_index)", (long long)(E ? E - 1 : 0), (long long)nscores);
        GS_CHECK(ncounts >= 0 && (ncounts == 0 || class_counts), GS_EINVAL, "class_counts is null");
        GS_HIP(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        const int smax = knob_limit(getenv("GSPARSE_SEGK_SHORT_MAX"), kSegkShortMax);
        const int lmax = knob_limit(getenv("GSPARSE_SEGK_LDS_MAX"), kSegkLdsMax);
        const int64_t E1 = E ? E : 1, n1 = n ? n : 1;
        const double *ds = (const double *)to_device(c, c->buf("segk_s"), scores, sizeof(double) * E, s_loc);
        const int64_t *dsrc = (const int64_t *)to_device(c, c->buf("segk_src"), src, sizeof(int64_t) * E,
                                                         src_loc);
        uint8_t *dm = (uint8_t *)out_device(c, c->buf("segk_mask"), mask, E1, mask_loc);
        uint8_t *dst = (uint8_t *)out_device(c, c->buf("segk_status"), status, n1, status_loc);
        hipEvent_t t0 = prof_begin(c);
        if (E) GS_HIP(hipMemsetAsync(dm, 0, E, st));
        if (n) GS_HIP(hipMemsetAsync(dst, 0, n, st));
        const SegBufs sb = seg_build(c, dsrc, E, n, k, smax, lmax);
        SegkHdr *hdr = sb.hdr;
        const int64_t *off = sb.off, *cols = sb.cols, *list = sb.list;
        const unsigned gn = grid_for(n, 256, 8192);
        // the list lengths stay on the device: fixed grids, workgroups without work leave
        k_segk_short<8, false><<<grid_for(n, 32, 8192), 256, 0, st>>>(ds, off, cols, hdr, list, 0, n, k, smax,
                                                                      dm, dst);
        k_segk_short<16, true><<<grid_for(n, 16, 2048), 256, 0, st>>>(ds, off, cols, hdr, list, SL_16, n, k,
                                                                      smax, dm, dst);
        k_segk_short<64, true><<<grid_for(n, 4, 2048), 256, 0, st>>>(ds, off, cols, hdr, list, SL_64, n, k,
                                                                     smax, dm, dst);
        k_segk_block<true, kSegkLdsSmall, 256><<<grid_for(n, 1, 2048), 256, 0, st>>>(ds, off, cols, hdr, list,
                                                                                     SL_LDS1, k, dm, dst);
        k_segk_block<true, kSegkLdsMax, 1024><<<grid_for(n, 1, 256), 1024, 0, st>>>(ds, off, cols, hdr, list,
                                                                                    SL_LDS2, k, dm, dst);
        k_segk_block<false, 1, 1024><<<grid_for(n, 1, 256), 1024, 0, st>>>(ds, off, cols, hdr, list,
                                                                           SL_STREAM, k, dm, dst);
        k_segk_tally<<<gn, 256, 0, st>>>(n, k, off, dst, hdr);
        GS_HIP(hipGetLastError());
        SegkHdr hh;
        GS_HIP(hipMemcpyAsync(&hh, hdr, sizeof(SegkHdr), hipMemcpyDeviceToHost, st));
        GS_HIP(hipStreamSynchronize(st));
        // src and the scores once, the mask (cleared, then its set bytes), the counts and
        // offsets (scan, two classify passes, selection, tally), the status bytes; an
        // unsorted src is read again and its column ids written and read; the STREAM
        // class's extra reads of its hubs are not counted
        double bytes = 8.0 * 2 * (double)E + 2.0 * (double)E + 8.0 * 6 * (double)n + 2.0 * (double)n;
        if (hh.unsorted) bytes += 8.0 * 3 * (double)E;
        prof_end(c, t0, "segment_topk", bytes);
        GS_CHECK(!hh.bad, GS_EINVAL, "edge_index source out of range [0, %lld)", (long long)n);
        finish_out(c, mask, dm, E, mask_loc);
        finish_out(c, status, dst, n, status_loc);
        if (n_guaranteed) *n_guaranteed = (int64_t)hh.nguar;
        if (n_ambiguous) *n_ambiguous = (int64_t)hh.namb;
        for (int i = 0; i < ncounts; ++i)
            class_counts[i] = i < GS_SEGK_CLASSES ? (int64_t)hh.cls[i] : 0;
    });
}
