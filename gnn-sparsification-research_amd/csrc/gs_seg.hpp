// gs_seg.hpp -- the segments of an edge_index by source node and their length classes, as
// the segmented top-k (gs_segtopk.hip) and the segment ranks (gs_segrank.hip) use them:
// the header the kernels share, the class and list of a segment by its length, and
// seg_build (gs_seg.hip), which builds the segments and the node lists.
#pragma once

#include "gs_internal.hpp"
#include "gs_util.hpp"

namespace gs {

static constexpr int kSegkShortMax = 64;     // one key per lane of a wave
static constexpr int kSegkLdsSmall = 2048;   // a small LDS image: several workgroups per CU
static constexpr int kSegkLdsMax = 16384;    // 128 KiB of keys: one workgroup per CU
// node lists by segment length (segments of <= 8 columns are read off the node range)
enum { SL_16 = 0, SL_64, SL_LDS1, SL_LDS2, SL_STREAM, SL_COUNT };

struct SegkHdr {
    int bad, unsorted;
    unsigned long long cls[GS_SEGK_CLASSES];
    unsigned long long nlist[SL_COUNT];  // nodes per list
    unsigned long long base[SL_COUNT];   // its start in the shared list array
    unsigned long long fill[SL_COUNT];   // fill cursors
    unsigned long long nguar, namb;
    unsigned long long maxdeg;           // the longest segment
    unsigned long long scols;            // columns of the STREAM list's segments
};

__device__ __forceinline__ int segk_class(int64_t d, int64_t k, int smax, int lmax) {
    if (d <= 0) return GS_SEGK_EMPTY;
    if (d <= k) return GS_SEGK_ALL;
    if (d <= smax) return GS_SEGK_SHORT;
    if (d <= lmax) return GS_SEGK_LDS;
    return GS_SEGK_STREAM;
}

// which kernel reads the segment: -1 none (empty, or the 8-lane pass over all nodes)
__device__ __forceinline__ int segk_list(int64_t d, int smax, int lmax) {
    if (d <= 0) return -1;
    if (d <= smax) return d <= 8 ? -1 : d <= 16 ? SL_16 : SL_64;
    if (d <= lmax) return d <= kSegkLdsSmall ? SL_LDS1 : SL_LDS2;
    return SL_STREAM;
}

// the context's segment buffers: the header, the offsets [n + 1], the column ids grouped
// by source [E] (written for an unsorted src only) and the node lists [n]
struct SegBufs {
    SegkHdr *hdr;
    int64_t *cnt, *off, *cols, *list;
};

// the segments of dsrc[0, E) and the node lists for the limits (k, smax, lmax), on the
// context's stream; the two callers lower smax and lmax by their GSPARSE_SEG*_* knobs
// (knob_limit: tests reach every class on small graphs)
SegBufs seg_build(gs_ctx *c, const int64_t *dsrc, int64_t E, int64_t n, int64_t k, int smax, int lmax);

}  // namespace gs
