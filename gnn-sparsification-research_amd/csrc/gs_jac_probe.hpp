// gs_jac_probe.hpp -- the device templates the probing Jaccard kernels share: a task's
// owned entries staged in LDS, the membership probes (LDS hash table, quotient table,
// sorted list, bitmap) and the probe loop over the staged entries.  Only the units that
// instantiate them include it (gs_jac_hash.hip, gs_jac_bitmap.hip).
#pragma once
#include "gs_jac.hpp"

#include <type_traits>

namespace gs {

static constexpr int kJacUnrollDef = 4;  // list elements per lane in flight
// the big-table classes run 1-2 workgroups per CU: more list loads in flight per lane
#ifndef GS_JAC_UNROLL_BIG
#define GS_JAC_UNROLL_BIG 8
#endif
#ifndef GS_JAC_UNROLL_Q8  // the two-workgroups-per-CU 32K class: 64 VGPRs
#define GS_JAC_UNROLL_Q8 4
#endif
#ifndef GS_JAC_LOADS_Q8  // ... with this many list loads per lane in flight
#define GS_JAC_LOADS_Q8 8
#endif

__device__ __forceinline__ uint32_t jac_hash(int32_t x) { return jac_mul((uint32_t)x); }

// Owned entries of a task, staged in LDS: (list base, length, entry offset).
// Entries with d_v > kJacSmall fill the front and are taken one per wave;
// short ones fill the back and are taken four per wave (16-lane groups).
struct JacStage {
    int64_t b[kJacMaxEnt];
    int32_t dv[kJacMaxEnt];
    int16_t off[kJacMaxEnt];
    int nbig, nsmall;
};

__device__ __forceinline__ void jac_stage(const int64_t *__restrict__ ip,
                                          const int32_t *__restrict__ ix, int32_t u, int64_t du,
                                          int64_t lo, int64_t hi, JacStage &st) {
    for (int64_t e = lo + threadIdx.x; e < hi; e += blockDim.x) {
        const int32_t v = ix[e];
        const int64_t b = ip[v], dv = ip[v + 1] - b;
        if (!jac_owns(du, dv, u, v)) continue;
        const int k = dv > kJacSmall ? atomicAdd(&st.nbig, 1)
                                     : kJacMaxEnt - 1 - atomicAdd(&st.nsmall, 1);
        st.b[k] = b;
        st.dv[k] = (int32_t)dv;
        st.off[k] = (int16_t)(e - lo);
    }
}

__device__ __forceinline__ void jac_task_range(const int64_t *__restrict__ ip,
                                               const int32_t *__restrict__ ntask, int32_t u,
                                               int32_t i, int64_t &a, int64_t &du, int64_t &lo,
                                               int64_t &hi) {
    a = ip[u];
    du = ip[u + 1] - a;
    const int64_t nt = ntask[u];
    lo = a + du * i / nt;
    hi = a + du * (i + 1) / nt;
}

// Membership tests in two steps, so a lane can have every first read in
// flight before it resolves any: first(x) issues the read, done(x, s)
// finishes (following full buckets of the LDS table when it must).
struct JacHashProbe {
    const int4 *tab;
    uint32_t shift, mask;
    struct S {
        int4 q;
        uint32_t h;
    };
    __device__ __forceinline__ S first(int32_t x) const {
        const uint32_t h = jac_hash(x) >> shift;
        return S{tab[h], h};
    }
    __device__ __forceinline__ bool done(int32_t x, S s) const {
        while (true) {
            if (s.q.x == x || s.q.y == x || s.q.z == x || s.q.w == x) return true;
            if (s.q.w == -1) return false;
            s.h = (s.h + 1) & mask;
            s.q = tab[s.h];
        }
    }
    // the home bucket alone, branch-free: hit, or more = the search must go on (done())
    __device__ __forceinline__ bool check1(int32_t x, S s, bool &more) const {
        const bool hit = s.q.x == x || s.q.y == x || s.q.z == x || s.q.w == x;
        more = !hit && s.q.w != -1;
        return hit;
    }
};

struct JacBitProbe {
    const uint32_t *m;
    struct S {
        uint32_t w;
    };
    __device__ __forceinline__ S first(int32_t x) const { return S{m[x >> 5]}; }
    __device__ __forceinline__ bool done(int32_t x, S s) const { return (s.w >> (x & 31)) & 1u; }
    __device__ __forceinline__ bool check1(int32_t x, S s, bool &more) const {
        more = false;
        return done(x, s);
    }
};

// the quotient tables of gs_jac.hpp
struct JacQProbe {
    const uint4 *tab;
    JacQParams p;
    uint32_t nbm;  // buckets - 1
    struct S {
        uint4 q;
        uint32_t h;
    };
    __device__ __forceinline__ S first(int32_t x) const {
        const uint32_t h = jac_mul((uint32_t)x) & p.hmask;
        return S{tab[h >> p.qb], h};
    }
    __device__ __forceinline__ bool done(int32_t, S s) const {
        const uint32_t home = s.h >> p.qb, rem = s.h & p.rmask;
        for (uint32_t d = 0;;) {
            const uint32_t t = jac_qslot(p.qb, d, rem), t2 = t | (t << 16);
            if (jac_bucket_has(s.q, t2)) return true;
            if ((s.q.w >> 16) == 0 || ++d > p.dmax) return false;
            s.q = tab[(home + d) & nbm];
        }
    }
    __device__ __forceinline__ bool check1(int32_t, S s, bool &more) const {
        const uint32_t t = jac_qslot(p.qb, 0, s.h & p.rmask), t2 = t | (t << 16);
        const bool hit = jac_bucket_has(s.q, t2);
        more = !hit && (s.q.w >> 16) != 0 && p.dmax >= 1;
        return hit;
    }
};

// the overflow path: binary search of the owner's sorted neighbour list
struct JacSortedProbe {
    const int32_t *row;
    int64_t du;
    struct S {};
    __device__ __forceinline__ S first(int32_t) const { return S{}; }
    __device__ __forceinline__ bool check1(int32_t, S, bool &more) const {
        more = true;
        return false;
    }
    __device__ __forceinline__ bool done(int32_t x, S) const {
        const int64_t lo = lower_bound(row, du, x);
        return lo < du && row[lo] == x;
    }
};

// Probe phase shared by the LDS-table and bitmap kernels (after jac_stage and
// a barrier).  The d_u of the owner and each entry's d_v give the union.
// UL list elements per lane are loaded at once (the global reads are what the
// loop waits on), then probed UP at a time (the probe state is what costs
// registers).  Measured and dropped (profiles/r04g_*, r04t_*, r04u_*): skipping
// the all-masked 64-element steps; a software-pipelined loop with the next step's
// loads in flight during this step's probes; and cutting long lists into chunks
// the waves take in turn (the slowest wave of a 16K / 32K task had ~1.45x the mean
// steps) -- the last two are 6-14 % faster per class run alone and 2-6 % slower
// with the classes overlapping on their streams, which fill each other's idle
// waves already.  Also settled: masked lanes issue no load rather
// than load and discard, and the home buckets are checked branch-free.
template <class Probe, int UL = kJacUnrollDef, int UP = UL>
__device__ __forceinline__ void jac_probe_staged(const int32_t *__restrict__ ix, int64_t du,
                                                 int64_t lo, const JacStage &st,
                                                 const JacSink &sk, const Probe &pr) {
    static_assert(UL % UP == 0, "probe groups split the loaded elements");
    static_assert(64 * UL <= kIxPad, "unconditional list steps stay inside the index padding");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    using gi32 = __attribute__((address_space(1))) const int32_t;  // global, not flat
    // one step: U list elements per lane loaded (all in flight before the first probe),
    // lanes past d_v masked (MASK), then probed in groups of min(UP, U)
    auto step = [&](auto Uc, auto MASKc, gi32 *lp, int32_t left, int64_t &cnt) {
        constexpr int U = decltype(Uc)::value;
        constexpr bool MASK = decltype(MASKc)::value;
        constexpr int P = UP < U ? UP : U;
        int32_t xs[U];
#pragma unroll
        for (int t = 0; t < U; ++t) {
            if constexpr (MASK) {  // lanes past d_v issue no load (exec-masked)
                xs[t] = -1;
                if (lane + t * 64 < left) xs[t] = lp[t * 64];
            } else {
                xs[t] = lp[t * 64];
            }
        }
#pragma unroll
        for (int g = 0; g < U; g += P) {
            typename Probe::S ps[P];
#pragma unroll
            for (int t = 0; t < P; ++t) ps[t] = pr.first(xs[g + t] >= 0 ? xs[g + t] : 0);
            // the home buckets branch-free; the rare lanes whose search goes on take
            // done() under one wave-uniform branch (a per-element search loop costs
            // ~20 scalar mask operations per element even when it ends at once)
            bool hit[P], more[P], any = false;
#pragma unroll
            for (int t = 0; t < P; ++t) {
                hit[t] = pr.check1(xs[g + t], ps[t], more[t]);
                more[t] = more[t] && xs[g + t] >= 0;
                any = any || more[t];
            }
            if (__builtin_amdgcn_ballot_w64(any)) {
#pragma unroll
                for (int t = 0; t < P; ++t)
                    if (more[t]) hit[t] = pr.done(xs[g + t], ps[t]);
            }
#pragma unroll
            for (int t = 0; t < P; ++t) cnt += __popcll(__ballot(xs[g + t] >= 0 && hit[t]));
        }
    };
    using T1 = std::true_type;
    using F0 = std::false_type;
    for (int k = wave; k < st.nbig; k += nw) {
        const int32_t dv = __builtin_amdgcn_readfirstlane(st.dv[k]);
        // the list's base is wave-uniform: loads from a scalar base, one lane offset and
        // immediate step offsets.  Whole 64 UL-element steps first (no mask), then one
        // step of the fewest loads (1, 2, 4 .. UL per lane) that covers the rest, its
        // lanes past d_v masked -- their addresses reach at most 63 entries past the list
        // (the next rows', or the kIxPad padding after the last row).
        const uint64_t lb = (uint64_t)(ix + st.b[k]);
        gi32 *lst = (gi32 *)(
            (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)lb) |
            (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(lb >> 32)) << 32);
        int64_t cnt = 0;
        int32_t j0 = 0;
        for (; j0 + 64 * UL <= dv; j0 += 64 * UL)
            step(std::integral_constant<int, UL>{}, F0{}, lst + (uint32_t)(j0 + lane), 64 * UL, cnt);
        const int32_t rem = dv - j0;  // wave-uniform
        gi32 *lp = lst + (uint32_t)(j0 + lane);
        if (rem > 0) {
            if (rem <= 64) step(std::integral_constant<int, 1>{}, T1{}, lp, rem, cnt);
            else if (UL >= 2 && rem <= 128) step(std::integral_constant<int, (UL >= 2 ? 2 : 1)>{}, T1{}, lp, rem, cnt);
            else if (UL >= 4 && rem <= 256) step(std::integral_constant<int, (UL >= 4 ? 4 : 1)>{}, T1{}, lp, rem, cnt);
            else step(std::integral_constant<int, UL>{}, T1{}, lp, rem, cnt);
        }
        if (lane == 0) sk.put(lo + st.off[k], cnt, du, dv);
    }
    const int grp = lane >> 4, gl = lane & 15;
    const uint64_t gmask = 0xFFFFull << (16 * grp);
    for (int r = wave * 4; r < st.nsmall; r += nw * 4) {
        const int idx = r + grp;
        const bool ok = idx < st.nsmall;
        const int k = kJacMaxEnt - 1 - (ok ? idx : 0);
        const int64_t dv = ok ? st.dv[k] : 0;
        const int32_t x = gl < dv ? ix[st.b[k] + gl] : -1;
        const typename Probe::S ps = pr.first(x >= 0 ? x : 0);
        bool more;
        bool hit = pr.check1(x, ps, more);
        more = more && x >= 0;
        if (__builtin_amdgcn_ballot_w64(more))
            if (more) hit = pr.done(x, ps);
        hit = hit && x >= 0;
        const int64_t cnt = __popcll(__ballot(hit) & gmask);
        if (ok && gl == 0) sk.put(lo + st.off[k], cnt, du, dv);
    }
}

}  // namespace gs
