// gs_sim.hpp -- the Simmelian backbone's host-side rules (gs_simmelian.hip): the pair
// classes, their bounds and the knobs that lower them.  Host and device code; also
// compiled for the host alone by tools/sim_host_check.cpp.
#pragma once

#include <cstdint>
#include <cstdlib>

#ifndef __host__
#define __host__
#define __device__
#endif

namespace gs {

// a pair {u, v} is classed by the shorter of its two neighbour lists, an upper bound on
// its common neighbours
enum { SIM_WAVE = 0, SIM_MID, SIM_LDS, SIM_STREAM, SIM_CLASSES };
static constexpr int kSimWaveMax = 64;   // one common neighbour per lane
static constexpr int kSimMidMax = 512;   // a wave's LDS slice: 2 KiB of ranks
static constexpr int kSimLdsMax = 8192;  // one workgroup: 32 KiB of ranks

struct SimBounds {
    int wave, mid, lds;
};

// a knob's text -> a bound in [0, dflt]: it can only lower the class limit
inline int sim_limit_text(const char *e, int dflt) {
    if (!e || !*e) return dflt;
    const long v = atol(e);
    return v < 0 ? 0 : v > dflt ? dflt : (int)v;
}

// GSPARSE_SIM_WAVE_MAX / _MID_MAX / _LDS_MAX as they are now
inline SimBounds sim_bounds() {
    return SimBounds{sim_limit_text(getenv("GSPARSE_SIM_WAVE_MAX"), kSimWaveMax),
                     sim_limit_text(getenv("GSPARSE_SIM_MID_MAX"), kSimMidMax),
                     sim_limit_text(getenv("GSPARSE_SIM_LDS_MAX"), kSimLdsMax)};
}

__host__ __device__ inline int sim_class(int64_t shorter, const SimBounds &b) {
    if (shorter <= b.wave) return SIM_WAVE;
    if (shorter <= b.mid) return SIM_MID;
    if (shorter <= b.lds) return SIM_LDS;
    return SIM_STREAM;
}

// where each class's pairs start in the shared list, from their counts
inline void sim_bases(const unsigned long long (&cls)[SIM_CLASSES], int64_t (&base)[SIM_CLASSES + 1]) {
    base[0] = 0;
    for (int k = 0; k < SIM_CLASSES; ++k) base[k + 1] = base[k] + (int64_t)cls[k];
}

// the library's argument check: 0 = the non-parametric score, k0 >= 1 the overlap at k0
inline bool sim_rank_ok(int64_t max_rank) { return max_rank >= 0 && max_rank < (int64_t(1) << 31); }

}  // namespace gs
