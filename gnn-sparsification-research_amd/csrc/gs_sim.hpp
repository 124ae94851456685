// gs_sim.hpp -- the Simmelian backbone's host-side rules (gs_simmelian.hip): the pair
// classes, their bounds and the knobs that lower them (gs_util.hpp's knob_limit).  Host and
// device code; also compiled for the host alone by tools/sim_host_check.cpp.
#pragma once

#include <cstdint>
#include <cstdlib>

#include "gs_util.hpp"

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

// GSPARSE_SIM_WAVE_MAX / _MID_MAX / _LDS_MAX as they are now (knob_limit: they only lower)
inline SimBounds sim_bounds() {
    return SimBounds{knob_limit(getenv("GSPARSE_SIM_WAVE_MAX"), kSimWaveMax),
                     knob_limit(getenv("GSPARSE_SIM_MID_MAX"), kSimMidMax),
                     knob_limit(getenv("GSPARSE_SIM_LDS_MAX"), kSimLdsMax)};
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
