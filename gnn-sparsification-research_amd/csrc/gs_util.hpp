// gs_util.hpp -- the small rules every unit would otherwise retype: the binary search and
// the knob that lowers a class bound.  Host and device code; also compiled for the host
// alone by tools/util_host_check.cpp.
#pragma once

#include <cstdint>
#include <cstdlib>

#ifndef __host__
#define __host__
#define __device__
#endif

namespace gs {

// the first i in [0, n] with !p(i), for a p that is true on a prefix of [0, n) and false
// after it.  lo <= hi <= n throughout, so the midpoint never leaves [0, n) for any n of I.
template <class I, class Pred>
__host__ __device__ inline I partition_point(I n, Pred p) {
    I lo = 0, hi = n;
    while (lo < hi) {
        const I mid = lo + ((hi - lo) >> 1);
        if (p(mid))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// the first position of the ascending a[0, n) whose value is not below x
template <class I, class T>
__host__ __device__ inline I lower_bound(const T *a, I n, T x) {
    return partition_point(n, [=](I i) { return a[i] < x; });
}

// a knob's text -> a bound in [0, dflt]: it can only lower the class limit (tests reach
// every class on small graphs).  Unset or empty reads as the default, garbage as 0.
inline int knob_limit(const char *text, int dflt) {
    if (!text || !*text) return dflt;
    const long v = atol(text);
    return v < 0 ? 0 : v > dflt ? dflt : (int)v;
}

}  // namespace gs
