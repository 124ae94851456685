// gs_tridiag.hpp -- the extreme eigenvalues of a Lanczos tridiagonal T (diagonal a[0, m),
// off-diagonal b[0, m - 1)) by Sturm counts and bisection, and the last component of a
// Ritz vector (the residual bound of a Ritz pair is beta_m |s_last|).  Per-element code
// for the device (gs_topology.hip, gs_fiedler_sparse.hip: one thread) and the host
// (gs_spectral_bounds.hip; tools/ritz_host_check.cpp compiles it alone).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace gs {

static constexpr int kLzMaxBasis = 512;  // >= max_iter + 1 coefficients: the basis and 1

// Sturm count: eigenvalues of the (m x m) tridiagonal (a, b) below x
__host__ __device__ inline int lz_sturm(const double *a, const double *b, int m, double x) {
    int cnt = 0;
    double q = 1.0;
    for (int i = 0; i < m; ++i) {
        const double bb = i ? b[i - 1] * b[i - 1] : 0.0;
        q = a[i] - x - (i ? bb / q : 0.0);
        if (q == 0.0) q = 1e-300;
        if (q < 0.0) ++cnt;
    }
    return cnt;
}

// largest eigenvalue of T (m x m): Gershgorin bracket, bisection (one thread)
__host__ __device__ inline double lz_ritz_max(const double *al, const double *be, int m) {
    double lo = 1e300, hi = -1e300;
    for (int i = 0; i < m; ++i) {
        const double r = (i ? fabs(be[i - 1]) : 0.0) + (i + 1 < m ? fabs(be[i]) : 0.0);
        lo = fmin(lo, al[i] - r);
        hi = fmax(hi, al[i] + r);
    }
    for (int it = 0; it < 200 && hi - lo > 1e-15 * fabs(hi); ++it) {
        const double mid = 0.5 * (lo + hi);
        if (lz_sturm(al, be, m, mid) < m) lo = mid;  // some eigenvalue above mid
        else hi = mid;
    }
    return hi;
}

// smallest eigenvalue of T: the same bracket and bisection from below.  The smallest one
// may be 0 exactly (a sparsifier that disconnects the graph), so the bracket closes
// relative to the larger end of the spectrum, not to the value itself.
__host__ __device__ inline double lz_ritz_min(const double *al, const double *be, int m) {
    double lo = 1e300, hi = -1e300;
    for (int i = 0; i < m; ++i) {
        const double r = (i ? fabs(be[i - 1]) : 0.0) + (i + 1 < m ? fabs(be[i]) : 0.0);
        lo = fmin(lo, al[i] - r);
        hi = fmax(hi, al[i] + r);
    }
    const double scale = fmax(fabs(lo), fabs(hi));
    for (int it = 0; it < 200 && hi - lo > 1e-15 * scale; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (lz_sturm(al, be, m, mid) >= 1) hi = mid;  // some eigenvalue below mid
        else lo = mid;
    }
    return lo;
}

// |last component| of the unit eigenvector of T (m <= kLzMaxBasis) for its eigenvalue
// theta, by the twisted factorisation: the pivots of T - theta I from the top (dp) and
// from the bottom (dm), the twist where they meet best, the vector from there outwards.
// A zero off-diagonal entry splits T; the components past it come out 0, as they should.
inline double lz_ritz_last(const double *al, const double *be, int m, double theta) {
    if (m <= 1) return 1.0;
    double dp[kLzMaxBasis], dm[kLzMaxBasis], z[kLzMaxBasis];
    double scale = fabs(theta);
    for (int i = 0; i < m; ++i) scale = fmax(scale, fabs(al[i]));
    const double tiny = 2.3e-16 * scale + 1e-300;  // a pivot at rounding level
    auto piv = [tiny](double d) { return fabs(d) < tiny ? (d < 0.0 ? -tiny : tiny) : d; };
    dp[0] = piv(al[0] - theta);
    for (int i = 1; i < m; ++i) dp[i] = piv(al[i] - theta - be[i - 1] * be[i - 1] / dp[i - 1]);
    dm[m - 1] = piv(al[m - 1] - theta);
    for (int i = m - 2; i >= 0; --i) dm[i] = piv(al[i] - theta - be[i] * be[i] / dm[i + 1]);
    int k = 0;
    double best = 1e300;
    for (int i = 0; i < m; ++i) {
        const double gam = fabs(dp[i] + dm[i] - (al[i] - theta));
        if (gam < best) {
            best = gam;
            k = i;
        }
    }
    z[k] = 1.0;
    for (int i = k - 1; i >= 0; --i) z[i] = -be[i] * z[i + 1] / dp[i];
    for (int i = k; i + 1 < m; ++i) z[i + 1] = -be[i] * z[i] / dm[i + 1];
    double nrm = 0.0;
    for (int i = 0; i < m; ++i) {
        if (!(fabs(z[i]) < 1e150)) return 1.0;  // overflowed: no bound, keep iterating
        nrm += z[i] * z[i];
    }
    return fabs(z[m - 1]) / sqrt(nrm);
}

}  // namespace gs
