// Host-side check of the tridiagonal routines of gs_tridiag.hpp (the extreme Ritz values
// of a Lanczos tridiagonal by Sturm counts and bisection, and the last component of their
// eigenvectors by the twisted factorisation), in plain C++ on the CPU.
//   ritz_check CASE_FILE
// CASE_FILE: int64 count; then per tridiagonal int64 m (1 <= m <= 512), double a[m],
// double b[m - 1].
// Writes one text line per tridiagonal: lambda_min lambda_max |s_last(min)| |s_last(max)|.
// Build: hipcc -O2 tools/ritz_host_check.cpp -o /tmp/ritz_check
// (add -Xarch_host -fsanitize=address,undefined for a checked run: host code only)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../gnn-sparsification-research_amd/csrc/gs_tridiag.hpp"

static bool read_all(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
    using namespace gs;
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t count = 0;
    if (!read_all(f, &count, 8) || count < 0) return 2;
    for (int64_t t = 0; t < count; ++t) {
        int64_t m = 0;
        if (!read_all(f, &m, 8) || m < 1 || m > kLzMaxBasis) return 2;
        std::vector<double> a(m), b(m);  // b[m - 1] is never read
        if (!read_all(f, a.data(), 8 * (size_t)m) || !read_all(f, b.data(), 8 * (size_t)(m - 1)))
            return 2;
        const double lo = lz_ritz_min(a.data(), b.data(), (int)m);
        const double hi = lz_ritz_max(a.data(), b.data(), (int)m);
        printf("%.17g %.17g %.17g %.17g\n", lo, hi, lz_ritz_last(a.data(), b.data(), (int)m, lo),
               lz_ritz_last(a.data(), b.data(), (int)m, hi));
    }
    fclose(f);
    return 0;
}
