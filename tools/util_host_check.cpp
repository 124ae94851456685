// Host-side check of the shared rules of gs_util.hpp: the binary search (partition_point,
// lower_bound) against std::lower_bound, its midpoint at the ends of the index types, and
// the knob that can only lower a class bound, in plain C++ on the CPU.
//   util_check           exit status 0 when every rule holds, 1 with the failed line
// Build: hipcc -O2 tools/util_host_check.cpp -o /tmp/util_check
// (add -fsanitize=address,undefined for a checked run: host code only)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "../gnn-sparsification-research_amd/csrc/gs_util.hpp"

#define EXPECT(cond)                                             \
    do {                                                         \
        if (!(cond)) {                                           \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);   \
            return 1;                                            \
        }                                                        \
    } while (0)

// every x from below the smallest to above the largest value, in both index types
template <class I>
static int check_sorted(const std::vector<int32_t> &a) {
    const I n = (I)a.size();
    for (int32_t x = -1; x <= 9; ++x) {
        const I want = (I)(std::lower_bound(a.begin(), a.end(), x) - a.begin());
        EXPECT(gs::lower_bound(a.data(), n, x) == want);
        EXPECT(gs::partition_point(n, [&](I i) { return a[(size_t)i] < x; }) == want);
    }
    return 0;
}

// i < t without an array: every probe is checked to lie in [0, n), so no midpoint overflowed
template <class I>
static int check_range(I n) {
    const I ts[] = {0, 1, (I)(n - 1), n};
    for (I t : ts) {
        bool inside = true;
        int probes = 0;
        const I got = gs::partition_point(n, [&](I i) {
            inside = inside && i >= 0 && i < n;
            ++probes;
            return i < t;
        });
        EXPECT(got == t && inside && probes <= 64);
    }
    return 0;
}

int main() {
    using namespace gs;
    // n = 0, 1, 2, 3; all-true and all-false; runs of duplicates
    const std::vector<std::vector<int32_t>> lists = {
        {}, {4}, {0}, {8}, {2, 6}, {3, 3}, {1, 4, 7}, {5, 5, 5}, {0, 0, 8}, {0, 2, 2, 2, 2, 5, 5, 8, 8, 8}};
    for (const auto &a : lists)
        if (check_sorted<int32_t>(a) || check_sorted<int64_t>(a)) return 1;
    for (int32_t n = 0; n <= 3; ++n) {
        EXPECT(partition_point(n, [](int32_t) { return true; }) == n);
        EXPECT(partition_point(n, [](int32_t) { return false; }) == 0);
    }
    // a descending row and the predicates "still >= val" / "still > t", as the Simmelian
    // tables search their sorted counts (the diagonal's -1 last)
    const std::vector<int32_t> desc = {7, 7, 5, 3, 3, 3, 0, -1};
    for (int32_t val = -2; val <= 8; ++val) {
        const int32_t n = (int32_t)desc.size();
        const int32_t ge = (int32_t)(std::lower_bound(desc.begin(), desc.end(), val, std::greater_equal<int32_t>()) - desc.begin());
        const int32_t gt = (int32_t)(std::lower_bound(desc.begin(), desc.end(), val, std::greater<int32_t>()) - desc.begin());
        EXPECT(partition_point(n, [&](int32_t q) { return desc[(size_t)q] >= val; }) == ge);
        EXPECT(partition_point(n, [&](int32_t q) { return desc[(size_t)q] > val; }) == gt);
    }
    // the largest ranges of both index types
    if (check_range<int32_t>(std::numeric_limits<int32_t>::max())) return 1;
    if (check_range<int64_t>(int64_t(1) << 62)) return 1;
    // a knob can only lower its bound; garbage reads as 0, nothing set as the default
    EXPECT(knob_limit(nullptr, 64) == 64 && knob_limit("", 64) == 64);
    EXPECT(knob_limit("7", 64) == 7 && knob_limit("64", 64) == 64 && knob_limit("65", 64) == 64);
    EXPECT(knob_limit("-3", 64) == 0 && knob_limit("x", 64) == 0 && knob_limit("0", 64) == 0);
    EXPECT(knob_limit("99999999999999999999", 8192) == 8192);
    puts("util_check ok");
    return 0;
}
