// Host-side check of the spanning forest's per-element rules (gs_forest.hpp) against
// NumPy: the key and the strict total order, the rank of a sorted position, and the
// Boruvka round (crossing test, far root, the one-way hook of a mutual pick), in plain
// C++ on the CPU, in the order the device kernels of gs_forest.hip take them.
//   forest_check CASE_FILE
// CASE_FILE: int64 n, E, keep_lowest; float64 scores[E]; int64 src[E], dst[E].
// Writes to stdout: int64 status (1: an id outside [0, n) or n < 1); with status 0,
// int64 order[E] (the columns, best first), int64 n_forest, int64 rounds, int64
// n_disagree (neighbours of `order` that forest_better does not rank that way), the E
// forest bytes and int64 labels[n] (one representative node per component).
// Build: hipcc -O2 tools/forest_host_check.cpp -o /tmp/forest_check
// (add -fsanitize=address,undefined for a checked run: host code only)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../gnn-sparsification-research_amd/csrc/gs_forest.hpp"

static bool read_all(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
    using namespace gs;
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t head[3];
    if (!read_all(f, head, sizeof(head))) return 2;
    const int64_t n = head[0], E = head[1];
    const int keep_lowest = (int)head[2];
    if (E < 0) return 2;
    std::vector<double> s(E);
    std::vector<int64_t> src(E), dst(E);
    if (!read_all(f, s.data(), 8 * (size_t)E) || !read_all(f, src.data(), 8 * (size_t)E) ||
        !read_all(f, dst.data(), 8 * (size_t)E))
        return 2;
    fclose(f);

    int64_t status = n >= 1 ? 0 : 1;
    for (int64_t i = 0; !status && i < E; ++i) status = forest_in_range(src[i], dst[i], n) ? 0 : 1;
    fwrite(&status, 8, 1, stdout);
    if (status) return 0;

    // the stable sort of (key, column) by key; pos[p] = the column at sorted position p
    std::vector<std::pair<uint64_t, int64_t>> kp(E);
    for (int64_t i = 0; i < E; ++i) kp[i] = {order_key(s[i]), i};
    std::stable_sort(kp.begin(), kp.end(),
                     [](const auto &a, const auto &b) { return a.first < b.first; });
    std::vector<int64_t> order(E);
    std::vector<int32_t> eu(E), ev(E);
    for (int64_t r = 0; r < E; ++r) {
        order[r] = kp[forest_flip(r, E, keep_lowest)].second;
        eu[r] = (int32_t)src[order[r]];
        ev[r] = (int32_t)dst[order[r]];
    }
    int64_t n_disagree = 0;
    for (int64_t r = 0; r + 1 < E; ++r)
        n_disagree += !forest_better(s[order[r]], order[r], s[order[r + 1]], order[r + 1], keep_lowest) ||
                      forest_better(s[order[r + 1]], order[r + 1], s[order[r]], order[r], keep_lowest);

    const int64_t none = -1;
    std::vector<int32_t> lab(n), hook(n);
    std::vector<int64_t> best(n, none), work(E), next;
    std::vector<unsigned char> forest(E > 0 ? E : 1, 0);
    for (int64_t u = 0; u < n; ++u) lab[u] = (int32_t)u;
    for (int64_t r = 0; r < E; ++r) work[r] = r;
    int64_t n_forest = 0, rounds = 0;
    while (!work.empty()) {
        next.clear();
        for (int64_t r : work) {  // k_forest_best
            const int32_t a = lab[eu[r]], b = lab[ev[r]];
            if (!forest_crossing(a, b)) continue;
            next.push_back(r);
            if (best[a] == none || r < best[a]) best[a] = r;
            if (best[b] == none || r < best[b]) best[b] = r;
        }
        int64_t hooked = 0;
        for (int64_t a = 0; a < n; ++a) {  // k_forest_hook
            if (lab[a] != (int32_t)a) continue;
            hook[a] = (int32_t)a;
            const int64_t r = best[a];
            if (r == none) continue;
            const int32_t other = forest_other((int32_t)a, lab[eu[r]], lab[ev[r]]);
            if (forest_hooks((int32_t)a, other, best[other] == r)) {
                hook[a] = other;
                forest[order[r]] = 1;
                ++hooked;
            }
        }
        for (int64_t a = 0; a < n; ++a)  // k_forest_apply
            if (lab[a] == (int32_t)a) {
                lab[a] = hook[a];
                best[a] = none;
            }
        for (int64_t u = 0; u < n; ++u) {  // k_forest_jump
            int32_t l = lab[u];
            for (int64_t step = 0; lab[l] != l; ++step) {
                if (step > n) return 3;  // a cycle among the hooks
                l = lab[l];
            }
            lab[u] = l;
        }
        if (!hooked) break;
        n_forest += hooked;
        ++rounds;
        work.swap(next);
    }
    fwrite(order.data(), 8, (size_t)E, stdout);
    fwrite(&n_forest, 8, 1, stdout);
    fwrite(&rounds, 8, 1, stdout);
    fwrite(&n_disagree, 8, 1, stdout);
    fwrite(forest.data(), 1, (size_t)E, stdout);
    std::vector<int64_t> labels(n);
    for (int64_t u = 0; u < n; ++u) labels[u] = lab[u];
    fwrite(labels.data(), 8, (size_t)n, stdout);
    return 0;
}
