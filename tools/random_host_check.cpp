// Host-side check of the random baseline's per-element logic (gs_random.hpp) against
// NumPy: the undirected key, the head flag / rank of np.unique(return_inverse=True) and
// the gather keep_undir[inverse] with NumPy's index wrap, element by element in plain
// C++ on the CPU, in the order the device kernels of gs_random.hip take them.
//   random_check CASE_FILE
// CASE_FILE: int64 n, E, m; int64 src[E], dst[E], idx[E]; uint8 keep[m].
// Writes to stdout: int64 status (1: an id outside [0, n), n < 1, n >= 2^31 or E < 1);
// with status 0, int64 n_undirected and int64 inverse[E]; then int64 n_bad and the E mask
// bytes of keep[idx] (0 where idx is out of bounds).
// Build: hipcc -O2 tools/random_host_check.cpp -o /tmp/random_check
// (add -fsanitize=address,undefined for a checked run: host code only)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../gnn-sparsification-research_amd/csrc/gs_random.hpp"

static bool read_all(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
    using namespace gs;
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t head[3];
    if (!read_all(f, head, sizeof(head))) return 2;
    const int64_t n = head[0], E = head[1], m = head[2];
    if (E < 0 || m < 0) return 2;
    std::vector<int64_t> src(E), dst(E), idx(E);
    std::vector<unsigned char> keep(m);
    if (!read_all(f, src.data(), 8 * (size_t)E) || !read_all(f, dst.data(), 8 * (size_t)E) ||
        !read_all(f, idx.data(), 8 * (size_t)E) || !read_all(f, keep.data(), (size_t)m))
        return 2;
    fclose(f);

    int64_t status = 1;
    bool ok = E >= 1 && n >= 1 && n < (int64_t(1) << 31);
    for (int64_t i = 0; ok && i < E; ++i) ok = undirected_in_range(src[i], dst[i], n);
    if (ok) {
        std::vector<std::pair<uint64_t, int64_t>> kp(E);
        for (int64_t i = 0; i < E; ++i) kp[i] = {undirected_key(src[i], dst[i], n), i};
        std::sort(kp.begin(), kp.end());
        std::vector<uint64_t> keys(E);
        for (int64_t i = 0; i < E; ++i) keys[i] = kp[i].first;
        std::vector<int64_t> inverse(E);
        int64_t before = 0, count = 0;  // the exclusive scan of the head flags
        for (int64_t i = 0; i < E; ++i) {
            const int64_t h = undirected_head(keys.data(), i);
            const int64_t r = undirected_rank(before, h);
            inverse[kp[i].second] = r;
            count = r + 1;
            before += h;
        }
        status = 0;
        fwrite(&status, 8, 1, stdout);
        fwrite(&count, 8, 1, stdout);
        fwrite(inverse.data(), 8, (size_t)E, stdout);
    } else {
        fwrite(&status, 8, 1, stdout);
    }
    int64_t n_bad = 0;
    std::vector<unsigned char> mask(E > 0 ? E : 1);
    for (int64_t i = 0; i < E; ++i) {
        const int64_t w = wrap_index(idx[i], m);
        mask[i] = w < 0 ? 0 : keep[w];
        n_bad += w < 0;
    }
    fwrite(&n_bad, 8, 1, stdout);
    fwrite(mask.data(), 1, (size_t)E, stdout);
    return 0;
}
