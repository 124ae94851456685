"""Shared inputs and references of the spanning-forest tests (test_connected_host.py,
test_gpu_forest.py): the small graphs where the rounds can go wrong, SciPy's component
partition, and Kruskal's forest on the host (computed once per case and kept)."""

import functools

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from conftest import load_golden

RATES = (0.8, 0.5, 0.2)
# goldens with one Jaccard score per column (directed_dup's CSR merged duplicates)
GOLDENS = ("karate_test", "isolated", "single_edge", "star", "tree", "triangle", "two_triangles",
           "cora_like", "roman2000")


def both(ei):
    ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
    return np.concatenate([ei, ei[::-1]], axis=1)


def path(n):
    return both([np.arange(n - 1), np.arange(1, n)])


def partition(labels):
    """Canonical form of a labelling: every node gets the first node of its class."""
    _, first, inv = np.unique(np.asarray(labels), return_index=True, return_inverse=True)
    return first[inv.reshape(-1)]


def components(src, dst, n, mask=None):
    """(count, canonical labels) of the undirected graph of the (kept) columns."""
    if mask is not None:
        src, dst = src[mask], dst[mask]
    a = sp.coo_matrix((np.ones(len(src)), (src, dst)), shape=(n, n)).tocsr()
    c, lab = connected_components(a, directed=False)
    return c, partition(lab)


def jaccard(ei, n):
    import gsparse_oracle as O

    ip, ix, _ = O.canonical_csr(ei, n)
    return O.jaccard(ip, ix)


@functools.lru_cache(maxsize=None)
def generated(name):
    """(edge_index, n, oracle Jaccard scores) of the generated graphs of the issue's table."""
    from gsparse import graphs

    ei, n = {"rmat10": lambda: (graphs.rmat(10), 1024),
             "rmat14": lambda: (graphs.rmat(14), 16384),
             "roman2000": lambda: (graphs.roman_like(2000, 2900, 0), 2000)}[name]()
    ei = np.ascontiguousarray(ei, dtype=np.int64)
    s = jaccard(ei, n)
    assert len(s) == ei.shape[1]
    for a in (ei, s):
        a.setflags(write=False)
    return ei, n, s


def golden(name):
    g = load_golden(name)
    return np.ascontiguousarray(g["edge_index"], dtype=np.int64), int(g["num_nodes"]), g["scores_jaccard"]


def _small_cases():
    rng = np.random.default_rng(7)
    cases = {}

    def add(name, n, ei, s):
        ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
        s = np.asarray(s, dtype=np.float64)
        assert len(s) == ei.shape[1]
        cases[name] = (n, ei, s)

    add("empty", 4, [[], []], [])
    add("one_node", 1, [[], []], [])
    add("one_node_loop", 1, [[0], [0]], [0.5])
    add("one_edge", 2, [[0], [1]], [0.3])
    add("loops_only", 5, [[0, 2, 2, 4], [0, 2, 2, 4]], [0.1, 0.9, 0.9, 0.4])
    add("isolated_nodes", 9, both([[1, 5], [3, 7]]), [0.2, 0.7, 0.2, 0.7])
    add("triangle_equal", 3, both([[0, 1, 2], [1, 2, 0]]), np.ones(6))
    tt = both([[0, 1, 2, 3, 4, 5], [1, 2, 0, 4, 5, 3]])
    add("two_triangles", 6, tt, rng.random(12))
    t = rng.integers(0, np.arange(1, 40))  # node i + 1 hangs on a node <= i
    tree = both([np.arange(1, 40), t])
    add("tree", 40, tree, rng.random(78))
    leaves = np.arange(1, 5001)
    star = both([np.zeros(5000, dtype=np.int64), leaves])
    add("star_5000", 5001, star, rng.random(10000))
    add("star_5000_equal", 5001, star, np.full(10000, 0.25))
    p = path(4097)
    up = np.arange(4096, dtype=np.float64)
    add("path_ascending", 4097, p, np.concatenate([up, up]))
    alt = np.where(np.arange(4096) % 2 == 0, 1.0, 2.0) + np.arange(4096) * 1e-6
    add("path_alternating", 4097, p, np.concatenate([alt, alt]))
    add("path_equal", 4097, p, np.zeros(8192))
    # the ruler sequence: every round can only join neighbouring pairs, 12 rounds
    k = np.arange(1, 4097)
    ruler = -np.log2(k & -k)
    add("path_ruler", 4097, p, np.concatenate([ruler, ruler]))
    rm, n_rm, _ = generated("rmat10")
    add("rmat10_equal", n_rm, rm, np.full(rm.shape[1], 3.0))
    add("rmat10_two_valued", n_rm, rm, rng.integers(0, 2, rm.shape[1]).astype(np.float64))
    er = rng.integers(0, 60, (2, 300))
    add("directions_differ", 60, both(er), rng.random(600))
    dup = np.concatenate([er[:, :100], er[:, :100], er[::-1, :100], er[:, :50]], axis=1)
    add("duplicates", 60, dup, rng.integers(0, 4, dup.shape[1]).astype(np.float64))
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, -1.0, np.nan, np.inf, -np.inf])
    sp_ei = rng.integers(0, 40, (2, 400))
    add("special_values", 40, sp_ei, special[rng.integers(0, len(special), 400)])
    perm = rng.permutation(rm.shape[1])
    add("rmat10_shuffled", n_rm, rm[:, perm], rng.random(rm.shape[1]).round(2))
    for E in (1, 63, 64, 65, 257):
        add(f"multigraph_{E}", 24, rng.integers(0, 24, (2, E)), rng.integers(0, 5, E).astype(np.float64))
    return cases


SMALL = _small_cases()


@functools.lru_cache(maxsize=None)
def kruskal(name, keep_lowest):
    """(forest, guaranteed, component count, canonical labels) of SMALL[name] or a
    generated graph, by the host restatement; computed once."""
    from gsparse import selection as S

    if name in SMALL:
        n, ei, s = SMALL[name]
    else:
        ei, n, s = generated(name)
    forest, _ = S.spanning_forest_host(s, ei[0], ei[1], n, keep_lowest)
    guaranteed = S.guaranteed_columns(forest, ei[0], ei[1], n)
    c, lab = components(ei[0], ei[1], n)
    for a in (forest, guaranteed, lab):
        a.setflags(write=False)
    return forest, guaranteed, c, lab
