"""Shared inputs and references of the trussness tests (test_truss_host.py,
test_gpu_truss.py): the small graphs where the peel can go wrong, their canonical CSR, the
NumPy specification (selection.trussness_host) and NetworkX's repeated k_truss, each
computed once per case and kept."""

import functools
import itertools

import numpy as np
import scipy.sparse as sp


def both(pairs):
    ei = np.asarray(pairs, dtype=np.int64).reshape(-1, 2).T
    return np.concatenate([ei, ei[::-1]], axis=1)


def clique(nodes):
    return list(itertools.combinations(nodes, 2))


def _cliques_pairs():
    # K6 on 0..5, K4 on 5..8, K5 on 8..12, the bridge 12-13, K4 on {0, 1, 14, 15} sharing
    # the edge (0, 1); node 16 is isolated
    p = clique(range(6)) + clique(range(5, 9)) + clique(range(8, 13)) + [(12, 13)]
    return p + [e for e in clique((0, 1, 14, 15)) if e != (0, 1)]


def _lattice_pairs(k):
    p = []
    for i in range(k):
        for j in range(k):
            if j + 1 < k:
                p.append((i * k + j, i * k + j + 1))
            if i + 1 < k:
                p.append((i * k + j, (i + 1) * k + j))
            if i + 1 < k and j + 1 < k:
                p.append((i * k + j, (i + 1) * k + j + 1))
    return p


def _hub_pairs():
    # 0 and 1 adjacent to each other and to the leaves 2..3001; a K5 on {0, 3002..3005};
    # the pendant path 1 - 3006 - 3007; node 3008 is isolated
    leaves = range(2, 3002)
    p = [(0, 1)] + [(0, w) for w in leaves] + [(1, w) for w in leaves]
    return p + clique((0, 3002, 3003, 3004, 3005)) + [(1, 3006), (3006, 3007)]


def _build():
    from gsparse import graphs

    cases = {}

    def add(name, n, ei):
        ei = np.ascontiguousarray(np.asarray(ei, dtype=np.int64).reshape(2, -1))
        ei.setflags(write=False)
        cases[name] = (n, ei)

    add("empty", 5, [[], []])
    add("single_edge", 2, both([(0, 1)]))
    add("tree5", 5, both([(0, 1), (0, 2), (1, 3), (1, 4)]))
    add("triangle", 3, both(clique(range(3))))
    for c in (4, 5, 70):
        add(f"K{c}", c, both(clique(range(c))))
    cl = both(_cliques_pairs())
    add("cliques", 17, cl)
    loops = np.array([[0, 5, 16], [0, 5, 16]])
    dup = np.array([[3, 4], [4, 3]])
    add("cliques_loops_dups", 17, np.concatenate([cl[:, :40], loops, cl[:, 40:], dup], axis=1))
    karate, n_karate = graphs.karate("csr")
    add("karate", n_karate, karate)
    add("lattice24", 576, both(_lattice_pairs(24)))
    add("hub_pair", 3009, both(_hub_pairs()))
    add("rmat10", 1024, graphs.rmat(10, 8, seed=1))
    add("chung_lu", 2708, graphs.chung_lu())
    add("roman2000", 2000, graphs.roman_like(2000, 2900, seed=0))
    return cases


CASES = _build()
NAMES = tuple(CASES)

# the issue's table: entries, {trussness: entries}, levels, sub-rounds (None: not listed)
KNOWN = {
    "empty": (0, {}, 0, 0),
    "single_edge": (2, {2: 2}, 1, 1),
    "tree5": (8, {2: 8}, 1, 1),
    "triangle": (6, {3: 6}, 1, 1),
    "K4": (12, {4: 12}, 1, 1),
    "K5": (20, {5: 20}, 1, 1),
    "K70": (4830, {70: 4830}, 1, 1),
    "cliques": (74, {2: 2, 4: 22, 5: 20, 6: 30}, 4, 4),
    "karate": (156, {2: 22, 3: 84, 4: 22, 5: 28}, 4, 7),
    "lattice24": (3266, {3: 3266}, 1, 24),
    "hub_pair": (12026, {2: 4, 3: 12002, 5: 20}, 3, 4),
    "rmat10": (12104, None, 16, 82),
    "chung_lu": (None, None, 4, 10),
    "roman2000": (None, None, 3, 4),
}


@functools.lru_cache(maxsize=None)
def csr(name):
    """(indptr int64, indices int32) of the canonical CSR of the case: duplicates merged."""
    n, ei = CASES[name]
    a = sp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(n, n))
    a.sum_duplicates()
    a.sort_indices()
    ip, ix = a.indptr.astype(np.int64), a.indices.astype(np.int32)
    for x in (ip, ix):
        x.setflags(write=False)
    return ip, ix


def rows_of(name):
    ip, _ = csr(name)
    return np.repeat(np.arange(len(ip) - 1, dtype=np.int64), np.diff(ip))


def reverse_positions(name):
    """CSR position of (v, u) for every entry (u, v)."""
    ip, ix = csr(name)
    n = len(ip) - 1
    rows = rows_of(name)
    keys = rows * n + ix
    return np.searchsorted(keys, ix.astype(np.int64) * n + rows)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(t int64 per CSR entry, levels, rounds) by the NumPy specification; computed once."""
    from gsparse.selection import trussness_host

    t, levels, rounds = trussness_host(*csr(name))
    t.setflags(write=False)
    return t, levels, rounds


@functools.lru_cache(maxsize=None)
def networkx_trussness(name):
    """t per CSR entry from NetworkX: the largest k whose nx.k_truss contains the edge (the
    k-truss of the (k - 1)-truss is the k-truss of the graph, so each call starts there)."""
    import networkx as nx

    ip, ix = csr(name)
    n = len(ip) - 1
    rows = rows_of(name)
    off = rows != ix
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(rows[off].tolist(), ix[off].tolist()))
    t = np.zeros(len(ix), dtype=np.int64)
    keys = rows * n + ix
    k = 2
    while g.number_of_edges():
        e = np.array(list(g.edges()), dtype=np.int64).reshape(-1, 2)
        for a, b in ((e[:, 0], e[:, 1]), (e[:, 1], e[:, 0])):
            t[np.searchsorted(keys, a * n + b)] = k
        k += 1
        g = nx.k_truss(g, k)
    t.setflags(write=False)
    return t
