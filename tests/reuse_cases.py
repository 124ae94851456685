"""Shared inputs and references of the context-reuse tests (test_reuse_cases_host.py,
test_gpu_context_reuse.py): the graphs one context is walked over, in the order SEQUENCE,
their canonical CSR, per-column scores with ties, and every CPU reference the walk compares
with -- each computed once, kept, and read-only.

G1  graphs.rmat(11, 8, seed=1): n = 2048, hubs of several hundred neighbours, isolated nodes
G2  the karate_test golden (n = 34)
G3  G1 with its node ids put through one fixed permutation and made canonical again: the
    same n, nnz and degree multiset, other arrays -- what a cache keyed by shape alone
    would serve G1's results for
G4  empty: n = 5, E = 0
G5  the directed_dup golden: asymmetric, multiplicities above 1

G2P (not in SEQUENCE) is a second connected graph of G2's shape for the entry points that
compute on connected graphs only (algebraic connectivity, spectral bounds): karate relabelled
by a fixed permutation with one edge moved, so that its Fiedler value differs as well.

G3 is given G1's features and G1's per-column scores: what differs between their references
comes from the graph alone.
"""

import functools

import numpy as np

import gsparse_oracle as O
from conftest import golden_features, load_golden

SEQUENCE = ("G1", "G2", "G3", "G4", "G5", "G1")
NAMES = ("G1", "G2", "G3", "G4", "G5")
PERM_SEED = 20261
FEAT_DIM = 16
ER_K, ER_ITERS = 12, 40  # a few JL columns and a short CG: seconds for the oracle's C solver


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def permutation():
    return _frozen(np.random.default_rng(PERM_SEED).permutation(2048).astype(np.int64))


@functools.lru_cache(maxsize=None)
def graph(name):
    """(n, edge_index int64[2, E]) as it is handed to the library."""
    from gsparse import graphs

    if name == "G1":
        n, ei = 2048, graphs.rmat(11, 8, seed=1)
    elif name == "G2":
        g = load_golden("karate_test")
        n, ei = int(g["num_nodes"]), g["edge_index"]
    elif name == "G3":
        n, e1 = graph("G1")
        ei = permutation()[e1]
        ei = ei[:, np.lexsort((ei[1], ei[0]))]  # canonical again: sorted by (row, column)
    elif name == "G2P":
        n, e2 = graph("G2")
        pairs = {(int(a), int(b)) for a, b in e2.T if a < b}
        deg = np.bincount(e2[0], minlength=n)
        # move one edge: drop the first edge whose ends both keep two other neighbours, add the
        # first absent pair; then relabel and sort
        drop = next(e for e in sorted(pairs) if deg[e[0]] > 2 and deg[e[1]] > 2)
        add = next((a, b) for a in range(n) for b in range(a + 1, n) if (a, b) not in pairs)
        und = np.array(sorted((pairs - {drop}) | {add}), dtype=np.int64).T
        perm = np.random.default_rng(PERM_SEED + 1).permutation(n).astype(np.int64)
        ei = perm[np.concatenate([und, und[::-1]], axis=1)]
        ei = ei[:, np.lexsort((ei[1], ei[0]))]
    elif name == "G4":
        n, ei = 5, np.zeros((2, 0), dtype=np.int64)
    elif name == "G5":
        g = load_golden("directed_dup")
        n, ei = int(g["num_nodes"]), g["edge_index"]
    else:
        raise KeyError(name)
    return n, _frozen(np.ascontiguousarray(ei, dtype=np.int64))


@functools.lru_cache(maxsize=None)
def csr(name):
    n, ei = graph(name)
    return _frozen(*O.canonical_csr(ei, n))


def rows_of(name):
    return O.csr_rows(csr(name)[0])


@functools.lru_cache(maxsize=None)
def symmetric(name):
    """The 0/1 pattern equals its transpose (what gs_graph_shape reports)."""
    ip, ix, _ = csr(name)
    n = len(ip) - 1
    keys = rows_of(name) * n + ix
    return bool(np.array_equal(np.sort(ix.astype(np.int64) * n + rows_of(name)), keys))


def _seed(name):
    """G3 shares G1's seeds, G2P G2's."""
    return NAMES.index({"G3": "G1", "G2P": "G2"}.get(name, name))


@functools.lru_cache(maxsize=None)
def features(name):
    from gsparse import graphs

    if name in ("G2", "G5"):
        x = golden_features(load_golden("karate_test" if name == "G2" else "directed_dup"))
    else:
        x = graphs.features(graph(name)[0], FEAT_DIM, seed=7 + _seed(name))
    return _frozen(np.ascontiguousarray(x))


@functools.lru_cache(maxsize=None)
def scores(name):
    """One score per edge_index column, multiples of 1/8 in [0, 5): heavy ties."""
    E = graph(name)[1].shape[1]
    return _frozen(np.random.default_rng(100 + _seed(name)).integers(0, 40, E) / 8.0)


def _approx_er(ip, ix, d, n):
    """O.approx_er with ER_K JL columns and ER_ITERS CG iterations (the oracle's C solver,
    one BLAS chunk): the calls Engine.approx_er makes, at a width a test can afford."""
    if np.count_nonzero(O.csr_rows(ip) < ix) == 0:
        return np.zeros(len(ix), dtype=np.float64)
    Y, _, _ = O.approx_er_projection(ip, ix, n, seed=42, k=ER_K)
    Z, _ = O.cg(O.laplacian_reg(ip, ix, d, n), Y, ER_ITERS, 1e-6, 1)
    return O.er_from_z(ip, ix, Z)


def _adj(name):
    import scipy.sparse as sp

    ip, ix, d = csr(name)
    n = len(ip) - 1
    return sp.csr_matrix((d, ix, ip), shape=(n, n))


@functools.lru_cache(maxsize=None)
def connected_refs(name):
    """For a connected graph: (algebraic connectivity by NetworkX, symmetric sparsifier
    weights per CSR entry, their spectral bounds by the dense specification)."""
    import networkx as nx
    import scipy.sparse as sp
    from gsparse.metrics import spectral_bounds_dense

    ip, ix, _ = csr(name)
    n = len(ip) - 1
    adj = _adj(name)
    ac = float(nx.algebraic_connectivity(nx.from_scipy_sparse_array(adj), method="tracemin_lu"))
    hw = _frozen(0.5 + ((rows_of(name) + ix) % 3) * 0.75)  # symmetric in (u, v)
    return ac, hw, spectral_bounds_dense(adj, sp.csr_matrix((hw, ix, ip), shape=(n, n)))


# per CSR entry, on every graph
ENTRY_REFS = ("jaccard", "adamic_adar", "degree", "feature_cosine", "approx_er")
# per CSR entry, symmetric graphs only (the entry points refuse G5)
SYMMETRIC_REFS = ("common_neighbors", "trussness", "simmelian", "simmelian_k3", "exact_er")
# per node, symmetric graphs only
NODE_REFS = ("clustering", "component_labels")
# per edge_index column (src / dst / scores entry points), on every graph
COLUMN_REFS = ("topk", "segment_rank", "local", "forest", "undirected_ids", "backbone", "sampled",
               "spectral_weight", "degree_aware_1", "degree_aware_2", "random")
# symmetric graphs with entries: the sharded Jaccard's counts and the distributed select
SHARD_REFS = ("part_counts", "jsel")
JSEL_KEEP = 0.4


def random_scores(count):
    """One distinct score per undirected pair (the random baseline's input)."""
    return np.random.default_rng(77).random(count)


KEEP = 0.3  # retention ratio of the top-k and the sampled selection
SPECTRAL_SEED = 9


@functools.lru_cache(maxsize=None)
def ref(name, what):
    """The CPU reference `what` of graph `name`; computed once."""
    from gsparse import selection as S

    ip, ix, d = csr(name)
    n, ei = graph(name)
    E = ei.shape[1]
    if what == "jaccard":
        r = O.jaccard(ip, ix)
    elif what == "adamic_adar":
        r = O.adamic_adar(ip, ix)
    elif what == "degree":
        r = np.asarray(O.degree(ip, ix, d), dtype=np.float64)
    elif what == "feature_cosine":
        r = O.feature_cosine(ip, ix, features(name))
    elif what == "approx_er":
        r = _approx_er(ip, ix, d, n)
    elif what == "common_neighbors":
        r = O.jaccard_counts(ip, ix).astype(np.float64) if len(ix) else np.zeros(0)
    elif what == "trussness":
        r = S.trussness_host(ip, ix)[0].astype(np.float64)
    elif what == "simmelian":
        r = np.asarray(S.simmelian_host(ip, ix)[0], dtype=np.float64)
    elif what == "simmelian_k3":
        r = np.asarray(S.simmelian_host(ip, ix, 3)[0], dtype=np.float64)
    elif what == "exact_er":
        r = O.exact_er(ip, ix, d, n) if len(ix) else np.zeros(0)
    elif what == "clustering":
        import networkx as nx

        g = nx.from_scipy_sparse_array(_adj(name))
        c = nx.clustering(g)
        r = np.array([c[i] for i in range(n)], dtype=np.float64)
    elif what == "component_labels":
        from scipy.sparse.csgraph import connected_components

        _, lab = connected_components(_adj(name), directed=False)
        first = np.full(lab.max() + 1 if n else 0, n, dtype=np.int64)
        np.minimum.at(first, lab, np.arange(n))
        r = first[lab].astype(np.int32)  # the smallest node id of each node's component
    elif what == "topk":
        r = O.topk_mask(scores(name), E, KEEP, False, kind="stable")
    elif what == "segment_rank":
        r = S.local_filter_scores(scores(name), ei, n)[1]
    elif what == "local":
        r = S.local_filter_scores(scores(name), ei, n)[0]
    elif what == "forest":
        r = S.spanning_forest_host(scores(name), ei[0], ei[1], n)[0]
    elif what == "undirected_ids":
        keys = np.minimum(ei[0], ei[1]) * (n + 1) + np.maximum(ei[0], ei[1])
        r = np.unique(keys, return_inverse=True)[1].astype(np.int64)
    elif what == "sampled":
        r = O.sampled_mask(scores(name) + 0.125, E, KEEP, seed=42) if E else np.zeros(0, dtype=bool)
    elif what == "spectral_weight":
        r = S.spectral_sample(scores(name), ei, n, max(E // 4, 1), SPECTRAL_SEED)[1] if E else np.zeros(0)
    elif what == "degree_aware_1":
        r = S.degree_aware_mask(scores(name), ei, n, E, KEEP, 1)
    elif what == "degree_aware_2":
        r = S.degree_aware_mask(scores(name), ei, n, E, KEEP, 2)
    elif what == "random":
        ids = ref(name, "undirected_ids")
        cnt = int(ids.max()) + 1
        keep = np.zeros(cnt, dtype=bool)
        keep[np.argsort(random_scores(cnt))[-max(1, cnt // 2):]] = True
        r = keep[ids]
    elif what == "jsel":
        r = O.topk_mask(ref(name, "jaccard"), len(ix), JSEL_KEEP, False, kind="stable")
    elif what == "part_counts":
        r = np.concatenate([O.jaccard_part_counts(ip, ix, p, 2) for p in (0, 1)])
    elif what == "backbone":
        r = O.metric_backbone(ei, n, 1.0 + scores(name)) if E else np.zeros(0, dtype=bool)
    else:
        raise KeyError(what)
    return _frozen(np.ascontiguousarray(r))


def topology(name):
    """(average clustering, components, largest component) as NetworkX / SciPy count them."""
    lab = ref(name, "component_labels")
    n = graph(name)[0]
    import networkx as nx

    avg = float(nx.average_clustering(nx.from_scipy_sparse_array(_adj(name)))) if n else 0.0
    return avg, len(np.unique(lab)), int(np.bincount(lab).max()) if n else 0
