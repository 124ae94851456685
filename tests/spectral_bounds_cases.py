"""Graph pairs (G, H) shared by the spectral-bounds tests (test_spectral_bounds_host.py,
test_gpu_spectral_bounds.py), with their closed-form bounds where one exists.  Every
adjacency is a symmetric scipy CSR in canonical form; H's support is a subset of G's."""

import functools

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import spectral_cases as C

# |got - want| <= RTOL * lambda_max(want) for both values on the device: the project's own
# tolerance for the algebraic connectivity; scaled by lambda_max because lambda_min may be 0
RTOL = 1e-6


def sym(r, c, w, n):
    A = sp.coo_matrix((np.asarray(w, dtype=np.float64), (r, c)), shape=(n, n)).tocsr()
    A = (A + A.T).tocsr()
    A.sort_indices()
    return A


def cycle(n):
    i = np.arange(n)
    return sym(i, (i + 1) % n, np.ones(n), n)


def path(n, w=1.0):
    i = np.arange(n - 1)
    return sym(i, i + 1, np.full(n - 1, w), n)


def star(leaves, w):
    return sym(np.zeros(leaves, dtype=np.int64), np.arange(1, leaves + 1),
               np.broadcast_to(w, (leaves,)), leaves + 1)


def cycle_and_path(n):
    """(C_n, the path on the same nodes: the edge {0, n - 1} removed) -> (1 / n, 1)."""
    return cycle(n), path(n), (1.0 / n, 1.0)


def k64_and_star():
    """(K_64, the star of weight 2.5 at node 0) -> (2.5 / 64, 2.5)."""
    G = sp.csr_matrix(np.ones((64, 64)) - np.eye(64))
    return G, star(63, 2.5), (2.5 / 64, 2.5)


def star_alternating(leaves):
    """(the unit star, its leaves weighted 0.5 and 2.0 in turn) -> (0.5, 2.0): on a tree the
    pencil's eigenvalues are the weights."""
    w = np.where(np.arange(leaves) % 2 == 0, 0.5, 2.0)
    return star(leaves, 1.0), star(leaves, w), (0.5, 2.0)


def random_tree(n, seed):
    """(a random tree, the same tree reweighted by w) -> (min w, max w)."""
    rng = np.random.default_rng(seed)
    child = np.arange(1, n)
    parent = (rng.random(n - 1) * child).astype(np.int64)
    w = rng.uniform(0.25, 3.0, n - 1)
    return sym(parent, child, np.ones(n - 1), n), sym(parent, child, w, n), (w.min(), w.max())


def two_cliques():
    """(K_5 and K_7 joined by the bridge {4, 5}, the bridge dropped) -> (0, 1)."""
    A = np.zeros((12, 12))
    A[:5, :5] = 1.0
    A[5:, 5:] = 1.0
    np.fill_diagonal(A, 0.0)
    H = sp.csr_matrix(A)
    A[4, 5] = A[5, 4] = 1.0
    return sp.csr_matrix(A), H, (0.0, 1.0)


def largest_component(adj):
    adj = sp.csr_matrix(adj)
    _, lab = connected_components(adj, directed=False)
    nodes = np.flatnonzero(lab == np.argmax(np.bincount(lab)))  # the first largest
    sub = adj[nodes][:, nodes].tocsr()
    sub.sort_indices()
    return sub


@functools.lru_cache(maxsize=None)
def rmat10():
    """R-MAT-10's largest component, binary, no self-loops: 819 nodes, 12,028 entries."""
    from gsparse import graphs

    ei = graphs.rmat(10, seed=0)
    n = 1 << 10
    keep = ei[0] != ei[1]
    A = sp.csr_matrix((np.ones(int(keep.sum())), (ei[0][keep], ei[1][keep])), shape=(n, n))
    A.sum_duplicates()
    A.data[:] = 1.0
    A = A.maximum(A.T).tocsr()
    sub = largest_component(A)
    assert sub.shape[0] == 819 and sub.nnz == 12_028
    return sub


def edge_index_of(adj):
    """The CSR entries as edge_index columns, in entry order: (edge_index[2, nnz], n)."""
    adj = sp.csr_matrix(adj)
    rows = np.repeat(np.arange(adj.shape[0], dtype=np.int64), np.diff(adj.indptr))
    return np.stack([rows, adj.indices.astype(np.int64)]), adj.shape[0]


def dense_er(adj):
    """R_uv per CSR entry from the dense pseudo-inverse of the weighted Laplacian."""
    A = adj.toarray()
    np.fill_diagonal(A, 0.0)
    Lp = np.linalg.pinv(np.diag(A.sum(axis=1)) - A, hermitian=True)
    ei, _ = edge_index_of(adj)
    d = np.diag(Lp)
    return d[ei[0]] + d[ei[1]] - 2.0 * Lp[ei[0], ei[1]]


def with_weights(adj, w):
    """adj's pattern with weight w per CSR entry (zeros dropped)."""
    H = sp.csr_matrix((np.array(w, dtype=np.float64), adj.indices.copy(), adj.indptr.copy()),
                      shape=adj.shape)
    H.eliminate_zeros()  # in place: on H's own copies of the index arrays
    return H


def sampled(adj, scores, q, method, seed=42):
    """H from selection.spectral_sample over adj's entries: its weight per CSR entry."""
    from gsparse import selection

    ei, n = edge_index_of(adj)
    mask, w, _, _ = selection.spectral_sample(scores, ei, n, q, seed=seed, method=method)
    return np.where(mask, w, 0.0)


def resistance_halves(adj, er):
    """Unit weights on the half of the pairs with the highest resistance, and on the half
    with the lowest (both directions of a pair together): (hw_high, hw_low)."""
    ei, n = edge_index_of(adj)
    keys = np.minimum(ei[0], ei[1]) * n + np.maximum(ei[0], ei[1])
    uk, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    order = np.argsort(er[first], kind="stable")
    m = len(uk)
    low = np.zeros(m, dtype=bool)
    low[order[: m // 2]] = True
    return (~low)[inv].astype(np.float64), low[inv].astype(np.float64)


def dense96_pairs():
    """(ei, n, G, [(mask, weight, H) of the two samples of
    test_spectral_host.test_quality_*]) on dense96: the same calls, column for column."""
    from gsparse import selection

    ei, n = C.dense96()
    er = C.exact_er(ei, n)
    m = ei.shape[1] // 2
    G = sp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(n, n))
    G.sort_indices()
    out = []
    for q, method in ((m, "multinomial"), (m // 2, "independent")):
        mask, w, _, _ = selection.spectral_sample(er, ei, n, q, seed=42, method=method)
        H = sp.csr_matrix((w[mask], (ei[0][mask], ei[1][mask])), shape=(n, n))
        H.sort_indices()
        out.append((mask, w, H))
    return ei, n, G, out


def weighted_components_loops():
    """test_gpu_fiedler_sparse's weighted case (components, self-loops), rebuilt."""
    rng = np.random.default_rng(7)
    n = 900
    r = rng.integers(0, 600, 2500)
    c = (r + rng.integers(1, 40, 2500)) % 600
    r = np.concatenate([r, np.arange(600, 850), [3, 17, 650]])
    c = np.concatenate([c, np.arange(601, 851) % 850 + (np.arange(600, 850) >= 849) * 600,
                        [3, 17, 650]])
    w = rng.uniform(0.5, 2.0, len(r))
    A = sp.coo_matrix((w, (r, c)), shape=(n, n)).tocsr()
    A = (A + A.T).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def component_nodes(adj):
    """The nodes of adj's first largest component."""
    _, lab = connected_components(sp.csr_matrix(adj), directed=False)
    return np.flatnonzero(lab == np.argmax(np.bincount(lab)))


def weights_on(G, H):
    """H's entries at the positions of G's CSR entries (0 where H has none)."""
    n = G.shape[0]
    eg, eh = edge_index_of(G)[0], edge_index_of(H)[0]
    kg, kh = eg[0] * n + eg[1], eh[0] * n + eh[1]
    pos = np.searchsorted(kg, kh)
    assert (kg[pos] == kh).all()
    hw = np.zeros(G.nnz)
    hw[pos] = H.data
    return hw
