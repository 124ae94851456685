"""Inputs and host references shared by the spectral-sampling tests (test_spectral_host.py,
test_gpu_spectral.py).  Every expected value is gsparse.selection.spectral_sample's (the
specification, NumPy calls only) or NumPy's own, computed in the test process."""

import numpy as np

# 1023..1025: the ordered cumsum's LDS tile; 2047..2049: the pairwise total's subtree;
# 8191 / 8193: np.sum's buffer block; 70001: many workgroups
PAIR_COUNTS = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 8191, 8193, 70001]
# 7..9: a thread's run of 8 draws; 2047..2049: one workgroup's 256 runs
DRAW_COUNTS = [1, 7, 8, 9, 2047, 2048, 2049]
SEEDS = [0, 42]


def sym_graph(m, seed, loops=0):
    """m distinct undirected pairs over m + 1 relabelled nodes, both directions of each,
    plus `loops` self-loop columns, in shuffled column order: (edge_index[2, E], n)."""
    rng = np.random.default_rng(seed)
    n = m + 1
    lab = rng.permutation(n).astype(np.int64)
    a, b = lab[:-1], lab[1:]
    lp = rng.integers(0, n, size=loops).astype(np.int64)
    ei = np.concatenate([np.stack([a, b]), np.stack([b, a]), np.stack([lp, lp])], axis=1)
    ei = ei[:, rng.permutation(ei.shape[1])]
    return np.ascontiguousarray(ei), n


def column_scores(E, seed, kind="plain"):
    """One positive score per column, the two directions of a pair differing.
    kind: "plain"; "zeros40" (40 % exact zeros); "odd" (NaN, +-inf, -0.0, negative and
    denormal entries mixed in)."""
    rng = np.random.default_rng(seed + 1000)
    s = rng.random(E) + 1e-3
    if kind == "zeros40":
        s[rng.random(E) < 0.4] = 0.0
    elif kind == "odd":
        odd = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -1.5, 5e-324, 2.2e-308])
        hit = rng.random(E) < 0.3
        s[hit] = odd[rng.integers(0, len(odd), size=int(hit.sum()))]
        s[0] = 0.75  # the total stays positive
    return s


def zero_ends(scores, ei, n):
    """scores with every pair whose id is among the first or the last eighth zeroed in all
    its columns: zeros at the front and at the end of p."""
    src, dst = ei
    keys = np.minimum(src, dst) * (n + 1) + np.maximum(src, dst)
    inv = np.unique(keys, return_inverse=True)[1]
    m = int(inv.max()) + 1
    cut = max(1, m // 8)
    s = scores.copy()
    s[(inv < cut) | (inv >= m - cut)] = 0.0
    return s


def multigraph(E, n, seed):
    """E columns over n nodes: pairs in both directions, one-way columns, duplicate
    columns (triples) and self-loops, shuffled (random_cases.multigraph's mix)."""
    rng = np.random.default_rng(seed)
    h = max(1, E // 3)
    a = rng.integers(0, n, size=(2, h))
    loops = np.repeat(rng.integers(0, n, size=(1, max(1, E // 10))), 2, axis=0)
    one_way = rng.integers(0, n, size=(2, h))
    ei = np.concatenate([a, a[::-1], loops, one_way, a[:, : max(1, h // 4)]], axis=1)
    while ei.shape[1] < E:
        ei = np.concatenate([ei, ei], axis=1)
    ei = ei[:, rng.permutation(ei.shape[1])[:E]]
    return np.ascontiguousarray(ei.astype(np.int64))


def np_irregular(ei, n):
    """Non-loop undirected pairs that do not have exactly two columns."""
    src, dst = ei
    keys = np.minimum(src, dst) * (n + 1) + np.maximum(src, dst)
    uk, cnt = np.unique(keys, return_counts=True)
    return int(((cnt != 2) & (uk // (n + 1) != uk % (n + 1))).sum())


def pair_probs(scores, ei, n):
    """(p[m], inverse[E]) of the specification, for the comparison with Generator.choice."""
    src, dst = ei
    E = len(src)
    keys = np.minimum(src, dst) * (n + 1) + np.maximum(src, dst)
    inv = np.unique(keys, return_inverse=True)[1]
    m = int(inv.max()) + 1
    first = np.full(m, E)
    np.minimum.at(first, inv, np.arange(E))
    r = np.asarray(scores, dtype=np.float64)[first]
    r = np.where(np.isfinite(r) & (r > 0) & (src[first] != dst[first]), r, 0.0)
    return r / np.sum(r), inv


# ---- the dense 96-node graph of the quality checks -------------------------------------
def dense96():
    """(edge_index[2, 2 * 2323], n = 96): G(96, 1/2), both directions, columns permuted."""
    n = 96
    A = np.triu(np.random.default_rng(5).random((n, n)) < 0.5, 1)
    iu, ju = np.nonzero(A)
    ei = np.concatenate([np.stack([iu, ju]), np.stack([ju, iu])], axis=1).astype(np.int64)
    ei = ei[:, np.random.default_rng(6).permutation(ei.shape[1])]
    return np.ascontiguousarray(ei), n


def laplacian(ei, n, w=None):
    """The Laplacian of the undirected graph whose two directions are both listed."""
    L = np.zeros((n, n))
    w = np.ones(ei.shape[1]) if w is None else np.asarray(w, dtype=np.float64)
    np.add.at(L, (ei[0], ei[1]), -w)
    L[np.arange(n), np.arange(n)] = 0.0
    L[np.arange(n), np.arange(n)] = -L.sum(axis=1)
    return L


def exact_er(ei, n):
    """R_uv per column from the dense pseudo-inverse."""
    Lp = np.linalg.pinv(laplacian(ei, n))
    d = np.diag(Lp)
    return d[ei[0]] + d[ei[1]] - 2.0 * Lp[ei[0], ei[1]]


def whitened_eigs(L, L2):
    """The eigenvalues of L^{+1/2} L2 L^{+1/2} on the range of L, ascending."""
    lam, U = np.linalg.eigh(L)
    keep = lam > 1e-9 * lam.max()
    W = U[:, keep] / np.sqrt(lam[keep])
    return np.linalg.eigvalsh(W.T @ L2 @ W)
