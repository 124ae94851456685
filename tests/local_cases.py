"""Shared inputs and references of the local-sparsification tests (test_local_host.py,
test_gpu_local.py): the graphs where the segment ranks can go wrong, per-column scores of
several kinds, and the NumPy specification (selection.local_filter_scores), computed once
per (graph, scores, direction) and kept."""

import functools

import numpy as np

import truss_cases as T

BORDER_DEGREES = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 66)  # the sub-wave group widths +- 1
LDS_DEGREES = (127, 128, 129, 255, 256, 257, 511, 512, 513, 700, 2047, 2048, 2049)  # one wave (by its
# compares per step) / small / large LDS image
WHEEL_HUB = 20000  # above the default LDS limit of gs_segment_rank (8192) and of gs_segment_topk


def _stars(degrees):
    """Disjoint stars: a centre of each degree, its leaves of degree 1; both directions."""
    pairs, n = [], 0
    for d in degrees:
        pairs += [(n, n + 1 + j) for j in range(d)]
        n += d + 1
    return n, T.both(pairs)


def _wheel(hub):
    """Node 0 adjacent to the rim 1..hub, the rim a ring: every rim node has degree 3."""
    rim = np.arange(1, hub + 1, dtype=np.int64)
    pairs = np.concatenate([np.stack([np.zeros(hub, dtype=np.int64), rim], axis=1),
                            np.stack([rim, np.roll(rim, -1)], axis=1)])
    return hub + 1, T.both(pairs)


def _build():
    cases = dict(T.CASES)

    def add(name, n, ei):
        ei = np.ascontiguousarray(np.asarray(ei, dtype=np.int64).reshape(2, -1))
        ei.setflags(write=False)
        cases[name] = (n, ei)

    add("borders", *_stars(BORDER_DEGREES))
    add("borders_lds", *_stars(LDS_DEGREES))
    add("wheel", *_wheel(WHEEL_HUB))
    add("isolated", 7, T.both([(1, 2), (2, 4), (4, 1), (4, 5)]))  # nodes 0, 3 and 6 have no column
    return cases


CASES = _build()
NAMES = tuple(CASES)
SMALL = ("karate", "rmat10", "hub_pair", "lattice24", "cliques_loops_dups", "K70")
KINDS = ("degsum", "mod101", "equal", "special", "distinct")


@functools.lru_cache(maxsize=None)
def scores(name, kind):
    """One score per column.  degsum: deg[src] + deg[dst], heavy ties; mod101: (7919 i) %
    101; equal: one value, only the index decides; special: NaN, +-inf, +-0.0 and a few
    ordinary values; distinct: a permutation, no ties."""
    n, ei = CASES[name]
    E = ei.shape[1]
    if kind == "degsum":
        deg = np.bincount(ei[0], minlength=n)
        s = (deg[ei[0]] + deg[ei[1]]).astype(np.float64)
    elif kind == "mod101":
        s = ((7919 * np.arange(E)) % 101).astype(np.float64)
    elif kind == "equal":
        s = np.full(E, 0.25)
    elif kind == "special":
        vals = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.5, -1.5, 0.0, np.nan, -0.0, 3.0])
        s = vals[np.random.default_rng(5).integers(0, len(vals), E)]
    elif kind == "distinct":
        s = (np.random.default_rng(6).permutation(E).astype(np.float64) - E / 3) / 7.0
    else:
        raise KeyError(kind)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def expected(name, kind, keep_lowest=False):
    """(local float64, rank int64, info) by the NumPy specification; computed once."""
    from gsparse.selection import local_filter_scores

    n, ei = CASES[name]
    local, rank, info = local_filter_scores(scores(name, kind), ei, n, keep_lowest)
    local.setflags(write=False)
    rank.setflags(write=False)
    return local, rank, info


def shuffled(name, seed=3):
    """(n, edge_index with its columns permuted, the permutation)."""
    n, ei = CASES[name]
    p = np.random.default_rng(seed).permutation(ei.shape[1])
    return n, np.ascontiguousarray(ei[:, p]), p


def brute_force(s, ei, n, keep_lowest=False):
    """The definition read literally, one Python loop per node and per pair -> (local,
    rank).  The exponent's table is the specification's (NumPy's log of the whole array)."""
    src, dst = ei[0].tolist(), ei[1].tolist()
    E = len(src)

    def key(i):
        v = float(s[i])
        return (1, 0.0, i) if v != v else (0, v + 0.0, i)  # NaN the largest; -0.0 + 0.0 == +0.0

    seg = {}
    for i, u in enumerate(src):
        seg.setdefault(u, []).append(i)
    keys = [key(i) for i in range(E)]
    rank = np.zeros(E, dtype=np.int64)
    for u, cols in seg.items():
        for i in cols:
            ki = keys[i]
            rank[i] = sum(1 for j in cols if (keys[j] < ki if keep_lowest else keys[j] > ki))
    max_deg = max((len(c) for c in seg.values()), default=0)
    table = np.log(np.maximum(np.arange(max(max_deg, 1) + 1), 1).astype(np.float64))
    best = {}
    x = np.zeros(E)
    for i in range(E):
        if rank[i] > 0:
            x[i] = table[rank[i] + 1] / table[len(seg[src[i]])]
        p = (min(src[i], dst[i]), max(src[i], dst[i]))
        best[p] = min(best.get(p, np.inf), x[i])
    local = np.array([1.0 - best[(min(a, b), max(a, b))] for a, b in zip(src, dst)], dtype=np.float64)
    return local, rank
