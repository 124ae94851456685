"""Host-side selection helpers whose results are DEFINED by NumPy calls.

``sparsify_sampled`` (core.py:333-350) is a draw from NumPy's
``Generator.choice`` stream and ``sparsify_degree_aware`` (core.py:415-453)
orders ties with ``np.argsort``.  The plain functions make the reference's
own calls on the host; the ``*_device`` forms run the
same selection on the MI355X and give the same result, with the reference's
call only where NumPy's own behaviour decides.  The plain functions take
arrays so they are testable without a GPU.

``connected_mask`` is the one selection here that is not the reference's: a
top-k that cannot change the component structure (the maximum spanning forest
under the scores is kept first).  Its order is the stable one, a strict total
order, so its result is unique and NumPy's unstable argsort is never consulted.
"""

from __future__ import annotations

import numpy as np


def sampled_mask(scores: np.ndarray, num_edges: int, retention_ratio: float,
                 seed: int = 42) -> np.ndarray:
    """core.py:333-350 (the rng is created before the scores, as there)."""
    rng = np.random.default_rng(seed)
    floor = 1e-8
    s = np.nan_to_num(scores, nan=floor, posinf=floor, neginf=floor)
    probs = np.maximum(s, floor)
    probs = probs / probs.sum()
    num_keep = int(num_edges * retention_ratio)
    selected = rng.choice(num_edges, size=num_keep, replace=False, p=probs)
    mask = np.zeros(num_edges, dtype=bool)
    mask[selected] = True
    return mask


def sampled_mask_rounds(scores: np.ndarray, num_edges: int, retention_ratio: float,
                        seed: int = 42):
    """sampled_mask with ``Generator.choice(replace=False, p=...)`` (NumPy 2.x) written
    out: the executable specification of gs_sample_mask.  Returns ``(mask, rounds,
    draws)``: the same mask, the rejection rounds run and the uint64s consumed.

    Each round draws ``size - n_uniq`` doubles, zeroes the found entries of p,
    rebuilds cdf = cumsum(p) / cumsum(p)[-1] and searches it (side='right'); the
    distinct indices of a round are all new (the cdf is flat on a zeroed entry), so
    their order does not matter for the mask.  Inputs on which ``choice`` raises are
    passed to sampled_mask, so its exception surfaces."""
    rng = np.random.default_rng(seed)
    floor = 1e-8
    s = np.nan_to_num(scores, nan=floor, posinf=floor, neginf=floor)
    probs = np.maximum(s, floor)
    with np.errstate(all="ignore"):
        total = probs.sum() if len(probs) else 0.0
        p = probs / total
    num_keep = int(num_edges * retention_ratio)
    if (num_edges < 1 or len(p) != num_edges or not 0 <= num_keep <= num_edges
            or not np.isfinite(total)
            or (p == 0).any()):
        return sampled_mask(scores, num_edges, retention_ratio, seed), 0, 0
    mask = np.zeros(num_edges, dtype=bool)
    n_uniq = rounds = draws = 0
    while n_uniq < num_keep:
        x = rng.random(num_keep - n_uniq)
        p[mask] = 0
        cdf = np.cumsum(p)
        cdf /= cdf[-1]
        mask[cdf.searchsorted(x, side="right")] = True
        rounds += 1
        draws += len(x)
        n_uniq = int(mask.sum())
    return mask, rounds, draws


def sampled_mask_device(engine, scores: np.ndarray, num_edges: int, retention_ratio: float,
                        seed: int = 42, info: dict | None = None) -> np.ndarray:
    """sampled_mask with the rounds of ``Generator.choice`` on the MI355X
    (gs_sample_mask); the same mask, bit for bit.

    Degenerate inputs (a non-finite total, a probability that underflowed to 0,
    ``len(scores) != num_edges``, a keep count outside [0, E]) are those on which
    NumPy raises or takes another branch: the device reports them and the
    reference's own call is made, so its exception surfaces unchanged.

    ``info`` (optional dict) receives ``path`` ("device" or "host"), ``rounds`` and
    ``draws`` (uint64s of the PCG64 stream consumed)."""
    if info is None:
        info = {}
    rng = np.random.default_rng(seed)  # before the scores, as the reference
    raw = scores
    scores = np.asarray(scores)
    if scores.dtype != np.float64 or scores.ndim != 1:  # NumPy works in the scores' own dtype
        info.update(path="host", rounds=0, draws=0)
        return sampled_mask(raw, num_edges, retention_ratio, seed)
    num_keep = int(num_edges * retention_ratio)
    mask, status, rounds, draws = engine.sample_mask(scores, num_edges, num_keep, rng)
    if status != 0:
        info.update(path="host", rounds=0, draws=0)
        return sampled_mask(scores, num_edges, retention_ratio, seed)
    info.update(path="device", rounds=rounds, draws=draws)
    return mask


def degree_aware_mask(scores: np.ndarray, edge_index: np.ndarray, num_nodes: int,
                      num_edges: int, retention_ratio: float,
                      min_edges_per_node: int = 1) -> np.ndarray:
    """core.py:415-453 without the O(N*E) scans, same result.

    Phase 1: per node, ``incident[np.argsort(scores[incident])[-k:]]`` over its
    columns in ascending order (the reference's exact call is made whenever
    the pick is not unique: ties at the segment maximum, NaNs, or k > 1).
    Phase 2: the first non-guaranteed entries of ``np.argsort(scores)[::-1]``
    until ``int(E*r)`` columns are kept."""
    num_keep = int(num_edges * retention_ratio)
    src = np.asarray(edge_index)[0]
    order = np.argsort(src, kind="stable")
    bounds = np.searchsorted(src[order], np.arange(num_nodes + 1))
    counts = np.diff(bounds)
    mask = np.zeros(num_edges, dtype=bool)
    nonempty = np.nonzero(counts > 0)[0]
    exact_nodes = nonempty
    if min_edges_per_node == 1 and len(nonempty):
        sc = scores[order]  # IndexError when a column has no score, as the reference
        starts = bounds[nonempty]
        seg_max = np.maximum.reduceat(sc, starts)
        seg_id = np.repeat(np.arange(len(nonempty)), counts[nonempty])
        is_max = sc == seg_max[seg_id]
        n_max = np.bincount(seg_id, weights=is_max, minlength=len(nonempty))
        has_nan = np.bincount(seg_id, weights=np.isnan(sc), minlength=len(nonempty)) > 0
        unique = (n_max == 1) & ~has_nan
        pos = np.nonzero(is_max & unique[seg_id])[0]
        mask[order[pos]] = True
        exact_nodes = nonempty[~unique]
    for node in exact_nodes:
        lo, hi = bounds[node], bounds[node + 1]
        incident = order[lo:hi]
        k = min(min_edges_per_node, hi - lo)
        top_k = incident[np.argsort(scores[incident])[-k:]]
        mask[top_k] = True
    have = int(mask.sum())
    if have < num_keep:
        sorted_indices = np.argsort(scores)[::-1]
        cand = sorted_indices[~mask[sorted_indices]]
        mask[cand[: num_keep - have]] = True
    return mask


def degree_aware_mask_device(engine, scores: np.ndarray, edge_index: np.ndarray,
                             num_nodes: int, num_edges: int, retention_ratio: float,
                             min_edges_per_node: int = 1, info: dict | None = None) -> np.ndarray:
    """degree_aware_mask with both phases on the MI355X; the same result.

    Phase 1: gs_segment_argmax (min_edges_per_node == 1) gives every node's unique
    top column, gs_segment_topk (>= 2) the unique set of its k best columns; nodes
    where np.argsort's order decides (ties at the node's cut, NaN) take the
    reference's own call.  Phase 2: a device radix select over the scores with
    the guaranteed columns removed; an ambiguous tie block at the cut (or any
    NaN) takes the reference's own descending argsort walk.

    ``info`` (optional dict) receives which path ran: ``phase1`` ("device" or
    "host"), ``n_ambiguous`` (nodes resolved by the reference's call) and, for the
    segmented top-k, its ``classes`` counts."""
    if info is None:
        info = {}
    scores = np.asarray(scores, dtype=np.float64)
    src = np.ascontiguousarray(np.asarray(edge_index)[0], dtype=np.int64)
    if (not isinstance(min_edges_per_node, (int, np.integer)) or min_edges_per_node < 1
            or num_edges > len(scores) or np.isnan(scores).any()):
        info.update(phase1="host", n_ambiguous=0)
        return degree_aware_mask(scores, edge_index, num_nodes, num_edges, retention_ratio,
                                 min_edges_per_node)
    num_keep = int(num_edges * retention_ratio)
    k = int(min_edges_per_node)
    if k == 1:
        pick = engine.segment_argmax(scores, src[:num_edges], num_nodes)
        mask = np.zeros(num_edges, dtype=bool)
        mask[pick[pick >= 0]] = True
        amb = np.nonzero(pick == -2)[0]
    else:
        mask, status, seg = engine.segment_topk(scores, src[:num_edges], num_nodes, k)
        mask = mask.copy()
        amb = np.nonzero(status == 2)[0]
        info["classes"] = seg["classes"]
    info.update(phase1="device", n_ambiguous=int(len(amb)))
    if len(amb):
        order = np.argsort(src, kind="stable")
        bounds = np.searchsorted(src[order], np.arange(num_nodes + 1))
        for node in amb:
            incident = order[bounds[node]:bounds[node + 1]]
            mask[incident[np.argsort(scores[incident])[-k:]]] = True
    have = int(mask.sum())
    if have >= num_keep:
        return mask
    k2 = num_keep - have
    masked = scores.copy()
    masked[np.nonzero(mask)[0]] = -np.inf
    sel, cut, beyond, tied = engine.topk_mask(masked, num_edges, k2, False)
    need = k2 - beyond
    if (0 < need < tied) or cut == -np.inf:
        # the reference's own walk: first non-guaranteed of argsort(scores)[::-1]
        sorted_indices = np.argsort(scores)[::-1]
        cand = sorted_indices[~mask[sorted_indices]]
        mask[cand[:k2]] = True
        return mask
    return mask | sel


def spanning_forest_host(scores: np.ndarray, src: np.ndarray, dst: np.ndarray, num_nodes: int,
                         keep_lowest: bool = False):
    """The forest of gs_spanning_forest on the host: Kruskal's walk with a union-find over
    the columns, best first.  Ascending order is ``np.lexsort((arange(E), scores))`` --
    (score, index) with -0.0 == +0.0 and NaN last; the walk runs it backwards, or
    forwards with ``keep_lowest``.  Returns ``(forest, parent)``: the bool mask of the
    columns that joined two components, and the union-find's parents."""
    E = len(src)
    if len(scores) < E:
        raise ValueError(f"{len(scores)} scores for {E} columns: one score per edge_index column "
                         "is needed")
    order = np.lexsort((np.arange(E), np.asarray(scores, dtype=np.float64)[:E]))
    if not keep_lowest:
        order = order[::-1]
    parent = list(range(num_nodes))
    forest = np.zeros(E, dtype=bool)
    us, vs = np.asarray(src)[order].tolist(), np.asarray(dst)[order].tolist()
    left = num_nodes - 1
    for col, u, v in zip(order.tolist(), us, vs):
        while parent[u] != u:
            parent[u] = parent[parent[u]]
            u = parent[u]
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        if u != v:
            parent[u] = v
            forest[col] = True
            left -= 1
            if not left:
                break
    return forest, np.asarray(parent, dtype=np.int64)


def guaranteed_columns(forest: np.ndarray, src: np.ndarray, dst: np.ndarray,
                       num_nodes: int) -> np.ndarray:
    """Every column whose unordered pair {src, dst} is the pair of a forest column."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    keys = np.minimum(src, dst) * (num_nodes + 1) + np.maximum(src, dst)
    return np.isin(keys, keys[forest])


def connected_mask(scores: np.ndarray, edge_index: np.ndarray, num_nodes: int, num_edges: int,
                   retention_ratio: float, keep_lowest: bool = False) -> np.ndarray:
    """Connectivity-preserving top-k: the maximum spanning forest under the scores, in
    both directions (and every duplicate of its pairs), then the best of the other
    columns until ``int(E * r)`` are kept.  The kept columns have the component
    partition of the whole graph; when the guaranteed set alone is over the budget it
    is the mask (the precedent of ``degree_aware_mask``).

    Column i is better than column j when ``(score, index)`` is larger (``keep_lowest``:
    smaller), -0.0 == +0.0, NaN the largest: the stable top-k's order, strict and
    total, so the result is unique."""
    ei = np.asarray(edge_index)
    src, dst = ei[0][:num_edges], ei[1][:num_edges]
    scores = np.asarray(scores, dtype=np.float64)
    forest, _ = spanning_forest_host(scores, src, dst, num_nodes, keep_lowest)
    mask = guaranteed_columns(forest, src, dst, num_nodes)
    num_keep = int(num_edges * retention_ratio)
    have = int(mask.sum())
    if have < num_keep:
        order = np.lexsort((np.arange(num_edges), scores[:num_edges]))
        if not keep_lowest:
            order = order[::-1]
        cand = order[~mask[order]]
        mask[cand[: num_keep - have]] = True
    return mask


def connected_mask_device(engine, scores: np.ndarray, edge_index: np.ndarray, num_nodes: int,
                          num_edges: int, retention_ratio: float, keep_lowest: bool = False,
                          info: dict | None = None) -> np.ndarray:
    """connected_mask on the MI355X; the same mask.  The guaranteed set is
    gs_spanning_forest's expanded forest (Boruvka rounds over the columns); the fill is
    gs_topk_mask's stable select over the scores of the other columns alone, in column
    order -- the guaranteed columns are taken out, not given a sentinel score, so
    +-inf and NaN scores cannot bring one back or push one out.

    ``info`` (optional dict) receives ``path`` ("device"), ``forest`` (``|F|``),
    ``guaranteed`` (``|G|``), ``rounds``, ``over_budget`` and, when columns were
    filled, the fill's ``cut`` / ``beyond`` / ``tied``."""
    if info is None:
        info = {}
    ei = np.asarray(edge_index)
    src = np.ascontiguousarray(ei[0][:num_edges], dtype=np.int64)
    dst = np.ascontiguousarray(ei[1][:num_edges], dtype=np.int64)
    scores = np.ascontiguousarray(scores, dtype=np.float64)
    mask, _, f = engine.spanning_forest(scores, src, dst, num_nodes, keep_lowest, expand=True)
    num_keep = int(num_edges * retention_ratio)
    have = int(f["n_marked"])
    info.update(path="device", forest=f["n_forest"], guaranteed=have, rounds=f["rounds"],
                over_budget=have > num_keep, cut=float("nan"), beyond=0, tied=0)
    mask = mask.copy()
    if have >= num_keep:
        return mask
    rest = np.nonzero(~mask)[0]
    sel, cut, beyond, tied = engine.topk_mask(scores[:num_edges][rest], len(rest), num_keep - have,
                                              keep_lowest)
    info.update(cut=cut, beyond=beyond, tied=tied)
    mask[rest[sel]] = True
    return mask


def trussness_host(indptr, indices):
    """The trussness of every entry of a symmetric CSR pattern: the NumPy specification of
    gs_trussness.  Returns ``(t, levels, rounds)``: ``t`` (int64, one per entry, 0 on the
    diagonal), the number of levels with a non-empty frontier and their sub-rounds summed.

    On the simple undirected graph of the pattern (diagonal entries take no part): level
    ``s`` starts at the smallest support among the alive edges; a sub-round gives every
    alive edge of support ``<= s`` the trussness ``s + 2`` and removes it; the supports
    are then counted again from scratch (a sparse product per sub-round: obviously right,
    and slow), and the level goes on while an alive edge has support ``<= s``."""
    import scipy.sparse as sp

    indptr = np.asarray(indptr, dtype=np.int64)
    cols = np.asarray(indices, dtype=np.int64)
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    keys = rows * n + cols
    if len(keys) and (np.any(np.diff(keys) <= 0) or not np.array_equal(np.sort(cols * n + rows), keys)):
        raise ValueError("trussness_host needs a canonical CSR with a symmetric pattern")
    t = np.zeros(len(cols), dtype=np.int64)
    alive = rows != cols

    def supports():
        a = sp.csr_matrix((np.ones(int(alive.sum())), (rows[alive], cols[alive])), shape=(n, n))
        tri = (a @ a).multiply(a).tocsr()
        sup = np.zeros(len(cols), dtype=np.int64)
        sup[alive] = np.asarray(tri[rows[alive], cols[alive]]).ravel().astype(np.int64)
        return sup

    levels = rounds = 0
    while alive.any():
        sup = supports()
        s = int(sup[alive].min())
        levels += 1
        frontier = alive & (sup <= s)
        while frontier.any():
            t[frontier] = s + 2
            alive &= ~frontier
            rounds += 1
            if not alive.any():
                break
            frontier = alive & (supports() <= s)
    return t, levels, rounds


def simmelian_prepare(indptr, indices):
    """What both modes of ``simmelian_host`` share, a function of the graph alone: the
    triangle count ``t`` of every entry (-1 on the diagonal), every row's counts in
    descending order, the tie-aware rank of every entry in its whole row, and the list of
    (pair, common neighbour) hits with the common neighbour's rank at either end, the
    other end removed.  Pass it to ``simmelian_host(..., prep=)`` to evaluate several
    ``max_rank`` on one graph."""
    indptr = np.asarray(indptr, dtype=np.int64)
    cols = np.asarray(indices, dtype=np.int64)
    n = len(indptr) - 1
    nnz = len(cols)
    deg = np.diff(indptr)
    rows = np.repeat(np.arange(n, dtype=np.int64), deg)
    keys = rows * n + cols
    if nnz and (np.any(np.diff(keys) <= 0) or not np.array_equal(np.sort(cols * n + rows), keys)):
        raise ValueError("simmelian_host needs a canonical CSR with a symmetric pattern")
    tpos = np.searchsorted(keys, cols * n + rows)
    hasdiag = np.zeros(n, dtype=np.int64)
    hasdiag[rows[rows == cols]] = 1
    up = np.nonzero(rows < cols)[0]  # one unit of work per pair u < v
    u, v = rows[up], cols[up]
    ufirst = deg[u] <= deg[v]
    a, b = np.where(ufirst, u, v), np.where(ufirst, v, u)  # a: the shorter list
    mn = deg[a]
    pid = np.repeat(np.arange(len(up), dtype=np.int64), mn)
    ea = indptr[a][pid] + (np.arange(len(pid), dtype=np.int64) - np.repeat(np.cumsum(mn) - mn, mn))
    w = cols[ea]
    want = b[pid] * n + w
    eb = np.minimum(np.searchsorted(keys, want), max(nnz - 1, 0))
    hit = (keys[eb] == want) & (w != a[pid]) & (w != b[pid]) if nnz else np.zeros(0, dtype=bool)
    pid, ea, eb = pid[hit], ea[hit], eb[hit]
    c = np.bincount(pid, minlength=len(up)).astype(np.int64)  # common neighbours = triangles
    t = np.full(nnz, -1, dtype=np.int64)  # the diagonal's sentinel ranks last
    t[up] = c
    t[tpos[up]] = c
    order = np.lexsort((-t, rows))
    st = t[order]  # every row's counts, descending
    tmax = int(t.max()) if nnz else 0
    K = tmax + 2
    G = rows * K + (tmax - st)  # ascending: a row's position of a count by one search
    rf = np.searchsorted(G, rows * K + (tmax - t), side="left") - indptr[rows]  # larger counts in the row
    tp = c[pid]
    m = np.maximum(rf[ea] - (tp > t[ea]), rf[eb] - (tp > t[eb]))
    return dict(indptr=indptr, n=n, nnz=nnz, deg=deg, hasdiag=hasdiag, tpos=tpos, up=up, u=u, v=v,
                c=c, t=t, st=st, tmax=tmax, K=K, G=G, rf=rf, pid=pid, m=m)


def _simmelian_size(p, x, exy, k, txy):
    """``|P_k(x|y)|`` for node ``x``, the entry ``exy`` of its alter ``y`` (count ``txy``)
    and rank bound ``k`` (arrays): the row's sorted counts with one copy of ``txy`` taken
    out at its first position; below the row's length the size is the end of the tie
    group that holds position ``k - 1``."""
    ip = p["indptr"]
    L = p["deg"][x] - p["hasdiag"][x] - 1
    full = k >= L
    pos = p["rf"][exy]
    j = np.minimum(k, np.maximum(L, 1)) - 1
    jj = np.where(j < pos, j, j + 1)
    val = p["st"][ip[x] + np.minimum(jj, p["deg"][x] - 1)]
    ge = np.searchsorted(p["G"], x * p["K"] + (p["tmax"] - val), side="right") - ip[x]
    return np.where(full, L, ge - (txy >= val))


def simmelian_host(indptr, indices, max_rank: int = 0, prep=None):
    """The Simmelian backbone score of every entry of a symmetric CSR pattern: the NumPy
    specification of gs_simmelian, in the candidate form.  Returns ``(score, num, den)``:
    float64 and two int64 arrays, one value per entry, ``score = num / den`` by one IEEE
    division, equal on ``(u, v)`` and ``(v, u)``, 0 (``0 / 1``) on the diagonal.

    On the simple undirected graph of the pattern: ``t(u, w)`` is the number of triangles
    through {u, w}; for an edge {u, v} the ego ``u`` ranks ``N(u) \\ {v}`` by ``t``, ties
    sharing the best rank (0-based), and ``P_k(u|v)`` holds the neighbours of rank below
    ``k``.  ``max_rank = 0``: the largest Jaccard ratio of ``P_k(u|v)`` and ``P_k(v|u)``
    over ``k >= 1``.  The intersection only grows at ``k = m_w + 1``, ``m_w`` the larger of
    a common neighbour's two ranks, so with the ``m`` sorted candidate ``j`` (the last of
    equal ``m``) is ``j / (|P_{m+1}(u|v)| + |P_{m+1}(v|u)| - j)``; the candidates are
    compared exactly (cross-multiplied int64).  ``max_rank = k0 >= 1``: the overlap
    ``|P_k0(u|v) ∩ P_k0(v|u)|`` itself, ``den = 1``."""
    k0 = int(max_rank)
    if k0 < 0:
        raise ValueError(f"max_rank must be >= 0, got {max_rank}")
    p = simmelian_prepare(indptr, indices) if prep is None else prep
    up, tpos, pid, m = p["up"], p["tpos"], p["pid"], p["m"]
    P = len(up)
    num = np.zeros(P, dtype=np.int64)
    den = np.ones(P, dtype=np.int64)
    if k0 >= 1:
        num = np.bincount(pid[m < k0], minlength=P).astype(np.int64)
    elif len(pid):
        o = np.lexsort((m, pid))
        sp_, sm = pid[o], m[o]
        start = np.concatenate([[0], np.cumsum(p["c"])])
        j = np.arange(len(o), dtype=np.int64) - start[sp_] + 1
        last = np.ones(len(o), dtype=bool)  # the last of equal m in its pair
        last[:-1] = (sp_[1:] != sp_[:-1]) | (sm[1:] != sm[:-1])
        cp, cj, ck = sp_[last], j[last], sm[last] + 1
        txy = p["c"][cp]
        cd = (_simmelian_size(p, p["u"][cp], up[cp], ck, txy)
              + _simmelian_size(p, p["v"][cp], tpos[up[cp]], ck, txy) - cj)
        # the best candidate of a pair: the largest quotient first (a correctly rounded
        # division is monotone, so the exact maximum is among the largest quotients) ...
        q = cj / cd
        heads = np.nonzero(np.concatenate([[True], cp[1:] != cp[:-1]]))[0]
        best = np.maximum.reduceat(q, heads)
        pairs = cp[heads]
        bq = np.zeros(P)
        bq[pairs] = best
        first = np.nonzero(q == bq[cp])[0]
        first = first[np.concatenate([[True], cp[first][1:] != cp[first][:-1]])]
        num[pairs], den[pairs] = cj[first], cd[first]
        # ... then the exact check, and an exact scan of the pairs it fails on
        for pr in np.unique(cp[cj * den[cp] > num[cp] * cd]):
            for i in np.nonzero(cp == pr)[0]:
                if int(cj[i]) * int(den[pr]) > int(num[pr]) * int(cd[i]):
                    num[pr], den[pr] = cj[i], cd[i]
    n_out = np.zeros(p["nnz"], dtype=np.int64)
    d_out = np.ones(p["nnz"], dtype=np.int64)
    n_out[up], d_out[up] = num, den
    n_out[tpos[up]], d_out[tpos[up]] = num, den
    return n_out / d_out, n_out, d_out


def simmelian_bruteforce(indptr, indices, max_rank: int = 0):
    """The literal definition of ``simmelian_host``: Python sets, every ``k`` at which a
    ranked neighbourhood gains a member, ``fractions.Fraction``.  Slow and obviously right.  Returns one ``Fraction`` per entry (the overlap for ``max_rank >=
    1``)."""
    from fractions import Fraction

    indptr = np.asarray(indptr, dtype=np.int64)
    cols = np.asarray(indices, dtype=np.int64)
    n = len(indptr) - 1
    k0 = int(max_rank)
    if k0 < 0:
        raise ValueError(f"max_rank must be >= 0, got {max_rank}")
    nb = [set(cols[indptr[x]:indptr[x + 1]].tolist()) - {x} for x in range(n)]
    tri = {}

    def t(x, y):
        key = (x, y) if x < y else (y, x)
        if key not in tri:
            tri[key] = len(nb[x] & nb[y])
        return tri[key]

    by_t = {}

    def ranked(x, y):
        """(ranks, neighbours) of N(x) minus y by ascending rank: the rank of w is the
        number of the others with strictly more triangles"""
        if x not in by_t:
            ws = np.array(sorted(nb[x]), dtype=np.int64)
            ts = np.array([t(x, int(w)) for w in ws], dtype=np.int64)
            o = np.argsort(-ts, kind="stable")
            by_t[x] = (ws[o], ts[o])
        ws, ts = by_t[x]
        keep = ws != y
        ws, ts = ws[keep], ts[keep]
        rank = np.searchsorted(-ts, -ts, side="left")  # ts is descending
        return rank, ws

    def prefix(lst, cur, pos, k):
        """the members of rank < k join ``cur``; ``pos`` of them were in already"""
        new = int(np.searchsorted(lst[0], k, side="left"))
        cur.update(lst[1][pos:new].tolist())
        return new

    res = [Fraction(0)] * len(cols)
    pos_of = {}
    for x in range(n):
        for e in range(indptr[x], indptr[x + 1]):
            pos_of[(x, int(cols[e]))] = e
    for (x, y), e in pos_of.items():
        if x >= y:
            continue
        lx, ly = ranked(x, y), ranked(y, x)
        px, py, ix, iy = set(), set(), 0, 0
        if k0 >= 1:
            prefix(lx, px, 0, k0)
            prefix(ly, py, 0, k0)
            best = Fraction(len(px & py))
        else:
            best = Fraction(0)
            # every k at which either set gains a member (k = a rank + 1): between two of
            # them both sets, and so the ratio, stay what they were
            for k in np.unique(np.concatenate([lx[0] + 1, ly[0] + 1, [1]])).tolist():
                ix, iy = prefix(lx, px, ix, k), prefix(ly, py, iy, k)
                inter = len(px & py)
                if inter:
                    best = max(best, Fraction(inter, len(px) + len(py) - inter))
        res[e] = res[pos_of[(y, x)]] = best
    return res


def local_filter_scores(scores, edge_index, num_nodes: int, keep_lowest: bool = False):
    """The local-filter score of every ``edge_index`` column: the NumPy specification of
    gs_segment_rank and gs_local_scores (L-Spar, Satuluri et al.; Local Degree / Local
    Similarity, Hamann et al.; NetworKit's local filter on top of any edge score).

    The segment of node ``u`` is the set of columns with ``src == u``, ``d_u`` its length
    (loops and duplicate columns are ordinary columns).  Column i is better than column j
    when ``(score, index)`` is lexicographically larger (``keep_lowest``: smaller), -0.0
    == +0.0, NaN the largest: ``connected_mask``'s strict total order.  ``rank[i]`` = the
    better columns of i's own segment.  ``x[i]`` = 0 for rank 0, else ``T[rank + 1] /
    T[d_src]`` with ``T = log(max(arange(max_deg + 1), 1))``: node ``u`` keeps column i at
    exponent ``e``, ``rank + 1 <= d_u ** e``, exactly when ``x[i] <= e``.  ``y`` = the
    minimum of ``x`` over the columns of an unordered pair, ``local = 1 - y`` in [0, 1];
    1.0 is some end's best edge.

    Returns ``(local, rank, info)``, ``info`` holding ``max_degree`` and ``n_top`` (columns
    with ``local == 1.0``).  ValueError for fewer scores than columns or an id outside
    ``[0, num_nodes)``."""
    ei = np.asarray(edge_index)
    src, dst = ei[0].astype(np.int64), ei[1].astype(np.int64)
    E = len(src)
    if len(scores) < E:
        raise ValueError(f"{len(scores)} scores for {E} columns: the canonical CSR "
                         "merged duplicate columns, one score per edge_index column is needed")
    if E and (min(src.min(), dst.min()) < 0 or max(src.max(), dst.max()) >= num_nodes):
        raise ValueError(f"edge_index id out of range [0, {num_nodes})")
    s = np.asarray(scores, dtype=np.float64)[:E]
    order = np.lexsort((np.arange(E), np.where(s == 0, 0.0, s)))  # ascending (score, index), NaN last
    if not keep_lowest:
        order = order[::-1]  # best first
    by = order[np.argsort(src[order], kind="stable")]
    deg = np.bincount(src, minlength=num_nodes)
    off = np.concatenate([[0], np.cumsum(deg)])
    rank = np.empty(E, dtype=np.int64)
    rank[by] = np.arange(E) - off[src[by]]
    max_deg = int(deg.max()) if E else 0
    table = np.log(np.maximum(np.arange(max(max_deg, 1) + 1), 1).astype(np.float64))
    x = np.zeros(E)
    nz = rank > 0
    x[nz] = table[rank[nz] + 1] / table[deg[src][nz]]
    inv = np.unique(np.minimum(src, dst) * (num_nodes + 1) + np.maximum(src, dst),
                    return_inverse=True)[1].reshape(-1)
    y = np.full(int(inv.max()) + 1 if E else 0, np.inf)
    np.minimum.at(y, inv, x)
    local = 1.0 - y[inv]
    return local, rank, {"max_degree": max_deg, "n_top": int((local == 1.0).sum())}


def local_mask(local, exponent: float):
    """The local sparsifier's mask at ``exponent`` in [0, 1]: ``local >= 1.0 - exponent``
    (that expression is the definition).  Every node keeps its ``ceil(d ** exponent)`` best
    columns and a column survives when either end keeps its pair: 1 keeps everything, 0
    every node's best edge in both directions."""
    if not 0 <= exponent <= 1:
        raise ValueError(f"exponent must be in [0, 1], got {exponent}")
    return local >= 1.0 - exponent


def local_mask_device(engine, scores, edge_index, num_nodes: int, exponent: float,
                      keep_lowest: bool = False, info: dict | None = None):
    """``local_mask(local_filter_scores(...)[0], exponent)`` on the MI355X
    (Engine.local_scores); the same mask.  ``edge_index``: a numpy array or a CUDA tensor
    (the mask then is one too).

    ``info`` (optional dict) receives ``path`` ("device"), ``exponent``, ``kept``,
    ``n_top``, ``max_degree`` and ``classes``."""
    if info is None:
        info = {}
    if not 0 <= exponent <= 1:
        raise ValueError(f"exponent must be in [0, 1], got {exponent}")
    if len(scores) < edge_index.shape[1]:
        raise ValueError(f"{len(scores)} scores for {edge_index.shape[1]} columns: the canonical CSR "
                         "merged duplicate columns, one score per edge_index column is needed")
    local, f = engine.local_scores(scores, edge_index[0], edge_index[1], num_nodes, keep_lowest)
    mask = local_mask(local, exponent)
    info.update(path="device", exponent=float(exponent), kept=int(mask.sum()), n_top=f["n_top"],
                max_degree=f["max_degree"], classes=f["classes"])
    return mask


SPECTRAL_METHODS =("multinomial", "independent")


def spectral_sample(scores, edge_index, num_nodes, num_samples, seed=42, method="multinomial"):
    """Spectral sparsification by effective-resistance sampling (Spielman-Srivastava): the
    executable specification of gs_spectral_sample and its host form.

    ``num_samples`` draws over the undirected pairs of ``edge_index`` with probability
    proportional to the pair's score -- for a unit-weight graph scored by an effective
    resistance, ``w_e R_e`` -- and a kept pair is given the weight ``count / (q p)``, so
    the weighted subgraph's Laplacian is an unbiased estimate of the whole graph's.  A
    pair takes the score of its lowest column (the two directions need not agree);
    loops and scores that are NaN, infinite or <= 0 are never drawn.  ``method``:
    "multinomial" is ``rng.choice(m, q, replace=True, p=p)`` written out (cumsum, divide,
    a right-sided search of ``rng.random(q)``); "independent" keeps every pair on its
    own with probability ``min(1, q p)`` and the weight ``1 / min(1, q p)`` (no cumsum;
    the expected number of kept pairs is at most q).

    Returns ``(mask[E], weight[E], counts[m], inverse[E])``: the kept columns, their
    float64 weights (0 where dropped), the draws per pair and every column's pair id.
    ValueError for fewer scores than columns, a total that is not finite and positive,
    ``num_samples`` outside [1, 2^31) and an unknown method."""
    if method not in SPECTRAL_METHODS:
        raise ValueError(f"method must be one of {SPECTRAL_METHODS}, got {method!r}")
    ei = np.asarray(edge_index)
    src, dst = ei[0].astype(np.int64, copy=False), ei[1].astype(np.int64, copy=False)
    E = len(src)
    q = int(num_samples)
    scores = np.asarray(scores, dtype=np.float64)
    if len(scores) < E:
        raise ValueError(f"{len(scores)} scores for {E} columns: one score per edge_index column "
                         "is needed")
    keys = np.minimum(src, dst) * (num_nodes + 1) + np.maximum(src, dst)
    inv = np.unique(keys, return_inverse=True)[1]  # random.py:23-30
    m = int(inv.max()) + 1
    first = np.full(m, E)
    np.minimum.at(first, inv, np.arange(E))  # a pair's lowest column
    r = scores[first]
    ok = np.isfinite(r) & (r > 0) & (src[first] != dst[first])  # loops, NaN, inf, <= 0: p = 0
    r = np.where(ok, r, 0.0)
    with np.errstate(all="ignore"):
        total = np.sum(r)  # NumPy's blocked pairwise sum, as gs_sample_probs
    if not (np.isfinite(total) and total > 0):
        raise ValueError(f"the scores of the {m} undirected pairs sum to {total}: a finite "
                         "positive total is needed")
    if not 1 <= q < 2**31:
        raise ValueError(f"num_samples must be in [1, 2^31), got {q}")
    p = r / total
    rng = np.random.default_rng(seed)
    w = np.zeros(m)
    if method == "multinomial":  # == rng.choice(m, size=q, replace=True, p=p)
        cdf = np.cumsum(p)
        cdf /= cdf[-1]
        idx = cdf.searchsorted(rng.random(q), side="right")
        cnt = np.bincount(idx, minlength=m)
        k = cnt > 0
        w[k] = cnt[k] / (q * p[k])  # fl(q*p) then one IEEE divide
    else:  # every pair on its own, no cumsum
        pk = np.minimum(1.0, q * p)
        k = rng.random(m) < pk
        cnt = k.astype(np.int64)
        w[k] = 1.0 / pk[k]
    return cnt[inv] > 0, w[inv], cnt, inv


def spectral_num_samples(num_samples=None, retention_ratio=None, m=None):
    """The draw count of ``sparsify_spectral``: ``num_samples`` itself, or
    ``max(1, int(m * retention_ratio))`` over the ``m`` undirected pairs (None while ``m``
    is not known yet).  ValueError unless exactly one of the two is given, and for a
    ratio outside (0, 1]."""
    if (num_samples is None) == (retention_ratio is None):
        raise ValueError("give exactly one of num_samples and retention_ratio")
    if num_samples is not None:
        return int(num_samples)
    if not 0 < retention_ratio <= 1:
        raise ValueError(f"retention_ratio must be in (0, 1], got {retention_ratio}")
    return None if m is None else max(1, int(m * retention_ratio))


def spectral_mask_device(engine, scores, edge_index, num_nodes: int, num_samples: int,
                         seed: int = 42, method: str = "multinomial", info: dict | None = None):
    """spectral_sample on the MI355X (gs_spectral_sample): the same mask, weights, counts
    and ids, bit for bit.  ``scores`` and ``edge_index`` are numpy arrays or CUDA tensors;
    the results live where ``edge_index`` does.

    Degenerate inputs (ids outside gs_undirected_ids' contract, fewer scores than
    columns, a total that is not finite and positive, ``num_samples`` outside
    [1, 2^31)) are reported by the device and handed to spectral_sample, so its
    exception surfaces.

    ``info`` (optional dict) receives ``path`` ("device" or "host"), ``method``, ``m``
    (undirected pairs), ``num_samples``, ``kept_pairs``, ``max_count``, ``draws``
    (doubles of the PCG64 stream consumed) and ``n_irregular`` (non-loop pairs that do
    not have exactly two columns)."""
    if info is None:
        info = {}
    if method not in SPECTRAL_METHODS:
        raise ValueError(f"method must be one of {SPECTRAL_METHODS}, got {method!r}")
    q = int(num_samples)
    rng = np.random.default_rng(seed)
    mask, weight, counts, inverse, st = engine.spectral_sample(
        scores, edge_index[0], edge_index[1], num_nodes, q, rng, method)
    if st["status"] != 0:
        to_np = lambda a: a if isinstance(a, np.ndarray) else a.detach().cpu().numpy()  # noqa: E731
        ei = np.stack([to_np(edge_index[0]), to_np(edge_index[1])])
        mask, weight, counts, inverse = spectral_sample(to_np(scores), ei, num_nodes, q, seed, method)
        src, dst = ei
        ncol = np.bincount(inverse, minlength=len(counts))
        first = np.full(len(counts), len(src))
        np.minimum.at(first, inverse, np.arange(len(src)))
        info.update(path="host", method=method, m=len(counts), num_samples=q,
                    kept_pairs=int((counts > 0).sum()), max_count=int(counts.max()),
                    draws=q if method == "multinomial" else len(counts),
                    n_irregular=int(((ncol != 2) & (src[first] != dst[first])).sum()))
        return mask, weight, counts, inverse
    info.update(path="device", method=method, m=st["m"], num_samples=q, kept_pairs=st["kept_pairs"],
                max_count=st["max_count"], draws=st["draws"], n_irregular=st["n_irregular"])
    return mask, weight, counts, inverse


def numpy_topk_mask(scores: np.ndarray, num_edges: int, num_keep: int,
                    keep_lowest: bool) -> np.ndarray:
    """core.py:233-240 verbatim: the reference's unstable argsort tie order."""
    idx = np.argsort(scores)
    sel = idx[:num_keep] if keep_lowest else idx[-num_keep:]
    mask = np.zeros(num_edges, dtype=bool)
    mask[sel] = True
    return mask
