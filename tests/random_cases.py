"""Inputs and NumPy references shared by the random-baseline tests (test_random_host.py,
test_gpu_random.py).  Every expected value is NumPy's own, from the reference's lines
(random.py:23-30 and :45-49) run in the test process."""

import numpy as np
import torch

ID_SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4097]
# the id kernels launch grid_for(E, 256, 8192) blocks: one element per thread up to
# 8192 * 256 = 2^21 columns, a grid-stride loop past that
GRID_STRIDE_E = (1 << 21) + 3
NODE_COUNTS = [1, 2, 1000]
MASK_SIZES = [1, 2, 257, 70001]
RETENTIONS = [1e-9, 0.2, 0.5, 0.999, 1.0, 1.5]


def multigraph(E, n, seed):
    """E columns over n nodes: pairs in both directions, pairs in one direction only,
    duplicate columns and self-loops, in shuffled column order."""
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


def np_inverse(src, dst, n):
    """random.py:26-30."""
    u = np.minimum(src, dst)
    v = np.maximum(src, dst)
    keys = u.astype(np.int64) * (n + 1) + v.astype(np.int64)
    _, inverse_idx = np.unique(keys, return_inverse=True)
    return inverse_idx, int(inverse_idx.max()) + 1


def np_keep_mask(undirected_scores, inverse_idx, retention_ratio, kind=None):
    """random.py:45-49 (kind="stable": the project's own tie rule)."""
    n_undirected = len(undirected_scores)
    n_keep = max(1, int(n_undirected * retention_ratio))
    keep_undir = np.zeros(n_undirected, dtype=bool)
    order = np.argsort(undirected_scores) if kind is None else np.argsort(undirected_scores, kind=kind)
    keep_undir[order[-n_keep:]] = True
    return keep_undir[inverse_idx]


def mask_case(m, seed, crowded=False):
    """(scores[m], inverse[E], edge_index[2, E]) with every undirected id used by one or
    two columns and some ids by none; inverse partly written as negative (wrapping) ids."""
    rng = np.random.default_rng(seed)
    s = rng.random(m)
    if crowded:
        s = np.round(s, 2)
    E = 2 * m + 3
    inv = rng.integers(0, m, size=E).astype(np.int64)
    neg = rng.random(E) < 0.25
    inv[neg] -= m  # NumPy wraps [-m, 0)
    ei = np.stack([np.arange(E, dtype=np.int64), np.arange(E, dtype=np.int64)[::-1].copy()])
    return s, inv, ei


def golden_data(g, device=None):
    from gsparse import Data

    ei = torch.from_numpy(np.ascontiguousarray(g["edge_index"]))
    if device is not None:
        ei = ei.to(device)
    return Data(edge_index=ei, num_nodes=int(g["num_nodes"]))
