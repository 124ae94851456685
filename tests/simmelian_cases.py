"""Shared inputs and references of the Simmelian backbone tests (test_simmelian_host.py,
test_gpu_simmelian.py): the trussness cases plus the graphs where the ordering of the
common neighbours' ranks, the last-of-ties choice or a ranked neighbourhood's size can go
wrong, their canonical CSR and the NumPy specification (selection.simmelian_host), each
computed once per case and rank and kept."""

import functools

import numpy as np
import scipy.sparse as sp

import truss_cases as T


def _two_hubs(commons, mod):
    """Hubs a = 0 and b = 1, adjacent, with the common neighbours w_i = 2 + i; w_i has
    i mod `mod` private nodes of its own that are adjacent to w_i and to a only: t(a, w_i)
    = 1 + i mod `mod` takes `mod` values with repeats, t(b, w_i) = 1 is constant, so the
    pair (a, b) has `commons` common neighbours with about `mod` distinct ranks."""
    i = np.arange(commons, dtype=np.int64)
    w = 2 + i
    owner = np.repeat(w, i % mod)
    priv = 2 + commons + np.arange(len(owner), dtype=np.int64)
    src = np.concatenate([[0], np.zeros(commons, dtype=np.int64), np.ones(commons, dtype=np.int64), owner,
                          np.zeros(len(priv), dtype=np.int64)])
    dst = np.concatenate([[1], w, w, priv, priv])
    n = 2 + commons + len(priv)
    return n, np.stack([np.concatenate([src, dst]), np.concatenate([dst, src])])


def _build():
    cases = dict(T.CASES)

    def add(name, n, ei):
        ei = np.ascontiguousarray(np.asarray(ei, dtype=np.int64).reshape(2, -1))
        ei.setflags(write=False)
        cases[name] = (n, ei)

    add("K4_minus_edge", 4, T.both([e for e in T.clique(range(4)) if e != (2, 3)]))
    add("bowtie", 5, T.both(T.clique((0, 1, 2)) + T.clique((2, 3, 4))))
    add("two_hubs_300", *_two_hubs(300, 13))  # small enough for the brute force
    add("two_hubs_graded", *_two_hubs(3000, 97))
    add("two_hubs_9000", *_two_hubs(9000, 13))  # past the LDS class without a knob
    return cases


CASES = _build()
NAMES = tuple(CASES)
BRUTE_MAX_ENTRIES = 13000


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
    ip, ix = csr(name)
    n = len(ip) - 1
    rows = rows_of(name)
    return np.searchsorted(rows * n + ix, ix.astype(np.int64) * n + rows)


def max_degree(name):
    ip, _ = csr(name)
    return int(np.diff(ip).max()) if len(ip) > 1 else 0


@functools.lru_cache(maxsize=None)
def prepared(name):
    from gsparse.selection import simmelian_prepare

    return simmelian_prepare(*csr(name))


@functools.lru_cache(maxsize=None)
def expected(name, max_rank=0):
    """(score float64, num int64, den int64) per CSR entry by the NumPy specification."""
    from gsparse.selection import simmelian_host

    out = simmelian_host(*csr(name), max_rank=max_rank, prep=prepared(name))
    for x in out:
        x.setflags(write=False)
    return out


def max_common(name):
    p = prepared(name)
    return int(p["c"].max()) if len(p["c"]) else 0


def relabelled(name, seed=0):
    """The case under a random node permutation: (indptr, indices, position of every
    entry of the original CSR in the new one)."""
    ip, ix = csr(name)
    n = len(ip) - 1
    perm = np.random.default_rng(seed).permutation(n)
    rows = rows_of(name)
    r2, c2 = perm[rows], perm[ix]
    a = sp.csr_matrix((np.ones(len(ix)), (r2, c2)), shape=(n, n))
    a.sort_indices()
    ip2, ix2 = a.indptr.astype(np.int64), a.indices.astype(np.int32)
    rows2 = np.repeat(np.arange(n, dtype=np.int64), np.diff(ip2))
    pos = np.searchsorted(rows2 * n + ix2, r2 * n + c2)
    return ip2, ix2, pos
