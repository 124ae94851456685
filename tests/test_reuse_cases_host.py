"""The graph sequence of the context-reuse tests is the probe it is meant to be
(reuse_cases.py): G3 has G1's shape and degrees but other arrays and other results under
every reference the GPU walk compares with, G1 reaches the kernel classes a graph of its
size can, G5 is asymmetric with multiplicities.  No GPU."""

import numpy as np
import pytest

import gsparse_oracle as O
import reuse_cases as C


def test_sequence_and_shapes():
    assert C.SEQUENCE == ("G1", "G2", "G3", "G4", "G5", "G1")
    assert C.graph("G1")[0] == 2048 and C.graph("G2")[0] == 34
    assert C.graph("G4")[0] == 5 and C.graph("G4")[1].shape == (2, 0)
    assert len(C.csr("G4")[1]) == 0 and np.array_equal(C.csr("G4")[0], np.zeros(6, dtype=np.int64))
    for name in C.NAMES:  # read-only: a test cannot change what the next one compares with
        n, ei = C.graph(name)
        assert not ei.flags.writeable and all(not a.flags.writeable for a in C.csr(name))
        assert ei.dtype == np.int64 and (ei.size == 0 or (0 <= ei.min() and ei.max() < n))
    assert [C.symmetric(k) for k in C.NAMES] == [True, True, True, True, False]


def test_g3_is_g1_relabelled():
    (ip1, ix1, d1), (ip3, ix3, d3) = C.csr("G1"), C.csr("G3")
    assert C.graph("G3")[0] == C.graph("G1")[0]
    assert len(ix3) == len(ix1)
    assert np.array_equal(np.sort(np.diff(ip3)), np.sort(np.diff(ip1)))
    assert not np.array_equal(ix3, ix1) and not np.array_equal(ip3, ip1)
    assert np.array_equal(d1, np.ones(len(ix1))) and np.array_equal(d3, d1)
    # the permutation moves nearly every node, and G3's columns arrive in canonical order
    p = C.permutation()
    assert np.array_equal(np.sort(p), np.arange(2048)) and (p != np.arange(2048)).sum() > 2000
    e3 = C.graph("G3")[1]
    assert (np.diff(e3[0] * 2048 + e3[1]) > 0).all()
    # the same graph: entry (u, v) of G1 is entry (p[u], p[v]) of G3
    k1 = np.sort(p[C.rows_of("G1")] * 2048 + p[ix1])
    assert np.array_equal(k1, C.rows_of("G3") * 2048 + ix3)


GRAPH_FREE = ("topk", "sampled")  # gs_topk_mask and gs_sample_mask read the scores alone


@pytest.mark.parametrize("what", C.ENTRY_REFS + C.SYMMETRIC_REFS + C.NODE_REFS + C.COLUMN_REFS + C.SHARD_REFS)
def test_every_reference_tells_g3_from_g1(what):
    """Arrays in CSR (or column, or node) order: a result served from G1's cache fails on G3.
    G3 has G1's features and G1's per-column scores, so the graph alone makes the difference;
    the two selections that never look at the graph are the same on both, as they must be."""
    assert C.features("G3") is C.features("G1") or np.array_equal(C.features("G3"), C.features("G1"))
    assert np.array_equal(C.scores("G3"), C.scores("G1"))
    a, b = C.ref("G1", what), C.ref("G3", what)
    assert a.shape == b.shape and a.dtype == b.dtype
    if what in GRAPH_FREE:
        assert np.array_equal(a, b)
        return
    assert not np.array_equal(a, b)
    assert (a != b).mean() > 0.01, (what, (a != b).mean())  # not a handful of entries


def test_g2p_is_a_second_connected_graph_of_g2s_shape():
    """What the connected-only entry points see after G2: the same n and nnz, other arrays,
    another algebraic connectivity, other sparsifier weights and other bounds."""
    (ip2, ix2, _), (ipp, ixp, _) = C.csr("G2"), C.csr("G2P")
    assert C.graph("G2P")[0] == C.graph("G2")[0] and len(ixp) == len(ix2)
    assert C.symmetric("G2P") and C.topology("G2P")[1] == 1 and C.topology("G2")[1] == 1
    assert not np.array_equal(ixp, ix2) and not np.array_equal(ipp, ip2)
    (ac2, hw2, b2), (acp, hwp, bp) = C.connected_refs("G2"), C.connected_refs("G2P")
    assert abs(ac2 - acp) > 1e-3 * ac2  # far above the 1e-6 the device value is held to
    assert not np.array_equal(hw2, hwp)
    assert abs(b2[0] - bp[0]) > 1e-3 * b2[1]
    assert not np.array_equal(C.ref("G2", "exact_er"), C.ref("G2P", "exact_er"))


def test_scalar_references_cannot_tell_them_apart():
    """Component counts (and, up to summation order, the average clustering) are the same
    on G1 and G3 by construction: the walk compares the per-node arrays as well."""
    (c1, k1, b1), (c3, k3, b3) = C.topology("G1"), C.topology("G3")
    assert (k1, b1) == (k3, b3) and k1 > 1
    assert abs(c1 - c3) < 1e-12


def test_g1_reaches_the_classes_its_size_allows():
    ip, ix, _ = C.csr("G1")
    deg = np.diff(ip)
    # Jaccard owner classes (gs_jac.hpp): merge rows (<= 32) and the first hash class (<= 1024).
    # The next class starts at 1025 neighbours, half of n = 2048; R-MAT's largest hub at this
    # scale has a few hundred.
    cls = set(O._jac_class(deg[deg > 0]).tolist())
    assert cls == {-1, 0} and deg.max() > 512
    # segment ranks (gs_segrank.hip): empty, short (<= 64), lds (<= 8192); stream needs > 8192 > n
    n, ei = C.graph("G1")
    seg = np.bincount(ei[0], minlength=n)
    assert (seg == 0).any() and ((seg > 0) & (seg <= 64)).any() and (seg > 64).any()
    # Simmelian pair classes by the shorter neighbour list: wave (<= 64) and mid (<= 512)
    short = np.minimum(deg[C.rows_of("G1")], deg[ix])
    assert (short <= 64).any() and (short > 64).any()
    # trussness: several levels, more sub-rounds than levels (the tail and the wide rounds)
    t = C.ref("G1", "trussness")
    assert len(np.unique(t)) >= 8


def test_g5_is_directed_with_multiplicities():
    ip, ix, d = C.csr("G5")
    n, ei = C.graph("G5")
    assert not C.symmetric("G5")
    assert d.max() > 1 and ei.shape[1] > len(ix)
    assert (C.rows_of("G5") == ix).any()  # self-loops too


def test_scores_have_ties_and_zeros():
    for name in ("G1", "G2", "G3", "G5"):
        s = C.scores(name)
        assert len(s) == C.graph(name)[1].shape[1] and not s.flags.writeable
        assert len(np.unique(s)) <= 40 < len(s) and (s == 0).any()
