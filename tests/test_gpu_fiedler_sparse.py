"""The sparse form of the algebraic connectivity (gs_fiedler_sparse, and gs_fiedler above
32768 nodes): closed forms, the NetworkX oracle, the dense form below the limit, loud
failure at the iteration caps, and repeatability.

The tolerance is test_topology_metrics_vs_networkx's: rtol 1e-6, atol 1e-14."""

import ctypes
import functools
import hashlib
import json
import math
import os

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import gsparse_oracle as O
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-14


@pytest.fixture(scope="module")
def gs():
    import gsparse

    return gsparse


@pytest.fixture(scope="module")
def ctx():
    from gsparse._lib import Context

    return Context()


def close(got, want):
    print(f"got {got!r} want {want!r} rel {abs(got - want) / abs(want):.3e}")
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


def fiedler(gs, ctx, adj, **kw):
    """Engine.fiedler on adj as it is stored (a diagonal entry stays in the CSR)."""
    a = sp.csr_matrix(adj, dtype=np.float64)
    a.sort_indices()
    ctx.set_graph_csr(a.shape[0], a.indptr, a.indices, a.data)
    eng = gs.engine.Engine(ctx)
    return eng.fiedler(**kw), eng


def largest_component(adj):
    adj = sp.csr_matrix(adj)
    _, lab = connected_components(adj, directed=False)
    nodes = np.flatnonzero(lab == np.argmax(np.bincount(lab)))  # the first largest
    return adj[nodes][:, nodes].tocsr()


def golden_adj(name):
    g = load_golden(name)
    n = int(g["num_nodes"])
    return sp.csr_matrix((g["data"], g["indices"], g["indptr"]), shape=(n, n))


def weighted_components_loops():
    """test_gpu_parity._topology_cases' weighted case (components, self-loops), rebuilt."""
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
    return A


@functools.lru_cache(maxsize=None)
def connected_case(name):
    """(adjacency of the largest component, the oracle's algebraic connectivity)."""
    adj = weighted_components_loops() if name == "weighted_components_loops" else golden_adj(name)
    sub = largest_component(adj)
    return sub, O.topology_metrics(sub)["algebraic_connectivity"]


def sym(r, c, w, n):
    A = sp.coo_matrix((w, (r, c)), shape=(n, n)).tocsr()
    return (A + A.T).tocsr()


def star(leaves, w=1.0):
    return sym(np.zeros(leaves, dtype=np.int64), np.arange(1, leaves + 1), np.full(leaves, w),
               leaves + 1)


def cycle(n):
    i = np.arange(n)
    return sym(i, (i + 1) % n, np.ones(n), n)


def path(n, w=1.0):
    i = np.arange(n - 1)
    return sym(i, i + 1, np.full(n - 1, w), n)


# ---- 1. above the dense limit, closed form, one row of 70,000 entries
def test_star_70000_through_topology_metrics(gs):
    got = gs.compute_topology_metrics(star(70_000))
    assert got["num_nodes"] == 70_001 and got["num_edges"] == 70_000
    assert got["num_connected_components"] == 1 and got["largest_component_ratio"] == 1.0
    assert got["clustering_coefficient"] == 0.0
    close(got["algebraic_connectivity"], 1.0)


def test_weighted_star_70000_through_engine(gs, ctx):
    val, eng = fiedler(gs, ctx, star(70_000, 2.5))  # "auto": gs_fiedler dispatches
    assert eng.fiedler_iterations >= 1
    close(val, 2.5)
    val, eng = fiedler(gs, ctx, star(70_000, 2.5), method="sparse")
    assert eng.fiedler_cg_iterations >= 1
    close(val, 2.5)
    with pytest.raises(NotImplementedError):
        fiedler(gs, ctx, star(70_000, 2.5), method="dense")


# ---- 2. above the dense limit, a power-law graph
def test_rmat16_through_topology_metrics(gs):
    """NetworkX's tracemin_lu takes over two minutes on this component, so its value is a
    fixture (tests/golden/fiedler_rmat16.json, with the SHA-256 of the graph it is of)."""
    from gsparse import graphs

    with open(os.path.join(GOLDEN, "fiedler_rmat16.json")) as f:
        ref = json.load(f)
    ei = graphs.rmat(16, seed=0)
    assert hashlib.sha256(np.ascontiguousarray(ei, dtype=np.int64).tobytes()).hexdigest() == \
        str(ref["edge_index_sha256"])
    n = 1 << 16
    adj = sp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(n, n))
    got = gs.compute_topology_metrics(adj)
    assert round(got["largest_component_ratio"] * n) == 40_229 == int(ref["largest_component"])
    assert got["num_connected_components"] == int(ref["num_connected_components"])
    assert got["num_edges"] == int(ref["num_edges"])
    close(got["algebraic_connectivity"], float(ref["algebraic_connectivity"]))


# ---- 3. sparse against dense below the limit
@pytest.mark.parametrize("name", ["karate_test", "rmat10", "weighted_components_loops"])
def test_sparse_agrees_with_dense_and_oracle(gs, ctx, name):
    sub, ref = connected_case(name)
    dense, _ = fiedler(gs, ctx, sub, method="dense")
    sparse, eng = fiedler(gs, ctx, sub, method="sparse")
    print(name, sub.shape[0], "outer", eng.fiedler_iterations, "cg", eng.fiedler_cg_iterations)
    close(sparse, dense)
    close(sparse, ref)
    close(dense, ref)


# ---- 4. closed forms at the kernels' tails and tile boundaries
@pytest.mark.parametrize("n", [3, 63, 64, 65, 1023, 1024, 1025])
def test_cycle(gs, ctx, n):
    val, eng = fiedler(gs, ctx, cycle(n), method="sparse")
    print("outer", eng.fiedler_iterations, "cg", eng.fiedler_cg_iterations)
    close(val, 2.0 - 2.0 * math.cos(2.0 * math.pi / n))


@pytest.mark.parametrize("n", [2, 64, 257])
def test_path(gs, ctx, n):
    val, eng = fiedler(gs, ctx, path(n), method="sparse")
    print("outer", eng.fiedler_iterations, "cg", eng.fiedler_cg_iterations)
    close(val, 2.0 - 2.0 * math.cos(math.pi / n))


def test_complete_64(gs, ctx):
    A = sp.csr_matrix(np.ones((64, 64)) - np.eye(64))
    val, eng = fiedler(gs, ctx, A, method="sparse")
    print("outer", eng.fiedler_iterations, "cg", eng.fiedler_cg_iterations)
    close(val, 64.0)


@pytest.mark.parametrize("w", [1.0, 0.37, 2.5])
def test_single_edge(gs, ctx, w):
    val, _ = fiedler(gs, ctx, path(2, w), method="sparse")
    close(val, 2.0 * w)


# ---- 5. ill-conditioned, small: a chain with chords
ROMAN_CAPS = dict(max_iter=300, cg_max_iter=20_000)


def test_roman2000_sparse(gs, ctx):
    sub, ref = connected_case("roman2000")
    val, eng = fiedler(gs, ctx, sub, method="sparse", **ROMAN_CAPS)
    print("n", sub.shape[0], "outer", eng.fiedler_iterations, "cg", eng.fiedler_cg_iterations)
    close(val, ref)


# ---- 6. honest failure
def test_cap_is_an_error_not_a_value(gs, ctx):
    from gsparse._lib import GS_ENOCONV

    sub, _ = connected_case("roman2000")
    with pytest.raises(RuntimeError) as ei:
        fiedler(gs, ctx, sub, method="sparse", cg_max_iter=1)
    assert isinstance(ei.value, gs.GsparseNotConverged)
    assert "cg_max_iter=1" in str(ei.value) and "residual" in str(ei.value)
    # the graph is still resident: the same call through the ABI writes no value
    val, it, cg = ctypes.c_double(-7.5), ctypes.c_int32(-1), ctypes.c_int64(-1)
    rc = ctx._L.gs_fiedler_sparse(ctx.handle, 1e-12, 300, 1e-10, 1, ctypes.byref(val),
                                  ctypes.byref(it), ctypes.byref(cg))
    assert rc == GS_ENOCONV
    assert val.value == -7.5
    assert it.value == 0 and cg.value == 1
    # Lanczos at its own cap: two steps cannot settle this graph
    rc = ctx._L.gs_fiedler_sparse(ctx.handle, 1e-12, 2, 1e-10, 20_000, ctypes.byref(val),
                                  ctypes.byref(it), ctypes.byref(cg))
    assert rc == GS_ENOCONV
    assert val.value == -7.5 and it.value == 2


def test_topology_metrics_raises_at_the_cap(gs):
    """A path of 40,000 nodes: information moves one node per CG iteration, so no solve
    can finish within the 5000 iterations gs_fiedler allows above the dense limit."""
    with pytest.raises(RuntimeError, match="cg_max_iter=5000.*residual"):
        gs.compute_topology_metrics(path(40_000))


def test_two_components_and_directed(gs, ctx):
    from gsparse._lib import GS_EINVAL, GS_EUNSUPPORTED

    two = sp.block_diag([path(5), cycle(7)]).tocsr()
    with pytest.raises(ValueError):
        fiedler(gs, ctx, two, method="sparse")
    val = ctypes.c_double(-7.5)
    args = (1e-12, 300, 1e-10, 100, ctypes.byref(val), None, None)
    assert ctx._L.gs_fiedler_sparse(ctx.handle, *args) == GS_EINVAL
    directed = sp.csr_matrix(np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], dtype=np.float64))
    with pytest.raises(NotImplementedError):
        fiedler(gs, ctx, directed, method="sparse")
    assert ctx._L.gs_fiedler_sparse(ctx.handle, *args) == GS_EUNSUPPORTED
    assert val.value == -7.5
    with pytest.raises(ValueError):
        fiedler(gs, ctx, path(4), method="lu")


# ---- 7. repeatability
def test_two_calls_give_the_same_bits(gs, ctx):
    sub, _ = connected_case("rmat10")
    a, eng = fiedler(gs, ctx, sub, method="sparse")
    ia = (eng.fiedler_iterations, eng.fiedler_cg_iterations)
    b, eng = fiedler(gs, ctx, sub, method="sparse")
    assert np.float64(a).tobytes() == np.float64(b).tobytes()
    assert ia == (eng.fiedler_iterations, eng.fiedler_cg_iterations)
