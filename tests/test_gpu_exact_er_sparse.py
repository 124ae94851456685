"""The sparse form of the exact effective resistance (gs_exact_er_sparse, and gs_exact_er
above 32768 nodes): closed forms and Foster's theorem above the dense limit, the lifted
oracle below it at every batch width, the dense form, symmetry, repeatability, and loud
failure at the iteration cap.

The expected values come from the lifted oracle (O.exact_er(lifted=True)) or from closed
forms.  The tolerance is the dense form's own (test_gpu_parity.test_exact_er_device):
rtol 1e-8, atol 1e-12."""

import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gsparse_oracle as O
from conftest import bits_equal, load_golden

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-8, 1e-12
LEAVES, STAR_W = 35_000, 2.5


@pytest.fixture(scope="module")
def gs():
    import gsparse

    return gsparse


def engine(gs, A):
    from gsparse._lib import Context

    ctx = Context()
    ctx.set_graph_csr(A.shape[0], A.indptr, A.indices, A.data)
    return gs.engine.Engine(ctx)


def worst(got, want):
    rel = float(np.max(np.abs(got - want) / np.abs(want), initial=0.0))
    print(f"entries {len(want)} worst relative error {rel:.3e}")
    return rel


def foster(A, scores):
    """(sum of w_e R_e over the undirected edges, n - components)."""
    from scipy.sparse.csgraph import connected_components

    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    up = rows < A.indices
    ncomp, _ = connected_components(A, directed=False)
    return float(np.sum(A.data[up] * scores[up])), A.shape[0] - ncomp


# ---- the graphs, each built once and left unchanged
@functools.lru_cache(maxsize=None)
def double_star():
    """Hubs 0 and 1 joined by an edge, 35,000 leaves each, every weight 2.5: n = 70,002,
    both hubs have 35,001 entries, the tie grounds hub 0 and hub 1's row is split."""
    n = 2 + 2 * LEAVES
    a = np.concatenate([[0], np.zeros(LEAVES, dtype=np.int64), np.ones(LEAVES, dtype=np.int64)])
    b = np.concatenate([[1], np.arange(2, 2 + LEAVES), np.arange(2 + LEAVES, n)])
    A = sp.coo_matrix((np.full(len(a), STAR_W), (a, b)), shape=(n, n)).tocsr()
    A = (A + A.T).tocsr()
    A.sort_indices()
    return A


def parts_graph(n, blocks):
    """test_gpu_parity._xer_parts_graph's recipe: `blocks` connected weighted parts over
    nodes [0, n - 3), the last three nodes isolated."""
    rng = np.random.default_rng(n)
    parts = np.array_split(np.arange(n - 3), blocks)
    rows, cols = [], []
    for p in parts:
        m = len(p)
        a = rng.integers(0, m, 4 * m)
        b = rng.integers(0, m, 4 * m)
        keep = a != b
        rows.append(p[a[keep]]), cols.append(p[b[keep]])
        rows.append(p[:-1]), cols.append(p[1:])  # a path keeps each part connected
    r = np.concatenate(rows)
    c = np.concatenate(cols)
    w = rng.uniform(0.5, 2.0, len(r))
    A = sp.coo_matrix((w, (r, c)), shape=(n, n)).tocsr()
    A = (A + A.T).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A, parts


@functools.lru_cache(maxsize=None)
def many_parts():
    """n = 38,403 in 600 parts of 64 nodes and three isolated nodes; the expected scores
    from the lifted oracle on each part's own submatrix, in the CSR order of the whole
    (a part's rows are consecutive and hold its own columns only)."""
    A, parts = parts_graph(38_403, 600)
    want = []
    for p in parts:
        sub = A[p[0]:p[-1] + 1, p[0]:p[-1] + 1].tocsr()
        sub.sort_indices()
        want.append(O.exact_er(sub.indptr, sub.indices, sub.data, len(p), lifted=True))
    want = np.concatenate(want)
    assert want.shape == A.data.shape
    want.setflags(write=False)
    return A, want


def golden_csr(name):
    g = load_golden(name)
    n = int(g["num_nodes"])
    A = sp.csr_matrix((g["data"].astype(np.float64), g["indices"], g["indptr"]), shape=(n, n))
    A.sort_indices()
    return A


SHAPES = ["parts-70-3", "parts-300-2", "parts-3000-5", "karate_test", "rmat10", "cora_like",
          "roman2000"]


@functools.lru_cache(maxsize=None)
def small_case(name):
    """(graph, the lifted oracle's scores), computed once per shape and left unchanged."""
    if name.startswith("parts-"):
        _, n, blocks = name.split("-")
        A, _ = parts_graph(int(n), int(blocks))
    else:
        A = golden_csr(name)
    want = O.exact_er(A.indptr, A.indices, A.data, A.shape[0], lifted=True)
    want.setflags(write=False)
    return A, want


@functools.lru_cache(maxsize=None)
def star_scores_sparse():
    """The double star through Engine.exact_er(method="sparse"): (scores, batches, CG
    iterations), computed once."""
    import gsparse

    eng = engine(gsparse, double_star())
    er = eng.exact_er(method="sparse")
    er.setflags(write=False)
    return er, eng.exact_er_iterations, eng.exact_er_cg_iterations


# ---- 1. above the dense limit, closed form, a row of 35,001 entries that is not the ground
def test_double_star_through_metrics(gs):
    A = double_star()
    assert A.shape[0] == 70_002 and np.diff(A.indptr)[:2].tolist() == [35_001, 35_001]
    er = gs.calculate_effective_resistance_scores(A)  # gs_exact_er dispatches
    assert er.dtype == np.float64 and er.shape == A.data.shape
    worst(er, np.full(len(er), 1.0 / STAR_W))
    np.testing.assert_allclose(er, 1.0 / STAR_W, rtol=RTOL, atol=ATOL)


def test_double_star_through_sparsifier(gs):
    """An edge_index carries no weights: the sparsifier's adjacency is the double star
    with unit weights, and the closed form is R = 1 / 1 on every edge."""
    A = double_star().tocoo()
    ei = np.stack([A.row, A.col]).astype(np.int64)
    data = gs.Data(edge_index=torch.from_numpy(ei), x=None, num_nodes=A.shape[0])
    sp_ = gs.GraphSparsifier(data, "cpu")
    er = sp_.compute_scores("effective_resistance")
    assert er.shape == (ei.shape[1],)
    worst(er, np.ones(len(er)))
    np.testing.assert_allclose(er, 1.0, rtol=RTOL, atol=ATOL)
    E = ei.shape[1]
    _, m = sp_.sparsify("effective_resistance", 0.5, return_mask=True)
    assert int(m.sum()) == int(E / 2)


def test_double_star_iterations_and_foster():
    """Grounded and Jacobi-scaled, the double star has three distinct eigenvalues: a solve
    ends within 4 iterations."""
    A = double_star()
    er, batches, cg = star_scores_sparse()
    columns = A.shape[0] - 1  # one component, one ground
    print("batches", batches, "cg iterations", cg, "columns", columns)
    np.testing.assert_allclose(er, 1.0 / STAR_W, rtol=RTOL, atol=ATOL)
    assert batches >= 1 and 0 < cg <= 4 * columns
    got, want = foster(A, er)
    print(f"foster {got!r} want {want}")
    np.testing.assert_allclose(got, want, rtol=1e-9)


# ---- 2. above the dense limit: many components, weights, isolated nodes
def test_many_parts_against_the_oracle(gs):
    A, want = many_parts()
    eng = engine(gs, A)
    er = eng.exact_er()  # "auto": gs_exact_er dispatches, and reports the batches
    print("batches", eng.exact_er_iterations)
    assert eng.exact_er_iterations >= 1 and eng.exact_er_cg_iterations is None
    worst(er, want)
    np.testing.assert_allclose(er, want, rtol=RTOL, atol=ATOL)
    got, expect = foster(A, er)
    print(f"foster {got!r} want {expect}")
    assert expect == 38_403 - 603
    np.testing.assert_allclose(got, expect, rtol=1e-9)
    with pytest.raises(NotImplementedError):
        eng.exact_er(method="dense")


# ---- 3. below the limit, the kernel at its awkward shapes, every batch width
@pytest.mark.parametrize("name", SHAPES)
def test_sparse_against_the_oracle_at_every_batch_width(gs, monkeypatch, name):
    """GSPARSE_XER_BATCH 64, 128 and the default: one partial batch (n = 70), a last batch
    that is not full, more than one 64-column group per batch -- and the same bits from
    every width."""
    A, want = small_case(name)
    outs = {}
    for batch in ("64", "128", None):
        if batch is None:
            monkeypatch.delenv("GSPARSE_XER_BATCH", raising=False)
        else:
            monkeypatch.setenv("GSPARSE_XER_BATCH", batch)
        eng = engine(gs, A)
        er = eng.exact_er(method="sparse")
        print(name, "B", batch or gs.engine.xer_sparse_plan(A.shape[0])["batch"], "batches",
              eng.exact_er_iterations, "cg", eng.exact_er_cg_iterations)
        worst(er, want)
        np.testing.assert_allclose(er, want, rtol=RTOL, atol=ATOL)
        assert eng.exact_er_iterations >= 1 and eng.exact_er_cg_iterations >= 1
        outs[batch] = er
    assert bits_equal(outs["64"], outs["128"])
    assert bits_equal(outs["64"], outs[None])


# ---- 4. symmetry and repeatability
def test_transposed_entries_equal_bit_for_bit_and_two_calls_agree(gs):
    A, _ = small_case("rmat10")
    pos = sp.csr_matrix((np.arange(A.nnz, dtype=np.float64) + 1.0, A.indices, A.indptr),
                        shape=A.shape)
    T = pos.T.tocsr()
    T.sort_indices()
    assert np.array_equal(T.indices, A.indices)
    tpos = T.data.astype(np.int64) - 1
    eng = engine(gs, A)
    a = eng.exact_er(method="sparse")
    ia = (eng.exact_er_iterations, eng.exact_er_cg_iterations)
    assert bits_equal(a, a[tpos])
    b = eng.exact_er(method="sparse")
    assert bits_equal(a, b)
    assert ia == (eng.exact_er_iterations, eng.exact_er_cg_iterations)


# ---- 5. sparse against dense
def test_sparse_agrees_with_dense(gs):
    A, _ = small_case("cora_like")
    eng = engine(gs, A)
    dense = eng.exact_er(method="dense")
    assert eng.exact_er_cg_iterations is None
    sparse = eng.exact_er(method="sparse")
    worst(sparse, dense)
    np.testing.assert_allclose(sparse, dense, rtol=RTOL, atol=ATOL)


def test_default_below_the_limit_is_the_dense_form(gs):
    A, want = small_case("parts-300-2")
    eng = engine(gs, A)
    er = eng.exact_er()
    assert eng.exact_er_cg_iterations is None
    assert eng.exact_er_iterations == 320 // 64  # N = 300 padded to 320
    np.testing.assert_allclose(er, want, rtol=RTOL, atol=ATOL)


# ---- 7. failure is loud
def path(n):
    i = np.arange(n - 1)
    A = sp.coo_matrix((np.ones(n - 1), (i, i + 1)), shape=(n, n)).tocsr()
    A = (A + A.T).tocsr()
    A.sort_indices()
    return A


def test_cap_is_an_error_not_a_value(gs):
    from gsparse._lib import GS_ENOCONV, GS_HOST, ptr

    A = path(300)
    eng = engine(gs, A)
    out = np.full(A.nnz, -7.5)
    with pytest.raises(RuntimeError) as ei:
        eng.exact_er(out=out, method="sparse", cg_max_iter=5)
    assert isinstance(ei.value, gs.GsparseNotConverged)
    msg = str(ei.value)
    print(msg)
    assert "batch 0" in msg and "cg_max_iter=5" in msg and "columns open" in msg
    assert "residual" in msg and "CG iterations" in msg
    assert np.all(out == -7.5)
    assert eng.exact_er_iterations == 0 and eng.exact_er_cg_iterations >= 5
    # the graph is still resident: the same call through the ABI
    b, cg = ctypes.c_int32(-1), ctypes.c_int64(-1)
    ctx = eng.ctx
    rc = ctx._L.gs_exact_er_sparse(ctx.handle, ptr(out), GS_HOST, 1e-12, 5, ctypes.byref(b),
                                   ctypes.byref(cg))
    assert rc == GS_ENOCONV
    assert np.all(out == -7.5) and b.value == 0 and cg.value >= 5
    # and with room to converge (298 free nodes in a chain: 298 iterations in exact arithmetic)
    er = eng.exact_er(out=out, method="sparse", cg_max_iter=1000)
    np.testing.assert_allclose(er, 1.0, rtol=RTOL, atol=ATOL)


def test_bad_arguments_and_unsupported_graphs(gs):
    from gsparse._lib import GS_EINVAL, GS_EUNSUPPORTED, GS_HOST, ptr

    eng = engine(gs, path(10))
    ctx = eng.ctx
    out = np.full(18, -7.5)
    for rtol, cap in ((0.0, 10), (1.0, 10), (-1e-3, 10), (1e-12, 0)):
        assert ctx._L.gs_exact_er_sparse(ctx.handle, ptr(out), GS_HOST, rtol, cap, None,
                                         None) == GS_EINVAL
        with pytest.raises(ValueError):
            eng.exact_er(method="sparse", cg_rtol=rtol, cg_max_iter=cap)
    with pytest.raises(ValueError):
        eng.exact_er(method="lu")
    directed = sp.csr_matrix(np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], dtype=np.float64))
    lopsided = sp.csr_matrix(np.array([[0, 1.0], [2.0, 0]]))
    for A in (directed, lopsided):
        eng = engine(gs, A)
        with pytest.raises(NotImplementedError):
            eng.exact_er(method="sparse")
        assert eng.ctx._L.gs_exact_er_sparse(eng.ctx.handle, ptr(out), GS_HOST, 1e-12, 100, None,
                                             None) == GS_EUNSUPPORTED
    assert np.all(out == -7.5)


def test_empty_graph(gs):
    eng = engine(gs, sp.csr_matrix((5, 5), dtype=np.float64))
    er = eng.exact_er(method="sparse")
    assert er.shape == (0,)
    assert eng.exact_er_iterations == 0 and eng.exact_er_cg_iterations == 0
