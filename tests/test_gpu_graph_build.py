"""How a graph gets onto a context, and what a refused one leaves behind.

* gs_graph_from_edge_index against SciPy's ``csr_matrix((ones, (s, d)))`` with duplicates
  summed and indices sorted (indptr, indices, data and shape for equality), at the sizes
  where the sort, the head flags and the compaction can go wrong -- E = 1, one node, every
  column the same, E around a block (255 / 256 / 257), and E = 8192 * 256 + 257, the first
  size at which the grid-stride loops of k_make_keys, k_head_flags and k_compact_unique take
  a second trip (reference there: np.unique on the keys) -- from host arrays and from CUDA
  tensors.
* the ``symmetric`` flag against ``(P != P.T).nnz == 0`` on the 0/1 pattern.
* gs_coalesce_edges at the same E boundaries, against the oracle's restatement.
* gs_graph_from_csr's refusals, each with the error include/gsparse.h documents, and the
  state after a refusal from either entry point: the empty graph (``shape()[:2] == (0, 0)``
  is asserted before any scorer runs, so against a library that kept a half-set graph the
  test stops there and launches nothing on it), then a valid graph that scores bit for bit.

A negative indptr entry is refused by the same bound as an overshooting one (k_check_csr
compares both ends of a row with [0, nnz] before it forms any idx[e]); it has no test here
on purpose: a kernel without that bound would read in front of the index buffer.  That case
is checked by reading csrc/gs_graph.hip."""

import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gsparse_oracle as O
from conftest import bits_equal

pytestmark = pytest.mark.gpu

GRID_CAP = 8192 * 256  # elements one trip of the edge kernels' grid covers
BIG_E, BIG_N = GRID_CAP + 257, 1000


@pytest.fixture(scope="module")
def ctx():
    from gsparse._lib import Context

    c = Context(0)
    yield c
    c.close()


def scipy_csr(n, s, d):
    a = sp.csr_matrix((np.ones(len(s)), (s, d)), shape=(n, n))
    a.sum_duplicates()
    a.sort_indices()
    return a.indptr.astype(np.int64), a.indices.astype(np.int32), a.data.astype(np.float64)


def _i64(*rows):
    return tuple(np.asarray(r, dtype=np.int64) for r in rows)


def _cases():
    rng = np.random.default_rng(31)
    c = {
        "E1": (3, *_i64([2], [0])),
        "one_node_loops": (1, *_i64([0, 0, 0], [0, 0, 0])),
        "loops_and_dups": (6, *_i64([0, 0, 0, 3, 3, 5, 5, 5, 2, 2], [0, 0, 1, 3, 4, 5, 5, 5, 1, 1])),
        "isolated_ends": (9, *_i64([3, 4, 4, 5], [4, 3, 5, 4])),  # nodes 0..2 and 6..8 have no entry
        "empty": (5, *_i64([], [])),
    }
    for E in (63, 64, 65, 257):
        c[f"same_column_{E}"] = (7, np.full(E, 4, dtype=np.int64), np.full(E, 2, dtype=np.int64))
    for E in (255, 256, 257):
        c[f"E{E}"] = (40, rng.integers(0, 40, E), rng.integers(0, 40, E))
    return c


CASES = _cases()


def _put(ctx, n, s, d, where):
    if where == "cuda":
        s, d = torch.from_numpy(np.ascontiguousarray(s)).cuda(), torch.from_numpy(np.ascontiguousarray(d)).cuda()
    ctx.set_graph_edge_index(n, s, d)


@pytest.mark.parametrize("where", ["host", "cuda"])
@pytest.mark.parametrize("name", list(CASES))
def test_edge_index_equals_scipy(ctx, name, where):
    n, s, d = CASES[name]
    _put(ctx, n, s, d, where)
    ip, ix, dat = scipy_csr(n, s, d)
    gip, gix, gd = ctx.csr()
    assert ctx.shape()[:2] == (n, len(ix))
    assert np.array_equal(gip, ip) and np.array_equal(gix, ix) and bits_equal(gd, dat)
    if name.startswith("same_column_"):
        assert len(gix) == 1 and gd[0] == len(s)


@pytest.fixture(scope="module")
def big():
    """E = GRID_CAP + 257 columns over n = 1000 nodes; np.unique on the keys is the reference.
    The last 257 columns (the second trip) hold keys found nowhere else."""
    rng = np.random.default_rng(8)
    s, d = rng.integers(0, BIG_N - 1, BIG_E), rng.integers(0, BIG_N, BIG_E)
    s[GRID_CAP:] = BIG_N - 1  # row 999 only in the tail
    d[GRID_CAP:] = rng.integers(0, BIG_N, 257)
    keys, counts = np.unique(s * BIG_N + d, return_counts=True)
    ip = np.zeros(BIG_N + 1, dtype=np.int64)
    np.cumsum(np.bincount(keys // BIG_N, minlength=BIG_N), out=ip[1:])
    assert ip[-1] - ip[-2] == len(np.unique(d[GRID_CAP:])) > 200
    return s, d, ip, (keys % BIG_N).astype(np.int32), counts.astype(np.float64)


@pytest.mark.parametrize("where", ["host", "cuda"])
def test_edge_index_past_one_grid_trip(ctx, big, where):
    s, d, ip, ix, dat = big
    _put(ctx, BIG_N, s, d, where)
    gip, gix, gd = ctx.csr()
    assert ctx.shape()[:2] == (BIG_N, len(ix))
    assert np.array_equal(gip, ip) and np.array_equal(gix, ix) and bits_equal(gd, dat)


SYM = {
    "symmetric": (5, [0, 1, 1, 2, 4, 3], [1, 0, 2, 1, 3, 4]),
    "one_reverse_missing": (5, [0, 1, 1, 2, 4], [1, 0, 2, 1, 3]),
    "only_loops": (4, [0, 2, 2, 3], [0, 2, 2, 3]),
    "empty": (5, [], []),
    "symmetric_pattern_other_multiplicities": (4, [0, 0, 0, 1, 2, 3, 3], [1, 1, 1, 0, 3, 2, 2]),
}


@pytest.mark.parametrize("name", list(SYM))
def test_symmetric_flag(ctx, name):
    n, s, d = SYM[name]
    s, d = _i64(s, d)
    ctx.set_graph_edge_index(n, s, d)
    ip, ix, dat = scipy_csr(n, s, d)
    P = sp.csr_matrix((np.ones(len(ix)), ix, ip), shape=(n, n))
    want = (P != P.T).nnz == 0
    assert want == (name != "one_reverse_missing")
    assert ctx.shape() == (n, len(ix), want)
    if name == "symmetric_pattern_other_multiplicities":
        gd = ctx.csr()[2]
        A = sp.csr_matrix((gd, ix, ip), shape=(n, n))
        assert (A != A.T).nnz > 0  # the weights are not symmetric, the pattern is


@pytest.mark.parametrize("undirected,loops", [(True, False), (False, True)])
@pytest.mark.parametrize("name", [k for k in CASES if k != "empty"])
def test_coalesce_at_the_same_sizes(ctx, name, undirected, loops):
    from gsparse.loader import coalesce_edges

    n, s, d = CASES[name]
    ei = np.stack([s, d])
    got = coalesce_edges(ei, n, undirected=undirected, remove_self_loops=loops, ctx=ctx)
    assert np.array_equal(got, O.coalesce(ei, n, undirected, loops))


def test_coalesce_past_one_grid_trip(ctx, big):
    """2E keys, device-resident ids and outputs: the same kernels' second trip."""
    from gsparse._lib import GS_DEVICE, ptr

    s, d = big[0], big[1]
    want = O.coalesce(np.stack([s, d]), BIG_N, True, True)
    ts, td = torch.from_numpy(s).cuda(), torch.from_numpy(d).cuda()
    os_, od = (torch.full((2 * BIG_E,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    m = ctypes.c_int64(2 * BIG_E)
    ctx.call("gs_coalesce_edges", BIG_N, BIG_E, ptr(ts), ptr(td), 1, 1, ptr(os_), ptr(od),
             ctypes.byref(m), GS_DEVICE)
    assert m.value == want.shape[1]
    assert np.array_equal(os_[: m.value].cpu().numpy(), want[0])
    assert np.array_equal(od[: m.value].cpu().numpy(), want[1])
    assert int(os_[m.value]) == -1 and int(od[m.value]) == -1


# ---- refusals -----------------------------------------------------------------------
def _valid():
    """(n, indptr, indices, data, jaccard): the graph set before and after every refusal."""
    from gsparse import graphs

    n = 300
    ip, ix, d = O.canonical_csr(graphs.roman_like(n, 420, seed=4), n)
    return n, ip, ix, d, O.jaccard(ip, ix)


VALID = None


def valid():
    global VALID
    if VALID is None:
        VALID = _valid()
    return VALID


# name -> (n, indptr, indices, exception, message)
BAD_CSR = {
    "unsorted_row": (3, [0, 2, 3, 4], [2, 1, 0, 1], NotImplementedError, "sorted"),
    "duplicate_column": (3, [0, 2, 3, 4], [1, 1, 0, 1], NotImplementedError, "duplicate"),
    "column_n": (3, [0, 2, 3, 4], [1, 3, 0, 1], ValueError, "out of range"),
    "column_minus_1": (3, [0, 2, 3, 4], [-1, 1, 0, 1], ValueError, "out of range"),
    "indptr_not_monotone": (3, [0, 3, 2, 4], [0, 1, 2, 1], ValueError, "monotone"),
    "indptr_end_is_not_nnz": (3, [0, 1, 2, 3], [0, 1, 2, 1], ValueError, "nnz"),
    "indptr_starts_at_1": (2, [1, 1, 2], [0, 1], ValueError, r"indptr\[0\]"),
    # overshoots in the middle: the entries a row [0, 7) would read lie inside the index padding
    "indptr_overshoots": (3, [0, 7, 3, 5], [0, 1, 2, 0, 1], ValueError, "monotone"),
}


def _after_refusal(ctx):
    """The empty graph first -- nothing runs on the context before that is known -- then an
    empty score vector, then a valid graph bit for bit."""
    from gsparse.engine import Engine

    assert ctx.shape()[:2] == (0, 0), "a refused graph call must leave the empty graph"
    eng = Engine(ctx)
    assert eng.jaccard().shape == (0,) and eng.degree().shape == (0,)
    gip, gix, gd = ctx.csr()
    assert np.array_equal(gip, [0]) and gix.shape == (0,) and gd.shape == (0,)
    n, ip, ix, d, jac = valid()
    ctx.set_graph_csr(n, ip, ix, d)
    eng = Engine(ctx)
    assert (eng.n, eng.nnz, eng.symmetric) == (n, len(ix), True)
    assert bits_equal(eng.jaccard(), jac)
    assert bits_equal(eng.common_neighbors(), O.jaccard_counts(ip, ix).astype(np.float64))


def _prime(ctx):
    """A valid graph with its transpose, Jaccard plan and an ApproxER state on the context:
    what a refusal must not leave in use."""
    from gsparse.engine import Engine

    n, ip, ix, d, jac = valid()
    ctx.set_graph_csr(n, ip, ix, d)
    eng = Engine(ctx)
    assert bits_equal(eng.jaccard(), jac)
    assert eng.er_prepare(4) == len(ix) // 2


@pytest.mark.parametrize("name", list(BAD_CSR))
def test_csr_refusals_leave_the_empty_graph(ctx, name):
    n, ip, ix, exc, msg = BAD_CSR[name]
    _prime(ctx)
    with pytest.raises(exc, match=msg):
        ctx.set_graph_csr(n, np.asarray(ip, dtype=np.int64), np.asarray(ix, dtype=np.int32), None)
    _after_refusal(ctx)


@pytest.mark.parametrize("where", ["host", "cuda"])
@pytest.mark.parametrize("bad", [("src", 7), ("dst", 7), ("src", -1)], ids=["src_n", "dst_n", "src_minus_1"])
def test_edge_index_refusals_leave_the_empty_graph(ctx, bad, where):
    """n = 7 after a 300-node graph: a library that kept the old arrays under the new n would
    score with the wrong bounds."""
    side, value = bad
    s, d = _i64([0, 1, 2, 6, 3], [1, 2, 0, 5, 3])
    (s if side == "src" else d)[3] = value
    _prime(ctx)
    with pytest.raises(ValueError, match="out of range"):
        _put(ctx, 7, s, d, where)
    _after_refusal(ctx)


def test_negative_sizes_are_refused_the_same_way(ctx):
    from gsparse._lib import GS_HOST

    _prime(ctx)
    with pytest.raises(ValueError, match="negative"):
        ctx.call("gs_graph_from_edge_index", -1, 0, None, None, GS_HOST)
    _after_refusal(ctx)
