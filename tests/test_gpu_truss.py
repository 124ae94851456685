"""GPU tests of the trussness on the device (gs_trussness) and of what is built on it: the
scores, the levels and the sub-rounds against the NumPy specification
(selection.trussness_host) for equality, on the small graphs where the peel can go wrong;
the tail knob; the "truss" metric and sparsify_truss through GraphSparsifier.  Every
expected value is computed on the host, once per case."""

import ctypes

import numpy as np
import pytest
import torch

import truss_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from gsparse._lib import Context

    return Context(0)


def _engine(ctx, name):
    from gsparse.engine import Engine

    n, ei = C.CASES[name]
    ctx.set_graph_edge_index(n, np.ascontiguousarray(ei[0]), np.ascontiguousarray(ei[1]))
    ip, ix = C.csr(name)
    gip, gix, _ = ctx.csr()
    assert np.array_equal(gip, ip) and np.array_equal(gix, ix)  # the CSR the expectation is for
    return Engine(ctx)


def _check(ctx, name):
    eng = _engine(ctx, name)
    t, levels, rounds = C.expected(name)
    got, info = eng.trussness()
    assert got.dtype == np.float64 and got.shape == t.shape
    assert np.array_equal(got, t.astype(np.float64)), name
    assert info["levels"] == levels and info["rounds"] == rounds, (name, info)
    assert info["max_truss"] == (int(t.max()) if len(t) else 0)
    assert info["host_waits"] >= (1 if len(t) else 0)
    assert np.array_equal(got, got[C.reverse_positions(name)])
    return eng, got, info


@pytest.mark.parametrize("name", C.NAMES)
def test_trussness_equals_the_specification(ctx, name):
    _check(ctx, name)


def test_known_answers(ctx):
    _, got, info = _check(ctx, "empty")
    assert got.shape == (0,) and info == {"max_truss": 0, "levels": 0, "rounds": 0, "host_waits": 0}
    _, got, info = _check(ctx, "K70")  # every triangle has three frontier edges
    assert (got == 70).all() and (info["levels"], info["rounds"]) == (1, 1)
    _, got, info = _check(ctx, "lattice24")  # one ring per sub-round
    assert (got == 3).all() and (info["levels"], info["rounds"]) == (1, 24)
    _, got, info = _check(ctx, "hub_pair")
    vals, cnt = np.unique(got, return_counts=True)
    assert dict(zip(vals.tolist(), cnt.tolist())) == {2.0: 4, 3.0: 12002, 5.0: 20}
    _, got, _ = _check(ctx, "cliques_loops_dups")
    ip, ix = C.csr("cliques_loops_dups")
    diag = C.rows_of("cliques_loops_dups") == ix
    assert diag.sum() == 3 and (got[diag] == 0).all() and (got[~diag] >= 2).all()


@pytest.mark.parametrize("name", ["rmat10", "lattice24", "hub_pair", "karate"])
def test_two_runs_give_identical_bytes(ctx, name):
    eng = _engine(ctx, name)
    a, ia = eng.trussness()
    b, ib = eng.trussness()
    assert a.tobytes() == b.tobytes() and ia == ib


@pytest.mark.parametrize("name", ["rmat10", "cliques_loops_dups", "empty"])
def test_cuda_tensor_out_equals_the_numpy_path(ctx, name):
    eng = _engine(ctx, name)
    want, info = eng.trussness()
    out = torch.full((eng.nnz + 3,), -7.0, dtype=torch.float64, device="cuda")
    got, info2 = eng.trussness(out=out)
    assert got is out and info2 == info
    assert out[: eng.nnz].cpu().numpy().tobytes() == want.tobytes()
    assert (out[eng.nnz:] == -7.0).all()
    host = np.full(eng.nnz, -7.0)
    assert eng.trussness(out=host)[0] is host and host.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", ["lattice24", "karate", "cliques", "rmat10"])
def test_tail_knob_changes_the_waits_only(ctx, name, monkeypatch):
    eng = _engine(ctx, name)
    t, levels, rounds = C.expected(name)
    res = {}
    for cap in ("0", "4096", "1", "64"):
        monkeypatch.setenv("GSPARSE_TRUSS_TAIL", cap)
        got, info = eng.trussness()
        assert np.array_equal(got, t.astype(np.float64)), (name, cap)
        assert (info["levels"], info["rounds"]) == (levels, rounds), (name, cap, info)
        res[cap] = info["host_waits"]
    monkeypatch.delenv("GSPARSE_TRUSS_TAIL")
    assert eng.trussness()[1]["rounds"] == rounds
    # without the tail: the edge count, one wait per level and one per sub-round
    assert res["0"] == 1 + levels + rounds
    assert res["4096"] <= res["0"]
    if name == "lattice24":
        assert res["4096"] < res["0"]
        assert res["4096"] == 1 + 1 + 1  # the 24 sub-rounds are one launch


@pytest.mark.parametrize("name", ["hub_pair", "K70", "rmat10"])
def test_waves_per_edge_change_nothing(ctx, name, monkeypatch):
    """1, 4 or 16 waves on a frontier edge (the hub edge's 3,001-entry list, K70's 69):
    the same scores, levels and sub-rounds."""
    eng = _engine(ctx, name)
    t, levels, rounds = C.expected(name)
    for waves in ("1", "4", "16"):
        monkeypatch.setenv("GSPARSE_TRUSS_WAVES", waves)
        for cap in ("0", "16"):
            monkeypatch.setenv("GSPARSE_TRUSS_TAIL", cap)
            got, info = eng.trussness()
            assert np.array_equal(got, t.astype(np.float64)), (name, waves, cap)
            assert (info["levels"], info["rounds"]) == (levels, rounds), (name, waves, cap, info)


def test_directed_graph_is_unsupported(ctx):
    from gsparse import _lib
    from gsparse.engine import Engine

    ctx.set_graph_edge_index(4, np.array([0, 1, 2], dtype=np.int64), np.array([1, 2, 0], dtype=np.int64))
    eng = Engine(ctx)
    out = np.zeros(eng.nnz)
    mx = ctypes.c_int64(-1)
    rc = _lib.lib().gs_trussness(ctx.handle, _lib.ptr(out), _lib.GS_HOST, ctypes.byref(mx), None, None, None)
    assert rc == _lib.GS_EUNSUPPORTED and mx.value == -1
    with pytest.raises(NotImplementedError) as a:
        eng.common_neighbors()
    with pytest.raises(a.type):
        eng.trussness()
    assert _lib.lib().gs_api_version() == 3


def test_null_counters_are_accepted(ctx):
    from gsparse import _lib

    eng = _engine(ctx, "karate")
    out = np.zeros(eng.nnz)
    rc = _lib.lib().gs_trussness(ctx.handle, _lib.ptr(out), _lib.GS_HOST, None, None, None, None)
    assert rc == _lib.GS_OK and np.array_equal(out, C.expected("karate")[0])


def _karate_sparsifier():
    import gsparse

    n, ei = C.CASES["karate"]
    data = gsparse.Data(edge_index=torch.from_numpy(np.array(ei)), num_nodes=n)
    return gsparse.GraphSparsifier(data, "cpu", tie_break="stable"), n, ei


def test_truss_metric_through_graph_sparsifier():
    sp_, n, ei = _karate_sparsifier()
    t, levels, rounds = C.expected("karate")
    s = sp_.compute_scores("truss")
    assert np.array_equal(s, t.astype(np.float64))
    assert sp_.compute_scores("trussness") is s and "trussness" in sp_._score_cache
    sd, mask = sp_.sparsify("trussness", 0.5, return_mask=True)
    assert int(mask.sum()) == int(156 * 0.5) == sd.edge_index.shape[1]
    with pytest.raises(ValueError, match="not supported"):
        sp_.compute_scores("trusses")


def test_sparsify_truss_keeps_exactly_the_k_truss():
    sp_, n, ei = _karate_sparsifier()
    t, levels, rounds = C.expected("karate")
    sd, mask = sp_.sparsify_truss(4, return_mask=True)
    mask = mask.numpy()
    assert np.array_equal(mask, t >= 4) and int(mask.sum()) == 50
    assert np.array_equal(sd.edge_index.numpy(), ei[:, mask])
    assert sp_.last_selection == {"path": "device", "k": 4, "kept": 50, "max_truss": 5,
                                  "levels": levels, "rounds": rounds}
    # the kept graph is a 4-truss: every kept edge lies in >= 2 triangles of it
    import scipy.sparse as sp

    a = sp.csr_matrix((np.ones(50), (ei[0, mask], ei[1, mask])), shape=(n, n))
    assert (np.asarray((a @ a)[ei[0, mask], ei[1, mask]]).ravel() >= 2).all()
    whole = sp_.sparsify_truss(2)
    assert whole.edge_index.shape[1] == 156 and sp_.last_selection["kept"] == 156
    assert sp_.sparsify_truss(np.int64(6)).edge_index.shape[1] == 0
    for bad in (1, 2.5):
        with pytest.raises(ValueError):
            sp_.sparsify_truss(bad)


def test_sparsify_truss_needs_one_score_per_column_and_drops_loops():
    import gsparse

    n, ei = C.CASES["cliques_loops_dups"]
    data = gsparse.Data(edge_index=torch.from_numpy(np.array(ei)), num_nodes=n)
    with pytest.raises(ValueError, match="duplicate"):
        gsparse.GraphSparsifier(data, "cpu").sparsify_truss(3)
    ip, ix = C.csr("cliques_loops_dups")  # the same graph, one column per CSR entry
    rows = C.rows_of("cliques_loops_dups")
    ei2 = np.stack([rows, ix.astype(np.int64)])
    data = gsparse.Data(edge_index=torch.from_numpy(ei2), num_nodes=n)
    sp_ = gsparse.GraphSparsifier(data, "cpu")
    _, mask = sp_.sparsify_truss(2, return_mask=True)
    assert np.array_equal(mask.numpy(), rows != ix) and sp_.last_selection["kept"] == 74


def test_sparsify_connected_composes_with_the_truss_metric():
    import forest_cases as F

    sp_, n, ei = _karate_sparsifier()
    c, lab = F.components(ei[0], ei[1], n)
    _, mask = sp_.sparsify_connected("truss", 0.3, return_mask=True)
    mask = mask.numpy()
    kc, klab = F.components(ei[0], ei[1], n, mask)
    assert kc == c and np.array_equal(klab, lab)
    assert int(mask.sum()) >= int(156 * 0.3)


def test_calculate_trussness_scores():
    import scipy.sparse as sp

    import gsparse

    ip, ix = C.csr("cliques")
    adj = sp.csr_matrix((np.ones(len(ix)), ix, ip), shape=(17, 17))
    got = gsparse.calculate_trussness_scores(adj)
    assert got.dtype == np.float64 and np.array_equal(got, C.expected("cliques")[0])
    # unsorted rows come back in storage order
    perm = np.arange(len(ix))
    for u in range(17):
        perm[ip[u]:ip[u + 1]] = perm[ip[u]:ip[u + 1]][::-1]
    shuffled = sp.csr_matrix((np.ones(len(ix)), ix[perm], ip), shape=(17, 17))
    assert np.array_equal(gsparse.calculate_trussness_scores(shuffled), C.expected("cliques")[0][perm])
