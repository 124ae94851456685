"""GPU tests of the Simmelian backbone on the device (gs_simmelian) and of what is built on
it: both modes against the NumPy specification (selection.simmelian_host) byte for byte,
under the default class bounds and lowered ones, with the pairs per kernel class asserted;
the "simmelian" metric, simmelian_overlap and sparsify_simmelian through GraphSparsifier.
Every expected value is computed on the host, once per case and rank."""

import ctypes

import numpy as np
import pytest
import torch

import simmelian_cases as C
import truss_cases as T

pytestmark = pytest.mark.gpu

CLASSES = ("wave", "mid", "lds", "stream")
DEFAULT = (64, 512, 8192)
# (GSPARSE_SIM_WAVE_MAX, _MID_MAX, _LDS_MAX); None = unset
KNOBS = {
    "default": (None, None, None),
    "tiny": ("2", "4", "16"),        # the small graphs reach every class
    "all_stream": ("0", "0", "0"),
    "all_mid": ("0", None, None),    # a lane's one rank, staged all the same
    "no_mid": (None, "0", None),     # 65 and more common neighbours through the bitonic sort
}


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


def _set_knobs(monkeypatch, knobs):
    for var, v in zip(("GSPARSE_SIM_WAVE_MAX", "GSPARSE_SIM_MID_MAX", "GSPARSE_SIM_LDS_MAX"), knobs):
        if v is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, v)


def _host_classes(name, knobs):
    """pairs u < v per class: by the shorter of the two neighbour lists"""
    ip, ix = C.csr(name)
    rows = C.rows_of(name)
    deg = np.diff(ip)
    up = rows < ix
    shorter = np.minimum(deg[rows[up]], deg[ix[up]])
    w, m, l = (d if v is None else min(int(v), d) for v, d in zip(knobs, DEFAULT))
    cls = np.where(shorter <= w, 0, np.where(shorter <= m, 1, np.where(shorter <= l, 2, 3)))
    return dict(zip(CLASSES, np.bincount(cls, minlength=4).tolist()))


def _ranks(name):
    return (0, 1, 2, 5, C.max_degree(name) + 1)


@pytest.mark.parametrize("name", C.NAMES)
def test_device_equals_the_specification_byte_for_byte(ctx, name, monkeypatch):
    eng = _engine(ctx, name)
    rev = C.reverse_positions(name)
    nonzero = int((C.prepared(name)["c"] > 0).sum())
    for label, knobs in KNOBS.items():
        _set_knobs(monkeypatch, knobs)
        for k0 in _ranks(name):
            want = C.expected(name, k0)[0]
            got, info = eng.simmelian(k0)
            assert got.dtype == np.float64 and got.shape == want.shape
            assert got.tobytes() == want.tobytes(), (name, label, k0)
            assert np.array_equal(got, got[rev])
            assert info["classes"] == _host_classes(name, knobs), (name, label, k0, info)
            assert info["max_common"] == C.max_common(name) and info["nonzero_pairs"] == nonzero


def test_every_class_is_reached():
    """Under the default bounds and under the lowered ones, some case puts pairs in every
    class: with the class counts asserted above, no kernel goes untested."""
    for label in ("default", "tiny"):
        seen = {c: 0 for c in CLASSES}
        for name in C.NAMES:
            for c, v in _host_classes(name, KNOBS[label]).items():
                seen[c] += v
        assert all(seen.values()), (label, seen)
    assert _host_classes("two_hubs_9000", KNOBS["default"])["stream"] == 1
    assert _host_classes("two_hubs_graded", KNOBS["default"])["lds"] >= 1
    assert _host_classes("K70", KNOBS["default"]) == {"wave": 0, "mid": 2415, "lds": 0, "stream": 0}
    assert _host_classes("K70", KNOBS["no_mid"])["lds"] == 2415
    assert _host_classes("rmat10", KNOBS["all_stream"])["stream"] == 12104 // 2


@pytest.mark.parametrize("name", ["single_edge", "triangle"])
def test_smallest_graphs_through_the_stream_class(ctx, name, monkeypatch):
    """All three bounds at 0: a single edge is one STREAM pair without a hit (one key slot:
    nothing to sort), a triangle three pairs with one hit each."""
    eng = _engine(ctx, name)
    _set_knobs(monkeypatch, KNOBS["all_stream"])
    pairs = {"single_edge": 1, "triangle": 3}[name]
    for k0 in (0, 1):
        want = C.expected(name, k0)[0]
        got, info = eng.simmelian(k0)
        assert got.tobytes() == want.tobytes(), (name, k0)
        assert info["classes"] == {"wave": 0, "mid": 0, "lds": 0, "stream": pairs}
        assert info["max_common"] == C.max_common(name) == (name == "triangle")
        assert info["nonzero_pairs"] == (pairs if name == "triangle" else 0)


def test_known_answers(ctx):
    got, info = _engine(ctx, "empty").simmelian()
    assert got.shape == (0,) and info == {"max_common": 0, "nonzero_pairs": 0,
                                          "classes": dict.fromkeys(CLASSES, 0)}
    for name, mc in (("hub_pair", 3000), ("rmat10", 135), ("K70", 68)):
        got, info = _engine(ctx, name).simmelian()
        assert info["max_common"] == mc
        if name == "K70":
            assert (got == 1.0).all()
    eng = _engine(ctx, "hub_pair")
    ip, ix = C.csr("hub_pair")
    assert eng.simmelian()[0][ip[0]] == 3000 / 3004 and eng.simmelian(5)[0][ip[0]] == 3000
    got, _ = _engine(ctx, "cliques_loops_dups").simmelian()
    diag = C.rows_of("cliques_loops_dups") == C.csr("cliques_loops_dups")[1]
    assert diag.sum() == 3 and not got[diag].any()
    assert got[~diag].tobytes() == C.expected("cliques")[0].tobytes()


@pytest.mark.parametrize("name", ["rmat10", "two_hubs_graded", "two_hubs_9000", "karate"])
def test_two_runs_give_identical_bytes(ctx, name, monkeypatch):
    eng = _engine(ctx, name)
    for label in ("default", "all_stream"):
        _set_knobs(monkeypatch, KNOBS[label])
        for k0 in (0, 3):
            a, ia = eng.simmelian(k0)
            b, ib = eng.simmelian(k0)
            assert a.tobytes() == b.tobytes() and ia == ib


@pytest.mark.parametrize("name", ["rmat10", "cliques_loops_dups", "empty"])
def test_cuda_tensor_out_equals_the_numpy_path(ctx, name):
    eng = _engine(ctx, name)
    for k0 in (0, 2):
        want, info = eng.simmelian(k0)
        out = torch.full((eng.nnz + 3,), -7.0, dtype=torch.float64, device="cuda")
        got, info2 = eng.simmelian(k0, out=out)
        assert got is out and info2 == info
        assert out[: eng.nnz].cpu().numpy().tobytes() == want.tobytes()
        assert (out[eng.nnz:] == -7.0).all()
        host = np.full(eng.nnz, -7.0)
        assert eng.simmelian(k0, out=host)[0] is host and host.tobytes() == want.tobytes()


def test_bare_c_abi_refusals_and_null_counters(ctx):
    from gsparse import _lib
    from gsparse.engine import Engine

    L = _lib.lib()
    eng = _engine(ctx, "karate")
    out = np.zeros(eng.nnz)
    assert L.gs_simmelian(ctx.handle, _lib.ptr(out), _lib.GS_HOST, 0, None, None, None, 0) == _lib.GS_OK
    assert out.tobytes() == C.expected("karate")[0].tobytes()
    mc, nz = ctypes.c_int64(-1), ctypes.c_int64(-1)
    counts = np.full(6, -1, dtype=np.int64)
    rc = L.gs_simmelian(ctx.handle, _lib.ptr(out), _lib.GS_HOST, 2, ctypes.byref(mc), ctypes.byref(nz),
                        _lib.ptr(counts), 6)
    assert rc == _lib.GS_OK and out.tobytes() == C.expected("karate", 2)[0].tobytes()
    assert mc.value == 10 and nz.value == (156 - 22) // 2
    assert counts[:4].sum() == 78 and not counts[4:].any()
    # a negative rank: refused, nothing written
    out[:] = -3.0
    rc = L.gs_simmelian(ctx.handle, _lib.ptr(out), _lib.GS_HOST, -1, ctypes.byref(mc), None, None, 0)
    assert rc == _lib.GS_EINVAL and (out == -3.0).all() and mc.value == 10
    with pytest.raises(ValueError):
        eng.simmelian(-1)
    # an asymmetric resident graph: the refusal of gs_trussness
    ctx.set_graph_edge_index(4, np.array([0, 1, 2], dtype=np.int64), np.array([1, 2, 0], dtype=np.int64))
    eng = Engine(ctx)
    out = np.zeros(eng.nnz)
    rc = L.gs_simmelian(ctx.handle, _lib.ptr(out), _lib.GS_HOST, 0, ctypes.byref(mc), None, None, 0)
    assert rc == _lib.GS_EUNSUPPORTED and mc.value == 10
    with pytest.raises(NotImplementedError) as a:
        eng.trussness()
    with pytest.raises(a.type):
        eng.simmelian()
    assert L.gs_api_version() == 3


@pytest.mark.parametrize("name", ["cliques", "karate", "rmat10"])
def test_trussness_is_unchanged_by_the_shared_support_step(ctx, name):
    n, ei = T.CASES[name]
    ctx.set_graph_edge_index(n, np.ascontiguousarray(ei[0]), np.ascontiguousarray(ei[1]))
    from gsparse.engine import Engine

    got, info = Engine(ctx).trussness()
    entries, counts, levels, rounds = T.KNOWN[name]
    assert len(got) == entries and (info["levels"], info["rounds"]) == (levels, rounds)
    if counts is not None:
        vals, cnt = np.unique(got, return_counts=True)
        assert dict(zip(vals.astype(int).tolist(), cnt.tolist())) == counts
    assert np.array_equal(got, T.expected(name)[0].astype(np.float64))


def _sparsifier(name="karate", **kw):
    import gsparse

    n, ei = C.CASES[name]
    data = gsparse.Data(edge_index=torch.from_numpy(np.array(ei)), num_nodes=n)
    return gsparse.GraphSparsifier(data, "cpu", **kw), n, ei


def test_simmelian_metric_and_overlap_through_graph_sparsifier():
    sp_, n, ei = _sparsifier(tie_break="stable")
    want = C.expected("karate")[0]
    s = sp_.compute_scores("simmelian")
    assert s.tobytes() == want.tobytes()
    assert sp_.compute_scores("simmelian_jaccard") is s and "simmelian" in sp_._score_cache
    for k0 in (1, 3):
        o = sp_.simmelian_overlap(k0)
        assert o.tobytes() == C.expected("karate", k0)[0].tobytes() and sp_.simmelian_overlap(k0) is o
    sd, mask = sp_.sparsify("simmelian", 0.5, return_mask=True)
    assert int(mask.sum()) == 78 == sd.edge_index.shape[1]
    sd, stats = sp_.sparsify_metric_backbone("simmelian")
    assert 0 < sd.edge_index.shape[1] <= 156
    with pytest.raises(ValueError, match="not supported"):
        sp_.compute_scores("simmel")


def test_sparsify_simmelian_modes_give_the_masks_numpy_gives():
    sp_, n, ei = _sparsifier(tie_break="stable")
    s = C.expected("karate")[0]
    info = {"max_common": 10, "classes": _host_classes("karate", KNOBS["default"])}
    # ratio: the stable top-k, (score, index) descending
    sd, mask = sp_.sparsify_simmelian(retention_ratio=0.4, return_mask=True)
    keep = int(156 * 0.4)
    order = np.lexsort((np.arange(156), s))[::-1][:keep]
    want = np.zeros(156, dtype=bool)
    want[order] = True
    assert np.array_equal(mask.numpy(), want)
    assert np.array_equal(sd.edge_index.numpy(), ei[:, want])
    assert sp_.last_selection == {"path": "device", "mode": "ratio", "kept": keep, **info}
    # threshold
    sd, mask = sp_.sparsify_simmelian(threshold=0.5, return_mask=True)
    assert np.array_equal(mask.numpy(), s >= 0.5) and sd.edge_index.shape[1] == int((s >= 0.5).sum())
    assert sp_.last_selection == {"path": "device", "mode": "threshold", "kept": int((s >= 0.5).sum()), **info}
    # NetworKit's parametric form
    o = C.expected("karate", 3)[0]
    sd, mask = sp_.sparsify_simmelian(max_rank=3, min_overlap=2, return_mask=True)
    assert np.array_equal(mask.numpy(), o >= 2) and 0 < int(mask.sum()) < 156
    assert sp_.last_selection == {"path": "device", "mode": "overlap", "kept": int((o >= 2).sum()), **info}
    assert sp_.sparsify_simmelian(retention_ratio=1.0).edge_index.shape[1] == 156
    with pytest.raises(ValueError):
        sp_.sparsify_simmelian(retention_ratio=0.5, threshold=0.5)


def test_sparsify_simmelian_needs_one_score_per_column():
    sp_, n, ei = _sparsifier("cliques_loops_dups")
    with pytest.raises(ValueError, match="duplicate"):
        sp_.sparsify_simmelian(threshold=0.5)
    with pytest.raises(ValueError, match="duplicate"):
        sp_.sparsify_simmelian(max_rank=2, min_overlap=1)


def test_local_and_connected_sparsifiers_compose_with_the_simmelian_metric():
    import forest_cases as F
    from gsparse.selection import connected_mask, local_filter_scores, local_mask

    sp_, n, ei = _sparsifier(tie_break="stable")
    s = C.expected("karate")[0]
    _, mask = sp_.sparsify_local("simmelian", exponent=0.5, return_mask=True)
    assert np.array_equal(mask.numpy(), local_mask(local_filter_scores(s, ei, n)[0], 0.5))
    _, mask = sp_.sparsify_connected("simmelian", 0.5, return_mask=True)
    mask = mask.numpy()
    assert np.array_equal(mask, connected_mask(s, ei, n, 156, 0.5))
    c, lab = F.components(ei[0], ei[1], n)
    kc, klab = F.components(ei[0], ei[1], n, mask)
    assert kc == c and np.array_equal(klab, lab)


def test_calculate_simmelian_scores():
    import scipy.sparse as sp

    import gsparse

    ip, ix = C.csr("cliques")
    adj = sp.csr_matrix((np.ones(len(ix)), ix, ip), shape=(17, 17))
    assert gsparse.calculate_simmelian_scores(adj).tobytes() == C.expected("cliques")[0].tobytes()
    assert gsparse.calculate_simmelian_scores(adj, 2).tobytes() == C.expected("cliques", 2)[0].tobytes()
    perm = np.arange(len(ix))  # unsorted rows come back in storage order
    for u in range(17):
        perm[ip[u]:ip[u + 1]] = perm[ip[u]:ip[u + 1]][::-1]
    shuffled = sp.csr_matrix((np.ones(len(ix)), ix[perm], ip), shape=(17, 17))
    assert np.array_equal(gsparse.calculate_simmelian_scores(shuffled), C.expected("cliques")[0][perm])
