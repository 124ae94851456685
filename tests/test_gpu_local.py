"""GPU tests of local sparsification on the device: gs_segment_rank's ranks, degrees and
counters and gs_local_scores' scores, n_top and exponent masks against the NumPy
specification (selection.local_filter_scores) -- ranks and masks exactly, the scores byte
for byte -- on the truss_cases graphs, stars at every sub-wave group border, a wheel whose
hub is above the LDS limit, empty and isolated-node graphs; under every knob; and what is
built on them (GraphSparsifier.sparsify_local, calculate_local_filter_scores).  Every
expected value is computed on the host, once per case."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import local_cases as C

pytestmark = pytest.mark.gpu

SHORT_MAX, LDS_SMALL, LDS_MAX = 64, 2048, 8192  # gs_segrank.hip's compile-time limits
EXPONENTS = (0, 0.3, 0.5, 0.7, 1)


@pytest.fixture(scope="module")
def gs():
    import gsparse

    return gsparse


@pytest.fixture(scope="module")
def eng(gs):
    ctx = gs._lib.Context()
    ctx.set_graph_csr(2, np.array([0, 1, 2]), np.array([1, 0], dtype=np.int32), None)
    return gs.engine.Engine(ctx)


def expected_classes(deg, smax=SHORT_MAX, lmax=LDS_MAX, sort=False):
    d = np.asarray(deg)
    if sort:
        smax = lmax = 0
    return {"empty": int((d == 0).sum()), "short": int(((d > 0) & (d <= smax)).sum()),
            "lds": int(((d > smax) & (d <= lmax)).sum()), "stream": int((d > max(smax, lmax)).sum())}


def check(eng, n, ei, s, want, keep_lowest=False, **limits):
    """One gs_segment_rank and one local_scores call against (local, rank, info) of the
    specification; returns the device's (rank, local, info)."""
    from gsparse.selection import local_mask

    local, rank, winfo = want
    E = ei.shape[1]
    deg = np.bincount(ei[0], minlength=n)
    r, d, info = eng.segment_rank(s, ei[0], n, keep_lowest)
    assert r.dtype == np.int32 and r.shape == (E,) and d.dtype == np.int64 and d.shape == (n,)
    assert np.array_equal(d, deg)
    assert np.array_equal(r, rank), np.nonzero(r != rank)[0][:10]
    assert info == {"max_degree": winfo["max_degree"], "classes": expected_classes(deg, **limits)}
    got, linfo = eng.local_scores(s, ei[0], ei[1], n, keep_lowest)
    assert got.dtype == np.float64 and got.shape == (E,)
    assert got.tobytes() == local.tobytes(), np.nonzero(got != local)[0][:10]
    assert linfo == {"max_degree": winfo["max_degree"], "n_top": winfo["n_top"], "classes": info["classes"]}
    for e in EXPONENTS:
        assert np.array_equal(local_mask(got, e), local_mask(local, e))
    return r, got, linfo


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("name", C.NAMES)
def test_equals_the_specification(eng, name, kind):
    n, ei = C.CASES[name]
    for keep_lowest in (False, True):
        check(eng, n, ei, C.scores(name, kind), C.expected(name, kind, keep_lowest), keep_lowest)


def test_every_class_is_reached_at_the_default_limits(eng):
    _, _, info = check(eng, *C.CASES["borders"], C.scores("borders", "mod101"),
                       C.expected("borders", "mod101"))
    deg = len(C.BORDER_DEGREES)  # centres of 65 and 66 columns are LDS, every leaf is SHORT
    assert info["classes"] == {"empty": 0, "short": sum(C.BORDER_DEGREES) + deg - 2, "lds": 2, "stream": 0}
    _, _, info = check(eng, *C.CASES["borders_lds"], C.scores("borders_lds", "mod101"),
                       C.expected("borders_lds", "mod101"))
    assert info["classes"]["lds"] == len(C.LDS_DEGREES) and info["classes"]["stream"] == 0
    _, _, info = check(eng, *C.CASES["hub_pair"], C.scores("hub_pair", "mod101"),
                       C.expected("hub_pair", "mod101"))
    assert info["classes"]["lds"] == 2 and info["max_degree"] > LDS_SMALL  # the large LDS image
    _, _, info = check(eng, *C.CASES["wheel"], C.scores("wheel", "mod101"), C.expected("wheel", "mod101"))
    assert info["classes"] == {"empty": 0, "short": C.WHEEL_HUB, "lds": 0, "stream": 1}
    assert info["max_degree"] == C.WHEEL_HUB
    _, _, info = check(eng, *C.CASES["empty"], C.scores("empty", "equal"), C.expected("empty", "equal"))
    assert info == {"max_degree": 0, "n_top": 0, "classes": {"empty": 5, "short": 0, "lds": 0, "stream": 0}}
    _, _, info = check(eng, *C.CASES["isolated"], C.scores("isolated", "equal"),
                       C.expected("isolated", "equal"))
    assert info["classes"]["empty"] == 3


@functools.lru_cache(maxsize=None)
def shuffled_case(name, kind, keep_lowest):
    from gsparse.selection import local_filter_scores

    n, ei, p = C.shuffled(name)
    s = np.ascontiguousarray(C.scores(name, kind)[p])
    return n, ei, s, local_filter_scores(s, ei, n, keep_lowest)


@pytest.mark.parametrize("kind", ["equal", "special", "degsum"])
@pytest.mark.parametrize("name", ["karate", "rmat10", "cliques_loops_dups", "borders", "borders_lds",
                                  "hub_pair", "wheel"])
def test_shuffled_columns(eng, name, kind):
    """An unsorted src with ties: the scatter's order inside a segment must not show."""
    for keep_lowest in (False, True):
        n, ei, s, want = shuffled_case(name, kind, keep_lowest)
        assert (np.diff(ei[0]) < 0).any()
        check(eng, n, ei, s, want, keep_lowest)


KNOBS = [{"GSPARSE_SEGR_SHORT_MAX": "4", "GSPARSE_SEGR_LDS_MAX": "32"},
         {"GSPARSE_SEGR_SHORT_MAX": "0", "GSPARSE_SEGR_LDS_MAX": "5000"},
         {"GSPARSE_SEGR_SHORT_MAX": "16", "GSPARSE_SEGR_LDS_MAX": "8"},
         {"GSPARSE_SEGR_MODE": "sort"}]


@pytest.mark.parametrize("knobs", KNOBS, ids=["short4_lds32", "short0_lds5000", "short16_lds8", "sort"])
@pytest.mark.parametrize("name", ["karate", "rmat10", "borders", "hub_pair", "cliques_loops_dups", "empty"])
def test_knobs_change_the_classes_only(eng, monkeypatch, name, knobs):
    n, ei = C.CASES[name]
    limits = {"smax": int(knobs.get("GSPARSE_SEGR_SHORT_MAX", SHORT_MAX)),
              "lmax": int(knobs.get("GSPARSE_SEGR_LDS_MAX", LDS_MAX)),
              "sort": knobs.get("GSPARSE_SEGR_MODE") == "sort"}
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    for kind in ("degsum", "special"):
        for keep_lowest in (False, True):
            check(eng, n, ei, C.scores(name, kind), C.expected(name, kind, keep_lowest), keep_lowest, **limits)
    _, sei, s, want = shuffled_case(name, "equal", False)
    _, _, info = check(eng, n, sei, s, want, **limits)
    if name == "rmat10":  # which classes the knobs leave in use
        used = {c for c in ("short", "lds", "stream") if info["classes"][c] > 0}
        assert used == ({"stream"} if limits["sort"] else {"lds"} if limits["smax"] == 0 else
                        {"short", "stream"} if limits["lmax"] == 8 else {"short", "lds", "stream"})


TINY_HUBS = {"one_column": (2, [[0], [1]]),                      # a sort of one item launches nothing
             "one_source": (3, [[0, 0], [1, 2]]),
             "unsorted_src": (3, [[1, 0, 1], [0, 1, 2]])}        # two sources, src not ascending


@pytest.mark.parametrize("name", list(TINY_HUBS))
def test_every_segment_a_hub_on_tiny_inputs(eng, monkeypatch, name):
    """Both class bounds at 0: every segment goes through the gather and the three sorts."""
    from gsparse.selection import local_filter_scores

    monkeypatch.setenv("GSPARSE_SEGR_SHORT_MAX", "0")
    monkeypatch.setenv("GSPARSE_SEGR_LDS_MAX", "0")
    n, ei = TINY_HUBS[name]
    ei = np.array(ei, dtype=np.int64)
    E = ei.shape[1]
    for s in (np.full(E, 0.25), np.arange(E, dtype=np.float64), -np.arange(E, dtype=np.float64)):
        for keep_lowest in (False, True):
            _, _, info = check(eng, n, ei, s, local_filter_scores(s, ei, n, keep_lowest), keep_lowest,
                               smax=0, lmax=0)
            assert info["classes"]["stream"] == len(set(ei[0].tolist())) and info["classes"]["short"] == 0


@pytest.mark.parametrize("name", ["rmat10", "wheel", "hub_pair"])
def test_two_runs_give_identical_bytes(eng, name):
    n, ei, s, _ = shuffled_case(name, "degsum", False)
    a, ia = eng.local_scores(s, ei[0], ei[1], n)
    b, ib = eng.local_scores(s, ei[0], ei[1], n)
    assert a.tobytes() == b.tobytes() and ia == ib
    ra, rb = eng.segment_rank(s, ei[0], n)[0], eng.segment_rank(s, ei[0], n)[0]
    assert ra.tobytes() == rb.tobytes()


@pytest.mark.parametrize("name", ["rmat10", "cliques_loops_dups", "wheel", "empty"])
def test_cuda_tensors_and_out_equal_the_numpy_path(eng, name):
    n, ei = C.CASES[name]
    E = ei.shape[1]
    s = C.scores(name, "degsum")
    local, rank, winfo = C.expected(name, "degsum")
    ts, tsrc, tdst = (torch.from_numpy(np.array(a)).cuda() for a in (s, ei[0], ei[1]))
    r, d, info = eng.segment_rank(ts, tsrc, n)
    assert r.is_cuda and d.is_cuda and r.dtype == torch.int32 and d.dtype == torch.int64
    assert np.array_equal(r.cpu().numpy(), rank)
    assert np.array_equal(d.cpu().numpy(), np.bincount(ei[0], minlength=n))
    got, linfo = eng.local_scores(ts, tsrc, tdst, n)
    assert got.is_cuda and got.shape == (E,) and got.cpu().numpy().tobytes() == local.tobytes()
    assert linfo["n_top"] == winfo["n_top"] and linfo["max_degree"] == winfo["max_degree"]
    out = torch.full((E + 3,), -7.0, dtype=torch.float64, device="cuda")
    got, linfo2 = eng.local_scores(ts, tsrc, tdst, n, out=out)
    assert got is out and linfo2 == linfo
    assert out[:E].cpu().numpy().tobytes() == local.tobytes() and (out[E:] == -7.0).all()
    host = np.full(E + 2, -7.0)  # numpy ids, a numpy out
    assert eng.local_scores(s, ei[0], ei[1], n, out=host)[0] is host
    assert host[:E].tobytes() == local.tobytes() and (host[E:] == -7.0).all()
    mixed = np.full(E, -7.0)  # CUDA ids, a numpy out
    eng.local_scores(ts, tsrc, tdst, n, out=mixed)
    assert mixed.tobytes() == local.tobytes()
    with pytest.raises(TypeError):
        eng.local_scores(s, ei[0], ei[1], n, out=np.zeros(E, dtype=np.float32))
    if E:
        with pytest.raises(ValueError):
            eng.local_scores(s, ei[0], ei[1], n, out=np.zeros(E - 1))


def test_errors(gs, eng):
    from gsparse.selection import local_mask_device

    L, h = gs._lib.lib(), eng.ctx.handle
    n, ei = C.CASES["karate"]
    E = ei.shape[1]
    s = np.array(C.scores("karate", "mod101"))
    src, dst = np.array(ei[0]), np.array(ei[1])
    with pytest.raises(ValueError, match="one score per edge_index column"):
        eng.segment_rank(s[:-1], src, n)
    with pytest.raises(ValueError, match="merged duplicate columns"):
        local_mask_device(eng, s[:-1], ei, n, 0.5)
    for bad in (-1, n):
        b = src.copy()
        b[7] = bad
        with pytest.raises(ValueError, match="out of range"):
            eng.segment_rank(s, b, n)
        with pytest.raises(ValueError, match="out of range"):
            eng.local_scores(s, b, dst, n)
        b = dst.copy()
        b[7] = bad
        with pytest.raises(ValueError, match="out of range"):
            eng.local_scores(s, src, b, n)
    with pytest.raises(ValueError):
        eng.segment_rank(s, src, 0)
    # through the ABI
    rank, deg = np.zeros(E, dtype=np.int32), np.zeros(n, dtype=np.int64)
    counts, mx = np.zeros(4, dtype=np.int64), ctypes.c_int64(-1)

    def seg(nscores, nodes=n, the_src=src):
        return L.gs_segment_rank(h, s.ctypes.data, 0, nscores, the_src.ctypes.data, 0, E, nodes, 0,
                                 rank.ctypes.data, 0, deg.ctypes.data, 0, ctypes.byref(mx),
                                 counts.ctypes.data, 4)

    assert seg(E - 1) == gs._lib.GS_EINVAL and mx.value == -1
    assert seg(E, nodes=0) == gs._lib.GS_EINVAL
    assert seg(E, the_src=np.where(np.arange(E) == 3, n, src)) == gs._lib.GS_EINVAL
    assert seg(E) == gs._lib.GS_OK and mx.value == 17
    assert np.array_equal(rank, C.expected("karate", "mod101")[1]) and counts.tolist() == [0, n, 0, 0]
    # NULL deg / max_deg / class_counts are accepted
    assert L.gs_segment_rank(h, s.ctypes.data, 0, E, src.ctypes.data, 0, E, n, 0, rank.ctypes.data, 0,
                             None, 0, None, None, 0) == gs._lib.GS_OK
    table = np.log(np.maximum(np.arange(18), 1).astype(np.float64))
    out, top = np.full(E, -7.0), ctypes.c_int64(-1)

    def loc(ntable, the_rank=rank, the_dst=dst):
        return L.gs_local_scores(h, the_rank.ctypes.data, 0, src.ctypes.data, the_dst.ctypes.data, 0, E, n,
                                 deg.ctypes.data, 0, table.ctypes.data, 0, ntable, out.ctypes.data, 0,
                                 ctypes.byref(top))

    assert loc(17) == gs._lib.GS_EINVAL  # ntable <= the maximum degree
    assert b"table" in L.gs_last_error() and (out == -7.0).all()
    assert loc(18, the_rank=np.where(np.arange(E) == 5, 40, rank).astype(np.int32)) == gs._lib.GS_EINVAL
    assert loc(18, the_dst=np.where(np.arange(E) == 5, n, dst)) == gs._lib.GS_EINVAL
    with pytest.raises(ValueError, match="table"):  # the same refusal as a Python exception
        eng.ctx.call("gs_local_scores", rank.ctypes.data, 0, src.ctypes.data, dst.ctypes.data, 0, E, n,
                     deg.ctypes.data, 0, table.ctypes.data, 0, 17, out.ctypes.data, 0, ctypes.byref(top))
    assert loc(18) == gs._lib.GS_OK
    local, _, winfo = C.expected("karate", "mod101")
    assert out.tobytes() == local.tobytes() and top.value == winfo["n_top"] == 62
    assert gs._lib.lib().gs_api_version() == 3
    # the context still works after the refused calls
    check(eng, n, ei, s, C.expected("karate", "mod101"))


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("name", ["karate", "rmat10", "hub_pair", "borders", "wheel", "cliques_loops_dups"])
def test_segment_topk_still_equals_its_host_form(eng, name, k):
    """gs_segment_topk's segment builder moved to a header shared with gs_segment_rank."""
    for kind, shuffle in (("distinct", False), ("degsum", True)):
        if shuffle:
            n, ei, s, _ = shuffled_case(name, kind, False)
        else:
            (n, ei), s = C.CASES[name], C.scores(name, kind)
        ref_mask, ref_status, ref_ng, ref_na = topk_rule(name, kind, shuffle, k)
        mask, status, info = eng.segment_topk(s, ei[0], n, k)
        assert np.array_equal(mask, ref_mask) and np.array_equal(status, ref_status)
        assert (info["n_guaranteed"], info["n_ambiguous"]) == (ref_ng, ref_na)
        d = np.bincount(ei[0], minlength=n)
        rest = d[d > k]
        assert info["classes"] == {"empty": int((d == 0).sum()), "all": int(((d > 0) & (d <= k)).sum()),
                                   "short": int((rest <= 64).sum()),
                                   "lds": int(((rest > 64) & (rest <= 16384)).sum()),
                                   "stream": int((rest > 16384).sum())}


@functools.lru_cache(maxsize=None)
def topk_rule(name, kind, shuffle, k):
    from test_segment_topk_host import segment_topk_rule

    if shuffle:
        n, ei, s, _ = shuffled_case(name, kind, False)
    else:
        (n, ei), s = C.CASES[name], C.scores(name, kind)
    return segment_topk_rule(s, ei[0], n, k)


def _sparsifier(gs, name="karate", device="cpu", cuda_ids=False):
    n, ei = C.CASES[name]
    t = torch.from_numpy(np.array(ei))
    data = gs.Data(edge_index=t.cuda() if cuda_ids else t, num_nodes=n)
    return gs.GraphSparsifier(data, device, tie_break="stable"), n, ei


LAST_KEYS = {"path", "mode", "exponent", "kept", "n_top", "max_degree", "classes"}


def test_sparsify_local_exponent_mode(gs):
    from gsparse.selection import local_filter_scores, local_mask

    sp_, n, ei = _sparsifier(gs)
    local, _, winfo = local_filter_scores(sp_.compute_scores("jaccard"), ei, n)
    sd, mask = sp_.sparsify_local("jaccard", exponent=0.5, return_mask=True)
    want = local_mask(local, 0.5)
    assert np.array_equal(mask.numpy(), want) and 0 < want.sum() < 156
    assert np.array_equal(sd.edge_index.numpy(), ei[:, want])
    assert set(sp_.last_selection) == LAST_KEYS
    assert sp_.last_selection == {"path": "device", "mode": "exponent", "exponent": 0.5, "kept": int(want.sum()),
                                  "n_top": winfo["n_top"], "max_degree": 17,
                                  "classes": {"empty": 0, "short": 34, "lds": 0, "stream": 0}}
    # the cache is hit on the second call, per direction
    cached = sp_._score_cache["local:jaccard:highest"]
    assert cached.tobytes() == local.tobytes()
    assert sp_.compute_local_scores("jaccard") is cached and "local:jaccard:lowest" not in sp_._score_cache
    assert sp_.sparsify_local("jaccard", exponent=1).edge_index.shape[1] == 156
    assert sp_.last_selection["kept"] == 156 and sp_._score_cache["local:jaccard:highest"] is cached
    _, m0 = sp_.sparsify_local("jaccard", exponent=0, return_mask=True)
    assert np.array_equal(m0.numpy(), local == 1.0) and len(set(ei[0][m0.numpy()])) == n
    low, _, _ = local_filter_scores(sp_.compute_scores("jaccard"), ei, n, keep_lowest=True)
    _, ml = sp_.sparsify_local("jaccard", exponent=0.3, keep_lowest=True, return_mask=True)
    assert np.array_equal(ml.numpy(), local_mask(low, 0.3))
    assert sp_._score_cache["local:jaccard:lowest"].tobytes() == low.tobytes()


def test_sparsify_local_ratio_mode_and_bad_arguments(gs):
    sp_, n, ei = _sparsifier(gs)
    for r in (0.1, 0.5, 0.77):
        sd, mask = sp_.sparsify_local("jaccard", retention_ratio=r, return_mask=True)
        assert int(mask.sum()) == int(156 * r) == sd.edge_index.shape[1]
        assert set(sp_.last_selection) == LAST_KEYS | {"cut", "beyond", "tied"}
        assert sp_.last_selection["mode"] == "ratio" and sp_.last_selection["exponent"] is None
        local = sp_.compute_local_scores("jaccard")
        assert local[mask.numpy()].min() >= local[~mask.numpy()].max()
    whole, mask = sp_.sparsify_local("jaccard", retention_ratio=1.0, return_mask=True)
    assert whole.edge_index.shape[1] == 156 and mask.all()
    for kw in ({}, {"exponent": 0.5, "retention_ratio": 0.5}, {"exponent": -0.1}, {"exponent": 1.1},
               {"retention_ratio": 0.0}, {"retention_ratio": 1.5}):
        with pytest.raises(ValueError):
            sp_.sparsify_local("jaccard", **kw)
    with pytest.raises(ValueError, match="not supported"):
        sp_.sparsify_local("jacard", exponent=0.5)


def test_sparsify_local_with_cuda_ids_and_duplicate_columns(gs):
    from gsparse.selection import local_filter_scores, local_mask

    sp_, n, ei = _sparsifier(gs, "rmat10", "cuda:0", cuda_ids=True)
    sc = sp_.compute_scores("degree")
    if len(sc) == ei.shape[1]:
        sd, mask = sp_.sparsify_local("degree", exponent=0.4, return_mask=True)
        want = local_mask(local_filter_scores(sc, ei, n)[0], 0.4)
        assert np.array_equal(mask.numpy(), want) and sd.edge_index.is_cuda
    else:  # rmat10 repeats columns: the canonical CSR merged them
        with pytest.raises(ValueError, match="merged duplicate columns"):
            sp_.sparsify_local("degree", exponent=0.4)
    sp_, n, ei = _sparsifier(gs, "cliques_loops_dups")
    with pytest.raises(ValueError, match="merged duplicate columns"):
        sp_.sparsify_local("jaccard", exponent=0.5)


def test_calculate_local_filter_scores(gs):
    import scipy.sparse as sp

    from gsparse.selection import local_filter_scores

    import truss_cases as T

    ip, ix = T.csr("cliques")
    rows = T.rows_of("cliques")
    s = ((7919 * np.arange(len(ix))) % 13).astype(np.float64)
    adj = sp.csr_matrix((np.ones(len(ix)), ix, ip), shape=(17, 17))
    want = local_filter_scores(s, np.stack([rows, ix.astype(np.int64)]), 17)[0]
    got = gs.calculate_local_filter_scores(adj, s)
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
    low = gs.calculate_local_filter_scores(adj, s, keep_lowest=True)
    assert low.tobytes() == local_filter_scores(s, np.stack([rows, ix.astype(np.int64)]), 17, True)[0].tobytes()
    # unsorted rows come back in storage order
    perm = np.arange(len(ix))
    for u in range(17):
        perm[ip[u]:ip[u + 1]] = perm[ip[u]:ip[u + 1]][::-1]
    shuffled = sp.csr_matrix((np.ones(len(ix)), ix[perm], ip), shape=(17, 17))
    assert gs.calculate_local_filter_scores(shuffled, s[perm]).tobytes() == want[perm].tobytes()
    with pytest.raises(ValueError):
        gs.calculate_local_filter_scores(adj, s[:-1])
