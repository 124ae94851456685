"""gs_segment_topk on the MI355X against the per-node rule restated in NumPy
(test_segment_topk_host.segment_topk_rule): mask, status and both counts are
equal exactly; every kernel class and every length at which the code takes
another path is reached; degree-aware selection with min_edges_per_node >= 2
runs its phase 1 on the device and equals the host restatement bit for bit."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_segment_topk_host import segment_topk_rule

pytestmark = pytest.mark.gpu

SHORT_MAX, LDS_SMALL, LDS_MAX = 64, 2048, 16384  # gs_segtopk.hip's compile-time limits


@pytest.fixture(scope="module")
def gs():
    import gsparse

    return gsparse


@pytest.fixture(scope="module")
def eng(gs):
    ctx = gs._lib.Context()
    ctx.set_graph_csr(2, np.array([0, 1, 2]), np.array([1, 0], dtype=np.int32), None)
    return gs.engine.Engine(ctx)


def expected_classes(lengths, k, smax=SHORT_MAX, lmax=LDS_MAX):
    d = np.asarray(lengths)
    out = {"empty": int((d == 0).sum()), "all": int(((d > 0) & (d <= k)).sum())}
    rest = d[d > k]
    out["short"] = int((rest <= smax).sum())
    out["lds"] = int(((rest > smax) & (rest <= lmax)).sum())
    out["stream"] = int((rest > max(smax, lmax)).sum())
    return out


def check(eng, scores, src, n, k, lengths=None, smax=SHORT_MAX, lmax=LDS_MAX):
    """One device call against the rule; returns (info, status)."""
    ref_mask, ref_status, ref_ng, ref_na = segment_topk_rule(scores, src, n, k)
    mask, status, info = eng.segment_topk(scores, src, n, k)
    assert mask.dtype == bool and mask.shape == (len(src),)
    assert status.dtype == np.uint8 and status.shape == (n,)
    assert np.array_equal(status, ref_status), np.nonzero(status != ref_status)[0][:10]
    assert np.array_equal(mask, ref_mask), np.nonzero(mask != ref_mask)[0][:10]
    assert (info["n_guaranteed"], info["n_ambiguous"]) == (ref_ng, ref_na)
    if lengths is None:
        lengths = np.bincount(src, minlength=n)
    exp = expected_classes(lengths, k, smax, lmax)
    assert info["classes"] == exp
    return info, status


def segments(lengths, seed, shuffled):
    """src with `lengths[u]` columns of node u and distinct scores (a permutation:
    no ties); shuffled: the columns in random order."""
    rng = np.random.default_rng(seed)
    src = np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)
    scores = (rng.permutation(len(src)).astype(np.float64) - len(src) / 3) / 7.0
    if shuffled:
        p = rng.permutation(len(src))
        src, scores = src[p], scores[p]
    return src, scores


# every boundary of the default limits: d = k-1, k, k+1 for k in {1, 2, 3, 5, 64}, the
# sub-wave group widths 8 / 16 / 64, the two LDS workgroup sizes (2048), empty nodes
BOUNDARY = [0, 1, 2, 3, 4, 5, 6, 0, 7, 8, 9, 15, 16, 17, 63, 64, 65, 0, 0, 100, 300,
            LDS_SMALL - 1, LDS_SMALL, LDS_SMALL + 1, 3000, 1, 8, 0]


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 64, 5000])
def test_boundary_lengths_distinct_scores(eng, k, shuffled):
    src, scores = segments(BOUNDARY, 1, shuffled)
    info, _ = check(eng, scores, src, len(BOUNDARY), k, BOUNDARY)
    assert info["n_ambiguous"] == 0
    reached = ["empty", "all"] + (["short", "lds"] if k <= 5 else ["lds"] if k == 64 else [])
    for c in reached:
        assert info["classes"][c] > 0, c
    if k == 5000:  # larger than the maximum degree: every column of every node
        assert info["n_guaranteed"] == len(src)


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("k", [2, 5, 300])
def test_lowered_limits_reach_stream(eng, monkeypatch, k, shuffled):
    """GSPARSE_SEGK_LDS_MAX = 256: the LDS limit +-1, and a hub of a few thousand
    columns in the STREAM class; GSPARSE_SEGK_SHORT_MAX = 16 moves 17..64 to LDS."""
    monkeypatch.setenv("GSPARSE_SEGK_LDS_MAX", "256")
    monkeypatch.setenv("GSPARSE_SEGK_SHORT_MAX", "16")
    lengths = [255, 256, 257, 0, 3000, 16, 17, 40, 64, 65, 3, 9, 301]
    src, scores = segments(lengths, 2, shuffled)
    info, _ = check(eng, scores, src, len(lengths), k, lengths, smax=16, lmax=256)
    assert info["n_ambiguous"] == 0
    for c in (["short", "lds", "stream"] if k < 300 else ["all", "stream"]):
        assert info["classes"][c] > 0, c


def tie_graph(k, seed, shuffled):
    """One node per (length, pattern): a tie block wholly above the cut, wholly below
    it, straddling it, -0.0 against +0.0 at the cut, +-inf, one NaN; the positions
    inside a segment are random."""
    rng = np.random.default_rng(seed)
    patterns = ["above", "below", "straddle", "zeros", "inf", "nan", "all_equal"]
    src, sc, expect = [], [], []
    u = 0
    for d in [6, 12, 40, 300, 2500]:
        for pat in patterns:
            v = np.arange(1, d + 1, dtype=np.float64)  # ascending: v[d - k] is the cut
            amb = False
            if pat == "above":
                v[d - 1] = v[d - 2]
            elif pat == "below":
                v[0] = v[1]
            elif pat == "straddle":
                v[d - k - 1] = v[d - k]
                amb = True
            elif pat == "zeros":
                v[: d - k - 1] = -v[: d - k - 1]
                v[d - k - 1], v[d - k] = -0.0, 0.0
                amb = True
            elif pat == "inf":
                v[0], v[d - 1] = -np.inf, np.inf
            elif pat == "nan":
                v[rng.integers(0, d)] = np.nan
                amb = True
            elif pat == "all_equal":
                v[:] = 0.25
                amb = True
            sc.append(rng.permutation(v))
            src.append(np.full(d, u, dtype=np.int64))
            expect.append(2 if amb else 1)
            u += 1
    src, sc = np.concatenate(src), np.concatenate(sc)
    if shuffled:
        p = rng.permutation(len(src))
        src, sc = src[p], sc[p]
    return src, sc, u, np.array(expect, dtype=np.uint8)


@pytest.mark.parametrize("limits", [None, (4, 256)], ids=["default", "short4_lds256"])
@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
def test_ties_zeros_inf_nan_in_every_class(eng, monkeypatch, shuffled, limits):
    smax, lmax = limits or (SHORT_MAX, LDS_MAX)
    if limits:
        monkeypatch.setenv("GSPARSE_SEGK_SHORT_MAX", str(smax))
        monkeypatch.setenv("GSPARSE_SEGK_LDS_MAX", str(lmax))
    k = 3
    src, sc, n, expect = tie_graph(k, 3, shuffled)
    info, status = check(eng, sc, src, n, k, smax=smax, lmax=lmax)
    assert np.array_equal(status, expect)
    for c in (["short", "lds"] if not limits else ["lds", "stream"]):
        assert info["classes"][c] > 0, c


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
def test_k1_agrees_with_segment_argmax(eng, shuffled):
    """Status 2 exactly where gs_segment_argmax gives -2; the decided picks agree."""
    src, sc, n, _ = tie_graph(1, 4, shuffled)
    lengths = [0, 1, 2, 1, 0, 70]
    s2, c2 = segments(lengths, 5, shuffled)
    src = np.concatenate([src, s2 + n])
    sc = np.concatenate([sc, c2])
    n += len(lengths)
    _, status = check(eng, sc, src, n, 1)
    mask, _, _ = eng.segment_topk(sc, src, n, 1)
    pick = eng.segment_argmax(sc, src, n)
    assert np.array_equal(status == 2, pick == -2)
    assert np.array_equal(status == 0, pick == -1)
    assert np.array_equal(np.sort(np.nonzero(mask)[0]), np.sort(pick[pick >= 0]))
    assert (src[pick[pick >= 0]] == np.nonzero(pick >= 0)[0]).all()


@pytest.mark.parametrize("k", [2, 3])
def test_duplicate_columns_and_heavy_ties(eng, k):
    """directed_dup repeats (src, dst) columns (its scores are per coalesced entry, fewer
    than its columns, so the scores here are per column): few distinct values, then
    distinct ones."""
    g = load_golden("directed_dup")
    ei, n = g["edge_index"], int(g["num_nodes"])
    E = ei.shape[1]
    assert len(set(zip(ei[0].tolist(), ei[1].tolist()))) < E
    rng = np.random.default_rng(7)
    info, _ = check(eng, rng.integers(0, 6, E) / 4.0, ei[0], n, k)
    assert info["n_ambiguous"] > 0
    info, _ = check(eng, rng.permutation(E).astype(np.float64), ei[0], n, k)
    assert info["n_ambiguous"] == 0


# ---- 4. end to end -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rmat12():
    from gsparse import graphs

    return graphs.rmat(12, 8, seed=6), 1 << 12


@pytest.mark.parametrize("metric", ["jaccard", "degree", "approx_er"])
def test_degree_aware_device_equals_host_for_any_budget(gs, metric):
    from gsparse.selection import degree_aware_mask, degree_aware_mask_device

    ei, n = rmat12()
    data = gs.Data(edge_index=torch.from_numpy(ei), num_nodes=n)
    sp_ = gs.GraphSparsifier(data, "cpu")
    if metric == "approx_er":
        sc = sp_._engine.approx_er(epsilon=0.9, blas_threads=1)
    else:
        sc = sp_.compute_scores(metric)
    E = ei.shape[1]
    for k in [2, 3, 5]:
        for r in [0.05, 0.2, 0.5, 0.8]:
            sel = {}
            dev = degree_aware_mask_device(sp_._engine, sc, ei, n, E, r, k, info=sel)
            assert sel["phase1"] == "device", (k, r)
            assert sel["classes"]["short"] > 0
            ref = degree_aware_mask(sc, ei, n, E, r, k)
            assert np.array_equal(ref, dev), (metric, k, r)
        if metric == "degree":
            assert sel["n_ambiguous"] > 0  # the reference's own call was needed and made


@pytest.mark.parametrize("name", ["rmat10", "cora_like"])
def test_sparsify_degree_aware_budget_two(gs, name):
    """Through the public call: device phase 1, the host restatement's mask."""
    from gsparse.selection import degree_aware_mask

    g = load_golden(name)
    ei, n = g["edge_index"], int(g["num_nodes"])
    data = gs.Data(edge_index=torch.from_numpy(ei), num_nodes=n)
    sp_ = gs.GraphSparsifier(data, "cpu")
    sc = sp_.compute_scores("jaccard")
    sd, mask = sp_.sparsify_degree_aware("jaccard", 0.5, min_edges_per_node=2, return_mask=True)
    assert sp_.last_selection["phase1"] == "device"
    ref = degree_aware_mask(sc, ei, n, ei.shape[1], 0.5, 2)
    assert np.array_equal(mask.numpy(), ref)
    assert sd.edge_index.shape[1] == int(ref.sum())
    # the paths that stay as they were say which one ran
    _, m0 = sp_.sparsify_degree_aware("jaccard", 0.5, min_edges_per_node=0, return_mask=True)
    assert sp_.last_selection["phase1"] == "host"
    assert np.array_equal(m0.numpy(), degree_aware_mask(sc, ei, n, ei.shape[1], 0.5, 0))
    _, m1 = sp_.sparsify_degree_aware("jaccard", 0.5, min_edges_per_node=1, return_mask=True)
    assert sp_.last_selection["phase1"] == "device"
    assert np.array_equal(m1.numpy(), g["degaware_jaccard_0.5"].astype(bool))


def test_sparsify_degree_aware_budget_two_on_directed_dup(gs):
    """directed_dup has fewer scores (coalesced entries) than columns: the reference
    raises IndexError from scores[incident] (the golden records it for every metric),
    and so do the host restatement and the public call, for min_edges_per_node = 2
    as for 1 -- the same behaviour on both sides, which is all "equal" can mean here."""
    from gsparse.selection import degree_aware_mask

    g = load_golden("directed_dup")
    assert str(g["degaware_jaccard_0.5_error"]) == "IndexError"
    ei, n = g["edge_index"], int(g["num_nodes"])
    data = gs.Data(edge_index=torch.from_numpy(ei), num_nodes=n)
    sp_ = gs.GraphSparsifier(data, "cpu")
    sc = sp_.compute_scores("jaccard")
    assert len(sc) < ei.shape[1]
    with pytest.raises(IndexError):
        degree_aware_mask(sc, ei, n, ei.shape[1], 0.5, 2)
    with pytest.raises(IndexError):
        sp_.sparsify_degree_aware("jaccard", 0.5, min_edges_per_node=2, return_mask=True)
    assert sp_.last_selection["phase1"] == "host"


# ---- 5. errors -----------------------------------------------------------------
def test_errors(gs, eng):
    from gsparse.selection import degree_aware_mask_device

    src = np.array([0, 0, 1, 1, 1], dtype=np.int64)
    sc = np.arange(5, dtype=np.float64)
    with pytest.raises(IndexError):
        eng.segment_topk(sc[:4], src, 2, 2)
    with pytest.raises(IndexError):
        degree_aware_mask_device(eng, sc[:4], np.stack([src, src]), 2, 5, 0.5, 2)
    for bad in ([0, 0, 2, 1, 1], [0, -1, 1, 1, 1]):
        with pytest.raises(ValueError):
            eng.segment_topk(sc, np.array(bad, dtype=np.int64), 2, 2)
    with pytest.raises(ValueError):
        eng.segment_topk(sc, src, 2, 0)
    # through the ABI: k = 0 and short scores are GS_EINVAL
    L, h = gs._lib.lib(), eng.ctx.handle
    mask, status = np.zeros(5, dtype=np.uint8), np.zeros(2, dtype=np.uint8)
    counts = np.zeros(5, dtype=np.int64)
    ng, na = ctypes.c_int64(0), ctypes.c_int64(0)

    def call(nscores, k):
        return L.gs_segment_topk(h, sc.ctypes.data, 0, nscores, src.ctypes.data, 0, 5, 2, k,
                                 mask.ctypes.data, 0, status.ctypes.data, 0, ctypes.byref(ng),
                                 ctypes.byref(na), counts.ctypes.data, 5)

    assert call(5, 0) == gs._lib.GS_EINVAL
    assert call(4, 2) == gs._lib.GS_EINVAL
    assert call(5, 2) == gs._lib.GS_OK
    assert mask.tolist() == [1, 1, 0, 1, 1] and status.tolist() == [1, 1]
    assert (ng.value, na.value) == (4, 0) and counts.tolist() == [0, 1, 1, 0, 0]
    # the context still works after the refused calls
    m, s, info = eng.segment_topk(sc, src, 3, 1)
    assert m.tolist() == [False, True, False, False, True] and s.tolist() == [1, 1, 0]
