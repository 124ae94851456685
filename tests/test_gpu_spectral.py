"""GPU tests of spectral sparsification by effective-resistance sampling on the device:
gs_spectral_sample against the specification (gsparse.selection.spectral_sample, NumPy
calls only) bit for bit, its edge inputs and status gate, GraphSparsifier.sparsify_spectral
on the goldens, and one end-to-end run whose weighted result is measured spectrally."""

import ctypes

import numpy as np
import pytest
import torch

import spectral_cases as C
from conftest import bits_equal, load_golden
from random_cases import golden_data

pytestmark = pytest.mark.gpu

METHODS = ["multinomial", "independent"]


@pytest.fixture(scope="module")
def S():
    from gsparse import selection

    return selection


@pytest.fixture(scope="module")
def eng():
    from gsparse._lib import Context
    from gsparse.engine import Engine

    return Engine(Context(0))


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _device(eng, s, ei, n, q, seed, method, cuda=False):
    rng = np.random.default_rng(seed)
    if cuda:
        t = torch.from_numpy(ei).cuda()
        return eng.spectral_sample(torch.from_numpy(s).cuda(), t[0], t[1], n, q, rng, method)
    return eng.spectral_sample(s, ei[0], ei[1], n, q, rng, method)


def _assert_same(got, want, q, method, where=None):
    mask, w, cnt, inv, info = got
    wmask, ww, wcnt, winv = want
    assert info["status"] == 0, where
    mask, w, cnt, inv = _np(mask), _np(w), _np(cnt), _np(inv)
    assert mask.dtype == bool and w.dtype == np.float64 and cnt.dtype == np.int64 and inv.dtype == np.int64
    assert np.array_equal(inv, winv), where
    assert info["m"] == len(wcnt) and np.array_equal(cnt, wcnt), where
    assert np.array_equal(mask, wmask), where
    assert np.array_equal(w.view(np.uint64), np.ascontiguousarray(ww).view(np.uint64)), where
    assert info["draws"] == (q if method == "multinomial" else len(wcnt)), where
    assert info["max_count"] == wcnt.max() and info["kept_pairs"] == (wcnt > 0).sum(), where


# ---- gs_spectral_sample against the specification --------------------------------------
@pytest.mark.parametrize("m", C.PAIR_COUNTS)
def test_matches_spec(S, eng, m):
    ei, n = C.sym_graph(m, seed=m)
    s = C.column_scores(ei.shape[1], m)
    for q in C.DRAW_COUNTS + [5 * m]:
        for seed in C.SEEDS:
            want = S.spectral_sample(s, ei, n, q, seed=seed)
            _assert_same(_device(eng, s, ei, n, q, seed, "multinomial"), want, q, "multinomial",
                         (m, q, seed))
            if q in (9, 5 * m):
                _assert_same(_device(eng, s, ei, n, q, seed, "multinomial", cuda=True), want, q,
                             "multinomial", (m, q, seed, "cuda"))
    for q in (1, max(1, m // 2), 5 * m):
        for seed in C.SEEDS:
            want = S.spectral_sample(s, ei, n, q, seed=seed, method="independent")
            for cuda in (False, True):
                _assert_same(_device(eng, s, ei, n, q, seed, "independent", cuda), want, q, "independent",
                             (m, q, seed, cuda))


def test_device_results_stay_on_the_device(eng):
    ei, n = C.sym_graph(257, seed=1)
    s = C.column_scores(ei.shape[1], 1)
    mask, w, cnt, inv, info = _device(eng, s, ei, n, 300, 42, "multinomial", cuda=True)
    assert all(t.is_cuda for t in (mask, w, cnt, inv))
    assert mask.dtype == torch.bool and w.dtype == torch.float64
    assert cnt.shape == (info["m"],) and inv.shape == (ei.shape[1],)
    assert info["n_irregular"] == 0


# ---- edge inputs -------------------------------------------------------------------------
def test_hot_pair_takes_every_draw(S, eng):
    ei, n = C.sym_graph(1025, seed=3)
    _, inv = C.pair_probs(np.ones(ei.shape[1]), ei, n)
    s = np.full(ei.shape[1], 1e-300)
    s[inv == 700] = 1.0
    q = 100_000
    want = S.spectral_sample(s, ei, n, q, seed=42)
    assert want[2][700] == q
    got = _device(eng, s, ei, n, q, 42, "multinomial")
    _assert_same(got, want, q, "multinomial")
    assert got[4]["max_count"] == q and got[4]["kept_pairs"] == 1


@pytest.mark.parametrize("method", METHODS)
def test_zero_and_odd_scores(S, eng, method):
    m = 4099
    ei, n = C.sym_graph(m, seed=8, loops=41)
    E = ei.shape[1]
    cases = {
        "zeros40": C.column_scores(E, 2, kind="zeros40"),
        "zero_ends": C.zero_ends(C.column_scores(E, 3), ei, n),
        "odd": C.column_scores(E, 4, kind="odd"),  # NaN, +-inf, -0.0, negative, denormal
    }
    p, _ = C.pair_probs(cases["zero_ends"], ei, n)
    assert p[0] == 0 and p[-1] == 0
    for name, s in cases.items():
        for q in (m // 2, 6 * m):
            want = S.spectral_sample(s, ei, n, q, seed=7, method=method)
            for cuda in (False, True):
                got = _device(eng, s, ei, n, q, 7, method, cuda)
                _assert_same(got, want, q, method, (name, q, cuda))
                assert got[4]["n_irregular"] == 0  # loops do not count
                assert not _np(got[0])[ei[0] == ei[1]].any()


@pytest.mark.parametrize("method", METHODS)
def test_directions_with_different_scores(S, eng, method):
    """Shuffled columns whose two directions carry different scores: the lower column's
    score is the pair's."""
    ei, n = C.sym_graph(3001, seed=12)
    E = ei.shape[1]
    s = C.column_scores(E, 6)
    want = S.spectral_sample(s, ei, n, 2500, seed=0, method=method)
    _assert_same(_device(eng, s, ei, n, 2500, 0, method), want, 2500, method)
    inv = want[3]
    last = np.zeros(3001, dtype=np.int64)
    np.maximum.at(last, inv, np.arange(E))
    s2 = s.copy()
    s2[last] = 99.0  # the higher column of every pair: not read
    got = _device(eng, s2, ei, n, 2500, 0, method)
    _assert_same(got, want, 2500, method)


@pytest.mark.parametrize("method", METHODS)
def test_multigraph_and_n_irregular(S, eng, method):
    """One-way columns, a triple column, duplicates and loops: the result is still the
    specification's and n_irregular counts the non-loop pairs without exactly two columns."""
    small = np.array([[0, 1, 1, 2, 3, 3, 4, 2, 5, 5], [1, 0, 2, 2, 4, 4, 3, 1, 0, 5]], dtype=np.int64)
    # pairs: {0,1} x2, {1,2} x2, {2,2} loop, {3,4} x3 (a triple), {0,5} one way, {5,5} loop
    assert C.np_irregular(small, 6) == 2
    s = np.linspace(0.5, 1.5, small.shape[1])
    got = _device(eng, s, small, 6, 50, 42, method)
    _assert_same(got, S.spectral_sample(s, small, 6, 50, seed=42, method=method), 50, method)
    assert got[4]["n_irregular"] == 2
    for E, n in ((4097, 1000), (20011, 3000)):
        ei = C.multigraph(E, n, seed=E)
        s = C.column_scores(E, E, kind="odd")
        for cuda in (False, True):
            got = _device(eng, s, ei, n, 2 * E, 42, method, cuda)
            _assert_same(got, S.spectral_sample(s, ei, n, 2 * E, seed=42, method=method), 2 * E, method)
            assert got[4]["n_irregular"] == C.np_irregular(ei, n) > 0


def test_status_gate_leaves_outputs_untouched(S, eng):
    from gsparse._lib import GS_DEVICE, GS_EINVAL, ptr
    from gsparse import _lib

    ei, n = C.sym_graph(300, seed=5)
    E = ei.shape[1]
    s = C.column_scores(E, 5)
    bad_id, neg_id = ei.copy(), ei.copy()
    bad_id[1, 7] = n
    neg_id[0, 9] = -1
    loops = np.stack([ei[0], ei[0]])
    degenerate = {
        "id == n": (s, bad_id, n, 10),
        "id < 0": (s, neg_id, n, 10),
        "n >= 2^31": (s, ei, 1 << 31, 10),
        "nscores < E": (s[:-1], ei, n, 10),
        "total 0": (np.zeros(E), ei, n, 10),
        "total inf": (np.full(E, 1e308), ei, n, 10),
        "loops only": (s, loops, n, 10),
        "q = 0": (s, ei, n, 0),
        "q = 2^31": (s, ei, n, 1 << 31),
    }
    L = _lib.lib()
    h = eng.ctx.handle
    words = eng._pcg64_words(np.random.default_rng(42))
    for name, (sc, e, nn, q) in degenerate.items():
        for method in METHODS:
            assert _device(eng, sc, e, nn, q, 42, method)[4]["status"] == 1, name
        # device buffers: nothing is written
        ds = torch.from_numpy(np.ascontiguousarray(sc)).cuda()
        de = torch.from_numpy(e).cuda()
        mask = torch.full((E,), 7, dtype=torch.uint8, device="cuda")
        w = torch.full((E,), -7.0, dtype=torch.float64, device="cuda")
        cnt = torch.full((E,), -7, dtype=torch.int64, device="cuda")
        inv = torch.full((E,), -7, dtype=torch.int64, device="cuda")
        out = [ctypes.c_int64(-5) for _ in range(5)]
        status = ctypes.c_int32(-5)
        rc = L.gs_spectral_sample(h, ptr(ds), GS_DEVICE, len(sc), ptr(de[0].contiguous()),
                                  ptr(de[1].contiguous()), GS_DEVICE, E, nn, q, 0, *words, ptr(mask),
                                  GS_DEVICE, ptr(w), GS_DEVICE, ptr(cnt), GS_DEVICE, ptr(inv), GS_DEVICE,
                                  *[ctypes.byref(o) for o in out], ctypes.byref(status))
        torch.cuda.synchronize()
        assert rc == 0 and status.value == 1, name
        assert bool((mask == 7).all()) and bool((w == -7.0).all()), name
        assert bool((cnt == -7).all()) and bool((inv == -7).all()), name
        assert all(o.value == -5 for o in out), name
        # the Python layer then evaluates the specification, whose exception surfaces
        # (ids outside the device contract are no error for NumPy)
        if name not in ("id == n", "id < 0", "n >= 2^31"):
            with pytest.raises(ValueError):
                S.spectral_sample(sc, e, nn, q)
            with pytest.raises(ValueError):
                S.spectral_mask_device(eng, sc, e, nn, q)
    # ids the device does not take but NumPy does: the host path gives the specification
    info = {}
    got = S.spectral_mask_device(eng, s, ei, 1 << 31, 10, info=info)
    want = S.spectral_sample(s, ei, 1 << 31, 10)
    assert info["path"] == "host" and info["n_irregular"] == 0 and info["draws"] == 10
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    # an unknown method is an argument error
    mask = np.zeros(E, dtype=np.uint8)
    w = np.zeros(E)
    rc = L.gs_spectral_sample(h, ptr(s), 0, E, ptr(ei[0].copy()), ptr(ei[1].copy()), 0, E, n, 10, 2, *words,
                              ptr(mask), 0, ptr(w), 0, None, 0, None, 0, None, None, None, None, None,
                              ctypes.byref(status))
    assert rc == GS_EINVAL and b"method" in L.gs_last_error()
    with pytest.raises(ValueError):
        eng.spectral_sample(s, ei[0], ei[1], n, 10, np.random.default_rng(0), "poisson")


def test_two_calls_return_identical_bytes(eng):
    ei, n = C.sym_graph(70001, seed=4)
    s = C.column_scores(ei.shape[1], 4, kind="zeros40")
    for method in METHODS:
        a = _device(eng, s, ei, n, 300_000, 42, method, cuda=True)
        b = _device(eng, s, ei, n, 300_000, 42, method, cuda=True)
        for x, y in zip(a[:4], b[:4]):
            assert torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x.view(torch.int64),
                               y.view(torch.uint8) if y.dtype == torch.bool else y.view(torch.int64))
        assert a[4] == b[4]


def test_optional_outputs_may_be_null(S, eng):
    from gsparse import _lib
    from gsparse._lib import ptr

    ei, n = C.sym_graph(65, seed=2)
    E = ei.shape[1]
    s = C.column_scores(E, 2)
    want = S.spectral_sample(s, ei, n, 40, seed=42)
    mask, w = np.zeros(E, dtype=np.uint8), np.zeros(E)
    status = ctypes.c_int32(1)
    words = eng._pcg64_words(np.random.default_rng(42))
    src, dst = ei[0].copy(), ei[1].copy()
    rc = _lib.lib().gs_spectral_sample(eng.ctx.handle, ptr(s), 0, E, ptr(src), ptr(dst), 0, E, n, 40, 0,
                                       *words, ptr(mask), 0, ptr(w), 0, None, 0, None, 0, None, None, None,
                                       None, None, ctypes.byref(status))
    assert rc == 0 and status.value == 0
    assert np.array_equal(mask.view(bool), want[0]) and bits_equal(w, want[1])


# ---- GraphSparsifier.sparsify_spectral on the goldens ------------------------------------
@pytest.mark.parametrize("device", [None, "cuda:0"], ids=["host", "device"])
@pytest.mark.parametrize("name", ["karate_test", "rmat10", "cora_like"])
def test_sparsify_spectral_goldens(S, name, device):
    import gsparse

    g = load_golden(name)
    data = golden_data(g, device)
    ei = np.ascontiguousarray(g["edge_index"]).astype(np.int64)
    n, E = int(g["num_nodes"]), ei.shape[1]
    sp_ = gsparse.GraphSparsifier(data, "cuda:0")
    for metric in ("approx_er", "effective_resistance"):
        scores = sp_.compute_scores(metric)
        m = len(np.unique(np.minimum(ei[0], ei[1]) * (n + 1) + np.maximum(ei[0], ei[1])))
        for method in METHODS:
            for kw, q in (({"num_samples": 2 * m + 1}, 2 * m + 1),
                          ({"retention_ratio": 0.4}, max(1, int(m * 0.4)))):
                wmask, ww, wcnt, _ = S.spectral_sample(scores, ei, n, q, seed=7, method=method)
                sd, (mask, weight) = sp_.sparsify_spectral(metric, seed=7, method=method,
                                                           return_mask=True, **kw)
                where = (name, metric, method, kw)
                assert mask.dtype == torch.bool and weight.dtype == torch.float64
                assert mask.shape == weight.shape == (E,)
                assert np.array_equal(mask.numpy(), wmask), where
                assert bits_equal(weight.numpy(), ww), where
                assert sd.edge_index.is_cuda and sd.edge_weight.is_cuda
                assert sd.edge_weight.dtype == torch.float32
                assert np.array_equal(sd.edge_index.cpu().numpy(), ei[:, wmask]), where
                assert np.array_equal(sd.edge_weight.cpu().numpy(), ww[wmask].astype(np.float32)), where
                assert sp_.last_selection == {
                    "path": "device", "method": method, "m": m, "num_samples": q,
                    "kept_pairs": int((wcnt > 0).sum()), "max_count": int(wcnt.max()),
                    "draws": q if method == "multinomial" else m, "n_irregular": 0}, where
                only = sp_.sparsify_spectral(metric, seed=7, method=method, **kw)
                assert np.array_equal(only.edge_index.cpu().numpy(), ei[:, wmask])
    for kw in ({}, {"num_samples": 5, "retention_ratio": 0.5}, {"retention_ratio": 0.0},
               {"num_samples": 5, "method": "poisson"}, {"num_samples": 0}):
        with pytest.raises(ValueError):
            sp_.sparsify_spectral("approx_er", **kw)


def test_sparsify_spectral_rejects_merged_and_one_way_columns():
    import gsparse

    g = load_golden("directed_dup")  # its canonical CSR merged duplicate columns
    sp_ = gsparse.GraphSparsifier(golden_data(g, "cuda:0"), "cuda:0")
    with pytest.raises(ValueError, match="merged duplicate columns"):
        sp_.sparsify_spectral("approx_er", num_samples=100)
    # one score per column, but a pair in one direction only
    ei = torch.tensor([[0, 1, 1, 2, 2], [1, 0, 2, 1, 3]], dtype=torch.int64)
    sp_ = gsparse.GraphSparsifier(gsparse.Data(edge_index=ei.cuda(), num_nodes=4), "cuda:0")
    with pytest.raises(ValueError, match="exactly two"):
        sp_.sparsify_spectral("degree", num_samples=10)
    assert sp_.last_selection["n_irregular"] == 1


# ---- end to end --------------------------------------------------------------------------
def test_end_to_end_spectral_quality():
    """The dense 96-node graph sparsified on the device with the device's exact effective
    resistance: Courant-Fischer bounds the weighted result's algebraic connectivity by
    [lambda_min, lambda_max] * lambda_2(G), the extreme eigenvalues of the whitened
    Laplacian of that same result (computed on the host).  The interval is widened by the
    topology tests' tolerance for the device's Fiedler value (rtol 1e-6)."""
    import scipy.sparse as sp

    import gsparse

    ei, n = C.dense96()
    m = ei.shape[1] // 2
    data = gsparse.Data(edge_index=torch.from_numpy(ei).cuda(), num_nodes=n)
    sp_ = gsparse.GraphSparsifier(data, "cuda:0")
    sd, (mask, weight) = sp_.sparsify_spectral("effective_resistance", num_samples=m, seed=42,
                                               return_mask=True)
    assert sp_.last_selection["path"] == "device" and sp_.last_selection["kept_pairs"] <= 1500
    mask, weight = mask.numpy(), weight.numpy()
    L = C.laplacian(ei, n)
    lam = C.whitened_eigs(L, C.laplacian(ei[:, mask], n, weight[mask]))
    assert 0.5 < lam[0] and lam[-1] < 1.6
    kept = sd.edge_index.cpu().numpy()
    assert np.array_equal(kept, ei[:, mask])
    assert np.array_equal(sd.edge_weight.cpu().numpy(), weight[mask].astype(np.float32))
    # the float64 weights: the very graph whose whitened eigenvalues were taken
    adj = sp.csr_matrix((weight[mask], (kept[0], kept[1])), shape=(n, n))
    got = gsparse.compute_topology_metrics(adj)
    assert got["num_connected_components"] == 1
    lam2 = np.linalg.eigvalsh(L)[1]
    print("fiedler", got["algebraic_connectivity"], "bounds", lam[0] * lam2, lam[-1] * lam2)
    tol = 1e-6
    assert lam[0] * lam2 * (1 - tol) <= got["algebraic_connectivity"] <= lam[-1] * lam2 * (1 + tol)
