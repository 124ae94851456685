"""GPU tests of the symmetric random baseline on the device: gs_undirected_ids against
np.unique(return_inverse=True), gs_random_mask against the reference's two NumPy lines,
the resident RandomBaseline handle and the public functions against the goldens.  Every
expected value is NumPy's, computed here, or a committed golden."""

import ctypes

import numpy as np
import pytest
import torch

import random_cases as C
from conftest import bits_equal, golden_names, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    from gsparse import random as R

    return R


@pytest.fixture(scope="module")
def eng():
    from gsparse._lib import Context
    from gsparse.engine import Engine

    return Engine(Context(0))


def _check_golden(R, name, device):
    g = load_golden(name)
    data = C.golden_data(g, device)
    us, inv = R.precompute_random_scores(data, seed=42)
    assert R.last_selection["path"] == "device"
    assert type(us) is np.ndarray and us.dtype == np.float64
    assert type(inv) is np.ndarray and inv.dtype == np.int64
    assert np.array_equal(inv, g["random_inverse"])
    assert bits_equal(us, g["random_undirected"])
    for r in (0.8, 0.5, 0.2):
        sd = R.random_sparsify(data, us, inv, r, "cpu")
        assert R.last_selection["path"] == "device", (name, r, R.last_selection)
        assert np.array_equal(sd.edge_index.numpy(), g[f"random_sparsify_{r}"]), (name, r)


@pytest.mark.parametrize("device", [None, "cuda:0"], ids=["host", "device"])
@pytest.mark.parametrize("name", golden_names(include_big=False))
def test_goldens(R, name, device):
    _check_golden(R, name, device)


def test_golden_roman_full(R):
    _check_golden(R, "roman_full", "cuda:0")


# ---- gs_undirected_ids vs np.unique ---------------------------------------------------
@pytest.mark.parametrize("n", C.NODE_COUNTS)
def test_undirected_ids_match_np_unique(eng, n):
    for E in C.ID_SIZES:
        ei = C.multigraph(E, n, seed=E + n)
        want, cnt = C.np_inverse(ei[0], ei[1], n)
        inv, got_cnt, status = eng.undirected_ids(ei[0], ei[1], n)
        assert status == 0 and got_cnt == cnt, (n, E)
        assert inv.dtype == np.int64 and np.array_equal(inv, want), (n, E)
        t = torch.from_numpy(ei).cuda()
        out = torch.full((E,), -7, dtype=torch.int64, device="cuda")
        inv_d, got_cnt, status = eng.undirected_ids(t[0], t[1], n, out=out)
        assert status == 0 and got_cnt == cnt and inv_d is out
        assert np.array_equal(out.cpu().numpy(), want), (n, E)


def test_undirected_ids_grid_stride(eng):
    E, n = C.GRID_STRIDE_E, 1000
    ei = C.multigraph(E, n, seed=5)
    want, cnt = C.np_inverse(ei[0], ei[1], n)
    inv, got_cnt, status = eng.undirected_ids(ei[0], ei[1], n)
    assert status == 0 and got_cnt == cnt
    assert np.array_equal(inv, want)


def test_undirected_ids_large_node_count(eng):
    """n = 2^31 - 1: keys near 2^62."""
    n = (1 << 31) - 1
    src = np.array([n - 1, 0, n - 1, n - 2, 5, n - 1, 0], dtype=np.int64)
    dst = np.array([n - 1, n - 1, 0, n - 1, 5, n - 2, 0], dtype=np.int64)
    want, cnt = C.np_inverse(src, dst, n)
    inv, got_cnt, status = eng.undirected_ids(src, dst, n)
    assert status == 0 and got_cnt == cnt and np.array_equal(inv, want)


def test_undirected_ids_status_gate(eng, R):
    from gsparse import Data

    a = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731
    out = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    for src, dst in ((a(0, 4, 1), a(1, 2, 3)), (a(0, 1, 1), a(1, -1, 3))):  # id == n, id < 0
        assert eng.undirected_ids(src, dst, 4)[2] == 1
        s, d = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
        assert eng.undirected_ids(s, d, 4, out=out)[2] == 1
        assert bool((out == -7).all())  # nothing was written
        # the public function then behaves as the reference does
        data = Data(edge_index=torch.from_numpy(np.stack([src, dst])), num_nodes=4)
        us, inv = R.precompute_random_scores(data)
        assert R.last_selection["path"] == "host"
        want, cnt = C.np_inverse(src, dst, 4)
        assert np.array_equal(inv, want) and bits_equal(us, np.random.default_rng(42).random(cnt))
    assert eng.undirected_ids(a(), a(), 4)[2] == 1  # E = 0
    assert eng.undirected_ids(a(0, 1, 2), a(1, 2, 0), 1 << 31)[2] == 1  # n >= 2^31
    for dev in ("cpu", "cuda:0"):
        data = Data(edge_index=torch.zeros((2, 0), dtype=torch.int64, device=dev), num_nodes=4)
        with pytest.raises(ValueError):
            R.precompute_random_scores(data)


# ---- gs_random_mask vs the two NumPy lines --------------------------------------------
def _data(ei, n, device=None):
    from gsparse import Data

    t = torch.from_numpy(ei)
    return Data(edge_index=t if device is None else t.to(device), num_nodes=n)


@pytest.mark.parametrize("m", C.MASK_SIZES)
def test_random_sparsify_matches_numpy(R, m):
    s, inv, ei = C.mask_case(m, seed=m)
    E = ei.shape[1]
    for device in (None, "cuda:0"):
        data = _data(ei, E, device)
        for r in C.RETENTIONS:
            sd = R.random_sparsify(data, s, inv, r, "cpu")
            if r == 1.0:
                assert np.array_equal(sd.edge_index.cpu().numpy(), ei)
                continue
            assert R.last_selection["path"] == "device", (m, r, R.last_selection)
            want = ei[:, C.np_keep_mask(s, inv, r)]
            assert np.array_equal(sd.edge_index.numpy(), want), (m, r, device)


@pytest.mark.parametrize("m", [257, 70001])
def test_crowded_scores_tie_rules(R, m):
    s, inv, ei = C.mask_case(m, seed=m + 1, crowded=True)
    E = ei.shape[1]
    data = _data(ei, E, "cuda:0")
    seen_ambiguous = False
    for r in (0.2, 0.5, 0.999):
        sd = R.random_sparsify(data, s, inv, r, "cpu")  # tie_break="numpy"
        seen_ambiguous = seen_ambiguous or R.last_selection["ambiguous"]
        assert np.array_equal(sd.edge_index.numpy(), ei[:, C.np_keep_mask(s, inv, r)]), (m, r)
        sd = R.random_sparsify(data, s, inv, r, "cpu", tie_break="stable")
        assert R.last_selection["path"] == "device"
        assert np.array_equal(sd.edge_index.numpy(), ei[:, C.np_keep_mask(s, inv, r, kind="stable")]), (m, r)
    assert seen_ambiguous


def test_signed_zero_and_infinite_scores(eng):
    s = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 0.0, -0.0, np.inf, 2.0, -np.inf, 0.5])
    m = len(s)
    inv = np.arange(-m, m, dtype=np.int64)
    for n_keep in range(1, m + 1):
        mask, cut, beyond, tied = eng.random_mask(s, inv, n_keep, 2 * m)
        keep_undir = np.zeros(m, dtype=bool)
        keep_undir[np.argsort(s, kind="stable")[-n_keep:]] = True
        assert np.array_equal(mask, keep_undir[inv]), n_keep
        assert beyond + min(tied, n_keep - beyond) == n_keep


def test_inverse_out_of_bounds_raises(eng, R):
    m = 257
    s, inv, ei = C.mask_case(m, seed=3)
    E = ei.shape[1]
    mask, *_ = eng.random_mask(s, inv, 100, E)  # entries in [-m, 0) wrap like NumPy
    keep_undir = np.zeros(m, dtype=bool)
    keep_undir[np.argsort(s)[-100:]] = True
    assert (inv < 0).any() and np.array_equal(mask, keep_undir[inv])
    for bad_entry in (m, -m - 1):
        bad = inv.copy()
        bad[E // 2] = bad_entry
        with pytest.raises(IndexError):
            keep_undir[bad]
        with pytest.raises(IndexError):
            eng.random_mask(s, bad, 100, E)
        with pytest.raises(IndexError):
            R.random_sparsify(_data(ei, E), s, bad, 0.4, "cpu")
        d_out = torch.empty(E, dtype=torch.bool, device="cuda")
        with pytest.raises(IndexError):
            eng.random_mask(torch.from_numpy(s).cuda(), torch.from_numpy(bad).cuda(), 100, E, out=d_out)


# ---- RandomBaseline -------------------------------------------------------------------
@pytest.mark.parametrize("device", [None, "cuda:0"], ids=["host", "device"])
def test_handle_sweep_nesting_symmetry(R, device, monkeypatch):
    import gsparse

    n = 1000
    ei = C.multigraph(4097, n, seed=9)
    data = _data(ei, n, device)
    rb = gsparse.RandomBaseline(data, seed=42)
    assert rb.path == "device"
    want_inv, cnt = C.np_inverse(ei[0], ei[1], n)
    assert rb.n_undirected == cnt
    assert type(rb.inverse_idx) is np.ndarray and np.array_equal(rb.inverse_idx, want_inv)
    assert bits_equal(rb.undirected_scores, np.random.default_rng(42).random(cnt))
    rates = [0.9, 0.6, 0.3]
    swept = rb.sweep(rates, "cpu")
    masks = []
    for r, sd in zip(rates, swept):
        one = R.random_sparsify(data, rb.undirected_scores, rb.inverse_idx, r, "cpu")
        assert np.array_equal(sd.edge_index.numpy(), one.edge_index.numpy()), r
        assert np.array_equal(sd.edge_index.numpy(), ei[:, C.np_keep_mask(rb.undirected_scores, want_inv, r)])
        mk = rb.mask(r)
        assert rb.last_selection["path"] == "device" and not rb.last_selection["ambiguous"]
        assert mk.dtype == torch.bool and mk.device == data.edge_index.device
        masks.append(mk.cpu().numpy())
    assert (masks[1] <= masks[0]).all() and (masks[2] <= masks[1]).all()  # the masks nest
    assert masks[2].sum() < masks[1].sum() < masks[0].sum()
    # both directions of an undirected pair (every column of its key) share their bit
    for mk in masks:
        per_key = np.zeros(cnt, dtype=np.int64)
        np.add.at(per_key, want_inv, mk)
        assert np.array_equal(per_key, np.bincount(want_inv, minlength=cnt) * (per_key > 0))
    assert bool(rb.mask(1.0).all())
    other = gsparse.RandomBaseline(data, seed=7)
    assert not np.array_equal(other.undirected_scores, rb.undirected_scores)
    assert not np.array_equal(other.mask(0.6).cpu().numpy(), masks[1])
    # the host form gives the same results
    monkeypatch.setenv("GSPARSE_RANDOM", "host")
    hb = gsparse.RandomBaseline(data, seed=42)
    assert hb.path == "host"
    assert bits_equal(hb.undirected_scores, rb.undirected_scores)
    assert np.array_equal(hb.inverse_idx, rb.inverse_idx)
    for mk, r in zip(masks, rates):
        assert np.array_equal(hb.mask(r).cpu().numpy(), mk)
        assert hb.last_selection["path"] == "host"


def test_handle_stable_tie_break_on_crowded_scores(R):
    """A handle whose resident scores are replaced by crowded ones: "numpy" makes the
    reference's call, "stable" keeps the device's rule."""
    import gsparse

    n = 1000
    ei = C.multigraph(4097, n, seed=11)
    want_inv, cnt = C.np_inverse(ei[0], ei[1], n)
    crowded = np.round(np.random.default_rng(1).random(cnt), 2)
    for tb, kind in (("numpy", None), ("stable", "stable")):
        rb = gsparse.RandomBaseline(_data(ei, n, "cuda:0"), tie_break=tb)
        rb._d_scores = torch.from_numpy(crowded).cuda()
        rb._scores = None
        got = rb.mask(0.5).cpu().numpy()
        assert rb.last_selection["ambiguous"]
        assert rb.last_selection["path"] == ("host" if tb == "numpy" else "device")
        assert np.array_equal(got, C.np_keep_mask(crowded, want_inv, 0.5, kind=kind)), tb


# ---- the C ABI directly ---------------------------------------------------------------
def test_c_abi_argument_checks(eng):
    from gsparse import _lib
    from gsparse._lib import GS_EINVAL, GS_HOST, ptr

    L = _lib.lib()
    src = np.array([0, 1], dtype=np.int64)
    inv = np.zeros(2, dtype=np.int64)
    cnt, status = ctypes.c_int64(0), ctypes.c_int32(0)
    assert L.gs_undirected_ids(None, 4, 2, ptr(src), ptr(src), GS_HOST, ptr(inv), GS_HOST,
                               ctypes.byref(cnt), ctypes.byref(status)) == GS_EINVAL
    s = np.array([0.5, 0.25])
    mask = np.zeros(2, dtype=np.uint8)
    cut, nb, nt, bad = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    tail = (ctypes.byref(cut), ctypes.byref(nb), ctypes.byref(nt), ctypes.byref(bad))
    assert L.gs_random_mask(None, ptr(s), GS_HOST, 2, 1, ptr(inv), GS_HOST, 2, ptr(mask), GS_HOST,
                            *tail) == GS_EINVAL
    h = eng.ctx.handle
    for n_keep in (0, -3):
        assert L.gs_random_mask(h, ptr(s), GS_HOST, 2, n_keep, ptr(inv), GS_HOST, 2, ptr(mask),
                                GS_HOST, *tail) == GS_EINVAL
        assert b"n_keep" in L.gs_last_error()
    assert L.gs_random_mask(h, ptr(s), GS_HOST, 2, 1, ptr(inv), GS_HOST, 2, ptr(mask), GS_HOST,
                            *tail) == 0
    assert mask.tolist() == [1, 1] and (nb.value, bad.value) == (0, 0) and cut.value == 0.5
