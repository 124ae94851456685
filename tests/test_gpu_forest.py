"""GPU tests of the maximum spanning forest on the device (gs_spanning_forest) and of the
connectivity-preserving top-k built on it: the mask, |F| and the marked count against
Kruskal's walk on the host (selection.spanning_forest_host / connected_mask) for
equality, the label partition against SciPy's.  Every expected value is computed on the
host, once per case."""

import ctypes
import math

import numpy as np
import pytest
import torch

import forest_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from gsparse._lib import Context
    from gsparse.engine import Engine

    return Engine(Context(0))


def _case(name):
    if name in C.SMALL:
        return C.SMALL[name]
    ei, n, s = C.generated(name)
    return n, ei, s


def _check(eng, name, keep_lowest, expand):
    n, ei, s = _case(name)
    forest, guaranteed, c, lab = C.kruskal(name, keep_lowest)
    want = guaranteed if expand else forest
    mask, labels, info = eng.spanning_forest(s, ei[0], ei[1], n, keep_lowest, expand)
    assert mask.dtype == bool and mask.shape == (ei.shape[1],)
    assert np.array_equal(mask, want), (name, keep_lowest, expand)
    assert info["n_forest"] == int(forest.sum()) == n - c
    assert info["n_marked"] == int(want.sum())
    assert labels.dtype == np.int32 and labels.shape == (n,)
    assert np.array_equal(C.partition(labels), lab)
    assert info["rounds"] <= (math.ceil(math.log2(n)) if n > 1 else 0)
    return mask, labels, info


@pytest.mark.parametrize("expand", [False, True], ids=["forest", "expanded"])
@pytest.mark.parametrize("keep_lowest", [False, True], ids=["top", "lowest"])
@pytest.mark.parametrize("name", sorted(C.SMALL))
def test_forest_equals_kruskal(eng, name, keep_lowest, expand):
    _check(eng, name, keep_lowest, expand)


def test_rounds_and_shapes(eng):
    assert _check(eng, "triangle_equal", False, False)[2]["n_forest"] == 2
    assert _check(eng, "path_ascending", False, False)[2]["rounds"] == 1  # one chain of depth n - 1
    assert _check(eng, "path_ruler", False, False)[2]["rounds"] == 12
    assert _check(eng, "empty", False, True)[2] == {"n_forest": 0, "n_marked": 0, "rounds": 0}
    mask, _, info = _check(eng, "tree", False, True)
    assert mask.all() and info["n_marked"] == 78  # a tree is kept whole


def test_two_runs_give_identical_bytes(eng):
    for name in ("rmat10_equal", "star_5000_equal", "special_values"):
        n, ei, s = _case(name)
        a = eng.spanning_forest(s, ei[0], ei[1], n, False, True)
        b = eng.spanning_forest(s, ei[0], ei[1], n, False, True)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


@pytest.mark.parametrize("name", ["rmat10_shuffled", "special_values", "empty"])
def test_cuda_tensors_with_out_equal_the_numpy_path(eng, name):
    n, ei, s = _case(name)
    E = ei.shape[1]
    for keep_lowest in (False, True):
        for expand in (False, True):
            mask, labels, info = eng.spanning_forest(s, ei[0], ei[1], n, keep_lowest, expand)
            t = torch.from_numpy(np.ascontiguousarray(ei)).cuda()
            out = torch.full((E + 3,), 7, dtype=torch.uint8, device="cuda")
            m2, l2, i2 = eng.spanning_forest(torch.from_numpy(np.array(s)).cuda(), t[0], t[1], n,
                                             keep_lowest, expand, out=out)
            assert m2 is out and l2.is_cuda and l2.dtype == torch.int32
            assert np.array_equal(out[:E].cpu().numpy().astype(bool), mask)
            assert (out[E:] == 7).all()
            assert np.array_equal(l2.cpu().numpy(), labels) and i2 == info


@pytest.mark.parametrize("name", ["rmat14", "roman2000"])
def test_connected_mask_device_with_device_jaccard(eng, name):
    from gsparse import selection as S
    from gsparse._lib import Context
    from gsparse.engine import Engine

    ei, n, s_host = C.generated(name)
    E = ei.shape[1]
    ctx = Context(0)
    ctx.set_graph_edge_index(n, np.ascontiguousarray(ei[0]), np.ascontiguousarray(ei[1]))
    s = Engine(ctx).jaccard()
    assert np.array_equal(s.view(np.uint64), s_host.view(np.uint64))
    for keep_lowest in (False, True):
        forest, guaranteed, c, lab = C.kruskal(name, keep_lowest)
        _check(eng, name, keep_lowest, False)
        _check(eng, name, keep_lowest, True)
        for r in C.RATES:
            info = {}
            mask = S.connected_mask_device(eng, s, ei, n, E, r, keep_lowest, info=info)
            assert np.array_equal(mask, S.connected_mask(s, ei, n, E, r, keep_lowest)), (name, r)
            assert info["path"] == "device" and info["forest"] == n - c
            assert info["guaranteed"] == int(guaranteed.sum())
            assert info["over_budget"] == (int(guaranteed.sum()) > int(E * r))
            kc, klab = C.components(ei[0], ei[1], n, mask)
            assert kc == c and np.array_equal(klab, lab)


def test_connected_mask_device_special_scores(eng):
    """The guaranteed columns are taken out of the fill exactly: -inf / NaN / +inf scores."""
    from gsparse import selection as S

    for name in ("special_values", "duplicates", "rmat10_two_valued", "tree"):
        n, ei, s = _case(name)
        E = ei.shape[1]
        for keep_lowest in (False, True):
            for r in C.RATES + (0.97,):
                mask = S.connected_mask_device(eng, s, ei, n, E, r, keep_lowest)
                assert np.array_equal(mask, S.connected_mask(s, ei, n, E, r, keep_lowest)), (name, r)
    n, ei, s = _case("tree")
    info = {}
    assert S.connected_mask_device(eng, s, ei, n, ei.shape[1], 0.2, info=info).all()
    assert info["over_budget"] and info["guaranteed"] == 78


@pytest.mark.parametrize("name", ["karate", "roman2000"])
def test_sparsify_connected_keeps_the_components(name):
    import gsparse

    if name == "karate":
        ei, n, _ = C.golden("karate_test")
        pieces = None
    else:
        ei, n, _ = C.generated(name)
        pieces = (427, 1059, 1540)
    E = ei.shape[1]
    c, lab = C.components(ei[0], ei[1], n)
    data = gsparse.Data(edge_index=torch.from_numpy(np.array(ei)), num_nodes=n)
    sp_ = gsparse.GraphSparsifier(data, "cpu", tie_break="stable")
    sd, mask = sp_.sparsify_connected("jaccard", 0.8, return_mask=True)
    sel = dict(sp_.last_selection)
    mask = mask.numpy()
    assert np.array_equal(sd.edge_index.numpy(), ei[:, mask])
    kc, klab = C.components(ei[0], ei[1], n, mask)
    assert kc == c and np.array_equal(klab, lab)
    assert set(sel) >= {"path", "forest", "guaranteed", "rounds", "over_budget", "cut", "beyond", "tied"}
    assert sel["path"] == "device" and sel["forest"] == n - c and not sel["over_budget"]
    assert int(mask.sum()) == int(E * 0.8)
    scores = sp_.compute_scores("jaccard")
    assert np.array_equal(mask, gsparse.selection.connected_mask(scores, ei, n, E, 0.8))
    # plain top-k at the same rates: the Roman-like graph falls apart (the counts of the
    # stable cut); karate's Jaccard cut happens to keep it whole at 0.8
    for i, r in enumerate(C.RATES):
        _, plain = sp_.sparsify("jaccard", r, return_mask=True)
        plain_c = C.components(ei[0], ei[1], n, plain.numpy())[0]
        assert plain_c >= c
        if pieces is not None:
            assert plain_c == pieces[i] > c
        _, kept = sp_.sparsify_connected("jaccard", r, return_mask=True)
        assert C.components(ei[0], ei[1], n, kept.numpy())[0] == c
    whole, ones = sp_.sparsify_connected("jaccard", 1.0, return_mask=True)
    assert bool(ones.all()) and whole.edge_index.shape[1] == E
    with pytest.raises(ValueError):
        sp_.sparsify_connected("jaccard", 0.0)


def test_fewer_scores_than_columns_raises(eng):
    import gsparse
    from conftest import load_golden

    n, ei, s = _case("duplicates")
    with pytest.raises(ValueError):
        eng.spanning_forest(s[:-1], ei[0], ei[1], n)
    g = load_golden("directed_dup")  # its canonical CSR merged duplicate columns
    data = gsparse.Data(edge_index=torch.from_numpy(g["edge_index"]), num_nodes=int(g["num_nodes"]))
    with pytest.raises(ValueError):
        gsparse.GraphSparsifier(data, "cpu").sparsify_connected("jaccard", 0.5)


def test_bad_arguments_through_ctypes(eng):
    from gsparse import _lib

    L, h = _lib.lib(), eng.ctx.handle
    s = np.ones(3)
    mask = np.zeros(3, dtype=np.uint8)
    nf, nm, rounds = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int32(-1)

    def call(src, dst, n, nscores=3, E=3, expand=1):
        src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
        return L.gs_spanning_forest(h, _lib.ptr(s), _lib.GS_HOST, nscores, _lib.ptr(src), _lib.ptr(dst),
                                    _lib.GS_HOST, E, n, 0, expand, _lib.ptr(mask), _lib.GS_HOST, None,
                                    _lib.GS_HOST, ctypes.byref(nf), ctypes.byref(nm), ctypes.byref(rounds))

    assert call([0, 1, 2], [1, 2, 0], 3) == _lib.GS_OK and nf.value == 2 and nm.value == 2
    assert call([0, 3, 2], [1, 2, 0], 3) == _lib.GS_EINVAL  # an id equal to n
    assert call([0, 1, 2], [1, -1, 0], 3) == _lib.GS_EINVAL  # a negative id
    assert call([0, 3, 2], [1, 2, 0], 3, expand=0) == _lib.GS_EINVAL
    assert call([0, 1, 2], [1, -1, 0], 3, expand=0) == _lib.GS_EINVAL
    assert call([0, 1, 2], [1, 2, 0], 3, nscores=2) == _lib.GS_EINVAL
    assert call([0, 1, 2], [1, 2, 0], 0) == _lib.GS_EINVAL
    assert call([0, 1, 2], [1, 2, 0], 3, E=0) == _lib.GS_OK and nf.value == 0 and nm.value == 0
    assert L.gs_api_version() == 3
