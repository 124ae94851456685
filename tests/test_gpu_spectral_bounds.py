"""The spectral bounds of a sparsifier on the device (gs_spectral_bounds,
Engine.spectral_bounds, compute_spectral_approximation,
GraphSparsifier.spectral_approximation): closed forms at the kernels' tails and tile
boundaries, a segmented row above 65,536 nodes, the NumPy specification
(metrics.spectral_bounds_dense) on sampled sparsifiers, loud failure at the caps, and
repeatability.

The tolerance, for both values: |got - want| <= 1e-6 lambda_max(want) (B.RTOL), scaled by
lambda_max because lambda_min may be exactly 0; 1e-6 is the project's tolerance for the
algebraic connectivity.  A NumPy model of the iteration (CG to 1e-10, the residual test at
1e-9) agrees with the specification to 1e-10 lambda_max on every case here."""

import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import spectral_bounds_cases as B
import spectral_cases as C
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gs():
    import gsparse

    return gsparse


@pytest.fixture(scope="module")
def ctx():
    from gsparse._lib import Context

    return Context()


def close(got, want):
    err = max(abs(got[0] - want[0]), abs(got[1] - want[1])) / want[1]
    print(f"got {got!r} want {want!r} err {err:.3e} lambda_max")
    assert abs(got[0] - want[0]) <= B.RTOL * want[1]
    assert abs(got[1] - want[1]) <= B.RTOL * want[1]


def bounds(gs, ctx, G, hw, **kw):
    """Engine.spectral_bounds of weights hw on G as it is stored."""
    G = sp.csr_matrix(G, dtype=np.float64)
    G.sort_indices()
    ctx.set_graph_csr(G.shape[0], G.indptr, G.indices, G.data)
    eng = gs.engine.Engine(ctx)
    got = eng.spectral_bounds(hw, **kw)
    print("steps", eng.spectral_bounds_iterations, "cg", eng.spectral_bounds_cg_iterations)
    return got, eng


# ---- 1. cycle and path: the tails and tile boundaries of the vector passes
@pytest.mark.parametrize("n", [3, 63, 64, 65, 1023, 1024, 1025])
def test_cycle_and_path(gs, ctx, n):
    G, H, want = B.cycle_and_path(n)
    got, _ = bounds(gs, ctx, G, B.weights_on(G, H))
    close(got, want)


# ---- 2. K_64 and the star of weight 2.5
def test_k64_and_star(gs, ctx):
    G, H, want = B.k64_and_star()
    got, _ = bounds(gs, ctx, G, B.weights_on(G, H))
    close(got, want)


# ---- 3. one row of 70,000 entries (the segmented path for L_G and L_H), n > 65,536
def test_star_70000_alternating_weights(gs, ctx):
    G, H, want = B.star_alternating(70_000)
    assert G.shape[0] > 65_536 and np.diff(G.indptr).max() == 70_000
    got, _ = bounds(gs, ctx, G, B.weights_on(G, H))
    close(got, want)


# ---- 4. H = 0.37 G: one step
def test_scaled_copy_takes_one_step(gs, ctx):
    G = B.rmat10()
    got, eng = bounds(gs, ctx, G, 0.37 * G.data)
    close(got, (0.37, 0.37))
    assert eng.spectral_bounds_iterations == 1


# ---- 5. a bridge dropped: lambda_min = 0
def test_bridge_dropped(gs, ctx):
    G, H, want = B.two_cliques()
    got, _ = bounds(gs, ctx, G, B.weights_on(G, H))
    close(got, want)


# ---- 6. one pair removed: lambda_min = 1 - R_e
def test_one_pair_removed(gs, ctx):
    G = B.rmat10()
    ei, n = B.edge_index_of(G)
    ctx.set_graph_csr(n, G.indptr, G.indices, G.data)
    er = gs.engine.Engine(ctx).exact_er()
    e = int(np.argmax(er < 0.9))  # a pair that is no bridge
    u, v = int(ei[0][e]), int(ei[1][e])
    hw = np.ones(G.nnz)
    hw[((ei[0] == u) & (ei[1] == v)) | ((ei[0] == v) & (ei[1] == u))] = 0.0
    assert (hw == 0).sum() == 2
    got, _ = bounds(gs, ctx, G, hw)
    close(got, (1.0 - float(er[e]), 1.0))


# ---- 7. against the specification on R-MAT-10's largest component
RMAT_SAMPLES = ("multinomial_4m", "multinomial_m", "independent_half", "high_half", "low_half")


@functools.lru_cache(maxsize=None)
def rmat10_exact_er():
    from gsparse._lib import Context
    from gsparse.engine import Engine

    G = B.rmat10()
    c = Context()
    c.set_graph_csr(G.shape[0], G.indptr, G.indices, G.data)
    return Engine(c).exact_er()


@functools.lru_cache(maxsize=None)
def rmat10_case(name):
    """(hw, the specification's bounds), computed once and shared."""
    from gsparse import metrics

    G = B.rmat10()
    er = rmat10_exact_er()
    m = G.nnz // 2
    if name == "multinomial_4m":
        hw = B.sampled(G, er, 4 * m, "multinomial")
    elif name == "multinomial_m":
        hw = B.sampled(G, er, m, "multinomial")
    elif name == "independent_half":
        hw = B.sampled(G, er, m // 2, "independent")
    else:
        hw = B.resistance_halves(G, er)[0 if name == "high_half" else 1]
    hw.setflags(write=False)
    return hw, metrics.spectral_bounds_dense(G, B.with_weights(G, hw))


@pytest.mark.parametrize("name", RMAT_SAMPLES)
def test_rmat10_against_the_specification(gs, ctx, name):
    hw, want = rmat10_case(name)
    got, _ = bounds(gs, ctx, B.rmat10(), hw)
    close(got, want)
    if name == "high_half":
        assert abs(want[1] - 1.0) <= 1e-9 and abs(want[0] - 0.1276) <= 5e-5
    if name == "low_half":  # H falls apart
        assert abs(want[0]) <= 1e-9 and abs(want[1] - 0.8724) <= 5e-5
        assert got[0] >= 0.0


# ---- 8. against the specification on dense96, the two samples of test_quality_*
def test_dense96_against_the_specification(gs, ctx):
    from gsparse import metrics

    _, _, G, samples = B.dense96_pairs()
    for _, _, H in samples:
        got, _ = bounds(gs, ctx, G, B.weights_on(G, H))
        close(got, metrics.spectral_bounds_dense(G, H))


# ---- 9. weighted G with self-loops and several components, through the metrics function
def test_weighted_components_loops_through_metrics(gs):
    from gsparse import selection

    G = B.weighted_components_loops()
    ei, n = B.edge_index_of(G)
    m = len(np.unique(np.minimum(ei[0], ei[1]) * (n + 1) + np.maximum(ei[0], ei[1])))
    mask, w, _, _ = selection.spectral_sample(np.ones(G.nnz), ei, n, 3 * m // 4, seed=42,
                                              method="independent")
    H = B.with_weights(G, G.data * np.where(mask, w, 0.0))
    assert 0 < H.nnz < G.nnz and G.diagonal().any()
    got = gs.compute_spectral_approximation(G, H)
    nodes = B.component_nodes(G)
    want = gs.spectral_bounds_dense(G[nodes][:, nodes], H[nodes][:, nodes])
    close((got["lambda_min"], got["lambda_max"]), want)
    assert got["nodes"] == len(nodes) < n and got["num_connected_components"] > 1
    assert got["epsilon"] == max(got["lambda_max"] - 1.0, 1.0 - got["lambda_min"])
    assert got["iterations"] >= 1 and got["cg_iterations"] >= 1
    assert set(got) == {"lambda_min", "lambda_max", "epsilon", "nodes",
                        "num_connected_components", "iterations", "cg_iterations"}


# ---- 10. through GraphSparsifier
def test_through_graph_sparsifier(gs):
    import torch

    ei, n = C.sym_graph(40, seed=3)  # a relabelled path: on a tree the bounds are the weights
    data = gs.Data(edge_index=torch.from_numpy(ei), num_nodes=n)
    sp_ = gs.GraphSparsifier(data, "cuda:0")
    sd, (mask, weight) = sp_.sparsify_spectral("effective_resistance", num_samples=120, seed=42,
                                               return_mask=True)
    got = sp_.spectral_approximation(sd)
    G = sp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(n, n))
    se = sd.edge_index.cpu().numpy()
    sw = sd.edge_weight.cpu().numpy().astype(np.float64)
    H = sp.csr_matrix((sw, (se[0], se[1])), shape=(n, n))
    assert got == gs.compute_spectral_approximation(G, H)
    assert got["epsilon"] == max(got["lambda_max"] - 1.0, 1.0 - got["lambda_min"])
    lo = 0.0 if not mask.all() else float(sw.min())
    close((got["lambda_min"], got["lambda_max"]), (lo, float(sw.max())))
    # the (mask, weight) pair carries the float64 weights
    pair = sp_.spectral_approximation((mask, weight))
    close((pair["lambda_min"], pair["lambda_max"]), (lo, float(weight.max())))
    # explicit weights override the Data's
    half = sp_.spectral_approximation(sd, edge_weight=0.5 * sd.edge_weight)
    close((half["lambda_min"], half["lambda_max"]), (0.5 * lo, 0.5 * float(sw.max())))
    # a Data without edge_weight (sparsify's) is read with unit weights
    plain = sp_.sparsify("jaccard", 1.0)
    assert getattr(plain, "edge_weight", None) is None
    unit = sp_.spectral_approximation(plain)
    close((unit["lambda_min"], unit["lambda_max"]), (1.0, 1.0))
    assert unit["iterations"] == 1
    keep = (ei[0] + ei[1]) % 7 != 0  # symmetric in the two directions of a pair
    cut = gs.Data(edge_index=torch.from_numpy(ei[:, keep]), num_nodes=n)
    assert 0 < keep.sum() < len(keep)
    unit = sp_.spectral_approximation(cut)
    close((unit["lambda_min"], unit["lambda_max"]), (0.0, 1.0))


# ---- 11. errors: the outputs stay at their sentinel
SENTINEL = -7.5


def abi(ctx, hw, nhw=None, tol=1e-9, max_iter=300, cg_rtol=1e-10, cg_max_iter=5000):
    from gsparse._lib import GS_HOST

    hw = np.ascontiguousarray(hw, dtype=np.float64)
    lo, hi = ctypes.c_double(SENTINEL), ctypes.c_double(SENTINEL)
    it, cg = ctypes.c_int32(-1), ctypes.c_int64(-1)
    rc = ctx._L.gs_spectral_bounds(ctx.handle, hw.ctypes.data, GS_HOST,
                                   len(hw) if nhw is None else nhw, tol, max_iter, cg_rtol,
                                   cg_max_iter, ctypes.byref(lo), ctypes.byref(hi),
                                   ctypes.byref(it), ctypes.byref(cg))
    return rc, lo.value, hi.value, it.value, cg.value


def test_bad_weights(gs, ctx):
    from gsparse._lib import GS_EINVAL, GS_EUNSUPPORTED, GS_OK

    G, H, want = B.cycle_and_path(8)
    hw = B.weights_on(G, H)
    ctx.set_graph_csr(8, G.indptr, G.indices, G.data)
    eng = gs.engine.Engine(ctx)
    rc, lo, hi, _, _ = abi(ctx, hw)
    assert rc == GS_OK
    close((lo, hi), want)
    neg, nan, inf, asym = hw.copy(), hw.copy(), hw.copy(), hw.copy()
    neg[3], nan[3], inf[3] = -1.0, np.nan, np.inf
    asym[0] = 0.5  # entry (0, 1) alone: (1, 0) keeps 1.0
    for bad, code, exc in ((hw[:-1], GS_EINVAL, ValueError), (neg, GS_EINVAL, ValueError),
                           (nan, GS_EINVAL, ValueError), (inf, GS_EINVAL, ValueError),
                           (asym, GS_EUNSUPPORTED, NotImplementedError)):
        rc, lo, hi, _, _ = abi(ctx, bad)
        assert rc == code and lo == SENTINEL and hi == SENTINEL
        with pytest.raises(exc):
            eng.spectral_bounds(bad)
    for kw in (dict(tol=0.0), dict(max_iter=1), dict(max_iter=501), dict(cg_rtol=0.0),
               dict(cg_rtol=1.0), dict(cg_max_iter=0)):
        rc, lo, hi, _, _ = abi(ctx, hw, **kw)
        assert rc == GS_EINVAL and lo == SENTINEL and hi == SENTINEL, kw
        with pytest.raises(ValueError):
            eng.spectral_bounds(hw, **kw)


def test_two_components_and_directed(gs, ctx):
    from gsparse._lib import GS_EINVAL, GS_EUNSUPPORTED

    two = sp.block_diag([B.path(5), B.cycle(7)]).tocsr()
    two.sort_indices()
    with pytest.raises(ValueError, match="components"):
        bounds(gs, ctx, two, two.data)
    rc, lo, hi, _, _ = abi(ctx, two.data)
    assert rc == GS_EINVAL and lo == SENTINEL and hi == SENTINEL
    directed = sp.csr_matrix(np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], dtype=np.float64))
    with pytest.raises(NotImplementedError):
        bounds(gs, ctx, directed, directed.data)
    rc, lo, hi, _, _ = abi(ctx, directed.data)
    assert rc == GS_EUNSUPPORTED and lo == SENTINEL and hi == SENTINEL
    single = sp.csr_matrix((1, 1))
    with pytest.raises(ValueError):
        bounds(gs, ctx, single, single.data)


def test_cap_is_an_error_not_a_value(gs, ctx):
    from gsparse._lib import GS_ENOCONV

    g = load_golden("roman2000")
    n = int(g["num_nodes"])
    G = B.largest_component(sp.csr_matrix((g["data"], g["indices"], g["indptr"]), shape=(n, n)))
    hw = G.data.copy()  # H = G: the first solve is the one that cannot finish
    with pytest.raises(RuntimeError) as ei:
        bounds(gs, ctx, G, hw, cg_max_iter=1)
    assert isinstance(ei.value, gs.GsparseNotConverged)
    assert "cg_max_iter=1" in str(ei.value) and "residual" in str(ei.value)
    eng = gs.engine.Engine(ctx)
    with pytest.raises(gs.GsparseNotConverged):
        eng.spectral_bounds(hw, cg_max_iter=1)
    assert eng.spectral_bounds_iterations == 0 and eng.spectral_bounds_cg_iterations == 1
    # the graph is still resident: the same call through the ABI writes no value
    rc, lo, hi, it, cg = abi(ctx, hw, cg_max_iter=1)
    assert rc == GS_ENOCONV and lo == SENTINEL and hi == SENTINEL
    assert it == 0 and cg == 1
    # Lanczos at its own cap: two steps cannot settle a sampled sparsifier
    hw, _ = rmat10_case("multinomial_m")
    G = B.rmat10()
    ctx.set_graph_csr(G.shape[0], G.indptr, G.indices, G.data)
    rc, lo, hi, it, cg = abi(ctx, hw, max_iter=2)
    assert rc == GS_ENOCONV and lo == SENTINEL and hi == SENTINEL
    assert it == 2 and cg >= 2
    with pytest.raises(gs.GsparseNotConverged, match="max_iter=2.*residual"):
        gs.engine.Engine(ctx).spectral_bounds(hw, max_iter=2)


# ---- 12. repeatability
def test_two_calls_give_the_same_bits(gs, ctx):
    hw, _ = rmat10_case("independent_half")
    a, eng = bounds(gs, ctx, B.rmat10(), hw)
    ia = (eng.spectral_bounds_iterations, eng.spectral_bounds_cg_iterations)
    b, eng = bounds(gs, ctx, B.rmat10(), hw)
    assert np.array(a).tobytes() == np.array(b).tobytes()
    assert ia == (eng.spectral_bounds_iterations, eng.spectral_bounds_cg_iterations)
    # the weights on the device give the same bits as on the host
    import torch

    c, eng = bounds(gs, ctx, B.rmat10(), torch.from_numpy(np.array(hw)).cuda())
    assert np.array(a).tobytes() == np.array(c).tobytes()
