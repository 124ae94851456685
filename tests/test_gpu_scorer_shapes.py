"""The scorers at the shapes the parity tests leave out.

* Feature cosine (k_normalise / k_cosine over pw_sum, csrc/gs_pairwise.hpp) at every
  feature dimension where NumPy's pairwise sum takes another path -- the n < 8 loop, the
  8-accumulator leaf and its tail, the 128/129 leaf/split edge, splits n2 = n/2 - (n/2)%8
  with small remainders -- in float32 and float64, with planted rows: all zero (the 1e-10
  floor), a NaN, an inf, a norm below the floor, and |x| next to -|x| (a negative dot,
  clamped).  References: the reference's own NumPy lines (metrics.py:344-358) restated
  here, and the oracle's C restatement.
* Every scorer on CSR sub-ranges [e0, e1), which is what a rank > 0 of
  sharded_edge_scores asks for: the out[e - e0] indexing, the symmetric graph's fall-back
  to the merge kernel for a partial range, device-resident inputs and outputs.

The bar is bit-identical float64; NaN positions must agree, NaN sign and payload are not
compared (x86 and gfx950 produce different default NaNs, the reference never looks)."""

import functools

import numpy as np
import pytest
import torch

import gsparse_oracle as O
from conftest import bits_equal, load_golden

pytestmark = pytest.mark.gpu

N = 257
DIMS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 135, 136, 137, 255, 256, 257, 263,
        264, 272, 511, 512, 513, 1000)
ZERO, NAN, INF, TINY, POS, NEG = 3, 10, 20, 30, 40, 41
PLANTED = ((POS, NEG), (ZERO, NAN), (NAN, INF), (TINY, POS), (ZERO, ZERO), (TINY, TINY), (ZERO, 5),
           (INF, 6), (TINY, ZERO))


@functools.lru_cache(maxsize=None)
def sweep_graph():
    """Symmetric random graph, n = 257, ~6,400 entries, with the planted rows adjacent."""
    rng = np.random.default_rng(257)
    ei = np.concatenate([rng.integers(0, N, (2, 3370)), np.array(PLANTED, dtype=np.int64).T], axis=1)
    ip, ix, d = O.canonical_csr(O.coalesce(ei, N), N)
    assert 6200 <= len(ix) <= 6600
    for a in (ip, ix, d):
        a.setflags(write=False)
    return ip, ix, d


@functools.lru_cache(maxsize=None)
def sweep_features(f, dtype):
    x = np.random.default_rng(1000 + f).standard_normal((N, f)).astype(dtype)
    x[ZERO] = 0
    x[NAN, f // 2] = np.nan
    x[INF, f - 1] = np.inf
    x[TINY] *= dtype(1e-30 if dtype is np.float64 else 1e-25)
    x[POS] = np.abs(x[POS]) + dtype(0.5)
    x[NEG] = -x[POS]
    x.setflags(write=False)
    return x


def numpy_cosine(x, rows, cols):
    """metrics.py:344-358 as the reference writes it."""
    with np.errstate(all="ignore"):
        norms = np.linalg.norm(x, axis=1, keepdims=True)
        norms = np.maximum(norms, 1e-10)
        normalized = x / norms
        scores = np.sum(normalized[rows] * normalized[cols], axis=1)
        scores = np.maximum(scores, 0.0)
    return scores.astype(np.float64)


@functools.lru_cache(maxsize=None)
def sweep_reference(f, dtype):
    ip, ix, _ = sweep_graph()
    x = sweep_features(f, dtype)
    rows = O.csr_rows(ip)
    ref = numpy_cosine(x, rows, ix)
    assert ref.dtype == np.float64 and x.dtype == dtype
    same(O.feature_cosine(ip, ix, x), ref)  # the two references agree
    # the planted rows do what they are there for
    e = {(int(r), int(c)): i for i, (r, c) in enumerate(zip(rows, ix))}
    assert np.isnan(ref[e[NAN, INF]]) and np.isnan(ref[e[ZERO, NAN]]) and np.isnan(ref[e[INF, 6]])
    assert ref[e[ZERO, 5]] == 0 and ref[e[ZERO, ZERO]] == 0
    assert ref[e[POS, NEG]] == 0 and ref[e[NEG, POS]] == 0  # about -1 before the clamp
    with np.errstate(all="ignore"):
        nrm = np.linalg.norm(x, axis=1)
    assert nrm[TINY] < 1e-10 and nrm[ZERO] == 0 and 0 <= ref[e[TINY, TINY]] < 1e-20
    assert np.isfinite(ref).sum() > 5500
    ref.setflags(write=False)
    return ref


def same(got, ref):
    """NaN in the same places, every other entry bit for bit."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == np.float64 and got.shape == ref.shape
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), np.nonzero(gn != rn)[0][:8]
    a, b = np.where(rn, 0.0, got), np.where(rn, 0.0, ref)
    bad = np.nonzero(a.view(np.uint64) != b.view(np.uint64))[0]
    assert len(bad) == 0, (len(bad), bad[:8], a[bad[:8]], b[bad[:8]])


def engine_csr(n, ip, ix, d):
    from gsparse._lib import Context
    from gsparse.engine import Engine

    ctx = Context(0)
    ctx.set_graph_csr(n, ip, ix, d)
    return Engine(ctx)


@pytest.fixture(scope="module")
def sweep_engine():
    eng = engine_csr(N, *sweep_graph())
    assert eng.symmetric
    return eng


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("f", DIMS)
def test_feature_cosine_dimension_sweep(sweep_engine, f, dtype):
    same(sweep_engine.feature_cosine(sweep_features(f, dtype)), sweep_reference(f, dtype))


@pytest.mark.parametrize("f,dtype", [(137, np.float32), (263, np.float64)], ids=["f32-137", "f64-263"])
def test_feature_cosine_device_resident(sweep_engine, f, dtype):
    """x as a CUDA tensor, out= a CUDA tensor, and both."""
    ref = sweep_reference(f, dtype)
    x = sweep_features(f, dtype)
    xd = torch.from_numpy(x.copy()).cuda()
    same(sweep_engine.feature_cosine(xd), ref)
    out = torch.full((len(ref),), -7.0, dtype=torch.float64, device="cuda")
    assert sweep_engine.feature_cosine(x, out=out) is out
    same(out.cpu().numpy(), ref)
    out.fill_(-7.0)
    sweep_engine.feature_cosine(xd, out=out)
    same(out.cpu().numpy(), ref)


# ---------------------------------------------------------------- sub-ranges
GRAPHS = ("rmat10", "directed_dup")
SCORERS = ("jaccard", "adamic_adar", "degree", "feature_cosine")


@functools.lru_cache(maxsize=None)
def range_case(name):
    g = load_golden(name)
    n, ip, ix, d = int(g["num_nodes"]), g["indptr"], g["indices"], g["data"]
    x = np.random.default_rng(32).standard_normal((n, 32), dtype=np.float32)
    ref = {"jaccard": O.jaccard(ip, ix), "adamic_adar": O.adamic_adar(ip, ix),
           "degree": O.degree(ip, ix, d), "feature_cosine": O.feature_cosine(ip, ix, x)}
    for s in ("jaccard", "adamic_adar", "degree"):
        assert bits_equal(ref[s], g[f"scores_{s}"])  # the oracle is the reference's here
    for a in (ip, ix, d, x, *ref.values()):
        a.setflags(write=False)
    return n, ip, ix, d, x, ref


def ranges(nnz):
    from gsparse.distributed import edge_ranges

    b = edge_ranges(nnz, 3)
    return [(0, 0), (nnz, nnz), (0, 1), (nnz - 1, nnz), (1, nnz), (255, 257),
            (b[0], b[1]), (b[1], b[2]), (b[2], b[3])]


def score(eng, scorer, x, e0, e1, out=None, **kw):
    if scorer == "feature_cosine":
        return eng.feature_cosine(x, e0, e1, out=out)
    return getattr(eng, scorer)(e0, e1, out=out, **kw)


@pytest.fixture(scope="module")
def range_engines():
    """Per graph: the engine and every scorer's full-range result (computed once)."""
    out = {}
    for name in GRAPHS:
        n, ip, ix, d, x, ref = range_case(name)
        eng = engine_csr(n, ip, ix, d)
        assert eng.symmetric == (name == "rmat10") and eng.nnz == len(ix) > 257
        full = {s: score(eng, s, x, 0, eng.nnz) for s in SCORERS}
        for s in SCORERS:
            assert bits_equal(full[s], ref[s]), (name, s)
        out[name] = eng, full
    return out


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("scorer", SCORERS)
@pytest.mark.parametrize("name", GRAPHS)
def test_sub_ranges(range_engines, name, scorer, where):
    """[e0, e1) into a host array / a device tensor of e1 - e0 values (device: the
    features too) == that slice of the full-range result and of the oracle's."""
    eng, full = range_engines[name]
    *_, x, ref = range_case(name)
    nnz = eng.nnz
    xin = torch.from_numpy(x.copy()).cuda() if where == "device" else x
    for e0, e1 in ranges(nnz):
        assert 0 <= e0 <= e1 <= nnz
        if where == "device":
            out = torch.full((e1 - e0,), -7.0, dtype=torch.float64, device="cuda")
            score(eng, scorer, xin, e0, e1, out=out)
            got = out.cpu().numpy()
        else:
            got = score(eng, scorer, xin, e0, e1)
        assert got.shape == (e1 - e0,)
        assert bits_equal(got, full[scorer][e0:e1]), (e0, e1)
        assert bits_equal(got, ref[scorer][e0:e1]), (e0, e1)


@pytest.mark.parametrize("name", GRAPHS)
def test_adamic_adar_device_weights(range_engines, name):
    """The weights c handed in as a device tensor, full range and sub-ranges."""
    from gsparse.engine import aa_weights

    eng, full = range_engines[name]
    c = torch.from_numpy(np.ascontiguousarray(aa_weights(eng.indptr()))).cuda()
    for e0, e1 in [(0, eng.nnz)] + ranges(eng.nnz):
        assert bits_equal(eng.adamic_adar(e0, e1, c=c), full["adamic_adar"][e0:e1]), (e0, e1)
        out = torch.full((e1 - e0,), -7.0, dtype=torch.float64, device="cuda")
        eng.adamic_adar(e0, e1, out=out, c=c)
        assert bits_equal(out.cpu().numpy(), full["adamic_adar"][e0:e1]), (e0, e1)


@pytest.mark.parametrize("scorer", SCORERS)
@pytest.mark.parametrize("name", GRAPHS)
def test_bad_ranges_raise(range_engines, name, scorer):
    eng, full = range_engines[name]
    x = range_case(name)[4]
    nnz = eng.nnz
    out = np.full(nnz + 1, -7.0)
    for e0, e1 in ((2, 1), (nnz, nnz - 1), (0, nnz + 1), (nnz + 1, nnz + 1), (-1, 1)):
        with pytest.raises(ValueError, match="edge range"):
            score(eng, scorer, x, e0, e1, out=out)
    assert (out == -7.0).all()  # a refused call writes nothing
    assert bits_equal(score(eng, scorer, x, 0, nnz), full[scorer])
