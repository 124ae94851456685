"""GPU tests of the binding's marshalling (gsparse/_args.py) with device tensors, on the
karate graph (34 nodes, 156 columns = CSR entries):

(a) a device tensor of the wrong dtype, one element short, strided, or on another GPU is
    refused before the library is reached -- ``Context.call`` is wrapped so that the test
    fails if the offending entry point is called at all; the bad buffer is never passed on;
(b) strided device inputs (the columns of an (E, 2) tensor) are read as their values, not
    as dense memory;
(c) the same result from a NumPy and from a CUDA argument, bit for bit, is already checked
    by test_gpu_scorer_shapes.py::test_adamic_adar_device_weights (``c=``),
    ::test_feature_cosine_device_resident and ::test_sub_ranges (``x`` as f32 / f64) and
    test_gpu_distributed.py::test_jaccard_count_shares_vs_oracle (``jaccard_from_counts``),
    so it is not repeated here.

Exception types: a wrong dtype is a TypeError, a strided, short or misplaced buffer a
ValueError -- except where a check existed before the marshalling layer and keeps its
type: the mask outputs raise ValueError for every fault, and the buffers ``Engine._need``
used to check (``undirected_ids``' ``out``, ``random_mask``'s ``inverse``, the ``jsel_*``
arrays) raise IndexError when short.
"""

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def karate():
    g = load_golden("karate_test")
    ei = np.ascontiguousarray(g["edge_index"])
    return int(g["num_nodes"]), ei, np.ascontiguousarray(g["scores_jaccard"])


@pytest.fixture(scope="module")
def eng(karate):
    from gsparse._lib import Context
    from gsparse.engine import Engine

    n, ei, _ = karate
    ctx = Context(0)
    ctx.set_graph_edge_index(n, ei[0].copy(), ei[1].copy())
    e = Engine(ctx)
    assert e.nnz == ei.shape[1] == 156 and e.symmetric
    return e


def dev(a, dtype=None, device=DEV):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return t if dtype is None else t.to(dtype)


def buf(n, dtype, device=DEV):
    return torch.zeros(n, dtype=dtype, device=device)


def strided(n, dtype, device=DEV):
    """n elements with stride 2: a ``[::2]`` view of a tensor twice the size."""
    v = buf(2 * n, dtype, device)[::2]
    assert v.numel() == n and not v.is_contiguous()
    return v


@pytest.fixture(scope="module")
def K(karate):
    """Conforming cuda:0 tensors of the karate graph, shared and never written."""
    n, ei, s = karate

    class K:
        E = ei.shape[1]
        src, dst, sc = dev(ei[0]), dev(ei[1]), dev(s)
        inv = dev(np.arange(ei.shape[1]) % 78)
        us = dev(np.linspace(0, 1, 78))

    K.n = n
    return K


F64, U8, I64 = torch.float64, torch.uint8, torch.int64
BAD = {  # a faulty stand-in for a buffer of k elements of dtype dt
    "dtype": lambda k, dt: buf(k, torch.float32 if dt is F64 else torch.int32),
    "short": lambda k, dt: buf(k - 1, dt),
    "strided": strided,
}
RNG = np.random.default_rng(1)
CASES = {}  # id -> (entry point that must not be reached, exception, call(engine, K))
for kind, mk in BAD.items():
    exc = TypeError if kind == "dtype" else ValueError
    need = IndexError if kind == "short" else exc  # what Engine._need checked keeps IndexError
    CASES.update({
        f"jaccard.out-{kind}": ("gs_jaccard", exc, lambda e, K, mk=mk: e.jaccard(out=mk(K.E, F64))),
        f"topk_mask.out-{kind}": ("gs_topk_mask", ValueError, lambda e, K, mk=mk: e.topk_mask(
            K.sc, K.E, K.E // 2, False, out=mk(K.E, U8))),
        f"random_mask.out-{kind}": ("gs_random_mask", ValueError, lambda e, K, mk=mk: e.random_mask(
            K.us, K.inv, 30, K.E, out=mk(K.E, U8))),
        f"spanning_forest.out-{kind}": ("gs_spanning_forest", ValueError,
                                        lambda e, K, mk=mk: e.spanning_forest(
                                            K.sc, K.src, K.dst, K.n, out=mk(K.E, U8))),
        f"undirected_ids.out-{kind}": ("gs_undirected_ids", need, lambda e, K, mk=mk: e.undirected_ids(
            K.src, K.dst, K.n, out=mk(K.E, I64))),
        f"jsel_mask.out-{kind}": ("gs_jsel_mask", need, lambda e, K, mk=mk: e.jsel_mask(
            1, buf(4, U8), 4, mk(K.E, U8))),
    })
f32, i32, short = (lambda k: BAD["dtype"](k, F64)), (lambda k: BAD["dtype"](k, I64)), BAD["short"]
CASES.update({
    # a CUDA tensor the library reads in place is never converted ...
    "topk_mask.scores-dtype": ("gs_topk_mask", TypeError, lambda e, K: e.topk_mask(
        f32(K.E), K.E, K.E // 2, False)),
    "random_mask.scores-dtype": ("gs_random_mask", TypeError, lambda e, K: e.random_mask(
        f32(78), K.inv, 30, K.E)),
    "spanning_forest.scores-dtype": ("gs_spanning_forest", TypeError, lambda e, K: e.spanning_forest(
        f32(K.E), K.src, K.dst, K.n)),
    "spectral_sample.scores-dtype": ("gs_spectral_sample", TypeError, lambda e, K: e.spectral_sample(
        f32(K.E), K.src, K.dst, K.n, 100, RNG)),
    "jsel_mask.keep_all-dtype": ("gs_jsel_mask", TypeError, lambda e, K: e.jsel_mask(
        1, i32(4), 4, buf(K.E, U8))),
    "set_graph_edge_index.src-dtype": ("gs_graph_from_edge_index", TypeError,
                                       lambda e, K: e.ctx.set_graph_edge_index(K.n, i32(K.E), K.dst)),
    # ... and one that is an element short is not read past its end
    "random_mask.inverse-short": ("gs_random_mask", IndexError, lambda e, K: e.random_mask(
        K.us, short(K.E, I64), 30, K.E)),
    "jsel_mask.keep_all-short": ("gs_jsel_mask", IndexError, lambda e, K: e.jsel_mask(
        1, buf(3, U8), 4, buf(K.E, U8))),
    "spanning_forest.dst-short": ("gs_spanning_forest", ValueError, lambda e, K: e.spanning_forest(
        K.sc, K.src, short(K.E, I64), K.n)),
    "spectral_sample.dst-short": ("gs_spectral_sample", ValueError, lambda e, K: e.spectral_sample(
        K.sc, K.src, short(K.E, I64), K.n, 100, RNG)),
    "undirected_ids.dst-short": ("gs_undirected_ids", ValueError, lambda e, K: e.undirected_ids(
        K.src, short(K.E, I64), K.n)),
    "set_graph_edge_index.dst-short": ("gs_graph_from_edge_index", ValueError,
                                       lambda e, K: e.ctx.set_graph_edge_index(
                                           K.n, K.src, short(K.E, I64))),
})


def guard(monkeypatch, ctx, entry):
    """Fail (with an error no ``pytest.raises`` here expects) if ``entry`` is called: the
    library is not reached, so the bad buffer is never passed on."""
    real = ctx.call

    def call(name, *args):
        if name == entry:
            raise RuntimeError(f"{name} was reached with a bad buffer")
        return real(name, *args)

    monkeypatch.setattr(ctx, "call", call)


@pytest.mark.parametrize("case", sorted(CASES))
def test_bad_device_buffer_is_refused_before_the_library(eng, K, monkeypatch, case):
    entry, exc, fn = CASES[case]
    guard(monkeypatch, eng.ctx, entry)
    with pytest.raises(exc) as info:
        fn(eng, K)
    assert info.type is exc  # not a subclass: IndexError / ValueError / TypeError as listed


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU")
def test_tensor_on_another_device_is_refused(eng, K, monkeypatch):
    other = "cuda:1"
    for entry, fn in (
            ("gs_jaccard", lambda: eng.jaccard(out=buf(K.E, F64, other))),
            ("gs_topk_mask", lambda: eng.topk_mask(K.sc.to(other), K.E, K.E // 2, False)),
            ("gs_topk_mask", lambda: eng.topk_mask(K.sc, K.E, K.E // 2, False,
                                                   out=buf(K.E, U8, other))),
            ("gs_undirected_ids", lambda: eng.undirected_ids(K.src.to(other), K.dst.to(other), K.n)),
            ("gs_graph_from_edge_index",
             lambda: eng.ctx.set_graph_edge_index(K.n, K.src.to(other), K.dst.to(other)))):
        with monkeypatch.context() as m:
            guard(m, eng.ctx, entry)
            with pytest.raises(ValueError):
                fn()


# ------------------------------------------------- (b) strided device inputs
def test_strided_edge_index_columns_build_the_same_graph(karate):
    from gsparse._lib import Context

    n, ei, _ = karate
    t = torch.stack([dev(ei[0]), dev(ei[1])], 1)  # (E, 2): both columns have stride 2
    assert t[:, 0].stride() == (2,) and not t[:, 1].is_contiguous()
    a, b, c = Context(0), Context(0), Context(0)
    a.set_graph_edge_index(n, t[:, 0], t[:, 1])
    b.set_graph_edge_index(n, t[:, 0].contiguous(), t[:, 1].contiguous())
    c.set_graph_edge_index(n, ei[0].copy(), ei[1].copy())
    for x, y, z in zip(a.csr(), b.csr(), c.csr()):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes() == z.tobytes()
    g = load_golden("karate_test")
    assert np.array_equal(a.csr()[0], g["indptr"]) and np.array_equal(a.csr()[1], g["indices"])


def test_strided_columns_give_the_same_undirected_ids(eng, karate):
    n, ei, _ = karate
    t = torch.stack([dev(ei[0]), dev(ei[1])], 1)
    inv_s, cnt_s, st_s = eng.undirected_ids(t[:, 0], t[:, 1], n)
    inv_c, cnt_c, st_c = eng.undirected_ids(t[:, 0].contiguous(), t[:, 1].contiguous(), n)
    inv_h, cnt_h, st_h = eng.undirected_ids(ei.T[:, 0], ei.T[:, 1], n)  # host views, stride 1
    assert (cnt_s, st_s) == (cnt_c, st_c) == (cnt_h, st_h) == (78, 0)
    assert inv_s.dtype == np.int64 and inv_s.tobytes() == inv_c.tobytes() == inv_h.tobytes()
    assert np.array_equal(inv_s, load_golden("karate_test")["random_inverse"])
