"""Host tests of the binding's marshalling (gsparse/_args.py) and of every call site's
agreement with the ctypes table -- no GPU, the library is never loaded.

(a) the ``_args`` functions with NumPy arrays, lists and CPU tensors;
(b) a recording stand-in for ``Context``: every ``Engine`` / ``BackboneStages`` method and
    the two ``Context.set_graph_*`` are driven with small conforming NumPy inputs, and every
    recorded call is checked against ``_lib.SIGNATURES`` argument by argument;
(c) the plan functions are importable from ``gsparse.engine`` and are ``gsparse.plans``'s.
"""

import ctypes

import numpy as np
import pytest
import torch

from gsparse import _lib
from gsparse._lib import GS_DEVICE, GS_HOST, SIGNATURES

DEV = 0


# ------------------------------------------------------------------ (a) _args
@pytest.fixture(scope="module")
def A():
    from gsparse import _args

    return _args


def _ptr(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


@pytest.mark.parametrize("dtype", [np.float64, np.int64, np.uint8, np.int32])
def test_conforming_input_is_not_copied(A, dtype):
    a = np.arange(7).astype(dtype)
    got, loc = A.inp(a, dtype, "a", DEV, count=7)
    assert got is a and loc == GS_HOST and _ptr(got) == _ptr(a)
    t = torch.from_numpy(a)
    got, loc = A.inp(t, dtype, "t", DEV)
    assert isinstance(got, np.ndarray) and loc == GS_HOST and _ptr(got) == t.data_ptr()
    got, loc = A.inp(a, None, "a", DEV)  # no dtype asked for: the array's own is kept
    assert got is a and loc == GS_HOST


@pytest.mark.parametrize("src", ["array", "list", "tensor"])
def test_wrong_dtype_host_input_is_converted(A, src):
    vals = [3, 1, 4, 1, 5]
    a = {"array": np.array(vals, dtype=np.int32), "list": vals,
         "tensor": torch.tensor(vals, dtype=torch.int32)}[src]
    for cast in ("host", "both"):
        got, loc = A.inp(a, np.float64, "a", DEV, cast=cast)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and loc == GS_HOST
        assert got.flags.c_contiguous and np.array_equal(got, np.array(vals, dtype=np.float64))
    with pytest.raises(TypeError):
        A.inp(np.asarray(a), np.float64, "a", DEV, cast="never")
    got, _ = A.inp(np.array(vals, dtype=np.int32), (np.uint32, np.int32), "a", DEV, cast="never")
    assert got.dtype == np.int32  # any of the accepted dtypes passes as it is


def test_strided_input_comes_back_contiguous(A):
    f = np.asfortranarray(np.arange(12, dtype=np.float64).reshape(3, 4))
    got, _ = A.inp(f, np.float64, "f", DEV)
    assert got.flags.c_contiguous and np.array_equal(got, f)
    ei = np.arange(10, dtype=np.int64).reshape(5, 2)  # (E, 2): the transposed rows are strided
    rows = ei.T
    assert not rows[1].flags.c_contiguous
    s, d, E, loc = A.pair(rows[0], rows[1], DEV)
    assert (E, loc) == (5, GS_HOST) and s.flags.c_contiguous and d.flags.c_contiguous
    assert np.array_equal(s, ei[:, 0]) and np.array_equal(d, ei[:, 1])
    t = torch.arange(10, dtype=torch.float64)[::2]
    got, _ = A.inp(t, np.float64, "t", DEV)
    assert got.flags.c_contiguous and np.array_equal(got, np.arange(0, 10, 2.0))


def test_short_input_raises(A):
    with pytest.raises(ValueError):
        A.inp(np.zeros(4), np.float64, "a", DEV, count=5)
    with pytest.raises(IndexError):
        A.inp(np.zeros(4), np.float64, "a", DEV, count=5, short=IndexError)
    assert A.inp(np.zeros(5), np.float64, "a", DEV, count=5)[0].shape == (5,)


def test_pair_needs_equal_length(A):
    with pytest.raises(ValueError):
        A.pair(np.zeros(4, dtype=np.int64), np.zeros(3, dtype=np.int64), DEV)
    s, d, E, loc = A.pair([0, 1], torch.tensor([1, 0], dtype=torch.int32), DEV)
    assert s.dtype == d.dtype == np.int64 and (E, loc) == (2, GS_HOST)
    with pytest.raises(TypeError):  # a graph's ids are int64 as given or converted on the host only
        A.pair(np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32), DEV, cast="never")


@pytest.mark.parametrize("kind", ["array", "tensor"])
def test_output_is_never_copied(A, kind):
    buf = np.zeros(6) if kind == "array" else torch.zeros(6, dtype=torch.float64)
    got, loc = A.out(buf, np.float64, 6, "out", DEV)
    assert got is buf and loc == GS_HOST  # a CPU tensor is a host buffer
    got, loc = A.out(buf, (np.float32, np.float64), 3, "out", DEV)
    assert got is buf
    fresh, loc = A.out(None, np.float64, 4, "out", DEV)
    assert fresh.shape == (4,) and fresh.dtype == np.float64 and loc == GS_HOST
    z, _ = A.out(None, (np.uint8, np.bool_), 4, "out", DEV, fresh=np.zeros)
    assert z.dtype == np.uint8 and not z.any()


@pytest.mark.parametrize("kind", ["array", "tensor"])
def test_output_rejections(A, kind):
    def mk(n, dt):
        a = np.zeros(n, dtype=dt)
        return a if kind == "array" else torch.from_numpy(a)

    with pytest.raises(TypeError):
        A.out(mk(6, np.float32), np.float64, 6, "out", DEV)
    with pytest.raises(TypeError):
        A.out([0.0] * 6, np.float64, 6, "out", DEV)
    with pytest.raises(ValueError):
        A.out(mk(5, np.float64), np.float64, 6, "out", DEV)
    with pytest.raises(IndexError):
        A.out(mk(5, np.float64), np.float64, 6, "out", DEV, short=IndexError)
    with pytest.raises(ValueError):
        A.out(mk(12, np.float64)[::2], np.float64, 6, "out", DEV)


def test_mask_output(A):
    m, loc = A.mask_out(None, 0, DEV)
    assert m.shape == (1,) and m.dtype == np.uint8 and loc == GS_HOST
    for buf in (np.zeros(5, dtype=np.uint8), torch.zeros(5, dtype=torch.bool)):
        assert A.mask_out(buf, 5, DEV)[0] is buf
    for bad in (np.zeros(5, dtype=np.int32), np.zeros(4, dtype=np.uint8),
                np.zeros(10, dtype=np.uint8)[::2]):
        with pytest.raises(ValueError):  # the mask outputs raise ValueError for every fault
            A.mask_out(bad, 5, DEV)


def test_pcg64_words(A):
    from gsparse.engine import Engine

    rng = np.random.default_rng(7)
    st = rng.bit_generator.state["state"]
    hi, lo, ihi, ilo = A.pcg64_words(rng)
    assert (hi << 64) | lo == st["state"] and (ihi << 64) | ilo == st["inc"]
    assert Engine._pcg64_words(rng) == (hi, lo, ihi, ilo)
    with pytest.raises(NotImplementedError):
        A.pcg64_words(np.random.Generator(np.random.MT19937(1)))


# ------------------------------------------------------ (b) recording Context
N, NNZ = 6, 12
SRC = np.array([0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 0], dtype=np.int64)
DST = np.array([1, 0, 2, 1, 3, 2, 4, 3, 5, 4, 0, 5], dtype=np.int64)
SCORES = np.linspace(0.1, 1.2, NNZ)

# index (the context handle not counted) of every GS_HOST / GS_DEVICE argument
LOCS = {
    "gs_graph_from_edge_index": (4,), "gs_coalesce_edges": (9,), "gs_graph_from_csr": (5,),
    "gs_graph_copy_csr": (3,), "gs_jaccard": (3,), "gs_jaccard_part": (3,),
    "gs_jaccard_part_counts": (3,), "gs_jaccard_from_counts": (3, 5), "gs_adamic_adar": (1, 5),
    "gs_degree": (3,), "gs_feature_cosine_f32": (2, 6), "gs_feature_cosine_f64": (2, 6),
    "gs_er_project_rows_cols": (3,), "gs_er_scores": (6,), "gs_er_iterations": (1,),
    "gs_er_copy_z": (3,), "gs_topk_mask": (1, 7), "gs_segment_argmax": (1, 4, 8),
    "gs_segment_topk": (1, 4, 9, 11), "gs_sample_mask": (1, 10), "gs_pcg64_doubles": (7,),
    "gs_sample_probs": (1, 4), "gs_cumsum_ordered": (1, 4), "gs_undirected_ids": (4, 6),
    "gs_random_mask": (1, 5, 8), "gs_spanning_forest": (1, 5, 11, 13),
    "gs_spectral_sample": (1, 5, 15, 17, 19, 21), "gs_metric_backbone_part": (6, 11),
    "gs_bb_begin": (6,), "gs_bb_landmarks_io": (2,), "gs_bb_state_io": (1,), "gs_bb_finish": (1,),
    "gs_jsel_begin": (3, 8), "gs_jsel_tie_positions": (2,), "gs_jsel_keep": (2, 5),
    "gs_jsel_mask": (3, 5), "gs_bb_class_counts": (4,), "gs_exact_er": (1,),
    "gs_exact_er_sparse": (1,), "gs_pair_distances": (6,), "gs_common_neighbors": (1,),
    "gs_clustering": (2,), "gs_components": (1,), "gs_spectral_bounds": (1,),
}


def _fill(ptr, ctype, values):
    (ctype * len(values)).from_address(ptr)[:] = list(values)


class Recorder:
    """Stands in for ``_lib.Context``: records every call, never loads the library.  A hook
    per entry point fills the outputs a method reads back."""

    device = DEV

    def __init__(self):
        self.calls = []
        self.hooks = {
            "gs_jaccard_shares": lambda np_, rc, oo: (_fill(rc, ctypes.c_int64, range(np_ + 1)),
                                                      _fill(oo, ctypes.c_int64,
                                                            [3 * i for i in range(np_ + 1)])),
            "gs_graph_copy_csr": lambda ip, ix, d, loc: _fill(ip, ctypes.c_int64,
                                                               range(0, 2 * N + 1, 2)),
            "gs_er_prepare": lambda k, reg, m: setattr(m._obj, "value", 5),
            "gs_undirected_ids": lambda *a: (setattr(a[7]._obj, "value", 6),
                                             setattr(a[8]._obj, "value", 0)),
            "gs_sample_mask": lambda *a: setattr(a[11]._obj, "value", 0),
            "gs_spectral_sample": lambda *a: (setattr(a[22]._obj, "value", 6),
                                              setattr(a[27]._obj, "value", 0)),
            "gs_bb_begin": lambda *a: setattr(a[10]._obj, "value", 2),
            "gs_bb_class_counts": lambda *a: a[5] is not None and setattr(a[5]._obj, "value", NNZ),
        }

    def shape(self):
        return N, NNZ, True

    def call(self, name, *args):
        self.calls.append((name, args))
        if name in self.hooks:
            self.hooks[name](*args)

    def ptrs(self, name):
        """Every integer argument of the last recorded call of ``name``."""
        args = [a for n, a in self.calls if n == name][-1]
        return [a for a in args if isinstance(a, int)]


def check_calls(rec):
    assert rec.calls
    for name, args in rec.calls:
        assert name in SIGNATURES, name
        argtypes = SIGNATURES[name][1]
        assert len(args) + 1 == len(argtypes), (name, len(args), len(argtypes))
        for i, (a, t) in enumerate(zip(args, argtypes[1:])):
            try:
                t.from_param(a)
            except (TypeError, ctypes.ArgumentError) as e:
                raise AssertionError(f"{name} argument {i}: {a!r} is no {t.__name__}: {e}")
        for i in LOCS.get(name, ()):
            assert args[i] in (GS_HOST, GS_DEVICE) and isinstance(args[i], int), (name, i, args[i])


@pytest.fixture()
def rec():
    return Recorder()


@pytest.fixture()
def eng(rec):
    from gsparse.engine import Engine

    return Engine(rec)


def test_locs_table_matches_signatures():
    for name, idx in LOCS.items():
        for i in idx:
            assert SIGNATURES[name][1][i + 1] is ctypes.c_int, (name, i)


def test_scorers(rec, eng):
    out = np.empty(NNZ)
    for call, name in ((lambda o: eng.jaccard(out=o), "gs_jaccard"),
                       (lambda o: eng.jaccard(2, 7, out=o), "gs_jaccard"),
                       (lambda o: eng.jaccard_part(0, 2, out=o), "gs_jaccard_part"),
                       (lambda o: eng.degree(out=o), "gs_degree"),
                       (lambda o: eng.er_scores(0, 3, out=o), "gs_er_scores"),
                       (lambda o: eng.common_neighbors(out=o), "gs_common_neighbors"),
                       (lambda o: eng.exact_er(out=o), "gs_exact_er"),
                       (lambda o: eng.exact_er(out=o, method="sparse"), "gs_exact_er_sparse"),
                       (lambda o: eng.adamic_adar(out=o), "gs_adamic_adar")):
        assert call(out) is out  # the caller's buffer comes back, not a copy
        assert out.ctypes.data in rec.ptrs(name)
        fresh = call(None)
        assert isinstance(fresh, np.ndarray) and fresh.dtype == np.float64
    assert eng.jaccard(2, 7).shape == (5,) and eng.jaccard().shape == (NNZ,)
    c = np.ones(N)
    eng.adamic_adar(c=c)
    assert c.ctypes.data in rec.ptrs("gs_adamic_adar")
    assert eng.exact_er_iterations == 0 and eng.exact_er_cg_iterations == 0
    check_calls(rec)


def test_scorer_cpu_tensor_out_is_a_host_buffer(rec, eng):
    """The one deliberate change: a CPU tensor ``out=`` used to be labelled GS_DEVICE."""
    out = torch.empty(NNZ, dtype=torch.float64)
    assert eng.jaccard(out=out) is out
    assert rec.calls[-1] == ("gs_jaccard", (0, NNZ, out.data_ptr(), GS_HOST))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_feature_cosine(rec, eng, dtype):
    x = np.ones((N, 3), dtype=dtype)
    out = np.empty(NNZ)
    assert eng.feature_cosine(x, out=out) is out
    name = "gs_feature_cosine_f32" if dtype == np.float32 else "gs_feature_cosine_f64"
    assert rec.calls[-1] == (name, (x.ctypes.data, 3, GS_HOST, 0, NNZ, out.ctypes.data, GS_HOST))
    t = torch.from_numpy(x)
    eng.feature_cosine(t, 1, 4)
    assert rec.calls[-1][1][:5] == (t.data_ptr(), 3, GS_HOST, 1, 4)
    xs = np.ones((N, 6), dtype=dtype)[:, ::2]  # strided: a contiguous copy is handed on
    eng.feature_cosine(xs)
    assert rec.calls[-1][1][0] != xs.ctypes.data
    with pytest.raises(ValueError):
        eng.feature_cosine(np.ones((N + 1, 3), dtype=dtype))
    with pytest.raises(NotImplementedError):
        eng.feature_cosine(np.ones((N, 3), dtype=np.float16))
    check_calls(rec)


def test_jaccard_shares_and_counts(rec, eng):
    rc, oo = eng.jaccard_shares(2)
    assert rc.tolist() == [0, 1, 2] and oo.tolist() == [0, 3, 6]
    cnt = eng.jaccard_part_counts(1, 2)
    assert cnt.dtype == np.uint32 and cnt.shape == (3,)
    with pytest.raises(ValueError):
        eng.jaccard_part_counts(2, 2)
    counts = np.zeros(6, dtype=np.uint32)
    out = np.empty(NNZ)
    assert eng.jaccard_from_counts(2, counts, 3, out=out) is out
    assert rec.calls[-1] == ("gs_jaccard_from_counts",
                             (2, counts.ctypes.data, 3, GS_HOST, out.ctypes.data, GS_HOST))
    with pytest.raises(IndexError):
        eng.jaccard_from_counts(2, counts, 4)
    check_calls(rec)


def test_jsel_family(rec, eng):
    counts = np.zeros(3, dtype=np.int32)
    hist = np.zeros(eng.JSEL_BINS, dtype=np.int64)
    with pytest.raises(ValueError):  # the ranks all-reduce hist on the device
        eng.jsel_begin(0, 2, counts, 5, False, hist)
    with pytest.raises(TypeError):
        eng.jsel_begin(0, 2, counts.astype(np.int64), 5, False, hist)
    with pytest.raises(IndexError):
        eng.jsel_begin(0, 2, counts[:2], 5, False, hist)
    assert eng.jsel_step(hist) == 0
    assert hist.ctypes.data in rec.ptrs("gs_jsel_step")
    assert eng.jsel_result() == (0.0, 0, 0, 0)
    pos = np.zeros(4, dtype=np.int64)
    assert eng.jsel_tie_positions(pos) is pos
    assert rec.calls[-1] == ("gs_jsel_tie_positions", (pos.ctypes.data, 4, GS_HOST))
    eng._jsel_pairs = 3
    keep = np.zeros(1, dtype=np.uint8)
    assert eng.jsel_keep(None, 0, 0, keep) is keep
    assert rec.calls[-1] == ("gs_jsel_keep", (None, 0, GS_HOST, 0, keep.ctypes.data, GS_HOST))
    assert eng.jsel_keep(pos, 4, 1, keep) is keep
    assert rec.calls[-1] == ("gs_jsel_keep",
                             (pos.ctypes.data, 4, GS_HOST, 1, keep.ctypes.data, GS_HOST))
    with pytest.raises(IndexError):
        eng.jsel_keep(pos, 5, 1, keep)
    kall = np.zeros(2, dtype=np.uint8)
    mask = np.zeros(NNZ, dtype=np.uint8)
    assert eng.jsel_mask(2, kall, 1, mask) is mask
    assert rec.calls[-1] == ("gs_jsel_mask",
                             (2, kall.ctypes.data, 1, GS_HOST, mask.ctypes.data, GS_HOST))
    with pytest.raises(IndexError):
        eng.jsel_mask(2, kall, 1, mask[:-1])
    with pytest.raises(TypeError):
        eng.jsel_mask(2, kall, 1, mask.astype(np.int32))
    check_calls(rec)


def test_approx_er_path(rec, eng):
    for mode in ("device", "host"):
        s = eng.approx_er(epsilon=3.0, rng_mode=mode, blas_threads=1)
        assert s.shape == (NNZ,) and eng.m == 5
    assert eng.er_iterations().dtype == np.int32
    assert eng.er_z(0, 2).shape == (N, 2)
    assert set(eng.er_reg_window()) == {"W", "slow_plain", "slow_window", "window_codes"}
    names = [n for n, _ in rec.calls]
    for n in ("gs_er_prepare", "gs_er_project_pcg64_cols", "gs_er_project_rows_cols", "gs_er_solve",
              "gs_er_scores", "gs_er_iterations", "gs_er_copy_z", "gs_er_reg_window"):
        assert n in names
    check_calls(rec)


def test_topology(rec, eng):
    assert eng.clustering() == 0.0
    avg, cv = eng.clustering(per_node=True)
    assert cv.shape == (N,)
    lab, cnt, big = eng.components()
    assert lab.shape == (N,) and lab.dtype == np.int32
    assert eng.fiedler() == 0.0 and eng.fiedler_cg_iterations is None
    assert eng.fiedler(method="sparse") == 0.0 and eng.fiedler_cg_iterations == 0
    hw = np.ones(NNZ)
    assert eng.spectral_bounds(hw) == (0.0, 0.0)
    assert rec.calls[-1][1][:3] == (hw.ctypes.data, GS_HOST, NNZ)
    eng.spectral_bounds(torch.ones(NNZ, dtype=torch.float32))
    eng.spectral_bounds([1.0] * NNZ)
    assert rec.calls[-1][1][1:3] == (GS_HOST, NNZ)
    assert eng.spectral_bounds_iterations == 0 and eng.spectral_bounds_cg_iterations == 0
    with pytest.raises(ValueError):
        eng.fiedler(method="qr")
    check_calls(rec)


def test_segment_and_sampling(rec, eng):
    pick = eng.segment_argmax(SCORES, SRC, N)
    assert pick.shape == (N,) and pick.dtype == np.int64
    assert rec.calls[-1][1][:7] == (SCORES.ctypes.data, GS_HOST, NNZ, SRC.ctypes.data, GS_HOST,
                                    NNZ, N)
    mask, status, info = eng.segment_topk(SCORES, SRC, N, 2)
    assert mask.dtype == bool and mask.shape == (NNZ,) and status.shape == (N,)
    assert set(info["classes"]) == set(eng.SEGK_CLASSES)
    with pytest.raises(IndexError):
        eng.segment_topk(SCORES[:4], SRC, N, 2)
    rng = np.random.default_rng(3)
    m, st, rounds, draws = eng.sample_mask(SCORES, NNZ, 4, rng)
    assert m.dtype == bool and m.shape == (NNZ,) and st == 0
    assert SCORES.ctypes.data in rec.ptrs("gs_sample_mask")
    d = eng.pcg64_doubles(rng, 2, 5)
    assert d.shape == (5,) and d.dtype == np.float64
    assert eng.pcg64_doubles(rng, 0, 0).shape == (0,)
    p, total = eng.sample_probs(SCORES)
    assert p.shape == (NNZ,) and total == 0.0
    assert eng.cumsum_ordered(SCORES).shape == (NNZ,)
    assert eng.cumsum_ordered(np.zeros(0)).shape == (0,)
    m, cut, nb, nt = eng.topk_mask(SCORES, NNZ, 6, False)
    assert m.dtype == bool and m.shape == (NNZ,)
    assert rec.calls[-1][1][:6] == (SCORES.ctypes.data, GS_HOST, NNZ, NNZ, 6, 0)
    m, *_ = eng.topk_mask(torch.from_numpy(SCORES.astype(np.float32)), NNZ, 6, True)
    assert m.shape == (NNZ,)
    assert eng.topk_mask(np.zeros(0), 0, 0, False)[0].shape == (0,)
    check_calls(rec)


def test_random_forest_spectral(rec, eng):
    inv, cnt, status = eng.undirected_ids(SRC, DST, N)
    assert inv.shape == (NNZ,) and inv.dtype == np.int64 and (cnt, status) == (6, 0)
    assert rec.calls[-1][1][:5] == (N, NNZ, SRC.ctypes.data, DST.ctypes.data, GS_HOST)
    eng.undirected_ids(SRC.astype(np.int32), torch.from_numpy(DST), N)  # cast, CPU tensor: host
    with pytest.raises(ValueError):
        eng.undirected_ids(SRC, DST[:-1], N)
    us = np.linspace(0, 1, 6)
    inverse = np.arange(NNZ, dtype=np.int64) % 6
    m, cut, nb, nt = eng.random_mask(us, inverse, 3, NNZ)
    assert m.dtype == bool and m.shape == (NNZ,)
    assert rec.calls[-1][1][:7] == (us.ctypes.data, GS_HOST, 6, 3, inverse.ctypes.data, GS_HOST, NNZ)
    with pytest.raises(IndexError):
        eng.random_mask(us, inverse[:-1], 3, NNZ)
    mask, labels, info = eng.spanning_forest(SCORES, SRC, DST, N, expand=True)
    assert mask.dtype == bool and mask.shape == (NNZ,)
    assert labels.dtype == np.int32 and labels.shape == (N,)
    assert set(info) == {"n_forest", "n_marked", "rounds"}
    assert rec.calls[-1][1][:10] == (SCORES.ctypes.data, GS_HOST, NNZ, SRC.ctypes.data,
                                     DST.ctypes.data, GS_HOST, NNZ, N, 0, 1)
    rng = np.random.default_rng(5)
    mask, weight, counts, inverse, info = eng.spectral_sample(SCORES, SRC, DST, N, 20, rng)
    assert mask.dtype == bool and mask.shape == (NNZ,) and weight.dtype == np.float64
    assert counts.shape == (6,) and counts.dtype == np.int64 and inverse.shape == (NNZ,)
    assert info["status"] == 0 and info["m"] == 6
    with pytest.raises(ValueError):
        eng.spectral_sample(SCORES, SRC, DST, N, 20, rng, method="nope")
    check_calls(rec)


def test_backbone_stages(rec):
    from gsparse.metric_backbone import BackboneStages

    st = BackboneStages(rec)
    ei = np.stack([SRC, DST])
    w = np.linspace(1, 2, NNZ)
    assert st.begin(ei, N, w, 1e-9, 0, 1) == 2 and (st.n, st.E, st.K) == (N, NNZ, 2)
    assert rec.calls[-1][1][:2] == (N, NNZ) and rec.calls[-1][1][5:7] == (NNZ, GS_HOST)
    st.begin(torch.from_numpy(ei).to(torch.int32), N, torch.from_numpy(w).float(), 1e-9, 0, 1)
    st.begin(ei.tolist(), N, w.tolist(), 1e-9, 0, 1)
    with pytest.raises(IndexError):
        st.begin(ei, N, w[:-1], 1e-9, 0, 1)
    keep = np.zeros(NNZ, dtype=np.uint8)
    assert st.pair_part(ei, N, w, 1e-9, 0, 1, keep) is keep
    assert rec.calls[-1][1][10:12] == (keep.ctypes.data, GS_HOST)
    with pytest.raises(TypeError):
        st.pair_part(ei, N, w, 1e-9, 0, 1, np.zeros(NNZ, dtype=np.int64))
    with pytest.raises(ValueError):
        st.pair_part(ei, N, w, 1e-9, 0, 1, np.zeros(NNZ - 1, dtype=np.uint8))
    D, comp = np.zeros(2 * N), np.zeros(2, dtype=np.int32)
    st.landmarks_io(D, comp, out=True)
    assert rec.calls[-1] == ("gs_bb_landmarks_io", (D.ctypes.data, comp.ctypes.data, GS_HOST, 0))
    st.landmarks_io(torch.from_numpy(D), torch.from_numpy(comp), out=False)
    assert rec.calls[-1] == ("gs_bb_landmarks_io", (D.ctypes.data, comp.ctypes.data, GS_HOST, 1))
    with pytest.raises(TypeError):
        st.landmarks_io(D.astype(np.float32), comp, out=True)
    st.certify(0, 1)
    state = np.zeros(NNZ, dtype=np.uint8)
    st.state_io(state, out=True)
    assert rec.calls[-1] == ("gs_bb_state_io", (state.ctypes.data, GS_HOST, 0))
    with pytest.raises(ValueError):
        st.state_io(state[:-1], out=False)
    assert st.plan() == 0
    st.search(0, 0, 0, 1)
    k2, relax = st.finish()
    assert k2.dtype == np.uint8 and k2.shape == (NNZ,) and relax == 0
    assert st.finish(keep)[0] is keep
    check_calls(rec)


def test_backbone_functions(rec):
    from gsparse.loader import coalesce_edges
    from gsparse.metric_backbone import backbone_mask, decision_classes, pair_distances

    ei = np.stack([SRC, DST])
    w = np.linspace(1, 2, NNZ)
    mask, relax = backbone_mask(ei, N, w, ctx=rec, return_relax=True)
    assert mask.dtype == bool and mask.shape == (NNZ,) and relax == 0
    assert backbone_mask(ei.astype(np.int32), N, w.astype(np.float32), ctx=rec).shape == (NNZ,)
    with pytest.raises(IndexError):
        backbone_mask(ei, N, w[:-1], ctx=rec)
    d = pair_distances(ei, N, w, [(0, 1), (2, 3)], ctx=rec)
    assert d.shape == (2,) and d.dtype == np.float64
    assert rec.calls[-1][1][:2] == (N, NNZ) and rec.calls[-1][1][5:8] == (NNZ, GS_HOST, 2)
    pair_distances(ei, N, None, [(0, 1)], ctx=rec)
    assert rec.calls[-1][1][4:7] == (None, 0, GS_HOST)
    with pytest.raises(IndexError):
        pair_distances(ei, N, w[:-1], [(0, 1)], ctx=rec)
    counts, why = decision_classes(ctx=rec, return_why=True)
    assert why.shape == (NNZ,) and why.dtype == np.uint8
    out = coalesce_edges(ei, N, ctx=rec)
    assert out.shape == (2, 2 * NNZ) and out.dtype == np.int64
    assert rec.calls[-1][1][:2] == (N, NNZ) and rec.calls[-1][1][-1] == GS_HOST
    check_calls(rec)


def test_context_set_graph(rec):
    """Context.set_graph_* run unbound on the recorder: they only marshal and call."""
    _lib.Context.set_graph_edge_index(rec, N, SRC, DST)
    assert rec.calls[-1] == ("gs_graph_from_edge_index",
                             (N, NNZ, SRC.ctypes.data, DST.ctypes.data, GS_HOST))
    ip = np.arange(0, 2 * N + 1, 2, dtype=np.int64)
    ix = DST.astype(np.int32)
    data = np.ones(NNZ)
    _lib.Context.set_graph_csr(rec, N, ip, ix, data)
    assert rec.calls[-1] == ("gs_graph_from_csr",
                             (N, NNZ, ip.ctypes.data, ix.ctypes.data, data.ctypes.data, GS_HOST))
    _lib.Context.set_graph_csr(rec, N, ip.astype(np.int32), DST, None)  # cast on the host
    assert rec.calls[-1][1][:2] == (N, NNZ) and rec.calls[-1][1][4:] == (None, GS_HOST)
    assert rec._keep[0].dtype == np.int64 and rec._keep[1].dtype == np.int32
    check_calls(rec)


# ---- rejections that are new: before, these buffers went on to the library
def test_new_rejections(rec, eng):
    n0 = len(rec.calls)
    with pytest.raises(TypeError):
        eng.jaccard(out=np.empty(NNZ, dtype=np.float32))
    with pytest.raises(ValueError):
        eng.degree(out=np.empty(NNZ - 1))
    with pytest.raises(ValueError):
        eng.jaccard(2, 7, out=np.empty(4))
    with pytest.raises(ValueError):
        eng.common_neighbors(out=np.empty(2 * NNZ)[::2])
    with pytest.raises(ValueError):
        eng.adamic_adar(c=np.ones(N - 1))
    with pytest.raises(TypeError):
        eng.jsel_step(np.zeros(eng.JSEL_BINS, dtype=np.int32))
    with pytest.raises(ValueError):
        eng.jsel_mask(2, np.zeros(2, dtype=np.uint8), 1, np.zeros(2 * NNZ, dtype=np.uint8)[::2])
    with pytest.raises(ValueError):
        _lib.Context.set_graph_edge_index(rec, N, SRC, DST[:-1])
    with pytest.raises(ValueError):
        _lib.Context.set_graph_csr(rec, N, np.zeros(N, dtype=np.int64), DST, None)
    assert len(rec.calls) == n0  # nothing reached the library


# ------------------------------------------------------------------ (c) imports
PLAN_NAMES = ("blas_threads_default", "jl_dim", "aa_weights", "er_split", "er_plan",
              "er_reg_layout", "er_reg_layout_w", "xer_sparse_plan", "bb_geometry")


def test_plan_functions_importable_from_engine():
    import gsparse.engine as E

    for name in PLAN_NAMES + ("Engine", "_ROW_CHUNK_BYTES"):
        assert hasattr(E, name), name
    assert jl_ok(E.jl_dim) and np.allclose(E.aa_weights(np.array([0, 1, 3])),
                                           1 / np.sqrt(np.log([2.0, 3.0])))


def jl_ok(jl_dim):
    return jl_dim(100, 0.5) == int(24 * np.log(100) / 0.25) and jl_dim(1, 1e9) == 1


def test_plan_functions_are_the_plans_modules():
    import gsparse.engine as E
    import gsparse.plans as P

    for name in PLAN_NAMES:
        assert getattr(E, name) is getattr(P, name), name


def test_engine_surface():
    from gsparse.engine import Engine

    assert (Engine.JSEL_BINS, Engine.JSEL_PASSES) == (8192, 5)
    assert Engine.SEGK_CLASSES == ("empty", "all", "short", "lds", "stream")
    assert (Engine.SAMPLE_TILE, Engine.SAMPLE_SUBTREE) == (1024, 2048)
    assert Engine.SPECTRAL_METHODS == {"multinomial": 0, "independent": 1}
