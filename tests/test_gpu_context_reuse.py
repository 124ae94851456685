"""One context, many graphs: a single Context walks reuse_cases.SEQUENCE (G1, G2, G3, G4, G5,
G1 -- a hub graph, a small one, the hub graph relabelled to the same n / nnz / degrees, an
empty one, a directed one with multiplicities, and the first again) and every family of
entry points is compared on every graph

* with its CPU specification or oracle, at the bar the family's own test file uses, and
* bit for bit with the same call on a fresh context, where README or DESIGN says the result
  is the same on every run: every scorer that is bit-exact with its oracle (Jaccard and its
  parts and counts, Adamic-Adar, degree, feature cosine, common neighbours, ApproxER), the
  trussness, segment ranks and local scores (4k), the Simmelian score (4l), the
  spanning forest (4g), the sampled and spectral selections (4c, 4h: draws of a seeded
  stream), the undirected ids and the metric backbone (integer / exact results).  The exact
  effective resistance (dense and sparse), the algebraic connectivity (dense and sparse) and
  the spectral bounds are compared with their references alone: DESIGN promises the dense
  Newton-Schulz form and the bounds' vector passes a fixed order, not the whole of each
  entry point.

What rides from one graph to the next -- grow-only buffers, scratch[0..5] handed between
subsystems, the caches keyed by the graph epoch -- is listed in DESIGN.md ("What a context
carries between graphs").  A stale cache shows on G3 (reuse_cases: every reference differs
from G1's), a buffer sized for a smaller graph on the last G1, a counter zeroed only on
first allocation on any second use."""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import reuse_cases as C
from conftest import EXACT_ER_ATOL, bits_equal

pytestmark = pytest.mark.gpu

XER_RTOL, XER_ATOL = 1e-8, 1e-12  # test_gpu_parity.py / test_gpu_exact_er_sparse.py, vs the lifted oracle
FIEDLER_RTOL, FIEDLER_ATOL = 1e-6, 1e-14  # test_gpu_fiedler_sparse.py
BOUNDS_RTOL = 1e-6  # spectral_bounds_cases.RTOL, times lambda_max

# the knobs that lower the class limits: the small graphs reach every kernel class too
KNOBS = {"GSPARSE_SEGR_SHORT_MAX": "4", "GSPARSE_SEGR_LDS_MAX": "16", "GSPARSE_SIM_WAVE_MAX": "2",
         "GSPARSE_SIM_MID_MAX": "4", "GSPARSE_SIM_LDS_MAX": "8", "GSPARSE_TRUSS_TAIL": "16"}


@pytest.fixture(scope="module")
def ctx():
    from gsparse._lib import Context

    c = Context(0)
    yield c
    c.close()


def put(ctx, name):
    """Set graph `name` on the context, from its edge list -> Engine."""
    from gsparse.engine import Engine

    n, ei = C.graph(name)
    ctx.set_graph_edge_index(n, np.array(ei[0]), np.array(ei[1]))
    ip, ix, d = C.csr(name)
    assert ctx.shape() == (n, len(ix), C.symmetric(name)), name
    gip, gix, gd = ctx.csr()
    assert np.array_equal(gip, ip) and np.array_equal(gix, ix) and bits_equal(gd, d), name
    return Engine(ctx)


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the families: each checks against the CPU side and returns what it got -------------
def fam_scorers(eng, name):
    ip, ix, _ = C.csr(name)
    r = {}
    for m in ("jaccard", "adamic_adar", "degree"):
        r[m] = getattr(eng, m)()
        assert bits_equal(r[m], C.ref(name, m)), (name, m)
    r["feature_cosine"] = eng.feature_cosine(C.features(name))
    assert bits_equal(r["feature_cosine"], C.ref(name, "feature_cosine")), name
    if C.symmetric(name):
        r["common_neighbors"] = eng.common_neighbors()
        assert bits_equal(r["common_neighbors"], C.ref(name, "common_neighbors")), name
    else:
        with pytest.raises(NotImplementedError):
            eng.common_neighbors()
    parts = [eng.jaccard_part(p, 2) for p in (0, 1)]
    r["part0"] = parts[0]
    assert bits_equal(parts[0] + parts[1], C.ref(name, "jaccard")), name
    if C.symmetric(name) and len(ix):
        for p in (0, 1):
            r[f"counts{p}"] = eng.jaccard_part_counts(p, 2)
        both = np.concatenate([r["counts0"], r["counts1"]])
        assert np.array_equal(both, C.ref(name, "part_counts")), name
    elif not C.symmetric(name):
        with pytest.raises(NotImplementedError):
            eng.jaccard_shares(2)
    if C.symmetric(name) and len(ix) >= 2:  # the select's slot table is keyed by the epoch too
        r["jsel"] = _jsel_one_part(eng, C.JSEL_KEEP)
        assert np.array_equal(r["jsel"], C.ref(name, "jsel")), name
    assert bits_equal(eng.jaccard(), C.ref(name, "jaccard")), name  # the whole after the parts
    return r


def _jsel_one_part(eng, ratio):
    """gs_jsel_* with one part (the all-reduce of the histograms is the identity): the keep
    mask of the int(nnz * ratio) highest Jaccard scores, gs_topk_mask's stable rule."""
    dev = torch.device("cuda", eng.ctx.device)
    nnz, num_keep = eng.nnz, int(eng.nnz * ratio)
    _, off = eng.jaccard_shares(1)
    stride = max(1, int(off[1] - off[0]))
    counts = torch.zeros(stride, dtype=torch.int32, device=dev)
    eng.jaccard_part_counts(0, 1, out=counts)
    hist = torch.zeros(eng.JSEL_BINS, dtype=torch.int64, device=dev)
    eng.jsel_begin(0, 1, counts, num_keep, False, hist, torch.empty(stride, dtype=torch.float64, device=dev))
    left = eng.JSEL_PASSES
    while left:
        left = eng.jsel_step(hist)
    _, beyond, tied, mine = eng.jsel_result()
    need, ties = num_keep - beyond, None
    if 0 < need < tied:
        assert mine == tied
        ties = torch.zeros(max(1, mine), dtype=torch.int64, device=dev)
        eng.jsel_tie_positions(ties)
        ties = ties[:mine]
    s4 = (stride + 3) // 4
    keep = torch.zeros(s4, dtype=torch.uint8, device=dev)
    eng.jsel_keep(ties, tied, need, keep)
    mask = torch.empty(nnz, dtype=torch.uint8, device=dev)
    eng.jsel_mask(1, keep, s4, mask)
    return mask.cpu().numpy().astype(bool)


def _approx_er(eng):
    """Engine.approx_er's calls with reuse_cases' few JL columns and short CG."""
    if eng.er_prepare(C.ER_K) == 0:
        return np.zeros(eng.nnz, dtype=np.float64)
    eng.er_project_device(np.random.default_rng(42), C.ER_K)
    eng.er_solve(0, C.ER_K, C.ER_ITERS, 1e-6, 1)
    return eng.er_scores(0, C.ER_K, True)


def fam_approx_er(eng, name):
    """Twice on the same graph: whatever the solver keeps per graph (the ELL copy of the
    register-resident form, the unit-weight flags) is reused once, then dropped at the next
    graph.  (The split form of the register-resident solver needs several BLAS chunks, n >
    10000: these graphs do not reach it.)"""
    first, second = _approx_er(eng), _approx_er(eng)
    assert bits_equal(first, C.ref(name, "approx_er")), name
    assert bits_equal(second, C.ref(name, "approx_er")), name
    return {"approx_er": second}


def fam_exact(eng, name):
    calls = {
        "xer_dense": lambda: eng.exact_er(method="dense"),
        "xer_sparse": lambda: eng.exact_er(method="sparse"),
        "fiedler_dense": lambda: eng.fiedler(method="dense"),
        "fiedler_sparse": lambda: eng.fiedler(method="sparse"),
        "bounds": lambda: eng.spectral_bounds(np.ones(eng.nnz)),
    }
    if not C.symmetric(name):  # G5: every one of them refuses a directed graph
        for k, f in calls.items():
            with pytest.raises(NotImplementedError):
                f()
        return {}
    r = {}
    want = C.ref(name, "exact_er")
    for k in ("xer_dense", "xer_sparse"):
        r[k] = calls[k]()
        assert r[k].shape == want.shape
        assert np.max(np.abs(r[k] - want), initial=0.0) <= EXACT_ER_ATOL, (name, k)
        np.testing.assert_allclose(r[k], want, rtol=XER_RTOL, atol=XER_ATOL, err_msg=f"{name} {k}")
    if C.topology(name)[1] != 1:  # G1, G3, G4: several components, no connectivity value
        for k in ("fiedler_dense", "fiedler_sparse", "bounds"):
            with pytest.raises(ValueError, match="components"):
                calls[k]()
        return r
    ac, hw, bounds = C.connected_refs(name)
    for k in ("fiedler_dense", "fiedler_sparse"):
        r[k] = calls[k]()
        np.testing.assert_allclose(r[k], ac, rtol=FIEDLER_RTOL, atol=FIEDLER_ATOL, err_msg=f"{name} {k}")
    lo, hi = eng.spectral_bounds(hw)
    assert abs(lo - bounds[0]) <= BOUNDS_RTOL * bounds[1] and abs(hi - bounds[1]) <= BOUNDS_RTOL * bounds[1], \
        (name, (lo, hi), bounds)
    r["bounds"] = np.array([lo, hi])
    return r


def fam_topology(eng, name):
    if not C.symmetric(name):
        for f in (eng.trussness, eng.simmelian, eng.clustering):
            with pytest.raises(NotImplementedError):
                f()
        return {}
    r = {}
    r["trussness"], info = eng.trussness()
    want = C.ref(name, "trussness")
    assert np.array_equal(r["trussness"], want), name
    assert info["max_truss"] == (int(want.max()) if len(want) else 0)
    r["simmelian"], _ = eng.simmelian(0)
    assert bits_equal(r["simmelian"], C.ref(name, "simmelian")), name
    r["simmelian_k3"], _ = eng.simmelian(3)
    assert bits_equal(r["simmelian_k3"], C.ref(name, "simmelian_k3")), name
    avg, r["clustering"] = eng.clustering(per_node=True)
    want_avg, want_cnt, want_big = C.topology(name)
    assert bits_equal(np.array([avg]), np.array([want_avg])), (name, avg, want_avg)
    assert bits_equal(r["clustering"], C.ref(name, "clustering")), name
    r["labels"], cnt, big = eng.components()
    assert np.array_equal(r["labels"], C.ref(name, "component_labels")), name
    assert (cnt, big) == (want_cnt, want_big), name
    return r


def fam_columns(eng, name):
    """The entry points that take src / dst / scores, on the edge list of the graph."""
    from gsparse import selection as S
    from gsparse.metric_backbone import backbone_mask

    n, ei = C.graph(name)
    E = ei.shape[1]
    src, dst, s = np.array(ei[0]), np.array(ei[1]), np.array(C.scores(name))
    r = {}
    r["rank"], deg, _ = eng.segment_rank(s, src, n)
    assert np.array_equal(r["rank"], C.ref(name, "segment_rank")), name
    assert np.array_equal(deg, np.bincount(src, minlength=n)), name
    r["local"], _ = eng.local_scores(s, src, dst, n)
    assert bits_equal(r["local"], C.ref(name, "local")), name
    r["forest"], _, info = eng.spanning_forest(s, src, dst, n)
    assert np.array_equal(r["forest"], C.ref(name, "forest")), name
    assert info["n_forest"] == int(C.ref(name, "forest").sum())
    if E == 0:  # G4: the selections below are defined over at least one column
        return r
    r["topk"], cut, beyond, tied = eng.topk_mask(s, E, int(E * C.KEEP), False)
    assert np.array_equal(r["topk"], C.ref(name, "topk")), name
    assert (beyond, tied) == (int((s > cut).sum()), int((s == cut).sum())), name
    for per_node in (1, 2):  # gs_segment_argmax, gs_segment_topk
        got = S.degree_aware_mask_device(eng, s, ei, n, E, C.KEEP, per_node)
        assert np.array_equal(got, C.ref(name, f"degree_aware_{per_node}")), (name, per_node)
    r["sampled"] = S.sampled_mask_device(eng, s + 0.125, E, C.KEEP, seed=42)
    assert np.array_equal(r["sampled"], C.ref(name, "sampled")), name
    ids = C.ref(name, "undirected_ids")
    r["ids"], cnt, status = eng.undirected_ids(src, dst, n)
    assert status == 0 and cnt == int(ids.max()) + 1 and np.array_equal(r["ids"], ids), name
    r["random"] = eng.random_mask(C.random_scores(cnt), r["ids"], max(1, cnt // 2), E)[0]
    assert np.array_equal(r["random"], C.ref(name, "random")), name
    got = eng.spectral_sample(s, src, dst, n, max(E // 4, 1), np.random.default_rng(C.SPECTRAL_SEED))
    r["spectral"] = got[1]
    assert bits_equal(got[1], C.ref(name, "spectral_weight")), name
    assert np.array_equal(got[0], C.ref(name, "spectral_weight") > 0), name
    r["backbone"] = backbone_mask(ei, n, 1.0 + s, ctx=eng.ctx)
    assert np.array_equal(r["backbone"], C.ref(name, "backbone")), name
    return r


FAMILIES = {"scorers": fam_scorers, "approx_er": fam_approx_er, "exact": fam_exact,
            "topology": fam_topology, "columns": fam_columns}
# compared with the fresh context's bytes; the others with their references alone (see above)
NOT_BITWISE = {"xer_dense", "xer_sparse", "fiedler_dense", "fiedler_sparse", "bounds"}
_FRESH = {}


def fresh(key, name):
    """The family's results for `name` on a context that has seen no other graph; once."""
    from gsparse._lib import Context

    if (key, name) not in _FRESH:
        c = Context(0)
        try:
            _FRESH[key, name] = FAMILIES[key](put(c, name), name)
        finally:
            c.close()
    return _FRESH[key, name]


def visit(ctx, key, name):
    got = FAMILIES[key](put(ctx, name), name)
    want = fresh(key, name)
    assert got.keys() == want.keys(), (key, name)
    for k in got:
        if k not in NOT_BITWISE:
            assert same_bytes(got[k], want[k]), f"{key}.{k} on {name}: not the fresh context's bytes"


def walk(ctx, key):
    for name in C.SEQUENCE:
        visit(ctx, key, name)


def test_scorers(ctx):
    walk(ctx, "scorers")


@pytest.mark.parametrize("mode", [None, "0", "4", "5"])
def test_approx_er(ctx, mode, monkeypatch):
    """The default plan and the batched (0), resident (4) and register-resident (5) solvers:
    reg_ell_key and unit_key are each keyed by the graph epoch."""
    if mode is not None:
        monkeypatch.setenv("GSPARSE_CG_MODE", mode)
    for name in C.SEQUENCE:  # no fresh context per mode: the oracle's bits are the bar
        fam_approx_er(put(ctx, name), name)


def test_exact_er_fiedler_bounds(ctx):
    """G2 is the walk's one connected graph; G2P (reuse_cases: G2's shape, another Fiedler
    value, other bounds) follows it, so the connectivity and bounds solvers compute on two
    distinct graphs on one context, then on the first again."""
    walk(ctx, "exact")
    for name in ("G2", "G2P", "G2"):
        visit(ctx, "exact", name)


def test_trussness_simmelian_clustering_components(ctx):
    walk(ctx, "topology")


def test_column_entry_points(ctx):
    walk(ctx, "columns")


def test_lowered_class_limits(ctx, monkeypatch):
    """The same walk with every class limit lowered, so karate and the directed graph reach
    the LDS and stream classes and the peel's tail on the reused context too."""
    for name in C.SEQUENCE:
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        eng = put(ctx, name)
        plain = eng.trussness()[1] if C.symmetric(name) else None
        for k, v in KNOBS.items():
            monkeypatch.setenv(k, v)
        fam_topology(eng, name)
        if C.symmetric(name) and eng.nnz:
            _knobs_took_effect(eng, name, plain, monkeypatch)
        n, ei = C.graph(name)
        s = np.array(C.scores(name))
        rank, _, info = eng.segment_rank(s, np.array(ei[0]), n)
        assert np.array_equal(rank, C.ref(name, "segment_rank")), name
        if name in ("G1", "G3"):
            assert info["classes"]["stream"] > 0 and info["classes"]["lds"] > 0, info
        local, _ = eng.local_scores(s, np.array(ei[0]), np.array(ei[1]), n)
        assert bits_equal(local, C.ref(name, "local")), name


def _knobs_took_effect(eng, name, plain, monkeypatch):
    """The Simmelian pair classes are the ones the lowered limits give (pairs u < v by the
    shorter of the two neighbour lists, as test_gpu_simmelian.py counts them), and the peel's
    tail is the one GSPARSE_TRUSS_TAIL=16 asks for: fewer host waits than without a tail
    (one per level and sub-round, plus the edge count), no fewer than with the default tail."""
    ip, ix, _ = C.csr(name)
    rows, deg = C.rows_of(name), np.diff(ip)
    up = rows < ix
    shorter = np.minimum(deg[rows[up]], deg[ix[up]])
    w, m, l = (int(KNOBS[f"GSPARSE_SIM_{k}_MAX"]) for k in ("WAVE", "MID", "LDS"))
    cls = np.where(shorter <= w, 0, np.where(shorter <= m, 1, np.where(shorter <= l, 2, 3)))
    want = dict(zip(eng.SIM_CLASSES, np.bincount(cls, minlength=4).tolist()))
    got = eng.simmelian(0)[1]["classes"]
    assert got == want, (name, got, want)
    assert want["lds"] > 0 and want["stream"] > 0, (name, want)  # karate reaches them too
    tail = eng.trussness()[1]
    monkeypatch.setenv("GSPARSE_TRUSS_TAIL", "0")
    none = eng.trussness()[1]
    monkeypatch.setenv("GSPARSE_TRUSS_TAIL", KNOBS["GSPARSE_TRUSS_TAIL"])
    print(name, "host waits: default tail", plain["host_waits"], "tail 16", tail["host_waits"],
          "no tail", none["host_waits"])
    assert none["host_waits"] == 1 + none["levels"] + none["rounds"], (name, none)
    assert plain["host_waits"] <= tail["host_waits"] <= none["host_waits"], (name, plain, tail, none)
    if name in ("G1", "G3"):  # 113 sub-rounds, most of them with a few edges: the tail takes some
        assert tail["host_waits"] < none["host_waits"], (name, tail, none)


def test_interleaved_families(ctx):
    """A different family after every graph change: scratch[0..5] and the named buffers pass
    between subsystems at other sizes than the one that grew them."""
    order = ("topology", "scorers", "columns", "approx_er", "exact", "topology")
    for shift in (0, 2):
        for i, name in enumerate(C.SEQUENCE):
            visit(ctx, order[(i + shift) % len(order)], name)


def test_module_level_contexts():
    """metrics.py, metric_backbone.py and random.py each keep one context for the process;
    every call below sets a new graph on it."""
    import gsparse as gs
    from gsparse import random as R
    from gsparse import selection as S

    for name in C.SEQUENCE:
        ip, ix, d = C.csr(name)
        n, ei = C.graph(name)
        E = ei.shape[1]
        adj = sp.csr_matrix((d, ix, ip), shape=(n, n))
        assert bits_equal(gs.calculate_jaccard_scores(adj), C.ref(name, "jaccard")), name
        if C.symmetric(name):
            assert np.array_equal(gs.calculate_trussness_scores(adj), C.ref(name, "trussness")), name
            assert bits_equal(gs.calculate_simmelian_scores(adj), C.ref(name, "simmelian")), name
        else:
            with pytest.raises(NotImplementedError):
                gs.calculate_trussness_scores(adj)
            with pytest.raises(NotImplementedError):
                gs.calculate_simmelian_scores(adj)
        es = (np.arange(len(ix)) * 7 % 11) / 4.0  # one score per entry, ties
        want = S.local_filter_scores(es, np.stack([C.rows_of(name), ix.astype(np.int64)]), n)[0]
        assert bits_equal(gs.calculate_local_filter_scores(adj, es), want), name
        if E == 0:
            continue
        data = gs.Data(edge_index=torch.from_numpy(np.array(ei)), num_nodes=n)
        _, st = gs.compute_metric_backbone(data, 1.0 + np.array(C.scores(name)), verbose=False)
        assert np.array_equal(st["keep_mask"], C.ref(name, "backbone")), name
        us, inv = gs.precompute_random_scores(data, seed=5)
        hus, hinv = R._host_precompute_random_scores(data, 5)
        assert bits_equal(us, hus) and np.array_equal(inv, hinv), name
        got = gs.random_sparsify(data, us, inv, 0.5, "cpu")
        want = R._host_random_sparsify(data, hus, hinv, 0.5, "cpu")
        assert torch.equal(got.edge_index, want.edge_index), name
