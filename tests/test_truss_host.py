"""The NumPy specification of the trussness (selection.trussness_host) against NetworkX's
repeated k_truss and the known answers of the small cases; the metric names and the
k-truss selection's argument checks.  No GPU."""

import numpy as np
import pytest

import truss_cases as C


@pytest.mark.parametrize("name", C.NAMES)
def test_specification_equals_networkx(name):
    t, levels, rounds = C.expected(name)
    assert t.dtype == np.int64 and t.shape == C.csr(name)[1].shape
    assert np.array_equal(t, C.networkx_trussness(name))
    vals = np.unique(t[t > 0])
    assert levels == len(vals) and rounds >= levels
    assert (t[t > 0] >= 2).all()


@pytest.mark.parametrize("name", sorted(C.KNOWN))
def test_known_counts_levels_and_rounds(name):
    entries, counts, levels, rounds = C.KNOWN[name]
    t, lv, rd = C.expected(name)
    if entries is not None:
        assert len(t) == entries
    if counts is not None:
        vals, cnt = np.unique(t, return_counts=True)
        assert dict(zip(vals.tolist(), cnt.tolist())) == counts
    assert (lv, rd) == (levels, rounds)
    if name == "rmat10":
        assert t.max() == 17


@pytest.mark.parametrize("name", C.NAMES)
def test_both_directions_agree_and_the_diagonal_is_zero(name):
    t, _, _ = C.expected(name)
    ip, ix = C.csr(name)
    assert np.array_equal(t, t[C.reverse_positions(name)])
    assert np.array_equal(t == 0, C.rows_of(name) == ix)


def test_loops_and_duplicates_change_nothing_off_the_diagonal():
    t0, lv0, rd0 = C.expected("cliques")
    t1, lv1, rd1 = C.expected("cliques_loops_dups")
    ip, ix = C.csr("cliques_loops_dups")
    off = C.rows_of("cliques_loops_dups") != ix
    assert len(t1) == len(t0) + 3 and int((~off).sum()) == 3
    assert np.array_equal(t1[off], t0) and (t1[~off] == 0).all()
    assert (lv1, rd1) == (lv0, rd0) == (4, 4)


def test_specification_rejects_a_directed_pattern():
    from gsparse.selection import trussness_host

    with pytest.raises(ValueError):
        trussness_host(np.array([0, 1, 1]), np.array([1]))


def test_metric_names_and_cost_transform():
    from gsparse.core import GraphSparsifier

    s = GraphSparsifier.__new__(GraphSparsifier)
    for name in ("truss", "trussness", "Truss", "TRUSSNESS"):
        assert s._normalize_metric_name(name) == "trussness"
    assert {"truss", "trussness"} <= GraphSparsifier.SUPPORTED_METRICS
    assert "trussness" not in GraphSparsifier._DISTANCE_METRICS
    # a similarity: the largest trussness costs 0, as the largest Jaccard score does
    t = np.array([2.0, 4.0, 3.0, 0.0])
    assert np.array_equal(s._scores_to_cost(t, "truss"), s._scores_to_cost(t, "jaccard"))
    assert s._scores_to_cost(t, "truss")[1] == 0.0


@pytest.mark.parametrize("k", [1, 0, -3, 2.5, "3", None, True])
def test_sparsify_truss_rejects_a_bad_k_before_any_device_work(k):
    from gsparse.core import GraphSparsifier

    with pytest.raises(ValueError):
        GraphSparsifier.__new__(GraphSparsifier).sparsify_truss(k)


def test_the_library_declares_and_binds_gs_trussness():
    import os

    from conftest import ROOT
    from gsparse import _lib

    assert "gs_trussness" in _lib.SIGNATURES
    assert "gs_trussness(" in open(os.path.join(ROOT, "include", "gsparse.h")).read()
    import gsparse
    import src.sparsification as shim

    assert "calculate_trussness_scores" in gsparse.__all__
    assert "calculate_trussness_scores" in shim.__all__
