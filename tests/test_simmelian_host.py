"""The NumPy specification of the Simmelian backbone (selection.simmelian_host, the
candidate form) against the literal definition (selection.simmelian_bruteforce: sets,
Fractions), the known answers of the small cases, its invariance under relabelling, and
the argument checks of what is built on it.  No GPU."""

from collections import Counter
from fractions import Fraction

import numpy as np
import pytest

import simmelian_cases as C

SMALL = [n for n in C.NAMES if len(C.csr(n)[1]) <= C.BRUTE_MAX_ENTRIES]


def _fractions(name, max_rank=0):
    _, num, den = C.expected(name, max_rank)
    return [Fraction(int(a), int(b)) for a, b in zip(num, den)]


def _histogram(name):
    return dict(Counter(_fractions(name)))


def test_the_graded_hub_graphs_are_what_they_are_meant_to_be():
    for name, commons, mod in (("two_hubs_300", 300, 13), ("two_hubs_graded", 3000, 97),
                               ("two_hubs_9000", 9000, 13)):
        p = C.prepared(name)
        ip, ix = C.csr(name)
        assert ix[ip[0]] == 1 and p["t"][ip[0]] == commons  # the pair (a, b)
        ta = p["t"][ip[0] + 1:ip[0] + 1 + commons]  # t(a, w_i) = 1 + i mod `mod`
        assert np.array_equal(ta, 1 + np.arange(commons) % mod)
        assert (p["t"][ip[1] + 1:ip[2]] == 1).all()  # t(b, w_i) is constant
        m = p["m"][p["pid"] == 0]
        assert len(m) == commons and len(np.unique(m)) == mod
    assert len(C.csr("two_hubs_300")[1]) <= C.BRUTE_MAX_ENTRIES < len(C.csr("two_hubs_graded")[1])


@pytest.mark.parametrize("max_rank", [0, 1, 2, 5])
@pytest.mark.parametrize("name", SMALL)
def test_specification_equals_the_literal_definition(name, max_rank):
    from gsparse.selection import simmelian_bruteforce

    score, num, den = C.expected(name, max_rank)
    want = simmelian_bruteforce(*C.csr(name), max_rank=max_rank)
    assert _fractions(name, max_rank) == want
    assert score.dtype == np.float64 and np.array_equal(score, num / den)
    if max_rank:
        assert (den == 1).all()


@pytest.mark.parametrize("max_rank", [0, 1, 3])
def test_known_answers_zero_and_one(max_rank):
    for name in ("empty", "single_edge", "tree5"):
        assert not C.expected(name, max_rank)[1].any()
    for name, c in (("triangle", 3), ("K4", 4), ("K5", 5), ("K70", 70)):
        s, num, den = C.expected(name, max_rank)
        if max_rank == 0:
            assert (s == 1.0).all() and (num == den).all()
        else:  # every neighbour is tied at rank 0: the overlap is all c - 2 common ones
            assert (num == c - 2).all()


def test_known_answers_of_the_issue():
    F = Fraction
    cl = {F(0): 2, F(2, 11): 2, F(2, 7): 4, F(1, 3): 4, F(1, 2): 8, F(1): 54}
    assert len(C.csr("cliques")[1]) == 74 and _histogram("cliques") == cl
    assert _histogram("cliques_loops_dups") == {**cl, F(0): 2 + 3}
    k = _histogram("karate")
    assert sum(k.values()) == 156 and len(k) == 13 and k[F(0)] == 22 and k[F(1, 16)] == 2
    r = _histogram("rmat10")
    assert sum(r.values()) == 12104 and r[F(0)] == 1092 and len(r) == 223 and C.max_common("rmat10") == 135
    assert C.max_common("hub_pair") == 3000 and C.max_common("K70") == 68


def test_known_answers_hub_pair():
    ip, ix = C.csr("hub_pair")
    _, num, den = C.expected("hub_pair")
    assert ix[ip[0]] == 1 and (num[ip[0]], den[ip[0]]) == (3000, 3004)
    leaves = (ix[ip[0]:ip[1]] >= 2) & (ix[ip[0]:ip[1]] < 3002)
    assert leaves.sum() == 3000 and (C.expected("hub_pair")[0][ip[0]:ip[1]][leaves] == 1.0).all()
    assert (C.expected("hub_pair")[0][ip[1]:ip[2]][1:3001] == 1.0).all()  # the leaf edges of node 1


def test_known_answers_small_new_graphs():
    # K4 minus the edge (2, 3): every edge's ends agree on their one or two strongest ties
    assert (C.expected("K4_minus_edge")[0] == 1.0).all()
    # two triangles sharing node 2: the outer edges score 1; an edge at the shared node has
    # its one common neighbour in P_1 of both ends, next to the other triangle's two nodes
    s = C.expected("bowtie")[0]
    assert sorted(Counter(s.tolist()).items()) == [(1 / 3, 8), (1.0, 4)]


@pytest.mark.parametrize("name", [n for n in C.NAMES if n != "empty"])
def test_a_relabelling_permutes_the_scores(name):
    from gsparse.selection import simmelian_host

    ip2, ix2, pos = C.relabelled(name, seed=3)
    for k0 in (0, 2):
        _, num, den = C.expected(name, k0)
        _, num2, den2 = simmelian_host(ip2, ix2, max_rank=k0)
        # equal as rationals (which of two equal candidates is reported may differ)
        assert np.array_equal(num * den2[pos], num2[pos] * den)
        assert np.array_equal(C.expected(name, k0)[0], (num2 / den2)[pos])


@pytest.mark.parametrize("name", C.NAMES)
def test_both_directions_agree_and_the_diagonal_is_zero(name):
    ip, ix = C.csr(name)
    diag = C.rows_of(name) == ix
    for k0 in (0, 1, 5):
        s, num, den = C.expected(name, k0)
        assert np.array_equal(s, s[C.reverse_positions(name)])
        assert not s[diag].any() and (s >= 0).all()
        if k0 == 0:
            assert (s <= 1).all() and np.array_equal(num == 0, C.prepared(name)["t"] <= 0)


@pytest.mark.parametrize("name", C.NAMES)
def test_the_overlap_grows_with_the_rank_and_ends_at_the_common_neighbours(name):
    prev = np.zeros(len(C.csr(name)[1]), dtype=np.int64)
    for k0 in (1, 2, 3, 5, 8, 50):
        o = C.expected(name, k0)[1]
        assert (o >= prev).all()
        prev = o
    top = C.expected(name, max(C.max_degree(name), 1))[1]
    assert (top >= prev).all()
    assert np.array_equal(top, np.maximum(C.prepared(name)["t"], 0))


def test_specification_rejects_a_directed_pattern_and_a_negative_rank():
    from gsparse.selection import simmelian_bruteforce, simmelian_host

    with pytest.raises(ValueError):
        simmelian_host(np.array([0, 1, 1]), np.array([1]))
    for f in (simmelian_host, simmelian_bruteforce):
        with pytest.raises(ValueError):
            f(*C.csr("triangle"), max_rank=-1)


def test_metric_names_and_cost_transform():
    from gsparse.core import GraphSparsifier

    s = GraphSparsifier.__new__(GraphSparsifier)
    for name in ("simmelian", "Simmelian", "simmelian_jaccard", "simmelian-jaccard", "SIMMELIAN JACCARD"):
        assert s._normalize_metric_name(name) == "simmelian"
    assert {"simmelian", "simmelian_jaccard"} <= GraphSparsifier.SUPPORTED_METRICS
    assert "simmelian" not in GraphSparsifier._DISTANCE_METRICS
    v = np.array([0.25, 1.0, 0.5, 0.0])
    assert np.array_equal(s._scores_to_cost(v, "simmelian"), s._scores_to_cost(v, "jaccard"))
    assert s._scores_to_cost(v, "simmelian")[1] == 0.0


@pytest.mark.parametrize("kwargs", [
    {}, {"retention_ratio": 0.5, "threshold": 0.5}, {"retention_ratio": 0.5, "max_rank": 2, "min_overlap": 1},
    {"threshold": 0.5, "max_rank": 2, "min_overlap": 1}, {"max_rank": 2}, {"min_overlap": 2},
    {"max_rank": 0, "min_overlap": 1}, {"max_rank": 2, "min_overlap": 0}, {"max_rank": 2.5, "min_overlap": 1},
    {"max_rank": True, "min_overlap": 1}, {"retention_ratio": 0.0}, {"retention_ratio": 1.5},
    {"threshold": "high"}, {"threshold": float("nan")},
])
def test_sparsify_simmelian_rejects_bad_arguments_before_any_device_work(kwargs):
    from gsparse.core import GraphSparsifier

    with pytest.raises(ValueError):
        GraphSparsifier.__new__(GraphSparsifier).sparsify_simmelian(**kwargs)


@pytest.mark.parametrize("k", [0, -1, 1.5, "2", None, True])
def test_simmelian_overlap_rejects_a_bad_rank(k):
    from gsparse.core import GraphSparsifier

    with pytest.raises(ValueError):
        GraphSparsifier.__new__(GraphSparsifier).simmelian_overlap(k)


def test_the_library_declares_and_binds_gs_simmelian():
    import os
    import re

    from conftest import ROOT
    from gsparse import _lib

    header = open(os.path.join(ROOT, "include", "gsparse.h")).read()
    assert "gs_simmelian" in _lib.SIGNATURES and "gs_simmelian(" in header
    assert re.search(r"#define GS_API_VERSION 3\b", header)  # the change is additive
    import gsparse
    import src.sparsification as shim

    assert "calculate_simmelian_scores" in gsparse.__all__
    assert "calculate_simmelian_scores" in shim.__all__
