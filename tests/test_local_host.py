"""The NumPy specification of local sparsification (selection.local_filter_scores,
selection.local_mask) on the CPU: against the definition read literally in Python loops,
against the known counts of kept columns, and its structural properties."""

import numpy as np
import pytest

import local_cases as C

EXPONENTS = (0, 0.3, 0.5, 0.7, 1)

# scores deg[src] + deg[dst] (heavy ties): columns with local >= 1 - e at the exponents above
KNOWN_DEGSUM = {
    "karate": (64, 66, 92, 112, 156),
    "rmat10": (1612, 2242, 4184, 7316, 12104),
    "hub_pair": (6014, 6032, 6126, 6560, 12026),
    "lattice24": (1152, 1152, 2290, 3094, 3266),
    "cliques_loops_dups": (32, 32, 47, 61, 79),
    "K70": (140, 420, 1120, 2660, 4830),
}
# scores (7919 i) % 101: (graph, keep_lowest) -> (kept at e = 0.5, n_top)
KNOWN_MOD101 = {
    ("karate", False): (100, 62),
    ("karate", True): (96, 66),
    ("rmat10", False): (4030, 1576),
    ("rmat10", True): (4034, 1570),
}


def _mask(name, kind, e, keep_lowest=False):
    from gsparse.selection import local_mask

    return local_mask(C.expected(name, kind, keep_lowest)[0], e)


@pytest.mark.parametrize("keep_lowest", [False, True], ids=["highest", "lowest"])
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("name", ["karate", "cliques_loops_dups", "isolated", "borders", "tree5",
                                  "rmat10", "empty"])
def test_specification_equals_the_definition_in_loops(name, kind, keep_lowest):
    n, ei = C.CASES[name]
    local, rank, info = C.expected(name, kind, keep_lowest)
    blocal, brank = C.brute_force(C.scores(name, kind), ei, n, keep_lowest)
    assert rank.dtype == np.int64 and np.array_equal(rank, brank)
    assert local.dtype == np.float64 and local.tobytes() == blocal.tobytes()
    deg = np.bincount(ei[0], minlength=n)
    assert info == {"max_degree": int(deg.max()) if ei.shape[1] else 0,
                    "n_top": int((local == 1.0).sum())}
    # every node's ranks are 0 .. d - 1, each once
    order = np.lexsort((rank, ei[0]))
    off = np.concatenate([[0], np.cumsum(deg)])
    assert np.array_equal(rank[order], np.arange(ei.shape[1]) - off[ei[0][order]])


@pytest.mark.parametrize("name", sorted(KNOWN_DEGSUM))
def test_known_counts_with_heavy_ties(name):
    got = tuple(int(_mask(name, "degsum", e).sum()) for e in EXPONENTS)
    assert got == KNOWN_DEGSUM[name]


@pytest.mark.parametrize("name,keep_lowest", sorted(KNOWN_MOD101))
def test_known_counts_mod101(name, keep_lowest):
    info = C.expected(name, "mod101", keep_lowest)[2]
    assert (int(_mask(name, "mod101", 0.5, keep_lowest).sum()), info["n_top"]) == \
        KNOWN_MOD101[(name, keep_lowest)]


@pytest.mark.parametrize("keep_lowest", [False, True], ids=["highest", "lowest"])
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("name", C.SMALL + ("borders", "isolated", "wheel"))
def test_properties(name, kind, keep_lowest):
    n, ei = C.CASES[name]
    E = ei.shape[1]
    local = C.expected(name, kind, keep_lowest)[0]
    assert ((local >= 0) & (local <= 1)).all()
    keys = np.minimum(ei[0], ei[1]) * (n + 1) + np.maximum(ei[0], ei[1])
    inv = np.unique(keys, return_inverse=True)[1].reshape(-1)
    prev = np.zeros(E, dtype=bool)
    for e in EXPONENTS:
        m = _mask(name, kind, e, keep_lowest)
        per_pair = np.zeros(inv.max() + 1, dtype=np.int64)
        np.add.at(per_pair, inv, m)
        assert np.array_equal(m, per_pair[inv] > 0) and np.array_equal(m, per_pair[inv] == np.bincount(inv)[inv])
        assert not (prev & ~m).any()  # nested as e grows
        prev = m
        if e == 0:  # every node with a column keeps one
            touched = np.zeros(n, dtype=bool)
            touched[ei[0][m]] = True
            assert np.array_equal(touched, np.bincount(ei[0], minlength=n) > 0)
    assert prev.all()  # e = 1 keeps everything


@pytest.mark.parametrize("name", ["karate", "rmat10", "cliques_loops_dups", "borders"])
def test_mask_is_invariant_under_a_column_permutation(name):
    from gsparse.selection import local_filter_scores, local_mask

    n, ei = C.CASES[name]
    s = C.scores(name, "distinct")
    local = C.expected(name, "distinct")[0]
    _, sei, p = C.shuffled(name)
    slocal, _, _ = local_filter_scores(s[p], sei, n)
    assert slocal.tobytes() == local[p].tobytes()
    for e in EXPONENTS:
        assert np.array_equal(local_mask(slocal, e), local_mask(local, e)[p])


def test_errors_and_empty():
    from gsparse.selection import local_filter_scores, local_mask

    n, ei = C.CASES["karate"]
    with pytest.raises(ValueError, match="merged duplicate columns"):
        local_filter_scores(np.zeros(ei.shape[1] - 1), ei, n)
    for bad in (-1, n):
        e2 = np.array(ei)
        e2[1, 3] = bad
        with pytest.raises(ValueError, match="out of range"):
            local_filter_scores(np.zeros(ei.shape[1]), e2, n)
    local, rank, info = local_filter_scores(np.zeros(0), np.zeros((2, 0), dtype=np.int64), 4)
    assert local.shape == rank.shape == (0,) and info == {"max_degree": 0, "n_top": 0}
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            local_mask(local, bad)
