"""The connectivity-preserving top-k without a GPU: the host restatement
(selection.connected_mask: union-find Kruskal over np.lexsort) against SciPy, and the
device kernels' per-element rules (csrc/gs_forest.hpp), compiled for the host by
tools/forest_host_check.cpp, against NumPy's order and the host restatement."""

import math
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import minimum_spanning_tree

import forest_cases as C
from conftest import ROOT, load_golden


def _graph(name):
    if name.startswith("gen:"):
        ei, n, s = C.generated(name[4:])
    else:
        ei, n, s = C.golden(name)
    return ei, n, s


GRAPHS = list(C.GOLDENS) + ["gen:rmat10", "gen:roman2000"]


@pytest.mark.parametrize("name", GRAPHS)
def test_connected_mask_properties(name):
    from gsparse import selection as S

    ei, n, s = _graph(name)
    E = ei.shape[1]
    src, dst = ei[0], ei[1]
    c, lab = C.components(src, dst, n)
    for keep_lowest in (False, True):
        forest, _ = S.spanning_forest_host(s, src, dst, n, keep_lowest)
        assert int(forest.sum()) == n - c
        assert not (src[forest] == dst[forest]).any()
        g = S.guaranteed_columns(forest, src, dst, n)
        for r in C.RATES:
            mask = S.connected_mask(s, ei, n, E, r, keep_lowest)
            assert mask.dtype == bool and mask.shape == (E,)
            kc, klab = C.components(src, dst, n, mask)
            assert kc == c and np.array_equal(klab, lab), (name, r)
            assert int(mask.sum()) == max(int(E * r), int(g.sum())), (name, r)
            assert (mask >= g).all()
            # every column that is the reverse of a forest column is kept
            fwd, rev = src * n + dst, dst * n + src
            assert mask[np.isin(fwd, rev[forest])].all()


def test_issue_table_on_the_roman_like_graph():
    """Plain stable top-k breaks the connected graph into 427 / 1059 / 1540 pieces."""
    from gsparse import selection as S

    ei, n, s = C.generated("roman2000")
    E = ei.shape[1]
    assert C.components(ei[0], ei[1], n)[0] == 1
    order = np.lexsort((np.arange(E), s))
    for r, pieces in zip(C.RATES, (427, 1059, 1540)):
        plain = np.zeros(E, dtype=bool)
        plain[order[E - int(E * r):]] = True
        assert C.components(ei[0], ei[1], n, plain)[0] == pieces
        assert C.components(ei[0], ei[1], n, S.connected_mask(s, ei, n, E, r))[0] == 1


@pytest.mark.parametrize("name", ["karate_test", "gen:rmat10", "gen:roman2000"])
def test_forest_is_scipys_spanning_tree_for_distinct_scores(name):
    from gsparse import selection as S

    ei, n, _ = _graph(name)
    src, dst = ei[0], ei[1]
    lo, hi = np.minimum(src, dst), np.maximum(src, dst)
    pair = lo * (n + 1) + hi
    _, inv = np.unique(pair, return_inverse=True)
    inv = inv.reshape(-1)
    w = np.random.default_rng(3).permutation(inv.max() + 1).astype(np.float64) + 1.0
    s = w[inv]  # distinct per unordered pair, equal in both directions
    nl = src != dst
    a = sp.coo_matrix((-s[nl], (lo[nl], hi[nl])), shape=(n, n)).tocsr()
    a.sum_duplicates()  # both directions fall on (lo, hi): halve back
    cnt = sp.coo_matrix((np.ones(int(nl.sum())), (lo[nl], hi[nl])), shape=(n, n)).tocsr()
    a.data /= cnt.data
    t = minimum_spanning_tree(a).tocoo()
    want = set(zip(t.row.tolist(), t.col.tolist()))
    forest, _ = S.spanning_forest_host(s, src, dst, n)
    got = set(zip(lo[forest].tolist(), hi[forest].tolist()))
    assert got == want


def test_fewer_scores_than_columns_is_an_error():
    from gsparse import selection as S

    g = load_golden("directed_dup")
    ei, n = g["edge_index"], int(g["num_nodes"])
    assert len(g["scores_jaccard"]) < ei.shape[1]
    with pytest.raises(ValueError):
        S.connected_mask(g["scores_jaccard"], ei, n, ei.shape[1], 0.5)


def test_header_declares_the_entry_point():
    text = open(os.path.join(ROOT, "include", "gsparse.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "gs_spanning_forest" in set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", text))
    from gsparse import _lib

    assert "gs_spanning_forest" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["gs_spanning_forest"][1]) == 18
    assert int(re.search(r"GS_API_VERSION\s+(\d+)", text).group(1)) == 3


# ---- the device rules compiled for the host ------------------------------------------
def _build(tmp, flags):
    exe = str(tmp / ("forest_check" + ("_san" if flags else "")))
    src = os.path.join(ROOT, "tools", "forest_host_check.cpp")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O2", *flags, src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _run(exe, tmp, n, ei, s, keep_lowest):
    E = ei.shape[1]
    path = str(tmp / "case.bin")
    with open(path, "wb") as f:
        np.array([n, E, int(keep_lowest)], dtype=np.int64).tofile(f)
        np.ascontiguousarray(s, dtype=np.float64).tofile(f)
        np.ascontiguousarray(ei[0], dtype=np.int64).tofile(f)
        np.ascontiguousarray(ei[1], dtype=np.int64).tofile(f)
    out = subprocess.run([exe, path], capture_output=True, check=True).stdout
    status = int(np.frombuffer(out[:8], dtype=np.int64)[0])
    if status:
        assert len(out) == 8
        return status, None
    order = np.frombuffer(out[8:8 + 8 * E], dtype=np.int64)
    off = 8 + 8 * E
    n_forest, rounds, n_disagree = (int(x) for x in np.frombuffer(out[off:off + 24], dtype=np.int64))
    forest = np.frombuffer(out[off + 24:off + 24 + E], dtype=np.uint8).astype(bool)
    labels = np.frombuffer(out[off + 24 + E:], dtype=np.int64)
    assert len(labels) == n
    return 0, dict(order=order, n_forest=n_forest, rounds=rounds, n_disagree=n_disagree,
                   forest=forest, labels=labels)


@pytest.fixture(scope="module")
def forest_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("forest")
    exe = _build(d, [])
    return lambda n, ei, s, kl: _run(exe, d, n, ei, s, kl)


def _check_case(run, name, keep_lowest):
    n, ei, s = C.SMALL[name]
    E = ei.shape[1]
    status, got = run(n, ei, s, keep_lowest)
    assert status == 0
    asc = np.lexsort((np.arange(E), s))
    assert np.array_equal(got["order"], asc if keep_lowest else asc[::-1]), name
    assert got["n_disagree"] == 0
    forest, _, c, lab = C.kruskal(name, keep_lowest)
    assert np.array_equal(got["forest"], forest), name
    assert got["n_forest"] == n - c
    assert np.array_equal(C.partition(got["labels"]), lab)
    assert got["rounds"] <= (math.ceil(math.log2(n)) if n > 1 else 0)


@pytest.mark.parametrize("keep_lowest", [False, True], ids=["top", "lowest"])
@pytest.mark.parametrize("name", sorted(C.SMALL))
def test_host_program_matches_numpy_and_kruskal(forest_check, name, keep_lowest):
    _check_case(forest_check, name, keep_lowest)


def test_host_program_rounds_on_paths(forest_check):
    n, ei, s = C.SMALL["path_ruler"]
    assert forest_check(n, ei, s, False)[1]["rounds"] == 12
    n, ei, s = C.SMALL["path_alternating"]
    assert forest_check(n, ei, s, False)[1]["rounds"] == 2
    n, ei, s = C.SMALL["path_ascending"]
    assert forest_check(n, ei, s, False)[1]["rounds"] == 1


def test_host_program_status_gate(forest_check):
    s3 = np.ones(3)
    assert forest_check(4, np.array([[0, 4, 1], [1, 2, 3]]), s3, False)[0] == 1  # an id equal to n
    assert forest_check(4, np.array([[0, 1, 1], [1, -1, 3]]), s3, False)[0] == 1  # a negative id
    assert forest_check(0, np.zeros((2, 0), dtype=np.int64), np.zeros(0), False)[0] == 1  # n < 1
    assert forest_check(4, np.array([[0, 1, 1], [1, 2, 3]]), s3, False)[0] == 0


def test_host_program_under_sanitizers(tmp_path):
    """The stand-alone program built with ASan + UBSan (host code only), on the cases
    with odd scores and odd shapes."""
    exe = _build(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    for name in ("special_values", "duplicates", "loops_only", "one_node", "empty", "multigraph_65",
                 "triangle_equal"):
        for keep_lowest in (False, True):
            _check_case(lambda n, ei, s, kl: _run(exe, tmp_path, n, ei, s, kl), name, keep_lowest)
