"""Spectral sparsification by effective-resistance sampling without a GPU: the
specification (gsparse.selection.spectral_sample) against NumPy's Generator.choice, its
invariants, the spectral quality it reaches on a dense graph, the C ABI's declarations
and the device kernels' per-element rules (csrc/gs_spectral.hpp), compiled for the host by
tools/spectral_host_check.cpp, against the specification."""

import os
import re
import subprocess

import numpy as np
import pytest

import spectral_cases as C
from conftest import ROOT, bits_equal


@pytest.fixture(scope="module")
def S():
    from gsparse import selection

    return selection


# ---- the specification against Generator.choice ---------------------------------------
def _choice_counts(p, q, seed):
    idx = np.random.default_rng(seed).choice(len(p), size=q, replace=True, p=p)
    return np.bincount(idx, minlength=len(p))


@pytest.mark.parametrize("seed", [0, 7, 42])
@pytest.mark.parametrize("m", [1, 2, 1000, 70000])
def test_multinomial_is_generator_choice(S, m, seed):
    ei, n = C.sym_graph(m, seed=m + seed)
    s = C.column_scores(ei.shape[1], seed)
    for kind in ("plain", "zeros") if m >= 1000 else ("plain",):
        sc = C.zero_ends(s, ei, n) if kind == "zeros" else s
        if kind == "zeros":  # and zeros in the middle
            sc = sc.copy()
            sc[C.pair_probs(s, ei, n)[1] == m // 2] = 0.0
        p, inv = C.pair_probs(sc, ei, n)
        if kind == "zeros":
            assert p[0] == 0 and p[-1] == 0 and p[m // 2] == 0
        for q in (max(1, m // 3), 20 * m + 5):  # below and far above m
            mask, w, cnt, inv2 = S.spectral_sample(sc, ei, n, q, seed=seed)
            assert np.array_equal(inv2, inv)
            assert np.array_equal(cnt, _choice_counts(p, q, seed)), (m, seed, q, kind)
            assert cnt.sum() == q and (cnt[p == 0] == 0).all()
            assert np.array_equal(mask, cnt[inv] > 0)


def test_single_hot_pair(S):
    ei, n = C.sym_graph(257, seed=3)
    _, inv = C.pair_probs(np.ones(ei.shape[1]), ei, n)
    s = np.full(ei.shape[1], 1e-300)
    s[inv == 100] = 1.0
    p, _ = C.pair_probs(s, ei, n)
    assert p[100] == 1.0
    mask, w, cnt, _ = S.spectral_sample(s, ei, n, 5000, seed=42)
    assert cnt[100] == 5000 and cnt.sum() == 5000
    assert np.array_equal(cnt, _choice_counts(p, 5000, 42))
    assert mask.sum() == 2 and (w[mask] == 1.0).all()


# ---- invariants -----------------------------------------------------------------------
@pytest.mark.parametrize("method", ["multinomial", "independent"])
def test_invariants(S, method):
    m, loops = 4000, 37
    ei, n = C.sym_graph(m, seed=11, loops=loops)
    E = ei.shape[1]
    s = C.column_scores(E, 5, kind="odd")
    q = 1500
    mask, w, cnt, inv = S.spectral_sample(s, ei, n, q, seed=7, method=method)
    assert mask.dtype == bool and w.dtype == np.float64 and cnt.dtype == np.int64
    assert mask.shape == w.shape == (E,) and inv.shape == (E,)
    mm = int(inv.max()) + 1
    assert cnt.shape == (mm,)
    if method == "multinomial":
        assert cnt.sum() == q and (cnt > 0).sum() <= q
    else:
        assert set(np.unique(cnt)) <= {0, 1}
    # loops, NaN, inf and scores <= 0 are never kept (the pair's first column decides)
    first = np.full(mm, E)
    np.minimum.at(first, inv, np.arange(E))
    r = s[first]
    dead = ~(np.isfinite(r) & (r > 0)) | (ei[0][first] == ei[1][first])
    assert dead.sum() > loops // 2 and (cnt[dead] == 0).all()
    assert not mask[ei[0] == ei[1]].any()
    # both columns of a pair carry the same mask and weight
    for arr in (mask, w):
        lo, hi = np.full(mm, np.inf), np.full(mm, -np.inf)
        np.minimum.at(lo, inv, arr.astype(np.float64))
        np.maximum.at(hi, inv, arr.astype(np.float64))
        assert np.array_equal(lo, hi)
    assert (w[mask] > 0).all() and (w[~mask] == 0).all()


def test_first_column_rule_on_shuffled_columns(S):
    """The two directions carry different scores: the lower column's is the pair's."""
    ei, n = C.sym_graph(1000, seed=2)
    E = ei.shape[1]
    s = C.column_scores(E, 9)
    p, inv = C.pair_probs(s, ei, n)
    # spelled out without ufunc.at: the first occurrence of each id in column order
    _, first = np.unique(inv, return_index=True)
    other = np.array([np.nonzero(inv == j)[0][-1] for j in range(0, 1000, 97)])
    assert (s[first[::97]] != s[other]).all()
    assert bits_equal(p, s[first] / np.sum(s[first]))
    for method in ("multinomial", "independent"):
        mask, w, cnt, _ = S.spectral_sample(s, ei, n, 800, seed=0, method=method)
        # swapping the scores of the two directions changes the draw
        s2 = s.copy()
        last = np.zeros(1000, dtype=np.int64)
        np.maximum.at(last, inv, np.arange(E))
        s2[first], s2[last] = s[last], s[first]
        mask2, w2, _, _ = S.spectral_sample(s2, ei, n, 800, seed=0, method=method)
        assert not np.array_equal(w, w2)
        # ... and scores on the higher column alone do not
        s3 = s.copy()
        s3[last] = 123.0
        mask3, w3, cnt3, _ = S.spectral_sample(s3, ei, n, 800, seed=0, method=method)
        assert np.array_equal(mask, mask3) and bits_equal(w, w3) and np.array_equal(cnt, cnt3)


def test_weights_are_count_over_q_p(S):
    ei, n = C.sym_graph(300, seed=4)
    s = C.column_scores(ei.shape[1], 4)
    p, inv = C.pair_probs(s, ei, n)
    q = 2000  # q p at and above 1 for some pairs
    assert (q * p >= 1).any() and (q * p < 1).any()
    _, w, cnt, _ = S.spectral_sample(s, ei, n, q, seed=1)
    k = cnt > 0
    want = np.zeros(300)
    want[k] = cnt[k] / (q * p[k])
    assert bits_equal(w, want[inv])
    _, w, cnt, _ = S.spectral_sample(s, ei, n, q, seed=1, method="independent")
    pk = np.minimum(1.0, q * p)
    u = np.random.default_rng(1).random(300)
    assert np.array_equal(cnt, (u < pk).astype(np.int64))
    assert (cnt[pk == 1.0] == 1).all()
    want = np.where(cnt > 0, 1.0 / pk, 0.0)
    assert bits_equal(w, want[inv])


# ---- the quality the specification reaches --------------------------------------------
@pytest.fixture(scope="module")
def dense():
    ei, n = C.dense96()
    assert ei.shape[1] == 2 * 2323
    return ei, n, C.exact_er(ei, n), C.laplacian(ei, n)


def test_quality_multinomial(S, dense):
    """q = m draws, seed 42: measured eigenvalue range [0.599, 1.465], 1476 pairs kept."""
    ei, n, er, L = dense
    m = ei.shape[1] // 2
    mask, w, cnt, _ = S.spectral_sample(er, ei, n, m, seed=42)
    lam = C.whitened_eigs(L, C.laplacian(ei[:, mask], n, w[mask]))
    kept = int((cnt > 0).sum())
    print("multinomial", lam[0], lam[-1], kept)
    assert len(lam) == n - 1 and 0.5 < lam[0] and lam[-1] < 1.6
    assert kept <= 1500 and mask.sum() == 2 * kept


def test_quality_independent(S, dense):
    """q = m // 2, seed 42: measured eigenvalue range [0.632, 1.535], 1193 pairs kept."""
    ei, n, er, L = dense
    m = ei.shape[1] // 2
    mask, w, cnt, _ = S.spectral_sample(er, ei, n, m // 2, seed=42, method="independent")
    lam = C.whitened_eigs(L, C.laplacian(ei[:, mask], n, w[mask]))
    print("independent", lam[0], lam[-1], int(cnt.sum()))
    assert len(lam) == n - 1 and 0.5 < lam[0] and lam[-1] < 1.6


# ---- declarations and errors ----------------------------------------------------------
def test_header_declares_the_entry_point():
    text = open(os.path.join(ROOT, "include", "gsparse.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", text))
    assert "gs_spectral_sample" in names
    from gsparse import _lib

    assert "gs_spectral_sample" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["gs_spectral_sample"][1]) == 29
    assert int(re.search(r"GS_API_VERSION\s+(\d+)", text).group(1)) == 3


def test_reexports():
    import gsparse
    from src.sparsification import GraphSparsifier

    assert gsparse.spectral_sample is gsparse.selection.spectral_sample
    assert "spectral_sample" in gsparse.__all__
    assert callable(GraphSparsifier.sparsify_spectral)


def test_errors(S):
    ei, n = C.sym_graph(20, seed=1)
    s = C.column_scores(ei.shape[1], 1)
    with pytest.raises(ValueError):
        S.spectral_sample(np.zeros_like(s), ei, n, 10)  # an all-zero total
    with pytest.raises(ValueError):
        S.spectral_sample(np.full_like(s, np.nan), ei, n, 10)
    for q in (0, -1, 2**31):
        with pytest.raises(ValueError):
            S.spectral_sample(s, ei, n, q)
    with pytest.raises(ValueError):
        S.spectral_sample(s, ei, n, 10, method="poisson")
    with pytest.raises(ValueError):
        S.spectral_sample(s[:-1], ei, n, 10)  # fewer scores than columns
    # sparsify_spectral's draw count: exactly one of the two forms
    with pytest.raises(ValueError):
        S.spectral_num_samples(None, None)
    with pytest.raises(ValueError):
        S.spectral_num_samples(5, 0.5)
    for r in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            S.spectral_num_samples(None, r, 100)
    assert S.spectral_num_samples(7, None, 100) == 7
    assert S.spectral_num_samples(None, 0.25, 100) == 25
    assert S.spectral_num_samples(None, 1e-9, 100) == 1
    from gsparse import GraphSparsifier

    for kw in ({}, {"num_samples": 5, "retention_ratio": 0.5}, {"num_samples": 5, "method": "poisson"}):
        with pytest.raises(ValueError):  # checked before anything of the instance is used
            GraphSparsifier.sparsify_spectral(None, "approx_er", **kw)


# ---- the device logic compiled for the host -------------------------------------------
@pytest.fixture(scope="module")
def spectral_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("spc")
    exe = str(d / "spectral_check")
    src = os.path.join(ROOT, "tools", "spectral_host_check.cpp")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O2", src, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("hipcc host build unavailable: " + r.stderr[-300:])

    def run(scores, ei, n, q, seed, method):
        from gsparse.engine import Engine

        E = ei.shape[1]
        words = Engine._pcg64_words(np.random.default_rng(seed))
        path = str(d / "case.bin")
        with open(path, "wb") as f:
            np.array([n, E, q, {"multinomial": 0, "independent": 1}[method]], dtype=np.int64).tofile(f)
            np.array(words, dtype=np.uint64).tofile(f)
            np.ascontiguousarray(scores, dtype=np.float64).tofile(f)
            np.ascontiguousarray(ei[0], dtype=np.int64).tofile(f)
            np.ascontiguousarray(ei[1], dtype=np.int64).tofile(f)
        out = subprocess.run([exe, path], capture_output=True, check=True).stdout
        if int(np.frombuffer(out[:8], dtype=np.int64)[0]) != 0:
            assert len(out) == 8
            return None
        st, m, irr, kept, mx = np.frombuffer(out[:40], dtype=np.int64).tolist()
        o = 40
        mask = np.frombuffer(out[o:o + E], dtype=np.uint8).astype(bool)
        w = np.frombuffer(out[o + E:o + 9 * E], dtype=np.float64)
        cnt = np.frombuffer(out[o + 9 * E:o + 9 * E + 8 * m], dtype=np.int64)
        inv = np.frombuffer(out[o + 9 * E + 8 * m:], dtype=np.int64)
        assert len(inv) == E
        return {"m": m, "n_irregular": irr, "kept": kept, "max_count": mx,
                "mask": mask, "weight": w, "counts": cnt, "inverse": inv}

    return run


def _same_as_spec(S, got, scores, ei, n, q, seed, method):
    mask, w, cnt, inv = S.spectral_sample(scores, ei, n, q, seed=seed, method=method)
    assert got is not None
    assert got["m"] == len(cnt) and np.array_equal(got["inverse"], inv)
    assert np.array_equal(got["counts"], cnt)
    assert np.array_equal(got["mask"], mask) and bits_equal(got["weight"], w)
    assert got["kept"] == (cnt > 0).sum() and got["max_count"] == cnt.max()


@pytest.mark.parametrize("method", ["multinomial", "independent"])
def test_host_program_multigraphs(S, spectral_check, method):
    for E, n in ((1, 1), (2, 2), (65, 9), (257, 40), (4097, 1000), (20011, 3000)):
        ei = C.multigraph(E, n, seed=E)
        if (ei[0] == ei[1]).all():  # a positive total needs a pair that is no loop
            continue
        for kind in ("plain", "odd"):
            s = C.column_scores(E, E, kind=kind)
            s[np.nonzero(ei[0] != ei[1])[0][0]] = 0.5
            for q in (1, 9, 3 * E):
                got = spectral_check(s, ei, n, q, 42, method)
                _same_as_spec(S, got, s, ei, n, q, 42, method)
                assert got["n_irregular"] == C.np_irregular(ei, n)


@pytest.mark.parametrize("m", [1, 2, 2047, 2048, 2049, 8193, 70001])
def test_host_program_sizes_and_saturation(S, spectral_check, m):
    ei, n = C.sym_graph(m, seed=m, loops=3)
    s = C.column_scores(ei.shape[1], m, kind="zeros40")
    s = C.zero_ends(s, ei, n) if m > 16 else np.abs(s) + 0.1
    for method in ("multinomial", "independent"):
        for q, seed in ((7, 0), (5 * m, 42)):  # q p above 1 on many pairs with 5 m draws
            got = spectral_check(s, ei, n, q, seed, method)
            _same_as_spec(S, got, s, ei, n, q, seed, method)
            assert got["n_irregular"] == 0


def test_host_program_status_gate(spectral_check):
    ei, n = C.sym_graph(10, seed=1)
    s = C.column_scores(ei.shape[1], 1)
    assert spectral_check(s, ei, n, 5, 42, "multinomial") is not None
    assert spectral_check(s, ei, n, 0, 42, "multinomial") is None  # q = 0
    assert spectral_check(s, ei, n, 2**31, 42, "independent") is None
    assert spectral_check(np.zeros_like(s), ei, n, 5, 42, "multinomial") is None  # total 0
    assert spectral_check(np.full_like(s, np.inf), ei, n, 5, 42, "multinomial") is None
    bad = ei.copy()
    bad[0, 3] = n
    assert spectral_check(s, bad, n, 5, 42, "multinomial") is None  # an id equal to n
    loops = np.stack([np.arange(5), np.arange(5)])
    assert spectral_check(np.ones(5), loops, 5, 5, 42, "multinomial") is None  # loops only
