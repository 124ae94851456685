"""The spectral bounds of a sparsifier without a GPU: the NumPy specification
(gsparse.metrics.spectral_bounds_dense) against closed forms and against the helper of the
sampler's quality checks, the C ABI's declarations, the host-side errors of
compute_spectral_approximation, and the tridiagonal routines of csrc/gs_tridiag.hpp,
compiled for the host by tools/ritz_host_check.cpp, against numpy.linalg.eigvalsh."""

import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import spectral_bounds_cases as B
import spectral_cases as C
from conftest import ROOT


@pytest.fixture(scope="module")
def M():
    from gsparse import metrics

    return metrics


def close(got, want, rtol=1e-9):
    print(f"got {got!r} want {want!r}")
    assert abs(got[0] - want[0]) <= rtol * want[1]
    assert abs(got[1] - want[1]) <= rtol * want[1]


# ---- the specification against closed forms --------------------------------------------
@pytest.mark.parametrize("n", [3, 64, 1025])
def test_dense_cycle_and_path(M, n):
    G, H, want = B.cycle_and_path(n)
    close(M.spectral_bounds_dense(G, H), want)


def test_dense_k64_and_star(M):
    G, H, want = B.k64_and_star()
    close(M.spectral_bounds_dense(G, H), want)


@pytest.mark.parametrize("n,seed", [(2, 0), (50, 1), (301, 2)])
def test_dense_tree_reweighted(M, n, seed):
    G, H, want = B.random_tree(n, seed)
    close(M.spectral_bounds_dense(G, H), want)
    G, H, want = B.star_alternating(40)
    close(M.spectral_bounds_dense(G, H), want)


def test_dense_scaled_copy(M):
    G = B.rmat10()
    close(M.spectral_bounds_dense(G, 0.37 * G), (0.37, 0.37))
    # dense arrays and stored diagonal entries: the diagonal is no part of either Laplacian
    A = G[:200][:, :200].toarray()
    A = A + np.diag(np.arange(200.0))
    lo, hi = M.spectral_bounds_dense(A, 0.37 * A)
    assert abs(lo - 0.37) <= 1e-9 and abs(hi - 0.37) <= 1e-9


def test_dense_bridge_dropped(M):
    G, H, want = B.two_cliques()
    close(M.spectral_bounds_dense(G, H), want)


# ---- the specification against the helper of the sampler's quality checks --------------
def test_dense_equals_whitened_eigs_on_dense96(M):
    ei, n, G, samples = B.dense96_pairs()
    L = C.laplacian(ei, n)
    for mask, w, H in samples:
        lam = C.whitened_eigs(L, C.laplacian(ei[:, mask], n, w[mask]))
        lo, hi = M.spectral_bounds_dense(G, H)
        print(lo, hi, lam[0], lam[-1])
        assert abs(lo - lam[0]) <= 1e-12 and abs(hi - lam[-1]) <= 1e-12


# ---- declarations ----------------------------------------------------------------------
def test_header_declares_the_entry_point():
    text = open(os.path.join(ROOT, "include", "gsparse.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", text))
    assert "gs_spectral_bounds" in names
    from gsparse import _lib

    assert "gs_spectral_bounds" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["gs_spectral_bounds"][1]) == 12
    assert int(re.search(r"GS_API_VERSION\s+(\d+)", text).group(1)) == 3


def test_reexports():
    import gsparse
    import src.sparsification as shim
    import src.sparsification.metrics as shim_metrics
    from gsparse.engine import Engine

    for name in ("compute_spectral_approximation", "spectral_bounds_dense"):
        assert getattr(gsparse, name) is getattr(gsparse.metrics, name)
        assert name in gsparse.__all__ and name in shim.__all__
        assert getattr(shim, name) is getattr(gsparse, name)
        assert getattr(shim_metrics, name) is getattr(gsparse, name)
    assert callable(gsparse.GraphSparsifier.spectral_approximation)
    assert callable(Engine.spectral_bounds)


# ---- errors that need no device --------------------------------------------------------
def test_errors_without_a_device(M):
    G, H, _ = B.cycle_and_path(8)
    with pytest.raises(ValueError, match="shape"):
        M.compute_spectral_approximation(G, B.path(9))
    chord = B.sym([0], [4], [1.0], 8)  # {0, 4} is no edge of the cycle
    with pytest.raises(ValueError, match="outside the support"):
        M.compute_spectral_approximation(G, H + chord)
    with pytest.raises(NotImplementedError):
        M.compute_spectral_approximation(G, -H)
    with pytest.raises(ValueError):
        M.spectral_bounds_dense(G, B.path(9))


# ---- the tridiagonal routines compiled for the host ------------------------------------
@pytest.fixture(scope="module")
def ritz_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("ritz")
    exe = str(d / "ritz_check")
    src = os.path.join(ROOT, "tools", "ritz_host_check.cpp")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O2", src, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("hipcc host build unavailable: " + r.stderr[-300:])

    def run(cases):
        path = str(d / "case.bin")
        with open(path, "wb") as f:
            np.array([len(cases)], dtype=np.int64).tofile(f)
            for a, b in cases:
                assert len(b) == len(a) - 1
                np.array([len(a)], dtype=np.int64).tofile(f)
                np.ascontiguousarray(a, dtype=np.float64).tofile(f)
                np.ascontiguousarray(b, dtype=np.float64).tofile(f)
        out = subprocess.run([exe, path], capture_output=True, check=True, text=True).stdout
        rows = np.array([[float(x) for x in line.split()] for line in out.splitlines()])
        assert rows.shape == (len(cases), 4)
        return rows

    return run


def _dense_tridiagonal(a, b):
    return np.diag(a) + np.diag(b, 1) + np.diag(b, -1)


def test_ritz_routines_against_eigvalsh(ritz_check):
    rng = np.random.default_rng(3)
    cases = []
    for m in (1, 2, 3, 64, 300):
        for _ in range(3):
            cases.append((rng.normal(size=m), np.abs(rng.normal(size=m - 1))))
    # a Lanczos-like one: positive spectrum, the smallest eigenvalue exactly 0
    cases.append((np.array([1.0, 2.0, 1.0]), np.array([1.0, 1.0])))
    # beta = 0 in the middle: two blocks, the extremes in different ones
    a = rng.normal(size=40)
    b = np.abs(rng.normal(size=39))
    b[17] = 0.0
    a[:18] += 10.0
    cases.append((a, b))
    rows = ritz_check(cases)
    for (a, b), (lo, hi, slo, shi) in zip(cases, rows):
        T = _dense_tridiagonal(a, b)
        lam, S = np.linalg.eigh(T)
        scale = max(abs(lam[0]), abs(lam[-1]))
        assert abs(lo - lam[0]) <= 1e-13 * scale + 1e-300, (len(a), lo, lam[0])
        assert abs(hi - lam[-1]) <= 1e-13 * scale + 1e-300, (len(a), hi, lam[-1])
        # the last components, where the extreme eigenvalues are simple and separated
        for got, k, other in ((slo, 0, 1), (shi, -1, -2)):
            if len(a) == 1:
                assert got == 1.0
            elif abs(lam[k] - lam[other]) > 1e-3 * scale:
                assert abs(got - abs(S[-1, k])) <= 1e-8 * max(abs(S[-1, k]), 1e-6), (len(a), got, S[-1, k])
    # the block case: the top eigenvalue lives in the first block, so its vector ends in 0
    assert rows[-1][3] == 0.0
