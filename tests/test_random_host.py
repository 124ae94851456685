"""The symmetric random baseline without a GPU: the host forms of gsparse.random (the
reference's own NumPy lines, the fallback of the device path) against the goldens, the
C ABI's declarations, and the device kernels' per-element logic (csrc/gs_random.hpp),
compiled for the host by tools/random_host_check.cpp, against NumPy."""

import os
import re
import subprocess

import numpy as np
import pytest
import torch

import random_cases as C
from conftest import ROOT, bits_equal, golden_names, load_golden


@pytest.fixture
def host_form(monkeypatch):
    monkeypatch.setenv("GSPARSE_RANDOM", "host")
    from gsparse import random as R

    return R


@pytest.mark.parametrize("name", golden_names())
def test_host_forms_match_golden(host_form, name):
    R = host_form
    g = load_golden(name)
    data = C.golden_data(g)
    us, inv = R.precompute_random_scores(data, seed=42)
    assert R.last_selection["path"] == "host"
    assert type(us) is np.ndarray and us.dtype == np.float64
    assert type(inv) is np.ndarray and inv.dtype == np.int64
    assert np.array_equal(inv, g["random_inverse"])
    assert bits_equal(us, g["random_undirected"])
    for r in (0.8, 0.5, 0.2):
        sd = R.random_sparsify(data, us, inv, r, "cpu")
        assert R.last_selection["path"] == "host"
        assert np.array_equal(sd.edge_index.numpy(), g[f"random_sparsify_{r}"]), (name, r)


def test_host_handle_sweeps_and_nests(host_form):
    R = host_form
    import gsparse

    assert gsparse.RandomBaseline is R.RandomBaseline
    g = load_golden("rmat10")
    data = C.golden_data(g)
    rb = gsparse.RandomBaseline(data, seed=42)
    assert rb.path == "host" and rb.n_undirected == len(g["random_undirected"])
    assert bits_equal(rb.undirected_scores, g["random_undirected"])
    assert np.array_equal(rb.inverse_idx, g["random_inverse"])
    rates = [0.8, 0.5, 0.2]
    for r, sd in zip(rates, rb.sweep(rates, "cpu")):
        assert np.array_equal(sd.edge_index.numpy(), g[f"random_sparsify_{r}"])
    masks = [rb.mask(r) for r in rates]
    assert rb.last_selection["path"] == "host"
    assert all(m.dtype == torch.bool and m.shape == (data.edge_index.size(1),) for m in masks)
    assert bool((masks[1] <= masks[0]).all()) and bool((masks[2] <= masks[1]).all())
    assert bool(rb.mask(1.0).all())
    other = gsparse.RandomBaseline(data, seed=7)
    assert not np.array_equal(other.undirected_scores, rb.undirected_scores)


def test_host_form_empty_graph_raises_like_numpy(host_form):
    from gsparse import Data

    data = Data(edge_index=torch.zeros((2, 0), dtype=torch.int64), num_nodes=4)
    with pytest.raises(ValueError):
        host_form.precompute_random_scores(data)


def test_shim_reexports_the_handle():
    import gsparse
    from src.sparsification import random as shim

    assert shim.RandomBaseline is gsparse.RandomBaseline
    assert "RandomBaseline" in gsparse.__all__


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "gsparse.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", text))
    assert {"gs_undirected_ids", "gs_random_mask"} <= names
    from gsparse import _lib

    assert {"gs_undirected_ids", "gs_random_mask"} <= set(_lib.SIGNATURES)
    assert int(re.search(r"GS_API_VERSION\s+(\d+)", text).group(1)) == 3


# ---- the device logic compiled for the host ----------------------------------------
@pytest.fixture(scope="module")
def random_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("rnd")
    exe = str(d / "random_check")
    src = os.path.join(ROOT, "tools", "random_host_check.cpp")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O2", src, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("hipcc host build unavailable: " + r.stderr[-300:])

    def run(n, src_ids, dst_ids, idx, keep):
        E = len(src_ids)
        path = str(d / "case.bin")
        with open(path, "wb") as f:
            np.array([n, E, len(keep)], dtype=np.int64).tofile(f)
            for a in (src_ids, dst_ids, idx):
                np.ascontiguousarray(a, dtype=np.int64).tofile(f)
            np.ascontiguousarray(keep, dtype=np.uint8).tofile(f)
        out = subprocess.run([exe, path], capture_output=True, check=True).stdout
        status = int(np.frombuffer(out[:8], dtype=np.int64)[0])
        off, inverse, count = 8, None, None
        if status == 0:
            count = int(np.frombuffer(out[8:16], dtype=np.int64)[0])
            inverse = np.frombuffer(out[16:16 + 8 * E], dtype=np.int64)
            off = 16 + 8 * E
        n_bad = int(np.frombuffer(out[off:off + 8], dtype=np.int64)[0])
        mask = np.frombuffer(out[off + 8:], dtype=np.uint8).astype(bool)
        assert len(mask) == E
        return status, count, inverse, n_bad, mask

    return run


@pytest.mark.parametrize("n", C.NODE_COUNTS)
def test_host_program_ids_match_np_unique(random_check, n):
    for E in C.ID_SIZES:
        ei = C.multigraph(E, n, seed=E + n)
        want, cnt = C.np_inverse(ei[0], ei[1], n)
        keep = np.zeros(1, dtype=np.uint8)
        status, count, inverse, _, _ = random_check(n, ei[0], ei[1], np.zeros(E, dtype=np.int64), keep)
        assert status == 0 and count == cnt, (n, E)
        assert np.array_equal(inverse, want), (n, E)


def test_host_program_ids_large_node_count(random_check):
    """n = 2^31 - 1: keys near 2^62."""
    n = (1 << 31) - 1
    src = np.array([n - 1, 0, n - 1, n - 2, 5, n - 1, 0], dtype=np.int64)
    dst = np.array([n - 1, n - 1, 0, n - 1, 5, n - 2, 0], dtype=np.int64)
    want, cnt = C.np_inverse(src, dst, n)
    status, count, inverse, _, _ = random_check(n, src, dst, np.zeros(7, dtype=np.int64), np.zeros(1))
    assert status == 0 and count == cnt and np.array_equal(inverse, want)


def test_host_program_status_gate(random_check):
    z = np.zeros(3, dtype=np.int64)
    one = np.zeros(1)
    assert random_check(4, [0, 4, 1], [1, 2, 3], z, one)[0] == 1  # an id equal to n
    assert random_check(4, [0, 1, 1], [1, -1, 3], z, one)[0] == 1  # a negative id
    assert random_check(4, [], [], [], one)[0] == 1  # E = 0
    assert random_check(1 << 31, [0, 1, 2], [1, 2, 0], z, one)[0] == 1  # n >= 2^31
    assert random_check(4, [0, 1, 1], [1, 2, 3], z, one)[0] == 0


@pytest.mark.parametrize("m", C.MASK_SIZES)
def test_host_program_gather_wraps_like_numpy(random_check, m):
    s, inv, ei = C.mask_case(m, seed=m)
    keep = np.random.default_rng(m).random(m) < 0.5
    _, _, _, n_bad, mask = random_check(len(inv) + 1, ei[0], ei[1], inv, keep)
    assert n_bad == 0 and np.array_equal(mask, keep[inv])
    for bad_entry in (m, -m - 1):
        bad = inv.copy()
        bad[len(bad) // 2] = bad_entry
        with pytest.raises(IndexError):
            keep[bad]
        assert random_check(len(inv) + 1, ei[0], ei[1], bad, keep)[3] == 1
