"""Shared inputs and the CPU reference of the normal-stream tests
(test_stream_cases_host.py, test_gpu_normal_stream.py): one table of (graph, k, seed)
cases whose need = m * k normals sit at the sizes where the device's block-parallel
parse of NumPy's Generator(PCG64).standard_normal can go wrong, and Z after a short CG
on the same stream drawn by NumPy itself (computed once per case and kept).

Z, not the scores, is what the tests compare: r_eff squares Z_u - Z_v, so it cannot see
the sign of a whole R column; Z = CG(L_reg, B @ R / sqrt(k)) depends on every normal
linearly."""

import functools

import numpy as np

import gsparse_oracle as O
from conftest import load_golden

# |x| beyond this came from the ziggurat's tail (kZigR, csrc/gs_ziggurat_tables.hpp): the
# restated log1p and the tail's own sign bit
ZIG_R = 3.6541528853610088

# (golden graph, k): k goes straight to er_prepare, need = m * k.  m = 1 / 3 / 78 / 10502
CASES = (
    ("single_edge", 1),    # need 1: one normal, the first block alone
    ("triangle", 5),       # need 15: k no power of two, three rows
    ("karate_test", 3),    # need 234: just inside one 256-draw block
    ("karate_test", 4),    # need 312: just past it
    ("karate_test", 13),   # need 1014: just inside one 1,024-draw emit span
    ("karate_test", 14),   # need 1092: just past it
    ("rmat10", 200),       # need 2,100,400: ~8,500 blocks, ~500 tail draws per seed
)
LARGE = ("rmat10", 200)
AROUND_1024 = (("karate_test", 13), ("karate_test", 14))
SEEDS = (42, 0, 1, 7, 12345, 2 ** 63 + 5)  # 42: the stream every other test reads

MAXITER, RTOL = 8, 1e-6  # eight iterations: cheap, and Z still depends on every Y entry


def case_id(case):
    return f"{case[0]}-k{case[1]}"


def seed_id(seed):
    return f"seed{seed}"


@functools.lru_cache(maxsize=None)
def graph(name):
    """(n, indptr, indices, data, m) of golden `name`; m = the u < v entries."""
    g = load_golden(name)
    ip, ix, d = g["indptr"], g["indices"], g["data"]
    m = int(np.count_nonzero(O.csr_rows(ip) < ix))
    for a in (ip, ix, d):
        a.setflags(write=False)
    return int(g["num_nodes"]), ip, ix, d, m


def need(case):
    return graph(case[0])[4] * case[1]


def normals(case, seed):
    """R = default_rng(seed).standard_normal((m, k)), NumPy's own (metrics.py:232, 272)."""
    return np.random.default_rng(seed).standard_normal((graph(case[0])[4], case[1]))


@functools.lru_cache(maxsize=None)
def reference(case, seed, maxiter=MAXITER):
    """(Z_ref, its): Y = B @ (R / sqrt(k)) as O.approx_er_projection forms it, then the
    oracle's CG (oracle.c, one BLAS thread) for maxiter iterations.  Read-only."""
    name, k = case
    n, ip, ix, d, m = graph(name)
    Y, m_, k_ = O.approx_er_projection(ip, ix, n, seed=seed, k=k)
    assert (m_, k_) == (m, k)
    Z, its = O.cg(O.laplacian_reg(ip, ix, d, n), Y, maxiter, RTOL, 1)
    for a in (Z, its):
        a.setflags(write=False)
    return Z, its
