"""Host-only plan functions: what NumPy itself defines for the reference (the JL
dimension, the Adamic-Adar weights, OpenBLAS's thread count) and the plans libgsparse
follows, read back from its host entry points.  None needs a context or a device.
"""

from __future__ import annotations

import os

import numpy as np

from . import _lib
from ._lib import ptr


def blas_threads_default() -> int:
    """OpenBLAS thread count NumPy would use for np.dot in this process.

    The reference's CG dot products are OpenBLAS ddot calls whose reduction
    order depends on it (n > 10000); GSPARSE_BLAS_THREADS overrides.  Clamped to
    OpenBLAS's MAX_THREADS (64 in NumPy's build), as OpenBLAS itself does."""
    return min(_blas_threads_requested(), OPENBLAS_MAX_THREADS)


OPENBLAS_MAX_THREADS = 64


def _blas_threads_requested() -> int:
    env = os.environ.get("GSPARSE_BLAS_THREADS")
    if env:
        return max(1, int(env))
    try:
        from threadpoolctl import threadpool_info

        for info in threadpool_info():
            if info.get("internal_api") == "openblas":
                return max(1, int(info.get("num_threads", 1)))
    except Exception:
        pass
    env = os.environ.get("OPENBLAS_NUM_THREADS")
    return max(1, int(env)) if env else 1


def jl_dim(n: int, epsilon: float) -> int:
    """metrics.py:248, evaluated with NumPy exactly as the reference does."""
    return max(int(24 * np.log(max(n, 2)) / (epsilon ** 2)), 1)


def aa_weights(indptr: np.ndarray) -> np.ndarray:
    """metrics.py:100-108 (adj_binary degrees -> c), NumPy ufuncs as the reference."""
    degrees = np.diff(indptr).astype(np.float64)
    log_degrees = np.log(degrees + 1)
    log_degrees = np.maximum(log_degrees, 1e-10)
    return 1.0 / np.sqrt(log_degrees)


def er_split(k: int, parts: int) -> list[int]:
    b = np.zeros(parts + 1, dtype=np.int64)
    _lib.check(_lib.lib().gs_er_split(k, parts, ptr(b)), "gs_er_split")
    return b.tolist()


def er_plan(n: int, lnnz: int, ncols: int, blas_threads: int) -> dict:
    """The plan gs_er_solve follows for ncols columns of an n-row system whose L_reg
    has lnnz entries, under the GSPARSE_CG_* / _RES_* / _REG_* variables as they are
    now (gs_er_plan; host code, no device): solver mode, columns per lane, chain rows
    per trip, BLAS chunks."""
    o = np.zeros(4, dtype=np.int32)
    _lib.check(_lib.lib().gs_er_plan(n, lnnz, ncols, blas_threads, ptr(o)), "gs_er_plan")
    return dict(zip(("mode", "cpl", "ru", "chunks"), o.tolist()))


def er_reg_layout(n: int, blas_threads: int, unit: bool = True) -> dict | None:
    """Where the register-resident solver (mode 5) keeps p for an n-row system, under
    GSPARSE_REG_NT / GSPARSE_REG_KEEP as they are now (gs_er_reg_layout; host code, no
    device); None where mode 5 does not apply.  threads per workgroup, G threads per
    chain, R row slots per thread, T chunks, zslot (the LDS slots of p), dsl diagonal
    slots, lds_bytes of a launch, and per chunk: start, len, its first keep rows in LDS
    from LDS slot lbase."""
    o = np.zeros(72, dtype=np.int64)
    _lib.check(_lib.lib().gs_er_reg_layout(n, blas_threads, int(bool(unit)), ptr(o)),
               "gs_er_reg_layout")
    if o[0] == 0:
        return None
    d = dict(zip(("threads", "G", "R", "T", "zslot", "dsl", "lds_bytes"), o[:7].tolist()))
    T = d["T"]
    for i, name in enumerate(("start", "len", "keep", "lbase")):
        d[name] = o[8 + 16 * i:8 + 16 * i + T].tolist()
    return d


def er_reg_layout_w(n: int, blas_threads: int, window: int, unit: bool = True) -> dict | None:
    """er_reg_layout with a p window of ``window`` wave-slots per chunk asked for (3 or 4;
    gs_er_reg_layout_w): also W, the window laid out -- 0 where the window kernel does
    not exist (other than two threads per chain, weighted) or a prefix is not a whole
    number of wave-slots, and the layout is then er_reg_layout's -- and per chunk wbase,
    the LDS slot its window starts at."""
    o = np.zeros(88, dtype=np.int64)
    _lib.check(_lib.lib().gs_er_reg_layout_w(n, blas_threads, int(bool(unit)), int(window), ptr(o)),
               "gs_er_reg_layout_w")
    if o[0] == 0:
        return None
    d = dict(zip(("threads", "G", "R", "T", "zslot", "dsl", "lds_bytes", "W"), o[:8].tolist()))
    T = d["T"]
    for i, name in enumerate(("start", "len", "keep", "lbase", "wbase")):
        d[name] = o[8 + 16 * i:8 + 16 * i + T].tolist()
    return d


def xer_sparse_plan(n: int, cus: int = 0) -> dict:
    """The plan the sparse exact effective resistance (gs_exact_er_sparse) follows for an
    n-node graph on a device of ``cus`` compute units (0: 256), under GSPARSE_XER_BATCH
    as it is now (gs_xer_sparse_plan; host code, no device): batch, the columns solved
    at a time (a multiple of 64); budget_bytes, what its four n x batch fp64 blocks may
    take; chunks and chunk_rows, the row chunks of its reductions (functions of n alone)."""
    o = np.zeros(4, dtype=np.int64)
    _lib.check(_lib.lib().gs_xer_sparse_plan(int(n), int(cus), ptr(o)), "gs_xer_sparse_plan")
    return dict(zip(("batch", "budget_bytes", "chunks", "chunk_rows"), o.tolist()))


def bb_geometry(n: int, nsrc: int, nranks: int = 1, lpart: int = 0) -> dict:
    """The numbers a metric backbone run of n nodes (E > 0) takes on rank lpart of nranks,
    under the GSPARSE_BB_* variables as they are now (gs_bb_geometry; host code, no
    device): K landmarks, whether their searches spread over the GPU and with how many
    workgroups each (lm_W, 0 when this rank has no landmark), and for nsrc sources with
    open columns the sources per workgroup, its threads, the batches and the slabs."""
    o = np.zeros(7, dtype=np.int64)
    _lib.check(_lib.lib().gs_bb_geometry(n, nsrc, nranks, lpart, ptr(o)), "gs_bb_geometry")
    return dict(zip(("K", "lm_coop", "lm_W", "S", "threads", "nbatch", "slabs"), o.tolist()))
