"""Scorer orchestration over one libgsparse context (host side of the hot path).

Everything numeric runs in libgsparse.so (HIP, gfx950).  The host keeps only
what the reference defines through NumPy itself and that must therefore be
evaluated by NumPy to stay bit-identical: the per-node Adamic-Adar weights
c = 1/sqrt(max(log(deg+1), 1e-10)) (metrics.py:104-108, n values), the JL
dimension k (metrics.py:248) and -- unless the device ziggurat is selected --
the PCG64 normal stream R (metrics.py:272), streamed row-chunk by row-chunk.
"""

from __future__ import annotations

import ctypes
import os
import queue
import threading

import numpy as np

from . import _args as A
from ._lib import GS_DEVICE, GS_HOST, Context, ptr
from .plans import (OPENBLAS_MAX_THREADS, aa_weights, bb_geometry,  # noqa: F401 (re-exported)
                    blas_threads_default, er_plan, er_reg_layout, er_reg_layout_w, er_split,
                    jl_dim, xer_sparse_plan)

_ROW_CHUNK_BYTES = 64 << 20


class Engine:
    """Scorers over the graph resident in ``ctx``."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.n, self.nnz, self.symmetric = ctx.shape()
        self._indptr = None

    # -- helpers ------------------------------------------------------------
    def indptr(self) -> np.ndarray:
        if self._indptr is None:
            ip = np.empty(self.n + 1, dtype=np.int64)
            self.ctx.call("gs_graph_copy_csr", ptr(ip), None, None, GS_HOST)
            self._indptr = ip
        return self._indptr

    def _scores_out(self, count, out):
        return A.out(out, np.float64, count, "out", self.ctx.device)

    # -- scorers ------------------------------------------------------------
    def jaccard(self, e0: int = 0, e1: int | None = None, out=None):
        e1 = self.nnz if e1 is None else e1
        o, loc = self._scores_out(e1 - e0, out)
        self.ctx.call("gs_jaccard", e0, e1, ptr(o), loc)
        return o

    def jaccard_part(self, part: int, nparts: int, out=None):
        """Share `part` of `nparts` of the whole Jaccard vector (zeros elsewhere;
        the shares sum to jaccard()) -- gs_jaccard_part."""
        o, loc = self._scores_out(self.nnz, out)
        self.ctx.call("gs_jaccard_part", part, nparts, ptr(o), loc)
        return o

    def jaccard_shares(self, nparts: int):
        """gs_jaccard_shares: (row_cut, owner_off), nparts + 1 values each -- the
        owner-pair shares of the sharded Jaccard (the same on every rank)."""
        rc = np.empty(nparts + 1, dtype=np.int64)
        oo = np.empty(nparts + 1, dtype=np.int64)
        self.ctx.call("gs_jaccard_shares", nparts, ptr(rc), ptr(oo))
        return rc, oo

    def jaccard_part_counts(self, part: int, nparts: int, out=None):
        """gs_jaccard_part_counts: |N(u) ∩ N(v)| of this part's owner pairs
        (uint32 numpy array, or the int32/uint32 device tensor ``out``)."""
        if not 0 <= part < nparts:
            raise ValueError(f"bad part {part} of {nparts}")
        _, oo = self.jaccard_shares(nparts)
        cnt = int(oo[part + 1] - oo[part])
        o, loc = A.out(out, (np.uint32, np.int32), cnt, "counts buffer", self.ctx.device,
                       short=IndexError)
        self.ctx.call("gs_jaccard_part_counts", part, nparts, ptr(o), loc)
        return o

    def jaccard_from_counts(self, nparts: int, counts, stride: int, out=None):
        """gs_jaccard_from_counts: every part's counts (part p at p * stride) ->
        the Jaccard score of every CSR entry."""
        counts, cloc = A.inp(counts, (np.uint32, np.int32), "counts", self.ctx.device,
                             nparts * stride, short=IndexError)
        o, loc = self._scores_out(self.nnz, out)
        self.ctx.call("gs_jaccard_from_counts", nparts, ptr(counts), stride, cloc, ptr(o), loc)
        return o

    # -- distributed Jaccard-T select (gs_jsel_*, include/gsparse.h) ---------
    JSEL_BINS, JSEL_PASSES = 8192, 5

    def jsel_begin(self, part: int, nparts: int, counts, num_keep: int, keep_lowest: bool, hist,
                   scores=None):
        """Keys (and, into ``scores``, the fp64 scores) of this part's owner pairs and the
        first weighted histogram into ``hist`` (JSEL_BINS int64/uint64 values)."""
        dev = self.ctx.device
        _, oo = self.jaccard_shares(nparts)
        np_ = int(oo[part + 1] - oo[part])
        counts, cloc = A.inp(counts, (np.uint32, np.int32), "counts", dev, np_, cast="never",
                             short=IndexError)
        hist, hloc = self._jsel_hist(hist)
        if hloc != GS_DEVICE:
            raise ValueError("hist must be a device tensor (the ranks all-reduce it there)")
        sloc = GS_HOST
        if scores is not None:
            scores, sloc = A.out(scores, np.float64, np_, "scores", dev, short=IndexError)
        self.ctx.call("gs_jsel_begin", int(part), int(nparts), ptr(counts), cloc,
                      int(num_keep), int(bool(keep_lowest)), ptr(hist), ptr(scores), sloc)
        self._jsel_pairs = np_
        return np_

    def _jsel_hist(self, hist):
        return A.out(hist, (np.int64, np.uint64), self.JSEL_BINS, "hist", self.ctx.device,
                     short=IndexError)

    def jsel_step(self, hist) -> int:
        """One pass of the select on the all-reduced ``hist``; returns the passes left."""
        left = ctypes.c_int(0)
        self.ctx.call("gs_jsel_step", ptr(self._jsel_hist(hist)[0]), ctypes.byref(left))
        return left.value

    def jsel_result(self):
        """(cut, #beyond, #tied, #tied positions on this rank)."""
        cut, nb, nt, mine = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self.ctx.call("gs_jsel_result", ctypes.byref(cut), ctypes.byref(nb), ctypes.byref(nt),
                      ctypes.byref(mine))
        return cut.value, nb.value, nt.value, mine.value

    def jsel_tie_positions(self, out):
        """This rank's tied CSR positions into ``out`` (int64)."""
        out, loc = A.out(out, np.int64, 0, "positions", self.ctx.device)
        self.ctx.call("gs_jsel_tie_positions", ptr(out), A.size(out), loc)
        return out

    def jsel_keep(self, tie_pos, ntie: int, need: int, out):
        """2-bit keep codes of this part's pairs (bit 0 owner entry, bit 1 reverse entry),
        four pairs per byte, into ``out`` (uint8, >= ceil(pairs / 4) bytes)."""
        dev = self.ctx.device
        np_ = getattr(self, "_jsel_pairs", 0)
        out, loc = A.out(out, np.uint8, (np_ + 3) // 4, "keep", dev, short=IndexError)
        tloc = GS_HOST
        if tie_pos is not None:
            tie_pos, tloc = A.inp(tie_pos, np.int64, "tie positions", dev, ntie, cast="never",
                                  short=IndexError)
        self.ctx.call("gs_jsel_keep", ptr(tie_pos), int(ntie), tloc, int(need), ptr(out), loc)
        return out

    def jsel_mask(self, nparts: int, keep_all, stride: int, out):
        """Every part's keep codes (part p's from byte p * stride) -> the CSR keep mask (uint8)."""
        dev = self.ctx.device
        keep_all, kloc = A.inp(keep_all, np.uint8, "keep_all", dev, nparts * stride, cast="never",
                               short=IndexError)
        out, loc = A.out(out, (np.uint8, np.bool_), self.nnz, "mask", dev, short=IndexError)
        self.ctx.call("gs_jsel_mask", int(nparts), ptr(keep_all), int(stride), kloc, ptr(out), loc)
        return out

    def adamic_adar(self, e0: int = 0, e1: int | None = None, out=None, c=None):
        e1 = self.nnz if e1 is None else e1
        c, cloc = A.inp(aa_weights(self.indptr()) if c is None else c, np.float64, "c",
                        self.ctx.device, self.n)
        o, loc = self._scores_out(e1 - e0, out)
        self.ctx.call("gs_adamic_adar", ptr(c), cloc, e0, e1, ptr(o), loc)
        return o

    def degree(self, e0: int = 0, e1: int | None = None, out=None):
        e1 = self.nnz if e1 is None else e1
        o, loc = self._scores_out(e1 - e0, out)
        self.ctx.call("gs_degree", e0, e1, ptr(o), loc)
        return o

    def feature_cosine(self, x, e0: int = 0, e1: int | None = None, out=None):
        """x: (n, f) float32/float64 numpy array or CUDA torch tensor."""
        e1 = self.nnz if e1 is None else e1
        x, xloc = A.inp(x, None, "features", self.ctx.device)
        dt = A.dtype_of(x)
        if x.ndim != 2 or x.shape[0] != self.n:
            raise ValueError(f"features must be ({self.n}, f), got {tuple(x.shape)}")
        o, loc = self._scores_out(e1 - e0, out)
        if dt == np.float32:
            self.ctx.call("gs_feature_cosine_f32", ptr(x), int(x.shape[1]), xloc, e0, e1, ptr(o), loc)
        elif dt == np.float64:
            self.ctx.call("gs_feature_cosine_f64", ptr(x), int(x.shape[1]), xloc, e0, e1, ptr(o), loc)
        else:
            raise NotImplementedError(f"feature_cosine supports float32/float64 features, got {dt}")
        return o

    # -- ApproxER -----------------------------------------------------------
    def er_prepare(self, k: int, reg: float = 1e-6) -> int:
        m = ctypes.c_int64(0)
        self.ctx.call("gs_er_prepare", k, reg, ctypes.byref(m))
        self.k = k
        self.m = m.value
        return self.m

    def er_project_host(self, rng: np.random.Generator, k: int, cols=None):
        """Stream R = rng.standard_normal((m, k)) row-chunk by row-chunk (identical
        NumPy stream, verified chunk-invariant) into Y = B @ (R / sqrt(k)),
        generating chunk i+1 on a worker thread while chunk i is projected.
        cols = (c0, c1): form only Y[:, c0:c1] (a rank's JL columns)."""
        c0, c1 = cols if cols is not None else (0, k)
        m = self.m
        sqrt_k = float(np.sqrt(k))
        rows = max(1, _ROW_CHUNK_BYTES // (8 * k))
        q: queue.Queue = queue.Queue(maxsize=2)

        def producer():
            for e0 in range(0, m, rows):
                e1 = min(m, e0 + rows)
                q.put((e0, e1, rng.standard_normal((e1 - e0, k))))
            q.put(None)

        th = threading.Thread(target=producer, daemon=True)
        th.start()
        while True:
            item = q.get()
            if item is None:
                break
            e0, e1, raw = item
            self.ctx.call("gs_er_project_rows_cols", e0, e1, ptr(raw), GS_HOST, sqrt_k, c0, c1)
        th.join()

    def er_project_device(self, rng: np.random.Generator, k: int, cols=None):
        """The same R drawn on the device (PCG64 + NumPy's ziggurat); cols = (c0, c1):
        every normal is parsed, only R[:, c0:c1] is stored and projected."""
        c0, c1 = cols if cols is not None else (0, k)
        self.ctx.call("gs_er_project_pcg64_cols", *self._pcg64_words(rng), float(np.sqrt(k)), c0, c1)

    def er_solve(self, col0: int, col1: int, maxiter: int, rtol: float, blas_threads: int):
        self.ctx.call("gs_er_solve", col0, col1, maxiter, rtol, blas_threads)

    def er_scores(self, col0: int, col1: int, finalize: bool = True, e0: int = 0,
                  e1: int | None = None, out=None):
        e1 = self.nnz if e1 is None else e1
        o, loc = self._scores_out(e1 - e0, out)
        self.ctx.call("gs_er_scores", col0, col1, e0, e1, int(finalize), ptr(o), loc)
        return o

    def er_iterations(self) -> np.ndarray:
        it = np.empty(self.k, dtype=np.int32)
        self.ctx.call("gs_er_iterations", ptr(it), GS_HOST)
        return it

    def er_reg_window(self) -> dict:
        """What the last register-resident solve (mode 5) chose for its p window
        (gs_er_reg_window): W wave-slots per chunk (0: the plain layout), the wave-slots
        with a global p code under the plain and under the windowed layout (-1 where no
        window was weighed) and the window codes in the ELL copy."""
        o = np.zeros(4, dtype=np.int64)
        self.ctx.call("gs_er_reg_window", ptr(o))
        return dict(zip(("W", "slow_plain", "slow_window", "window_codes"), o.tolist()))

    def er_z(self, col0: int, col1: int) -> np.ndarray:
        """The solved Z columns [col0, col1) as an (n, col1 - col0) array (gs_er_copy_z)."""
        z = np.empty((self.n, col1 - col0), dtype=np.float64)
        self.ctx.call("gs_er_copy_z", col0, col1, ptr(z), GS_HOST)
        return z

    def approx_er(self, epsilon: float = 0.3, seed: int = 42, max_cg_iters: int = 500,
                  cg_tol: float = 1e-6, blas_threads: int | None = None,
                  rng_mode: str | None = None):
        """calculate_approx_effective_resistance_scores (metrics.py:178-298)."""
        rng = np.random.default_rng(seed)
        n = self.n
        k = jl_dim(n, epsilon)
        m = self.er_prepare(k)
        if m == 0:
            return np.zeros(self.nnz, dtype=np.float64)
        mode = rng_mode or os.environ.get("GSPARSE_ER_RNG", "device")
        if mode == "device":
            self.er_project_device(rng, k)
        else:
            self.er_project_host(rng, k)
        bt = blas_threads_default() if blas_threads is None else blas_threads
        self.er_solve(0, k, max_cg_iters, cg_tol, bt)
        return self.er_scores(0, k, True)

    # -- topology analytics (compute_topology_metrics, metrics.py:445-520) ----
    def common_neighbors(self, out=None):
        """gs_common_neighbors: |N(u) ∩ N(v)| per CSR entry (symmetric graph)."""
        o, loc = self._scores_out(self.nnz, out)
        self.ctx.call("gs_common_neighbors", ptr(o), loc)
        return o

    def trussness(self, out=None):
        """gs_trussness: the trussness of every CSR entry (symmetric graph; exact integers
        as float64, 0 on diagonal entries) -> ``(scores, info)``, ``info`` holding
        ``max_truss``, ``levels`` (distinct trussness values), ``rounds`` (sub-rounds of
        the level-synchronous peel, ``selection.trussness_host``'s layering) and
        ``host_waits`` (which alone depends on GSPARSE_TRUSS_TAIL)."""
        o, loc = self._scores_out(self.nnz, out)
        mx, lv = ctypes.c_int64(0), ctypes.c_int32(0)
        rd, hw = ctypes.c_int64(0), ctypes.c_int64(0)
        self.ctx.call("gs_trussness", ptr(o), loc, ctypes.byref(mx), ctypes.byref(lv),
                      ctypes.byref(rd), ctypes.byref(hw))
        return o, {"max_truss": mx.value, "levels": lv.value, "rounds": rd.value,
                   "host_waits": hw.value}

    # gs_simmelian's pair classes (GS_SIM_*), by the shorter of a pair's neighbour lists
    SIM_CLASSES = ("wave", "mid", "lds", "stream")

    def simmelian(self, max_rank: int = 0, out=None):
        """gs_simmelian: the Simmelian backbone score of every CSR entry (symmetric graph;
        ``selection.simmelian_host`` on the device, bit for bit) -> ``(scores, info)``.
        ``max_rank = 0``: the largest Jaccard ratio of the two ends' ranked neighbourhoods
        over every rank bound; ``max_rank = k0 >= 1``: their overlap at ``k0``, an exact
        integer as float64 (ValueError for a negative ``max_rank``).  0 on diagonal
        entries.  ``info`` holds ``max_common`` (the most common neighbours of a pair),
        ``nonzero_pairs`` and ``classes`` (pairs per kernel class, keyed by SIM_CLASSES;
        they alone depend on GSPARSE_SIM_WAVE_MAX / _MID_MAX / _LDS_MAX)."""
        o, loc = self._scores_out(self.nnz, out)
        mc, nzp = ctypes.c_int64(0), ctypes.c_int64(0)
        counts = np.zeros(len(self.SIM_CLASSES), dtype=np.int64)
        self.ctx.call("gs_simmelian", ptr(o), loc, int(max_rank), ctypes.byref(mc), ctypes.byref(nzp),
                      ptr(counts), len(counts))
        return o, {"max_common": mc.value, "nonzero_pairs": nzp.value,
                   "classes": dict(zip(self.SIM_CLASSES, (int(v) for v in counts)))}

    def clustering(self, per_node: bool = False):
        """gs_clustering: nx.average_clustering of the resident (symmetric,
        self-loop-free) graph, bit-identical; optionally the per-node values."""
        avg = ctypes.c_double(0.0)
        cv = np.empty(max(self.n, 1), dtype=np.float64) if per_node else None
        self.ctx.call("gs_clustering", ctypes.byref(avg), ptr(cv) if cv is not None else None,
                      GS_HOST)
        return (avg.value, cv[: self.n]) if per_node else avg.value

    def components(self):
        """gs_components: (labels = smallest node id per component, count, largest)."""
        lab = np.empty(max(self.n, 1), dtype=np.int32)
        cnt, big = ctypes.c_int64(0), ctypes.c_int64(0)
        self.ctx.call("gs_components", ptr(lab), GS_HOST, ctypes.byref(cnt), ctypes.byref(big))
        return lab[: self.n], cnt.value, big.value

    def fiedler(self, tol: float = 1e-12, max_iter: int = 300, method: str = "auto",
                cg_rtol: float = 1e-10, cg_max_iter: int = 5000):
        """Algebraic connectivity of the (connected) resident graph.

        method "auto": gs_fiedler (the dense Cholesky form up to 32768 nodes, the sparse
        form with its default inner tolerances above); "dense": gs_fiedler on a graph the
        dense form takes (NotImplementedError above 32768 nodes); "sparse":
        gs_fiedler_sparse at any size, each Lanczos step a Jacobi-preconditioned CG solve
        to relative residual cg_rtol within cg_max_iter iterations.  fiedler_iterations:
        Lanczos steps; fiedler_cg_iterations: CG iterations of all solves of the last
        method="sparse" call (None otherwise: gs_fiedler reports the steps only).  A solver that stops at a cap unconverged
        raises GsparseNotConverged (a RuntimeError); the counts are recorded then too."""
        if method not in ("auto", "dense", "sparse"):
            raise ValueError(f"method must be 'auto', 'dense' or 'sparse', got {method!r}")
        v, it, cg = ctypes.c_double(0.0), ctypes.c_int32(0), ctypes.c_int64(0)
        self.fiedler_iterations = self.fiedler_cg_iterations = None
        if method == "dense" and self.n > 32768:
            raise NotImplementedError(f"the dense algebraic connectivity is O(n^3): n={self.n}")
        try:
            if method == "sparse":
                self.ctx.call("gs_fiedler_sparse", float(tol), int(max_iter), float(cg_rtol),
                              int(cg_max_iter), ctypes.byref(v), ctypes.byref(it),
                              ctypes.byref(cg))
            else:
                self.ctx.call("gs_fiedler", float(tol), int(max_iter), ctypes.byref(v),
                              ctypes.byref(it))
        finally:
            self.fiedler_iterations = it.value
            if method == "sparse":
                self.fiedler_cg_iterations = cg.value
        return v.value

    def spectral_bounds(self, hw, tol: float = 1e-9, max_iter: int = 300,
                        cg_rtol: float = 1e-10, cg_max_iter: int = 5000):
        """gs_spectral_bounds: ``(lambda_min, lambda_max)`` of the pencil
        ``L_H x = lambda L_G x`` over the mean-free vectors, G the (connected, symmetric)
        resident graph and H the graph with weight ``hw[e]`` on CSR entry ``e`` of G (a
        float64 numpy array or CUDA tensor of nnz entries in the order of ``Context.csr()``;
        0 drops the entry, diagonal entries are ignored).  H is a ``(1 +- eps)`` spectral
        approximation of G with ``eps = max(lambda_max - 1, 1 - lambda_min)``.

        Lanczos on ``L_G^+ L_H`` in the ``L_G`` inner product, each step one
        Jacobi-preconditioned CG solve to relative residual ``cg_rtol`` within
        ``cg_max_iter`` iterations, until the residual bounds of both extreme Ritz pairs are
        below ``tol * lambda_max`` or ``max_iter`` steps.  ``spectral_bounds_iterations``:
        Lanczos steps; ``spectral_bounds_cg_iterations``: CG iterations of all solves.  A
        solver that stops at a cap unconverged raises GsparseNotConverged (a RuntimeError);
        the counts are recorded then too."""
        hw, loc = A.inp(hw, np.float64, "hw", self.ctx.device, cast="both")
        lo, hi = ctypes.c_double(0.0), ctypes.c_double(0.0)
        it, cg = ctypes.c_int32(0), ctypes.c_int64(0)
        self.spectral_bounds_iterations = self.spectral_bounds_cg_iterations = None
        try:
            self.ctx.call("gs_spectral_bounds", ptr(hw), loc, A.size(hw),
                          float(tol), int(max_iter), float(cg_rtol), int(cg_max_iter),
                          ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(it), ctypes.byref(cg))
        finally:
            self.spectral_bounds_iterations = it.value
            self.spectral_bounds_cg_iterations = cg.value
        return lo.value, hi.value

    # -- selection ------------------------------------------------------------
    def exact_er(self, out=None, method: str = "auto", cg_rtol: float = 1e-12,
                 cg_max_iter: int = 5000):
        """calculate_effective_resistance_scores (metrics.py:124-175), one score per CSR
        entry from the grounded Laplacian's inverse.

        method "auto": gs_exact_er (up to 32768 nodes the dense form, a blocked fp64-MFMA
        Cholesky, GSPARSE_XER_METHOD=ns: Newton-Schulz; above, the sparse form with its
        default tolerances); "dense": gs_exact_er on a graph the dense form takes
        (NotImplementedError above 32768 nodes); "sparse": gs_exact_er_sparse at any size,
        the inverse's columns by a Jacobi-preconditioned CG, a batch of columns at a time
        (GSPARSE_XER_BATCH overrides the batch width), each column to relative residual
        cg_rtol within cg_max_iter iterations.  exact_er_iterations: 64-row blocks, the last
        Newton-Schulz step, or the sparse form's batches; exact_er_cg_iterations: the
        columns' CG iterations summed, of a method="sparse" call (None otherwise: gs_exact_er
        reports the batches only).  A batch that stops
        at the cap with a column open raises GsparseNotConverged (a RuntimeError): ``out`` is
        left as it was, the counts are recorded."""
        if method not in ("auto", "dense", "sparse"):
            raise ValueError(f"method must be 'auto', 'dense' or 'sparse', got {method!r}")
        self.exact_er_iterations = self.exact_er_cg_iterations = None
        if method == "dense" and self.n > 32768:
            raise NotImplementedError(f"the dense exact effective resistance is O(n^3): n={self.n}")
        o, loc = self._scores_out(self.nnz, out)
        it, cg = ctypes.c_int32(0), ctypes.c_int64(0)
        sparse = method == "sparse"
        try:
            if sparse:
                self.ctx.call("gs_exact_er_sparse", ptr(o), loc, float(cg_rtol), int(cg_max_iter),
                              ctypes.byref(it), ctypes.byref(cg))
            else:
                self.ctx.call("gs_exact_er", ptr(o), loc, ctypes.byref(it))
        finally:
            self.exact_er_iterations = it.value
            if sparse:
                self.exact_er_cg_iterations = cg.value
        return o

    def segment_argmax(self, scores: np.ndarray, src: np.ndarray, num_nodes: int) -> np.ndarray:
        """gs_segment_argmax: per node the column of its unique top score, -1 (no
        column) or -2 (np.argsort's order decides)."""
        scores, sloc = A.inp(scores, np.float64, "scores", self.ctx.device)
        src, loc = A.inp(src, np.int64, "src", self.ctx.device, cast="both")
        pick = np.empty(max(num_nodes, 1), dtype=np.int64)
        self.ctx.call("gs_segment_argmax", ptr(scores), sloc, int(scores.shape[0]), ptr(src),
                      loc, int(src.shape[0]), int(num_nodes), ptr(pick), GS_HOST)
        return pick[:num_nodes]

    SEGK_CLASSES = ("empty", "all", "short", "lds", "stream")

    def segment_topk(self, scores: np.ndarray, src: np.ndarray, num_nodes: int, k: int):
        """gs_segment_topk: per node the set of its min(k, d) top-scoring columns.

        Returns ``(mask, status, info)``: ``mask`` bool[E], True on the guaranteed
        columns of the decided nodes; ``status`` uint8[n], 0 (no column), 1
        (decided) or 2 (np.argsort's order decides: no byte of that node is set);
        ``info`` = ``n_guaranteed``, ``n_ambiguous`` and ``classes`` (nodes handled
        per kernel class, keyed by SEGK_CLASSES)."""
        scores, sloc = A.inp(scores, np.float64, "scores", self.ctx.device)
        src, loc = A.inp(src, np.int64, "src", self.ctx.device, cast="both")
        E = int(src.shape[0])
        if E > scores.shape[0]:  # NumPy's error for scores[column], as the reference raises it
            raise IndexError(f"index {E - 1} is out of bounds for axis 0 with size "
                             f"{scores.shape[0]}")
        mask = np.zeros(max(E, 1), dtype=np.uint8)
        status = np.zeros(max(num_nodes, 1), dtype=np.uint8)
        counts = np.zeros(len(self.SEGK_CLASSES), dtype=np.int64)
        ng, na = ctypes.c_int64(0), ctypes.c_int64(0)
        self.ctx.call("gs_segment_topk", ptr(scores), sloc, int(scores.shape[0]), ptr(src),
                      loc, E, int(num_nodes), int(k), ptr(mask), GS_HOST, ptr(status), GS_HOST,
                      ctypes.byref(ng), ctypes.byref(na), ptr(counts), len(counts))
        info = {"n_guaranteed": ng.value, "n_ambiguous": na.value,
                "classes": dict(zip(self.SEGK_CLASSES, (int(v) for v in counts)))}
        return mask[:E].view(bool), status[:num_nodes], info

    # -- local sparsification (gs_segment_rank / gs_local_scores) ---------------
    SEGR_CLASSES = ("empty", "short", "lds", "stream")

    def _segment_rank(self, scores, src, n: int, keep_lowest: bool):
        """``src`` as ``_args.inp`` returned it -> ``(rank, deg, info)`` where ``src`` lives."""
        scores, sloc = A.inp(scores, np.float64, "scores", self.ctx.device)
        E = int(src.shape[0])
        loc = GS_DEVICE if A.on_device(src, self.ctx.device) else GS_HOST
        rank = A.alloc(max(E, 1), np.int32, src)
        deg = A.alloc(max(n, 1), np.int64, src)
        counts = np.zeros(len(self.SEGR_CLASSES), dtype=np.int64)
        mx = ctypes.c_int64(0)
        self.ctx.call("gs_segment_rank", ptr(scores), sloc, int(scores.shape[0]), ptr(src), loc, E, n,
                      int(bool(keep_lowest)), ptr(rank), loc, ptr(deg), loc, ctypes.byref(mx),
                      ptr(counts), len(counts))
        info = {"max_degree": mx.value,
                "classes": dict(zip(self.SEGR_CLASSES, (int(v) for v in counts)))}
        return rank[:E], deg[:max(n, 0)], info

    def segment_rank(self, scores, src, num_nodes: int, keep_lowest: bool = False):
        """gs_segment_rank: for every column its rank inside its source node's segment,
        the number of columns of that node that are better in the strict total order
        ``(key(score), index)`` larger -- ``keep_lowest``: smaller -- of
        ``spanning_forest``; 0 is the node's best edge.  ``scores`` (float64, one per
        column) and ``src`` (int64): numpy arrays or CUDA tensors.

        Returns ``(rank, deg, info)``: ``rank`` (int32 per column) and ``deg`` (int64 per
        node, its columns) live where ``src`` does; ``info`` holds ``max_degree`` and
        ``classes`` (nodes per kernel class, keyed by SEGR_CLASSES).  ValueError for fewer
        scores than columns or a source outside ``[0, num_nodes)``."""
        src, _ = A.inp(src, np.int64, "src", self.ctx.device, cast="both")
        return self._segment_rank(scores, src, int(num_nodes), keep_lowest)

    def local_scores(self, scores, src, dst, num_nodes: int, keep_lowest: bool = False, out=None):
        """The local-filter score of every column (``selection.local_filter_scores`` on
        the device, bit for bit): gs_segment_rank, the table ``log(max(j, 1))`` for ``j``
        up to the largest degree by NumPy, gs_local_scores.  ``scores`` (float64, one per
        column) and ``src`` / ``dst`` (int64): numpy arrays or CUDA tensors; ``out``: an
        optional float64 array or CUDA tensor of >= E elements that receives the scores.

        Returns ``(local, info)``: ``local`` lives where the ids do (or is ``out``);
        ``info`` holds ``max_degree``, ``n_top`` (columns scoring 1.0: some end's best
        edge) and ``classes``."""
        src, dst, E, loc = A.pair(src, dst, self.ctx.device)
        n = int(num_nodes)
        o, oloc = (A.alloc(max(E, 1), np.float64, src), loc) if out is None else \
            A.out(out, np.float64, E, "out", self.ctx.device)
        rank, deg, info = self._segment_rank(scores, src, n, keep_lowest)
        table = np.log(np.maximum(np.arange(max(info["max_degree"], 1) + 1), 1).astype(np.float64))
        top = ctypes.c_int64(0)
        self.ctx.call("gs_local_scores", ptr(rank), loc, ptr(src), ptr(dst), loc, E, n, ptr(deg), loc,
                      ptr(table), GS_HOST, len(table), ptr(o), oloc, ctypes.byref(top))
        info = {"max_degree": info["max_degree"], "n_top": top.value, "classes": info["classes"]}
        return (o[:E] if out is None else out), info

    # -- score-proportional sampling (gs_sample_*, include/gsparse.h) ----------
    # GS_SAMPLE_TILE / GS_SAMPLE_SUBTREE: the sizes at which the ordered cumsum starts
    # a new LDS tile and the pairwise total a new subtree
    SAMPLE_TILE, SAMPLE_SUBTREE = 1024, 2048

    _pcg64_words = staticmethod(A.pcg64_words)

    def sample_mask(self, scores: np.ndarray, num_edges: int, num_keep: int,
                    rng: np.random.Generator):
        """gs_sample_mask: the set ``rng.choice(num_edges, num_keep, replace=False, p=probs)``
        draws from ``rng``'s current state (the generator itself is not advanced).

        Returns ``(mask, status, rounds, draws)``: ``status`` 0 = ``mask`` (bool[E]) was
        written by the device rounds, 1 = degenerate input, NumPy's own call decides
        (``mask`` is None)."""
        scores, sloc = A.inp(scores, np.float64, "scores", self.ctx.device)
        words = self._pcg64_words(rng)
        mask = np.zeros(max(int(num_edges), 1), dtype=np.uint8)
        status, rounds, draws = ctypes.c_int32(1), ctypes.c_int64(0), ctypes.c_int64(0)
        self.ctx.call("gs_sample_mask", ptr(scores), sloc, int(scores.shape[0]), int(num_edges),
                      int(num_keep), *words, ptr(mask), GS_HOST, ctypes.byref(status),
                      ctypes.byref(rounds), ctypes.byref(draws))
        if status.value != 0:
            return None, status.value, 0, 0
        return mask[:num_edges].view(bool), 0, rounds.value, draws.value

    def pcg64_doubles(self, rng: np.random.Generator, offset: int, n: int, out=None):
        """gs_pcg64_doubles: ``rng.random(offset + n)[offset:]`` drawn on the device
        (into the CUDA float64 tensor ``out`` of >= n elements when given)."""
        o, loc = A.out(out, np.float64, max(n, 1) if out is None else n, "out", self.ctx.device,
                       short=IndexError)
        self.ctx.call("gs_pcg64_doubles", *self._pcg64_words(rng), int(offset), int(n), ptr(o), loc)
        return o[:n] if out is None else out

    # -- symmetric random baseline (gs_undirected_ids / gs_random_mask) ---------
    def undirected_ids(self, src, dst, num_nodes: int, out=None):
        """gs_undirected_ids: ``np.unique(keys, return_inverse=True)[1]`` of the undirected
        keys ``min * (num_nodes + 1) + max`` (random.py:23-30).  ``src`` / ``dst``: int64
        numpy arrays or CUDA tensors (both alike); ``out``: an optional CUDA int64 tensor
        of >= E elements that receives the ids on the device.

        Returns ``(inverse, n_undirected, status)``; status 1 = the input is outside the
        device contract, nothing was written (``inverse`` is None) and the reference's own
        NumPy calls decide."""
        src, dst, E, loc = A.pair(src, dst, self.ctx.device)
        inv, iloc = A.out(out, np.int64, max(E, 1) if out is None else E, "out", self.ctx.device,
                          short=IndexError)
        cnt, status = ctypes.c_int64(0), ctypes.c_int32(1)
        self.ctx.call("gs_undirected_ids", int(num_nodes), E, ptr(src), ptr(dst), loc, ptr(inv), iloc,
                      ctypes.byref(cnt), ctypes.byref(status))
        if status.value != 0:
            return None, 0, status.value
        return (inv[:E] if out is None else out), cnt.value, 0

    def random_mask(self, scores, inverse, n_keep: int, num_edges: int, out=None):
        """gs_random_mask: ``keep_undir[inverse]`` with ``keep_undir`` the ``n_keep`` highest
        of ``scores`` (random.py:45-49).  ``scores`` (float64) and ``inverse`` (int64, >=
        num_edges entries): numpy arrays or CUDA tensors; ``out``: an optional CUDA
        uint8/bool tensor of >= num_edges elements that receives the mask on the device.

        Returns ``(mask, cut, beyond, tied)`` as topk_mask does; IndexError when an
        ``inverse`` entry is outside ``[-len(scores), len(scores))``, as NumPy raises."""
        scores, sloc = A.inp(scores, np.float64, "scores", self.ctx.device)
        m, E = int(scores.shape[0]), int(num_edges)
        inverse, iloc = A.inp(inverse, np.int64, "inverse", self.ctx.device, E, cast="both",
                              short=IndexError)
        mask, mloc = A.mask_out(out, E, self.ctx.device)
        cut, nb, nt, bad = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self.ctx.call("gs_random_mask", ptr(scores), sloc, m, int(n_keep), ptr(inverse), iloc, E,
                      ptr(mask), mloc, ctypes.byref(cut), ctypes.byref(nb), ctypes.byref(nt),
                      ctypes.byref(bad))
        if bad.value:
            raise IndexError(f"{bad.value} index entries are out of bounds for axis 0 with size {m}")
        return (mask[:E].view(bool) if out is None else out), cut.value, nb.value, nt.value

    # -- maximum spanning forest (gs_spanning_forest) ---------------------------
    def spanning_forest(self, scores, src, dst, num_nodes: int, keep_lowest: bool = False,
                        expand: bool = False, out=None):
        """gs_spanning_forest: the forest ``F`` Kruskal's walk adds over the columns of
        ``(src, dst)``, best first in the strict total order ``(key(score), index)`` --
        gs_topk_mask's keys and stable tie rule; ``keep_lowest`` reverses it.  With
        ``expand`` the mask holds every column whose unordered pair is a forest column's
        (the reverse direction, duplicates).  ``scores`` (float64, one per column) and
        ``src`` / ``dst`` (int64): numpy arrays or CUDA tensors; ``out``: an optional CUDA
        uint8/bool tensor of >= E elements that receives the mask on the device.

        Returns ``(mask, labels, info)``: ``labels`` (int32, one representative node per
        component; a CUDA tensor when the ids are) and ``info`` with ``n_forest``
        (``|F|`` = num_nodes - components), ``n_marked`` (mask bytes set) and ``rounds``.
        ValueError for fewer scores than columns or an id outside ``[0, num_nodes)``."""
        scores, sloc = A.inp(scores, np.float64, "scores", self.ctx.device)
        src, dst, E, loc = A.pair(src, dst, self.ctx.device)
        n = int(num_nodes)
        mask, mloc = A.mask_out(out, E, self.ctx.device)
        labels = A.alloc(max(n, 1), np.int32, src)
        nf, nm, rounds = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(0)
        self.ctx.call("gs_spanning_forest", ptr(scores), sloc, int(scores.shape[0]), ptr(src), ptr(dst),
                      loc, E, n, int(bool(keep_lowest)), int(bool(expand)), ptr(mask), mloc,
                      ptr(labels), loc, ctypes.byref(nf), ctypes.byref(nm), ctypes.byref(rounds))
        info = {"n_forest": nf.value, "n_marked": nm.value, "rounds": rounds.value}
        return (mask[:E].view(bool) if out is None else out), labels[:max(n, 0)], info

    # -- spectral sparsification by effective-resistance sampling ---------------
    SPECTRAL_METHODS = {"multinomial": 0, "independent": 1}

    def spectral_sample(self, scores, src, dst, num_nodes: int, num_samples: int,
                        rng: np.random.Generator, method: str = "multinomial"):
        """gs_spectral_sample: ``selection.spectral_sample`` drawn from ``rng``'s current
        state on the device (the generator itself is not advanced).  ``scores`` (float64,
        one per column) and ``src`` / ``dst`` (int64): numpy arrays or CUDA tensors; the
        results live where the ids do.

        Returns ``(mask, weight, counts, inverse, info)``: bool[E], float64[E], int64[m],
        int64[E] and ``info`` with ``status``, ``m``, ``kept_pairs``, ``max_count``,
        ``n_irregular`` and ``draws``.  ``status`` 1 = degenerate input, nothing was
        written (the arrays are None) and the specification decides on the host."""
        if method not in self.SPECTRAL_METHODS:
            raise ValueError(f"method must be one of {tuple(self.SPECTRAL_METHODS)}, got {method!r}")
        scores, sloc = A.inp(scores, np.float64, "scores", self.ctx.device)
        src, dst, E, loc = A.pair(src, dst, self.ctx.device)
        words = self._pcg64_words(rng)
        mask, weight, counts, inverse = (A.alloc(max(E, 1), dt, src)
                                         for dt in (np.uint8, np.float64, np.int64, np.int64))
        m, kept, mx, irr, draws = (ctypes.c_int64(0) for _ in range(5))
        status = ctypes.c_int32(1)
        self.ctx.call("gs_spectral_sample", ptr(scores), sloc, int(scores.shape[0]), ptr(src), ptr(dst),
                      loc, E, int(num_nodes), min(max(int(num_samples), 0), 1 << 31),
                      self.SPECTRAL_METHODS[method], *words,
                      ptr(mask), loc, ptr(weight), loc, ptr(counts), loc, ptr(inverse), loc,
                      ctypes.byref(m), ctypes.byref(kept), ctypes.byref(mx), ctypes.byref(irr),
                      ctypes.byref(draws), ctypes.byref(status))
        info = {"status": status.value, "m": m.value, "kept_pairs": kept.value, "max_count": mx.value,
                "n_irregular": irr.value, "draws": draws.value}
        if status.value != 0:
            return None, None, None, None, info
        return A.as_bool(mask[:E]), weight[:E], counts[:m.value], inverse[:E], info

    def sample_probs(self, scores: np.ndarray):
        """gs_sample_probs: (probs, total) of sparsify_sampled's normalisation."""
        scores, sloc = A.inp(scores, np.float64, "scores", self.ctx.device)
        p = np.empty(scores.shape[0], dtype=np.float64)
        total = ctypes.c_double(0.0)
        self.ctx.call("gs_sample_probs", ptr(scores), sloc, int(scores.shape[0]), ptr(p), GS_HOST,
                      ctypes.byref(total))
        return p, total.value

    def cumsum_ordered(self, p: np.ndarray) -> np.ndarray:
        """gs_cumsum_ordered: ``np.cumsum(p)`` (the sequential fp64 add chain)."""
        p, ploc = A.inp(p, np.float64, "p", self.ctx.device)
        out = np.empty(max(p.shape[0], 1), dtype=np.float64)
        self.ctx.call("gs_cumsum_ordered", ptr(p), ploc, int(p.shape[0]), ptr(out), GS_HOST)
        return out[:p.shape[0]]

    def topk_mask(self, scores, num_edges: int, num_keep: int, keep_lowest: bool, out=None):
        """Device mask + (cut, #beyond, #tied) -- see gs_topk_mask.  ``scores``: a
        numpy array or a CUDA float64 tensor; ``out``: an optional CUDA uint8/bool
        tensor of >= num_edges elements that receives the mask on the device (then
        returned as is) instead of a host numpy bool array."""
        scores, sloc = A.inp(scores, np.float64, "scores", self.ctx.device)
        nnz = int(scores.shape[0])
        mask, mloc = A.mask_out(out, num_edges, self.ctx.device)
        cut, nb, nt = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self.ctx.call("gs_topk_mask", ptr(scores), sloc, nnz, num_edges, num_keep,
                      int(keep_lowest), ptr(mask), mloc, ctypes.byref(cut), ctypes.byref(nb),
                      ctypes.byref(nt))
        return (mask[:num_edges].view(bool) if out is None else out), cut.value, nb.value, nt.value
