"""GraphSparsifier -- drop-in for ``src/sparsification/core.py``.

Same class name, constructor, attributes (``data, device, num_nodes,
num_edges, adj, verbose, _score_cache, SUPPORTED_METRICS,
_DISTANCE_METRICS``), methods and error behaviour as the reference
(core.py:24-490).  The canonical CSR is built on the MI355X and stays
resident there for every scorer; ``adj`` (a SciPy CSR) is materialised on
first access.  ``SparsificationEngine`` is an alias (BASELINE north_star name).

Selection semantics (core.py:229-242): the device top-k keeps exactly the
``int(E*r)`` highest (lowest) CSR-ordered scores.  Edges strictly beyond the
cut are identical to the reference by construction.  Inside a tie block at
the cut the reference's ``np.argsort`` (unstable, SIMD-dispatch dependent)
decides; ``tie_break="numpy"`` (default, the drop-in behaviour) resolves an
ambiguous tie block with that very call on the host, ``tie_break="stable"``
keeps the device rule (= ``np.argsort(kind="stable")``).
"""

from __future__ import annotations

import os
from typing import Dict, Tuple

import numpy as np
import scipy.sparse as sp
import torch

from ._lib import Context
from .data import Data
from .engine import Engine
from .metric_backbone import compute_metric_backbone
from .selection import (SPECTRAL_METHODS, connected_mask_device, degree_aware_mask_device,
                        local_mask, numpy_topk_mask, sampled_mask_device, spectral_mask_device,
                        spectral_num_samples)


def _device_index(device) -> int | None:
    s = str(device)
    if s.startswith("cuda:"):
        try:
            return int(s.split(":", 1)[1])
        except ValueError:
            return None
    return None


class GraphSparsifier:
    """Engine for graph sparsification via edge metric thresholding.

    Args:
        data: PyG ``Data`` (or ``gsparse.Data``) with ``edge_index`` [2, E].
        device: where returned graphs are placed (as in the reference).
        tie_break: "numpy" (default) or "stable", see module docstring.
        gpu: libgsparse device ordinal (default: cuda:N of ``device``,
            else $GSPARSE_DEVICE / $LOCAL_RANK / 0).
    """

    SUPPORTED_METRICS = {
        "jaccard",
        "adamic-adar",
        "adamic_adar",
        "aa",
        "effective_resistance",
        "effective-resistance",
        "er",
        "approx_effective_resistance",
        "approx_er",
        "random",
        "rand",
        "degree",
        "feature_cosine",
        "feature-cosine",
        "truss",
        "trussness",
        "simmelian",
        "simmelian_jaccard",
    }

    _DISTANCE_METRICS = {"effective_resistance", "approx_effective_resistance"}

    def __init__(self, data: Data, device: str, tie_break: str | None = None,
                 gpu: int | None = None) -> None:
        self.data = data
        self.device = device
        self.num_nodes = data.num_nodes
        self.num_edges = data.edge_index.size(1)
        self.verbose: bool = False
        self.tie_break = tie_break or os.environ.get("GSPARSE_TIE_BREAK", "numpy")
        if self.tie_break not in ("numpy", "stable"):
            raise ValueError(f"tie_break must be 'numpy' or 'stable', got {self.tie_break!r}")
        if gpu is None:
            gpu = _device_index(device)
        self._ctx = Context(gpu)
        ei = data.edge_index
        if ei.is_cuda and ei.device.index == self._ctx.device:
            src = ei[0].contiguous().to(torch.int64)
            dst = ei[1].contiguous().to(torch.int64)
        else:
            e = ei.detach().cpu().numpy().astype(np.int64, copy=False)
            src = np.ascontiguousarray(e[0])
            dst = np.ascontiguousarray(e[1])
        self._ctx.set_graph_edge_index(int(self.num_nodes), src, dst)
        self._engine = Engine(self._ctx)
        self._adj = None
        self._score_cache: Dict[str, np.ndarray] = {}
        self.last_selection: dict = {}
        self._truss_info: dict = {}  # gs_trussness' counters, kept with the cached scores
        self._simmelian_info: dict = {}  # gs_simmelian's counters of the cached score
        self._local_info: Dict[str, dict] = {}  # gs_local_scores' counters, by cache key

    # ------------------------------------------------------------------ adj
    @property
    def adj(self) -> sp.csr_matrix:
        """Canonical CSR (core.py:71-74), downloaded from the device on first use."""
        if self._adj is None:
            indptr, indices, data = self._ctx.csr()
            a = sp.csr_matrix((data, indices, indptr), shape=(self.num_nodes, self.num_nodes))
            a.has_sorted_indices = True
            self._adj = a
        return self._adj

    @adj.setter
    def adj(self, value):
        self._adj = value

    # ------------------------------------------------------------- helpers
    def _scores_to_cost(self, scores: np.ndarray, metric: str) -> np.ndarray:
        """Proximity -> distance transform of Simas et al. (core.py:82-116)."""
        metric_key = self._normalize_metric_name(metric)
        if metric_key in self._DISTANCE_METRICS:
            safe = np.maximum(scores, 1e-10)
            similarity = 1.0 / safe
        else:
            similarity = scores.copy()
        s_max = similarity.max()
        if s_max <= 0:
            return np.ones_like(scores)
        proximity = similarity / s_max
        nonzero = proximity[proximity > 0]
        floor = (nonzero.min() * 0.01) if len(nonzero) > 0 else 1e-6
        proximity[proximity <= 0] = floor
        return 1.0 / proximity - 1.0

    def _normalize_metric_name(self, metric: str) -> str:
        """core.py:118-138."""
        metric_lower = metric.lower().replace("-", "_").replace(" ", "_")
        if metric_lower in {"jaccard"}:
            return "jaccard"
        if metric_lower in {"adamic_adar", "aa"}:
            return "adamic_adar"
        if metric_lower in {"effective_resistance", "er"}:
            return "effective_resistance"
        if metric_lower in {"approx_effective_resistance", "approx_er"}:
            return "approx_effective_resistance"
        if metric_lower in {"random", "rand"}:
            return "random"
        if metric_lower in {"degree"}:
            return "degree"
        if metric_lower in {"feature_cosine"}:
            return "feature_cosine"
        if metric_lower in {"truss", "trussness"}:
            return "trussness"
        if metric_lower in {"simmelian", "simmelian_jaccard"}:
            return "simmelian"
        raise ValueError(
            f"Metric '{metric}' not supported. " f"Choose from: {self.SUPPORTED_METRICS}"
        )

    # --------------------------------------------------------------- scores
    def compute_scores(self, metric: str) -> np.ndarray:
        """Compute or retrieve cached edge scores (core.py:140-191), CSR order.

        "effective_resistance" has no size limit: up to 32768 nodes the grounded inverse is
        dense (fp64-MFMA Cholesky), above its columns come from the batched sparse CG
        (Engine.exact_er), which raises GsparseNotConverged rather than return a value
        when a solve stops at its iteration cap."""
        metric_key = self._normalize_metric_name(metric)
        if metric_key in self._score_cache:
            return self._score_cache[metric_key]
        eng = self._engine
        if metric_key == "jaccard":
            scores = eng.jaccard()
        elif metric_key == "adamic_adar":
            scores = eng.adamic_adar()
        elif metric_key == "effective_resistance":
            scores = eng.exact_er()
        elif metric_key == "approx_effective_resistance":
            scores = eng.approx_er()
        elif metric_key == "random":
            # legacy global NumPy RNG, exactly as core.py:166
            scores = np.random.rand(eng.nnz)
        elif metric_key == "degree":
            scores = eng.degree()
        elif metric_key == "feature_cosine":
            x = self.data.x if getattr(self.data, "x", None) is not None else None
            if x is None:
                raise ValueError("feature_cosine requires node features (data.x)")
            if x.is_cuda and x.device.index == self._ctx.device:
                scores = eng.feature_cosine(x)
            else:
                scores = eng.feature_cosine(x.detach().cpu().numpy())
        elif metric_key == "trussness":
            scores, self._truss_info = eng.trussness()
        elif metric_key == "simmelian":
            scores, self._simmelian_info = eng.simmelian(0)
        else:  # pragma: no cover - unreachable, mirrors core.py:186-188
            raise ValueError(f"Internal error: Unhandled metric '{metric_key}'")
        self._score_cache[metric_key] = scores
        return scores

    # ------------------------------------------------------------ selection
    def _select_mask(self, scores: np.ndarray, num_keep: int, keep_lowest: bool) -> np.ndarray:
        mask, cut, beyond, tied = self._engine.topk_mask(scores, self.num_edges, num_keep,
                                                         keep_lowest)
        need = num_keep - beyond
        ambiguous = 0 < need < tied
        self.last_selection = {"cut": cut, "beyond": beyond, "tied": tied, "need": need,
                               "ambiguous": ambiguous}
        if ambiguous and self.tie_break == "numpy":
            # The reference's unstable np.argsort orders the tie block; reproduce
            # it by making that same call (core.py:233-240).
            mask = numpy_topk_mask(scores, self.num_edges, num_keep, keep_lowest)
        return mask

    def sparsify(self, metric: str, retention_ratio: float, return_mask: bool = False,
                 keep_lowest: bool = False):
        """Keep exactly the top (bottom) ``int(E*r)`` edges by score (core.py:193-249)."""
        if not 0 < retention_ratio <= 1:
            raise ValueError(f"retention_ratio must be in (0, 1], got {retention_ratio}")
        if retention_ratio == 1.0:
            if return_mask:
                return self.data.clone(), torch.ones(self.num_edges, dtype=torch.bool)
            return self.data.clone()
        scores = self.compute_scores(metric)
        num_keep = int(self.num_edges * retention_ratio)
        mask = self._select_mask(scores, num_keep, keep_lowest)
        sparse_edge_index = self.data.edge_index[:, torch.from_numpy(mask).to(
            self.data.edge_index.device)].to(self.device)
        sparse_data = self.data.clone()
        sparse_data.edge_index = sparse_edge_index
        if return_mask:
            return sparse_data, torch.from_numpy(mask)
        return sparse_data

    def sparsify_metric_backbone(self, metric: str, epsilon: float = 1e-9):
        """Global metric backbone with costs from ``_scores_to_cost`` (core.py:251-279)."""
        distances = self._scores_to_cost(self.compute_scores(metric), metric)
        sparse_data, stats = compute_metric_backbone(
            self.data, distances, epsilon=epsilon, verbose=self.verbose, _ctx=self._ctx
        )
        return sparse_data.to(self.device), stats

    def sparsify_sampled(self, metric: str, retention_ratio: float, seed: int = 42,
                         return_mask: bool = False):
        """Score-proportional sampling without replacement (core.py:281-357).

        NumPy's ``Generator.choice`` stream defines the result: its rejection rounds
        run on the device (gs_sample_mask) and give the same mask bit for bit, with
        the reference's own call only for degenerate scores, where NumPy raises
        (SURVEY §8(f) rank 1).  ``last_selection`` records the path: ``path``
        ("device" or "host"), ``rounds`` and ``draws``."""
        if not 0 < retention_ratio <= 1:
            raise ValueError(f"retention_ratio must be in (0, 1], got {retention_ratio}")
        if retention_ratio == 1.0:
            if return_mask:
                return self.data.clone(), torch.ones(self.num_edges, dtype=torch.bool)
            return self.data.clone()
        scores = self.compute_scores(metric)
        self.last_selection = {}
        mask = sampled_mask_device(self._engine, scores, self.num_edges, retention_ratio, seed,
                                   info=self.last_selection)
        sparse_edge_index = self.data.edge_index[:, torch.from_numpy(mask).to(
            self.data.edge_index.device)].to(self.device)
        sparse_data = self.data.clone()
        sparse_data.edge_index = sparse_edge_index
        if return_mask:
            return sparse_data, torch.from_numpy(mask)
        return sparse_data

    def sparsify_degree_aware(self, metric: str, retention_ratio: float,
                              min_edges_per_node: int = 1, return_mask: bool = False):
        """Per-node minimum budget, then global fill (core.py:359-461).

        Same result as the reference's O(N*E) loops: each node's guaranteed
        columns are chosen by the same ``np.argsort`` over its incident scores,
        and the fill takes the first non-guaranteed entries of
        ``np.argsort(scores)[::-1]`` -- both on the device, with the reference's
        own calls only where its argsort order decides.
        ``last_selection`` records the path: ``phase1`` ("device", or "host" for
        ``min_edges_per_node < 1`` or NaN scores) and ``n_ambiguous``."""
        if not 0 < retention_ratio <= 1:
            raise ValueError(f"retention_ratio must be in (0, 1], got {retention_ratio}")
        if retention_ratio == 1.0:
            if return_mask:
                return self.data.clone(), torch.ones(self.num_edges, dtype=torch.bool)
            return self.data.clone()
        scores = self.compute_scores(metric)
        self.last_selection = {}
        mask = degree_aware_mask_device(self._engine, scores, self.data.edge_index.cpu().numpy(),
                                        self.num_nodes, self.num_edges, retention_ratio,
                                        min_edges_per_node, info=self.last_selection)
        sparse_edge_index = self.data.edge_index[:, torch.from_numpy(mask).to(
            self.data.edge_index.device)].to(self.device)
        sparse_data = self.data.clone()
        sparse_data.edge_index = sparse_edge_index
        if return_mask:
            return sparse_data, torch.from_numpy(mask)
        return sparse_data

    def sparsify_connected(self, metric: str, retention_ratio: float, return_mask: bool = False,
                           keep_lowest: bool = False):
        """Top-k with a retention budget that cannot change the component structure: the
        maximum spanning forest under the scores is kept first, in both directions, and
        the rest of ``int(E*r)`` is spent on the best other columns (not in the
        reference).  The order is the stable one -- (score, index), a strict total order
        -- so the result is unique and ``tie_break`` is not consulted.  When the forest
        alone is over the budget it is kept whole (as ``sparsify_degree_aware`` keeps its
        guarantees).  One score per ``edge_index`` column is needed: ValueError when the
        canonical CSR merged duplicate columns.

        ``last_selection`` records ``path``, ``forest`` (columns of the forest),
        ``guaranteed`` (with reverse directions and duplicates), ``rounds``,
        ``over_budget`` and the fill's ``cut`` / ``beyond`` / ``tied``."""
        if not 0 < retention_ratio <= 1:
            raise ValueError(f"retention_ratio must be in (0, 1], got {retention_ratio}")
        if retention_ratio == 1.0:
            if return_mask:
                return self.data.clone(), torch.ones(self.num_edges, dtype=torch.bool)
            return self.data.clone()
        scores = self.compute_scores(metric)
        self.last_selection = {}
        mask = connected_mask_device(self._engine, scores, self.data.edge_index.cpu().numpy(),
                                     self.num_nodes, self.num_edges, retention_ratio, keep_lowest,
                                     info=self.last_selection)
        sparse_edge_index = self.data.edge_index[:, torch.from_numpy(mask).to(
            self.data.edge_index.device)].to(self.device)
        sparse_data = self.data.clone()
        sparse_data.edge_index = sparse_edge_index
        if return_mask:
            return sparse_data, torch.from_numpy(mask)
        return sparse_data

    def sparsify_spectral(self, metric: str = "approx_er", num_samples: int | None = None,
                          retention_ratio: float | None = None, seed: int = 42,
                          method: str = "multinomial", return_mask: bool = False):
        """Spectral sparsification by effective-resistance sampling (Spielman-Srivastava;
        not in the reference): ``q`` draws with replacement over the undirected pairs with
        probability proportional to the pair's score, and every kept pair reweighted by
        ``count / (q p)``, so the weighted subgraph's Laplacian is an unbiased estimate of
        the whole graph's.  The ``(1 +- eps)`` guarantee holds for the two effective
        resistance metrics ("approx_er", "effective_resistance"); any other metric is
        accepted and gives an unbiased, reweighted sample without that guarantee.

        Exactly one of ``num_samples`` (``q`` itself) and ``retention_ratio`` (in (0, 1]:
        ``q = max(1, int(m * ratio))`` over the ``m`` undirected pairs) is given.
        ``method``: "multinomial" (at most ``q`` pairs survive) or "independent" (every
        pair kept on its own with probability ``min(1, q p)``, no cumsum: the form for
        very large graphs).  ``selection.spectral_sample`` defines the result; it is
        drawn on the device (gs_spectral_sample), bit for bit.  One score per
        ``edge_index`` column is needed -- ValueError when the canonical CSR merged
        duplicate columns -- and every non-loop pair must have exactly its two columns:
        ValueError otherwise (the weighted graph would not be symmetric).

        The returned ``Data`` has ``edge_index[:, mask]`` and ``edge_weight`` (float32) on
        ``self.device``; with ``return_mask`` also ``(mask, weight)``, a bool and a float64
        tensor of length E.  ``last_selection`` records ``path``, ``method``, ``m``,
        ``num_samples``, ``kept_pairs``, ``max_count``, ``draws`` and ``n_irregular``."""
        spectral_num_samples(num_samples, retention_ratio)
        if method not in SPECTRAL_METHODS:
            raise ValueError(f"method must be one of {SPECTRAL_METHODS}, got {method!r}")
        scores = self.compute_scores(metric)
        if len(scores) < self.num_edges:
            raise ValueError(f"{len(scores)} scores for {self.num_edges} columns: the canonical CSR "
                             "merged duplicate columns, one score per edge_index column is needed")
        ei = self.data.edge_index
        if ei.is_cuda and ei.device.index == self._ctx.device:
            ids = ei.to(torch.int64)
        else:
            ids = ei.detach().cpu().numpy().astype(np.int64, copy=False)
        if num_samples is None:
            _, m, status = self._engine.undirected_ids(ids[0], ids[1], self.num_nodes)
            if status != 0:  # outside the device contract: the reference's own lines
                e = ei.detach().cpu().numpy().astype(np.int64, copy=False)
                keys = np.minimum(e[0], e[1]) * (self.num_nodes + 1) + np.maximum(e[0], e[1])
                m = len(np.unique(keys))
            num_samples = spectral_num_samples(None, retention_ratio, m)
        self.last_selection = {}
        mask, weight, _, _ = spectral_mask_device(self._engine, scores, ids, self.num_nodes,
                                                  num_samples, seed, method, info=self.last_selection)
        if self.last_selection["n_irregular"] > 0:
            raise ValueError(f"{self.last_selection['n_irregular']} undirected pairs do not have "
                             "exactly two edge_index columns (one direction only, or duplicates): "
                             "the weighted graph would not be symmetric")
        if isinstance(mask, np.ndarray):
            mask, weight = torch.from_numpy(mask), torch.from_numpy(weight)
        sparse_data = self.data.clone()
        sparse_data.edge_index = ei[:, mask.to(ei.device)].to(self.device)
        sparse_data.edge_weight = weight[mask].to(torch.float32).to(self.device)
        if return_mask:
            return sparse_data, (mask.cpu(), weight.cpu())
        return sparse_data

    def sparsify_truss(self, k: int, return_mask: bool = False):
        """Keep exactly the k-truss (not in the reference): the columns whose trussness
        (``compute_scores("truss")``, gs_trussness on the device) is ``>= k``, i.e. the
        largest subgraph in which every edge lies in at least ``k - 2`` triangles.  ``k`` is
        an integer ``>= 2`` (ValueError otherwise); ``k = 2`` keeps every column but the
        self-loops, which score 0 and are always dropped.  One score per ``edge_index``
        column is needed: ValueError when the canonical CSR merged duplicate columns.

        ``last_selection`` records ``path``, ``k``, ``kept``, ``max_truss``, ``levels`` and
        ``rounds`` (the peel's levels and sub-rounds)."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 2:
            raise ValueError(f"k must be an integer >= 2, got {k!r}")
        scores = self.compute_scores("trussness")
        if len(scores) != self.num_edges:
            raise ValueError(f"{len(scores)} scores for {self.num_edges} columns: the canonical CSR "
                             "merged duplicate columns, one score per edge_index column is needed")
        mask = np.asarray(scores) >= int(k)
        info = self._truss_info
        self.last_selection = {"path": "device", "k": int(k), "kept": int(mask.sum()),
                               "max_truss": info.get("max_truss"), "levels": info.get("levels"),
                               "rounds": info.get("rounds")}
        sparse_edge_index = self.data.edge_index[:, torch.from_numpy(mask).to(
            self.data.edge_index.device)].to(self.device)
        sparse_data = self.data.clone()
        sparse_data.edge_index = sparse_edge_index
        if return_mask:
            return sparse_data, torch.from_numpy(mask)
        return sparse_data

    def simmelian_overlap(self, max_rank: int) -> np.ndarray:
        """The parametric Simmelian overlap of every CSR entry (not in the reference;
        ``selection.simmelian_host(..., max_rank)`` on the device, gs_simmelian): the number
        of neighbours that both ends of the edge rank below ``max_rank`` by the triangles
        through the tie, ties sharing a rank.  ``max_rank`` is an integer ``>= 1``
        (ValueError otherwise).  Cached per rank."""
        if isinstance(max_rank, bool) or not isinstance(max_rank, (int, np.integer)) or max_rank < 1:
            raise ValueError(f"max_rank must be an integer >= 1, got {max_rank!r}")
        key = f"simmelian_overlap:{int(max_rank)}"
        if key not in self._score_cache:
            self._score_cache[key], info = self._engine.simmelian(int(max_rank))
            self._simmelian_info = self._simmelian_info or info
        return self._score_cache[key]

    def sparsify_simmelian(self, retention_ratio: float | None = None, threshold: float | None = None,
                           max_rank: int | None = None, min_overlap: int | None = None,
                           return_mask: bool = False):
        """The Simmelian backbone (Nick et al., ASONAM 2013; NetworKit's Simmelian
        sparsifiers; not in the reference): an edge is kept when its two ends agree on who
        their strongest ties are -- the sparsifier that separates communities in dense,
        noisy graphs.  Exactly one mode is given (ValueError otherwise):

        ``retention_ratio`` in (0, 1]: the ``int(E * r)`` highest non-parametric scores
        (``compute_scores("simmelian")``), the same cut, ``tie_break`` handling and 1.0
        shortcut as ``sparsify``.  ``threshold``: the columns with score ``>= threshold``.
        ``max_rank`` with ``min_overlap`` (integers ``>= 1``): the columns whose ends share
        at least ``min_overlap`` of their neighbours of rank below ``max_rank``
        (``simmelian_overlap``), NetworKit's parametric form.

        One score per ``edge_index`` column is needed: ValueError when the canonical CSR
        merged duplicate columns.  ``last_selection`` records ``path``, ``mode`` ("ratio",
        "threshold" or "overlap"), ``kept``, ``max_common`` and ``classes``."""
        modes = (retention_ratio is not None, threshold is not None,
                 max_rank is not None or min_overlap is not None)
        if sum(modes) != 1:
            raise ValueError("give exactly one of retention_ratio, threshold, and max_rank with min_overlap")
        if modes[0] and not 0 < retention_ratio <= 1:
            raise ValueError(f"retention_ratio must be in (0, 1], got {retention_ratio}")
        if modes[1] and not (isinstance(threshold, (int, float, np.integer, np.floating))
                             and not isinstance(threshold, bool) and threshold == threshold):
            raise ValueError(f"threshold must be a number, got {threshold!r}")
        if modes[2]:
            for name, v in (("max_rank", max_rank), ("min_overlap", min_overlap)):
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                    raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
        if retention_ratio == 1.0:
            if return_mask:
                return self.data.clone(), torch.ones(self.num_edges, dtype=torch.bool)
            return self.data.clone()
        scores = self.simmelian_overlap(max_rank) if modes[2] else self.compute_scores("simmelian")
        if len(scores) != self.num_edges:
            raise ValueError(f"{len(scores)} scores for {self.num_edges} columns: the canonical CSR "
                             "merged duplicate columns, one score per edge_index column is needed")
        if modes[0]:
            mask = self._select_mask(scores, int(self.num_edges * retention_ratio), False)
        elif modes[1]:
            mask = np.asarray(scores) >= threshold
        else:
            mask = np.asarray(scores) >= int(min_overlap)
        info = self._simmelian_info
        self.last_selection = {"path": "device", "mode": ("ratio", "threshold", "overlap")[modes.index(True)],
                               "kept": int(mask.sum()), "max_common": info.get("max_common"),
                               "classes": info.get("classes")}
        sparse_edge_index = self.data.edge_index[:, torch.from_numpy(mask).to(
            self.data.edge_index.device)].to(self.device)
        sparse_data = self.data.clone()
        sparse_data.edge_index = sparse_edge_index
        if return_mask:
            return sparse_data, torch.from_numpy(mask)
        return sparse_data

    def compute_local_scores(self, metric: str, keep_lowest: bool = False) -> np.ndarray:
        """The local-filter score of every ``edge_index`` column under ``metric`` (not in
        the reference; ``selection.local_filter_scores`` is the specification, computed on
        the device by gs_segment_rank and gs_local_scores, bit for bit): every node ranks
        its own columns by ``compute_scores(metric)``, and a column scores ``1 - x`` with
        ``x`` the smallest exponent at which either end keeps it, ``rank + 1 <= d ** x``.
        Any exponent or retention ratio of ``sparsify_local`` is then a threshold or a
        top-k over this one array: a sweep costs one ranking.  Cached like the metrics'
        scores.  One score per ``edge_index`` column is needed: ValueError when the
        canonical CSR merged duplicate columns."""
        metric_key = self._normalize_metric_name(metric)
        key = f"local:{metric_key}:{'lowest' if keep_lowest else 'highest'}"
        if key in self._score_cache:
            return self._score_cache[key]
        scores = self.compute_scores(metric)
        if len(scores) != self.num_edges:
            raise ValueError(f"{len(scores)} scores for {self.num_edges} columns: the canonical CSR "
                             "merged duplicate columns, one score per edge_index column is needed")
        ei = self.data.edge_index
        if ei.is_cuda and ei.device.index == self._ctx.device:
            ids = ei.to(torch.int64)
        else:
            ids = ei.detach().cpu().numpy().astype(np.int64, copy=False)
        local, self._local_info[key] = self._engine.local_scores(
            scores, ids[0], ids[1], self.num_nodes, keep_lowest, out=np.empty(self.num_edges))
        self._score_cache[key] = local
        return local

    def sparsify_local(self, metric: str, exponent: float | None = None,
                       retention_ratio: float | None = None, keep_lowest: bool = False,
                       return_mask: bool = False):
        """Local sparsification (L-Spar, Satuluri et al.; Local Degree / Local Similarity,
        Hamann et al.; not in the reference): every node keeps its best edges by its own
        ranking of ``metric``, so sparse regions are not stripped bare as a global cut of a
        similarity score strips them.  Exactly one of ``exponent`` and ``retention_ratio``
        is given (ValueError otherwise).

        ``exponent`` in [0, 1]: node ``u`` keeps its ``ceil(d_u ** exponent)`` best columns
        and a column survives when either end keeps its pair -- ``selection.local_mask`` of
        ``compute_local_scores``; the kept count is whatever results (1 keeps everything, 0
        every node's best edge in both directions).  ``retention_ratio`` in (0, 1]: the
        ``int(E * r)`` highest local scores, the same cut, ``tie_break`` handling and 1.0
        shortcut as ``sparsify``.

        ``last_selection`` records ``path``, ``mode`` ("exponent" or "ratio"), ``exponent``
        (None in ratio mode), ``kept``, ``n_top``, ``max_degree`` and ``classes``; in ratio
        mode also the cut's ``cut`` / ``beyond`` / ``tied``."""
        if (exponent is None) == (retention_ratio is None):
            raise ValueError("exactly one of exponent and retention_ratio must be given")
        if exponent is not None and not 0 <= exponent <= 1:
            raise ValueError(f"exponent must be in [0, 1], got {exponent}")
        if retention_ratio is not None and not 0 < retention_ratio <= 1:
            raise ValueError(f"retention_ratio must be in (0, 1], got {retention_ratio}")
        if retention_ratio == 1.0:
            if return_mask:
                return self.data.clone(), torch.ones(self.num_edges, dtype=torch.bool)
            return self.data.clone()
        local = self.compute_local_scores(metric, keep_lowest)
        metric_key = self._normalize_metric_name(metric)
        f = self._local_info[f"local:{metric_key}:{'lowest' if keep_lowest else 'highest'}"]
        if exponent is not None:
            mask = local_mask(local, exponent)
            cut = {}
        else:
            mask = self._select_mask(local, int(self.num_edges * retention_ratio), False)
            cut = {k: self.last_selection[k] for k in ("cut", "beyond", "tied")}
        self.last_selection = {"path": "device", "mode": "exponent" if exponent is not None else "ratio",
                               "exponent": None if exponent is None else float(exponent),
                               "kept": int(mask.sum()), "n_top": f["n_top"],
                               "max_degree": f["max_degree"], "classes": f["classes"], **cut}
        sparse_edge_index = self.data.edge_index[:, torch.from_numpy(mask).to(
            self.data.edge_index.device)].to(self.device)
        sparse_data = self.data.clone()
        sparse_data.edge_index = sparse_edge_index
        if return_mask:
            return sparse_data, torch.from_numpy(mask)
        return sparse_data

    def spectral_approximation(self, sparse, edge_weight=None, **caps) -> dict:
        """How well a sparsifier of this graph approximates it spectrally (not in the
        reference): ``metrics.compute_spectral_approximation`` of this graph's adjacency
        and the sparsifier's, i.e. ``lambda_min``, ``lambda_max`` and ``epsilon`` of
        ``(1 - epsilon) L_G <= L_H <= (1 + epsilon) L_G`` on the largest component.

        ``sparse``: a ``Data`` returned by any ``sparsify_*`` method, or the ``(mask,
        weight)`` pair ``sparsify_spectral(..., return_mask=True)`` returns (one entry per
        ``edge_index`` column of this graph).  The weights are ``edge_weight`` when given
        (one per column of ``sparse``), else ``Data.edge_weight`` when present, else 1.
        Columns listing the same ordered pair add up, as they do in this graph's own
        adjacency.  ``caps``: ``tol``, ``max_iter``, ``cg_rtol``, ``cg_max_iter``."""
        from .metrics import compute_spectral_approximation

        def host(t, dtype):
            return np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=dtype)

        if isinstance(sparse, (tuple, list)):
            mask, weight = sparse
            mask = host(mask, bool)
            ei = host(self.data.edge_index, np.int64)[:, mask]
            w = host(weight, np.float64)[mask]
        else:
            ei = host(sparse.edge_index, np.int64)
            w = getattr(sparse, "edge_weight", None)
            w = np.ones(ei.shape[1]) if w is None else host(w, np.float64)
        if edge_weight is not None:
            w = host(edge_weight, np.float64)
        if w.shape != (ei.shape[1],):
            raise ValueError(f"{w.shape} weights for {ei.shape[1]} columns")
        n = self.num_nodes
        sparse_adj = sp.csr_matrix((w, (ei[0], ei[1])), shape=(n, n))
        sparse_adj.sum_duplicates()
        return compute_spectral_approximation(self.adj, sparse_adj, **caps)

    def get_retention_curve_data(self, metric: str, retention_rates: list[float]) -> list[Data]:
        """core.py:463-480."""
        return [self.sparsify(metric, rate) for rate in retention_rates]

    @property
    def stats(self) -> dict:
        """core.py:482-490."""
        return {
            "num_nodes": self.num_nodes,
            "num_edges": self.num_edges,
            "density": self.num_edges / (self.num_nodes * (self.num_nodes - 1)),
            "avg_degree": self.num_edges / self.num_nodes,
        }


SparsificationEngine = GraphSparsifier
