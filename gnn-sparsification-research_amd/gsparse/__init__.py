"""gsparse -- MI355X-native graph-sparsification edge scoring.

Drop-in for the reference's ``src/sparsification`` package: the same public
names, backed by libgsparse.so (hand-written HIP for gfx950).  Importing the
package does not touch the GPU; the first scorer call does, and fails loudly
(``GsparseUnavailable``) when the HIP library or device is missing.
"""

from ._lib import GsparseError, GsparseNotConverged, GsparseUnavailable
from .core import GraphSparsifier, SparsificationEngine
from .data import Data
from .metric_backbone import compute_metric_backbone
from .metrics import (
    calculate_adamic_adar_scores,
    calculate_approx_effective_resistance_scores,
    calculate_effective_resistance_scores,
    calculate_feature_cosine_scores,
    calculate_jaccard_scores,
    calculate_local_filter_scores,
    calculate_simmelian_scores,
    calculate_trussness_scores,
    compute_geodesic_preservation,
    compute_spectral_approximation,
    compute_topology_metrics,
    compute_topology_preservation,
    spectral_bounds_dense,
)
from .random import RandomBaseline, precompute_random_scores, random_sparsify
from .selection import local_filter_scores, local_mask, spectral_sample

__all__ = [
    "GraphSparsifier",
    "SparsificationEngine",
    "Data",
    "GsparseError",
    "GsparseNotConverged",
    "GsparseUnavailable",
    "compute_metric_backbone",
    "calculate_jaccard_scores",
    "calculate_adamic_adar_scores",
    "calculate_effective_resistance_scores",
    "calculate_approx_effective_resistance_scores",
    "calculate_feature_cosine_scores",
    "calculate_trussness_scores",
    "calculate_simmelian_scores",
    "calculate_local_filter_scores",
    "compute_geodesic_preservation",
    "compute_topology_metrics",
    "compute_topology_preservation",
    "compute_spectral_approximation",
    "spectral_bounds_dense",
    "precompute_random_scores",
    "random_sparsify",
    "RandomBaseline",
    "spectral_sample",
    "local_filter_scores",
    "local_mask",
]
