"""``src.sparsification`` drop-in (reference: src/sparsification/__init__.py)."""

from gsparse import (  # noqa: F401
    GraphSparsifier,
    calculate_adamic_adar_scores,
    calculate_approx_effective_resistance_scores,
    calculate_effective_resistance_scores,
    calculate_feature_cosine_scores,
    calculate_jaccard_scores,
    calculate_simmelian_scores,
    calculate_trussness_scores,
    compute_geodesic_preservation,
    compute_spectral_approximation,
    compute_topology_metrics,
    compute_topology_preservation,
    spectral_bounds_dense,
    precompute_random_scores,
    random_sparsify,
)

__all__ = [
    "GraphSparsifier",
    "calculate_jaccard_scores",
    "calculate_adamic_adar_scores",
    "calculate_effective_resistance_scores",
    "calculate_approx_effective_resistance_scores",
    "calculate_feature_cosine_scores",
    "calculate_trussness_scores",
    "calculate_simmelian_scores",
    "compute_geodesic_preservation",
    "compute_topology_metrics",
    "compute_topology_preservation",
    "compute_spectral_approximation",
    "spectral_bounds_dense",
    "precompute_random_scores",
    "random_sparsify",
]
