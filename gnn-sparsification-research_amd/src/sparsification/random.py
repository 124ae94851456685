"""``src.sparsification.random`` drop-in (reference random.py)."""

from gsparse.random import RandomBaseline, precompute_random_scores, random_sparsify  # noqa: F401
