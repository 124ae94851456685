"""Inputs shared by test_sampled_host.py and test_gpu_sampled.py: the synthetic
score sets of the sampled selection, the special inputs, and the golden cases."""

import numpy as np

from conftest import golden_names, load_golden

SIZES = [1, 2, 7, 8, 9, 128, 129, 300, 65854]
RETENTIONS = [0.2, 0.5, 0.9, 0.99]
SEEDS = [0, 7, 42]
METRICS = ["jaccard", "adamic_adar", "degree", "approx_er", "feature_cosine"]
GOLDEN_RETENTIONS = (0.5, 0.2)


def synthetic_scores(E, seed):
    """Uniform scores with 40 % exact zeros (the 1e-8 floor is in play)."""
    g = np.random.default_rng(1000003 * E + seed)
    s = g.random(E)
    s[g.random(E) < 0.4] = 0.0
    return s


def nasty_scores(E=300):
    """NaN, +-inf, -0.0 and negative scores among ordinary ones."""
    s = synthetic_scores(E, 5)
    s[3::11] = np.nan
    s[4::13] = np.inf
    s[5::17] = -np.inf
    s[6::19] = -0.0
    s[7::23] = -3.5
    return s


def denormal_scores(E=64):
    """One huge score: every other probability is 1e-8 / 1e300, a denormal."""
    s = np.zeros(E)
    s[0] = 1e300
    return s


def overflow_scores():
    """A total that overflows: p becomes 0 everywhere and NumPy raises."""
    return np.array([1.7e308, 1.7e308, 1.0, 0.5])


def special_cases():
    """(label, scores, E, retention, seed) of the non-degenerate special inputs."""
    return [("nasty", nasty_scores(), 300, 0.5, 42),
            ("nasty99", nasty_scores(), 300, 0.99, 3),
            ("denormal", denormal_scores(), 64, 0.5, 42),
            ("keep0", synthetic_scores(5, 1), 5, 0.1, 42)]


def golden_cases(include_big=True):
    """(name, metric, retention, scores, E, expected mask or None when the reference raises)."""
    out = []
    for name in golden_names(include_big=include_big):
        g = load_golden(name)
        E = g["edge_index"].shape[1]
        for m in METRICS:
            for r in GOLDEN_RETENTIONS:
                if f"sampled_{m}_{r}" in g:
                    out.append((name, m, r, g[f"scores_{m}"], E, g[f"sampled_{m}_{r}"]))
                elif f"sampled_{m}_{r}_error" in g:
                    out.append((name, m, r, g[f"scores_{m}"], E, None))
    return out
