"""Score-proportional sampling on the MI355X (gs_sample_mask): the pieces against the
NumPy expressions they restate, bits equal; the mask against the reference's own
rng.choice call and the golden masks, with the device path asserted (a silent
fall-back to the host fails), the round and draw counts against
selection.sampled_mask_rounds; degenerate inputs raise as the reference does."""

import ctypes
import os

import numpy as np
import pytest
import torch

import sampled_cases as C
from conftest import PKG, bits_equal, golden_names, load_golden
from gsparse.engine import Engine
from gsparse.selection import sampled_mask, sampled_mask_device, sampled_mask_rounds

pytestmark = pytest.mark.gpu

TILE, SUB = Engine.SAMPLE_TILE, Engine.SAMPLE_SUBTREE


@pytest.fixture(scope="module")
def gs():
    import gsparse

    return gsparse


@pytest.fixture(scope="module")
def eng(gs):
    ctx = gs._lib.Context()
    ctx.set_graph_csr(2, np.array([0, 1, 2]), np.array([1, 0], dtype=np.int32), None)
    return gs.engine.Engine(ctx)


# ---- pieces ------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 12345])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 100003])
def test_pcg64_doubles(eng, n, offset):
    for seed in (42, 7):
        got = eng.pcg64_doubles(np.random.default_rng(seed), offset, n)
        want = np.random.default_rng(seed).random(offset + n)[offset:]
        assert bits_equal(got, want), (seed, n, offset)


PIECE_SIZES = sorted({1, 7, 8, 9, 128, 129, 136, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1,
                      SUB - 1, SUB, SUB + 1, 2 * SUB - 1, 2 * SUB, 2 * SUB + 1,
                      8191, 8192, 8193, 16385, 65854})


@pytest.mark.parametrize("n", PIECE_SIZES)
def test_sample_probs(eng, n):
    for s in (C.synthetic_scores(n, 1), C.nasty_scores(n) if n >= 32 else C.synthetic_scores(n, 2)):
        ref = np.maximum(np.nan_to_num(s, nan=1e-8, posinf=1e-8, neginf=1e-8), 1e-8)
        p, total = eng.sample_probs(s)
        assert total == ref.sum(), n
        assert bits_equal(p, ref / ref.sum()), n


@pytest.mark.parametrize("n", PIECE_SIZES)
def test_cumsum_ordered(eng, n):
    g = np.random.default_rng(n)
    p = g.random(n) * 10.0 ** g.integers(-12, 3, n)  # wide exponent range: every add rounds
    p[g.random(n) < 0.3] = 0.0
    p[n // 2] = 0.5
    assert bits_equal(eng.cumsum_ordered(p), np.cumsum(p)), n
    q = p / p.sum()
    assert bits_equal(eng.cumsum_ordered(q), np.cumsum(q)), n


def test_cumsum_ordered_denormals(eng):
    p = np.full(300, 5e-324)
    p[::7] = 1e-310
    assert bits_equal(eng.cumsum_ordered(p), np.cumsum(p))


# ---- end to end ----------------------------------------------------------------------
def _check_device(eng, s, E, r, seed):
    want = sampled_mask(s, E, r, seed)
    _, rounds, draws = sampled_mask_rounds(s, E, r, seed)
    info = {}
    got = sampled_mask_device(eng, s, E, r, seed, info=info)
    assert info["path"] == "device", (E, r, seed)
    assert np.array_equal(got, want), (E, r, seed)
    assert (info["rounds"], info["draws"]) == (rounds, draws), (E, r, seed)
    again = sampled_mask_device(eng, s, E, r, seed)
    assert np.array_equal(again, got), (E, r, seed)


@pytest.mark.parametrize("E", C.SIZES)
def test_device_matches_choice_synthetic(eng, E):
    for seed in C.SEEDS:
        s = C.synthetic_scores(E, seed)
        for r in C.RETENTIONS:
            _check_device(eng, s, E, r, seed)


@pytest.mark.parametrize("case", C.special_cases(), ids=lambda c: c[0])
def test_device_matches_choice_special(eng, case):
    _, s, E, r, seed = case
    _check_device(eng, s, E, r, seed)


def test_keep_zero_is_an_empty_device_mask(eng):
    s = C.synthetic_scores(5, 1)
    mask, status, rounds, draws = eng.sample_mask(s, 5, 0, np.random.default_rng(42))
    assert (status, rounds, draws) == (0, 0, 0) and mask.shape == (5,) and not mask.any()


def test_device_large(eng):
    """E = 2^20 + 3: many blocks per kernel, about 14 rounds."""
    E = (1 << 20) + 3
    _check_device(eng, C.synthetic_scores(E, 42), E, 0.6, 42)


def test_degenerate_inputs_take_the_reference_call(eng):
    with np.errstate(all="ignore"):
        for s, E in ((C.overflow_scores(), 4), (C.synthetic_scores(9, 0), 8),
                     (C.synthetic_scores(8, 0), 9)):
            with pytest.raises(ValueError) as ref:
                sampled_mask(s, E, 0.5, 42)
            info = {}
            with pytest.raises(ValueError) as got:
                sampled_mask_device(eng, s, E, 0.5, 42, info=info)
            assert info["path"] == "host"
            assert str(got.value) == str(ref.value)


# ---- through GraphSparsifier ---------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in golden_names() if any(
    c[0] == n and c[5] is not None for c in C.golden_cases())])
def test_sparsifier_sampled_matches_golden(gs, name):
    g = load_golden(name)
    data = gs.Data(edge_index=torch.from_numpy(g["edge_index"]), x=None,
                   num_nodes=int(g["num_nodes"]))
    sp_ = gs.GraphSparsifier(data, "cpu")
    seen = 0
    for m in C.METRICS:
        for r in C.GOLDEN_RETENTIONS:
            if f"sampled_{m}_{r}" not in g:
                continue
            # the golden scores stand in for the scorers (their parity is test_gpu_parity's)
            sp_._score_cache[sp_._normalize_metric_name(m)] = g[f"scores_{m}"]
            _, mk = sp_.sparsify_sampled(m, r, seed=42, return_mask=True)
            assert np.array_equal(mk.numpy(), g[f"sampled_{m}_{r}"]), (m, r)
            assert sp_.last_selection["path"] == "device", (m, r)
            assert sp_.last_selection["rounds"] >= (1 if int(len(mk) * r) else 0)
            seen += 1
    assert seen


def test_exports():
    lib = ctypes.CDLL(os.path.join(PKG, "gsparse", "libgsparse.so"))
    for name in ("gs_sample_mask", "gs_pcg64_doubles", "gs_sample_probs", "gs_cumsum_ordered"):
        assert getattr(lib, name)
