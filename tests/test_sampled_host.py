"""Score-proportional sampling without a GPU: selection.sampled_mask_rounds (the
executable specification of gs_sample_mask) equals the reference's rng.choice call,
and the device sampler's per-element logic (csrc/gs_sample.hpp), compiled for the
host by tools/sample_host_check.cpp, gives the same mask, rounds and draws."""

import os
import re
import subprocess

import numpy as np
import pytest

import sampled_cases as C
from conftest import PKG, ROOT
from gsparse.selection import sampled_mask, sampled_mask_rounds


@pytest.mark.parametrize("case", C.golden_cases(), ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_rounds_match_golden(case):
    name, m, r, scores, E, want = case
    if want is None:
        with pytest.raises(ValueError):
            sampled_mask_rounds(scores, E, r, 42)
        return
    mask, rounds, draws = sampled_mask_rounds(scores, E, r, 42)
    assert np.array_equal(mask, want)
    assert np.array_equal(mask, sampled_mask(scores, E, r, 42))
    assert draws >= int(E * r) and (rounds >= 1) == (int(E * r) >= 1)


@pytest.mark.parametrize("E", C.SIZES)
def test_rounds_match_choice_synthetic(E):
    for seed in C.SEEDS:
        s = C.synthetic_scores(E, seed)
        for r in C.RETENTIONS:
            mask, rounds, draws = sampled_mask_rounds(s, E, r, seed)
            assert np.array_equal(mask, sampled_mask(s, E, r, seed)), (E, r, seed)
            assert int(mask.sum()) == int(E * r) <= draws


@pytest.mark.parametrize("case", C.special_cases(), ids=lambda c: c[0])
def test_rounds_match_choice_special(case):
    _, s, E, r, seed = case
    mask, rounds, draws = sampled_mask_rounds(s, E, r, seed)
    assert np.array_equal(mask, sampled_mask(s, E, r, seed))
    assert (rounds == 0) == (int(E * r) == 0)


def test_rounds_degenerate_raise_like_the_reference():
    with np.errstate(all="ignore"):
        for s, E in ((C.overflow_scores(), 4), (C.synthetic_scores(9, 0), 8)):
            with pytest.raises(ValueError):
                sampled_mask(s, E, 0.5, 42)
            with pytest.raises(ValueError):
                sampled_mask_rounds(s, E, 0.5, 42)


def test_engine_constants_match_header():
    from gsparse.engine import Engine

    text = open(os.path.join(ROOT, "include", "gsparse.h")).read()
    tile = int(re.search(r"GS_SAMPLE_TILE\s*=\s*(\d+)", text).group(1))
    sub = int(re.search(r"GS_SAMPLE_SUBTREE\s*=\s*(\d+)", text).group(1))
    assert (Engine.SAMPLE_TILE, Engine.SAMPLE_SUBTREE) == (tile, sub)


# ---- the device logic compiled for the host ----------------------------------------
@pytest.fixture(scope="module")
def sample_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("smp")
    exe = str(d / "sample_check")
    src = os.path.join(ROOT, "tools", "sample_host_check.cpp")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-ffp-contract=off", src, "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("hipcc host build unavailable: " + r.stderr[-300:])

    def run(scores, E, num_keep, seed):
        st = np.random.default_rng(seed).bit_generator.state["state"]
        s, inc = st["state"], st["inc"]
        m64 = (1 << 64) - 1
        path = str(d / "scores.bin")
        np.ascontiguousarray(scores, dtype=np.float64).tofile(path)
        out = subprocess.run([exe, f"{s >> 64:x}", f"{s & m64:x}", f"{inc >> 64:x}", f"{inc & m64:x}",
                              str(E), str(num_keep), path], capture_output=True, check=True).stdout
        status, rounds, draws = (int(v) for v in np.frombuffer(out[:24], dtype=np.int64))
        total = float(np.frombuffer(out[24:32], dtype=np.float64)[0])
        mask = np.frombuffer(out[32:], dtype=np.uint8).astype(bool) if status == 0 else None
        return status, rounds, draws, total, mask

    return run


def _check_host(run, s, E, r, seed):
    want, rounds, draws = sampled_mask_rounds(s, E, r, seed)
    status, hr, hd, total, mask = run(s, E, int(E * r), seed)
    assert status == 0, (E, r, seed)
    assert np.array_equal(mask, want), (E, r, seed)
    assert (hr, hd) == (rounds, draws), (E, r, seed)
    probs = np.maximum(np.nan_to_num(s, nan=1e-8, posinf=1e-8, neginf=1e-8), 1e-8)
    assert total == probs.sum()  # the cut, blocked pairwise tree is np.sum's


@pytest.mark.parametrize("E", C.SIZES)
def test_host_program_synthetic(sample_check, E):
    for seed in C.SEEDS:
        s = C.synthetic_scores(E, seed)
        for r in C.RETENTIONS:
            _check_host(sample_check, s, E, r, seed)


@pytest.mark.parametrize("case", C.special_cases(), ids=lambda c: c[0])
def test_host_program_special(sample_check, case):
    _, s, E, r, seed = case
    _check_host(sample_check, s, E, r, seed)


@pytest.mark.parametrize("E", [2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 10007,
                               16385])
def test_host_program_total_around_the_subtree_size(sample_check, E):
    """Sizes around GS_SAMPLE_SUBTREE, where a block's tree gains a level of subtrees, and
    around np.sum's 8192-element blocks."""
    _check_host(sample_check, C.synthetic_scores(E, 3), E, 0.5, 3)


def test_host_program_gate(sample_check):
    """Status 1 where NumPy raises: an overflowing total, and the goldens whose scores
    are not one per edge_index column (their sampled_*_error keys)."""
    assert sample_check(C.overflow_scores(), 4, 2, 42)[0] == 1
    errors = [c for c in C.golden_cases() if c[5] is None]
    assert errors
    for name, m, r, scores, E, _ in errors:
        assert sample_check(scores, E, int(E * r), 42)[0] == 1, (name, m, r)
