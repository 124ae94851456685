"""The batch plan of the sparse exact effective resistance (gs_xer_sparse_plan ->
xer_sparse_plan, csrc/gs_xer_sparse.hip), no GPU: B is a multiple of 64, the four
n x B fp64 blocks stay inside the byte budget, GSPARSE_XER_BATCH is honoured and clamped,
and the reductions' row chunks are a function of n alone."""

import os
import subprocess

import pytest

from conftest import PKG

LIB = os.path.join(PKG, "gsparse", "libgsparse.so")
SIZES = [1, 2, 63, 64, 65, 70, 300, 2000, 2708, 32768, 32769, 40_229, 70_002, 169_343, 1_000_000,
         2_999_999, 3_000_000]


@pytest.fixture
def plan(monkeypatch):
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    monkeypatch.delenv("GSPARSE_XER_BATCH", raising=False)
    from gsparse import engine

    return engine.xer_sparse_plan


@pytest.mark.parametrize("cus", [0, 64, 256, 304])
def test_batch_is_a_multiple_of_64_inside_the_budget(plan, cus):
    for n in SIZES + list(range(1, 3_000_001, 99_991)):
        p = plan(n, cus)
        B = p["batch"]
        assert B >= 64 and B % 64 == 0, (n, p)
        assert 4 * n * B * 8 <= p["budget_bytes"], (n, p)
        assert B <= max(256, 64 * -(-8 * (cus or 256) // n)), (n, p)  # the default or the CU fill
        assert B <= max(64, -(-n // 64) * 64), (n, p)                  # no wider than the graph


def test_default_and_fill(plan):
    assert plan(169_343)["batch"] == 256 and plan(40_229)["batch"] == 256
    assert plan(70)["batch"] == 128 and plan(64)["batch"] == 64
    assert plan(2000)["batch"] == 256 and plan(2000, 1024)["batch"] == 320
    assert plan(3_000_000)["batch"] == 64  # the budget: 8 GiB / (32 B x 3 M rows) = 89 columns
    assert plan(1_000_000)["batch"] == 256 and plan(2_000_000)["batch"] == 128


@pytest.mark.parametrize("text,want", [("64", 64), ("128", 128), ("100", 64), ("1", 64),
                                       ("1000", 960), ("1024", 1024), ("5000", 1024),
                                       ("0", None), ("-64", None), ("abc", None)])
def test_override_is_honoured_and_clamped(plan, monkeypatch, text, want):
    default = plan(40_229)["batch"]
    monkeypatch.setenv("GSPARSE_XER_BATCH", text)
    assert plan(40_229)["batch"] == (default if want is None else want)
    # the budget clamps the override too
    p = plan(3_000_000)
    assert p["batch"] == 64 and 4 * 3_000_000 * 64 * 8 <= p["budget_bytes"]


def test_chunks_depend_on_n_alone(plan, monkeypatch):
    for n in SIZES:
        base = plan(n)
        assert 1 <= base["chunks"] <= 128 and base["chunk_rows"] % 4 == 0
        assert (base["chunks"] - 1) * base["chunk_rows"] < n <= base["chunks"] * base["chunk_rows"]
        for text in ("64", "512"):
            monkeypatch.setenv("GSPARSE_XER_BATCH", text)
            for cus in (0, 64):
                p = plan(n, cus)
                assert (p["chunks"], p["chunk_rows"]) == (base["chunks"], base["chunk_rows"])
        monkeypatch.delenv("GSPARSE_XER_BATCH")
