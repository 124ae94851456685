"""The ApproxER solver plan (gs_er_plan -> cg_plan, csrc/gs_cg.hpp), no GPU.

The default plan -- which solver a solve takes, columns per lane, chain rows per trip,
BLAS chunks -- is what the benchmark runs; the GPU parity tests force the mode, so
this table is what pins the default selection.  The expected values restate the rules
by hand (make_chunks, columns per lane, the mode chain, rows per trip, the register-
resident solver's geometry) and were confirmed against the code before the plan was
split out of gs_er_solve.
"""

import os
import subprocess

import pytest

from conftest import PKG

LIB = os.path.join(PKG, "gsparse", "libgsparse.so")
ROMAN = (22662, 88516, 2674)  # n, entries of L_reg, JL columns of the flagship workload


@pytest.fixture
def plan(monkeypatch):
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    for name in list(os.environ):
        if name.startswith(("GSPARSE_CG_", "GSPARSE_RES_", "GSPARSE_REG_")):
            monkeypatch.delenv(name)
    from gsparse import engine

    return engine.er_plan


# n, lnnz, ncols, threads -> mode, cpl, ru, chunks (None: not asserted)
DEFAULTS = [
    ((22662, 88516, 2674, 8), (5, 2, 1, 8)),
    ((22662, 88516, 334, 8), (5, 1, 4, 8)),
    ((22662, 88516, 2674, 3), (0, 1, 2, 3)),
    ((20000, 60000, 1000, 4), (5, 1, 2, 4)),
    ((24576, 73728, 1000, 16), (4, None, None, 16)),
    ((24576, 73728, 1000, 8), (4, None, None, 8)),
    ((24577, 73731, 2048, 8), (0, 2, 1, 8)),
    ((24577, 73731, 2047, 8), (1, 2, 1, 8)),
    ((24577, 73731, 511, 8), (3, 1, 2, 8)),
    ((169343, 2484941, 1024, 8), (3, 1, 1, 8)),
    ((10000, 30000, 4096, 8), (0, 1, 2, 1)),
]


@pytest.mark.parametrize("args,want", DEFAULTS, ids=["-".join(map(str, a)) for a, _ in DEFAULTS])
def test_default_plan(plan, args, want):
    got = plan(*args)
    for key, w in zip(("mode", "cpl", "ru", "chunks"), want):
        if w is not None:
            assert got[key] == w, (key, got)


def test_mode_out_of_range_is_mode_0(plan, monkeypatch):
    monkeypatch.setenv("GSPARSE_CG_MODE", "9")
    assert plan(*ROMAN, 8)["mode"] == 0


def test_mode_5_falls_back_to_4_where_it_does_not_apply(plan, monkeypatch):
    monkeypatch.setenv("GSPARSE_CG_MODE", "5")
    assert plan(24576, 73728, 1000, 16)["mode"] == 4
    assert plan(*ROMAN, 8)["mode"] == 5


def test_storeq_is_applied_after_mode(plan, monkeypatch):
    monkeypatch.setenv("GSPARSE_CG_MODE", "3")
    monkeypatch.setenv("GSPARSE_CG_STOREQ", "0")
    assert plan(*ROMAN, 8)["mode"] == 0


def test_narrow_form_is_not_a_default(plan, monkeypatch):
    """With only the 256-thread form allowed the default is the resident solver: the
    default chain takes the register-resident one for its 512-thread form alone."""
    monkeypatch.setenv("GSPARSE_REG_NT", "256")
    assert plan(*ROMAN, 8)["mode"] == 4


def test_more_than_64_threads_plan_as_64(plan):
    assert plan(*ROMAN, 200) == plan(*ROMAN, 64)
    assert plan(*ROMAN, 200)["chunks"] == 64
