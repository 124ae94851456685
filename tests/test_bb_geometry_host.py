"""The metric backbone's geometry (gs_bb_geometry -> bb_geometry, csrc/gs_backbone.hip), no GPU.

The defaults -- landmarks and how their searches run, sources per workgroup, threads,
batches, slabs -- are what the benchmark runs; the GPU tests force the knobs, so this
table is what pins the default selection.  The expected values restate the rules by
hand (K and the 65,536-node size class, the landmarks of a rank and their workgroups,
S by rank count, the slab limit and its 48 GB cap) and were confirmed against the code
before the rules were moved out of bb_begin and bb_plan.
"""

import os
import subprocess

import pytest

from conftest import PKG

LIB = os.path.join(PKG, "gsparse", "libgsparse.so")
KEYS = ("K", "lm_coop", "lm_W", "S", "threads", "nbatch", "slabs")


@pytest.fixture
def geometry(monkeypatch):
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    for name in list(os.environ):
        if name.startswith("GSPARSE_BB_"):
            monkeypatch.delenv(name)
    from gsparse import engine

    return engine.bb_geometry


# n, nsrc, nranks, lpart -> K, coop, W, S, threads, nbatch, slabs (None: not asserted)
DEFAULTS = [
    ((22662, 5000, 1, 0), (16, 0, None, 1, 256, 5000, 1024)),
    ((65536, 5000, 1, 0), (16, 0, None, 1, 256, 5000, 1024)),
    ((65537, 5000, 1, 0), (48, 1, 11, 16, 512, 313, 313)),
    ((262144, 100000, 1, 0), (48, 1, 11, 16, 512, 6250, 512)),
    ((262144, 100000, 2, 0), (48, 1, 22, 8, 512, 12500, 512)),
    ((262144, 100000, 4, 3), (48, 1, 43, 8, 512, 12500, 512)),
    ((262144, 100000, 8, 0), (48, 1, 86, 2, 1024, 50000, 256)),
    ((262144, 100000, 48, 0), (48, 1, 256, 2, 1024, 50000, 256)),
    ((4194304, 1000000, 1, 0), (48, 1, 11, 16, 512, 62500, 73)),  # the 48 GB cap binds
    ((10, 3, 1, 0), (10, 0, None, 1, 256, 3, 3)),
    ((22662, 0, 1, 0), (16, 0, None, None, None, 0, 0)),
]


@pytest.mark.parametrize("args,want", DEFAULTS, ids=["-".join(map(str, a)) for a, _ in DEFAULTS])
def test_default_geometry(geometry, args, want):
    got = geometry(*args)
    for key, w in zip(KEYS, want):
        if w is not None:
            assert got[key] == w, (key, got)


def test_multi_rounds_down_to_a_power_of_two(geometry, monkeypatch):
    monkeypatch.setenv("GSPARSE_BB_MULTI", "5")
    assert geometry(262144, 100000)["S"] == 4


def test_threads_other_than_512_or_1024_are_256(geometry, monkeypatch):
    monkeypatch.setenv("GSPARSE_BB_THREADS", "300")
    assert geometry(262144, 100000)["threads"] == 256


def test_slabs_zero_is_ignored(geometry, monkeypatch):
    monkeypatch.setenv("GSPARSE_BB_SLABS", "0")
    assert geometry(262144, 100000)["slabs"] == 512


def test_negative_landmarks_are_none(geometry, monkeypatch):
    monkeypatch.setenv("GSPARSE_BB_LANDMARKS", "-3")
    assert geometry(262144, 100000)["K"] == 0


def test_landmarks_are_clamped_to_n(geometry, monkeypatch):
    monkeypatch.setenv("GSPARSE_BB_LANDMARKS", "100")
    assert geometry(10, 3)["K"] == 10


def test_lmcoop_0_is_one_workgroup_per_landmark(geometry, monkeypatch):
    monkeypatch.setenv("GSPARSE_BB_LMCOOP", "0")
    assert geometry(262144, 100000)["lm_coop"] == 0


def test_lmw_is_clamped_to_256(geometry, monkeypatch):
    monkeypatch.setenv("GSPARSE_BB_LMW", "1000")
    assert geometry(262144, 100000)["lm_W"] == 256
