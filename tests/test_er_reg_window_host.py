"""The register-resident CG's LDS layout with a p window (gs_er_reg_layout_w ->
reg_layout, csrc/gs_cg.hpp), no GPU.

A window of W wave-slots per chunk is reserved out of the capacity before the prefixes
are apportioned (the rule of test_er_reg_layout_host.py, restated here with the smaller
capacity); the windows sit between the prefixes and the zero slot, aligned to wave-slots.
The window kernel exists for two threads per chain and unit weights only, and streams
every row past a prefix from the global slot, so a layout whose prefixes are not whole
wave-slots (a graph that fits LDS whole) reports W = 0 and is the plain layout.
"""

import os
import subprocess

import pytest

from conftest import PKG

LIB = os.path.join(PKG, "gsparse", "libgsparse.so")
LDS = 160 * 1024
NS = (12000, 18600, 22662)
WS = (0, 3, 4)
KEEPS = (None, 0, 64, 640)


@pytest.fixture
def engine(monkeypatch):
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    for name in list(os.environ):
        if name.startswith(("GSPARSE_CG_", "GSPARSE_RES_", "GSPARSE_REG_")):
            monkeypatch.delenv(name)
    from gsparse import engine

    return engine


def windowed_keeps(ln, W, reg_keep):
    """The apportioning rule by hand, T chunks of a 512-thread unit launch with two
    threads per chain: capacity less T windows of W x 64 slots, shared in proportion to
    the chunk lengths in whole wave-slots, the rest one wave-slot at a time to the chunk
    with the most rows outside LDS, then the GSPARSE_REG_KEEP cap."""
    T, align = len(ln), 64
    cap = (LDS - (6 * 32 * T + 2 * 16 + 2 + 512) * 8) // 8 - T * W * align
    tot = sum(ln)
    keep = [l if tot <= cap else (cap * l // tot) // align * align for l in ln]
    if tot > cap:
        left = cap - sum(keep)
        while left >= align:
            cand = [t for t in range(T) if keep[t] + align <= ln[t]]
            if not cand:
                break
            best = cand[0]
            for t in cand:
                if ln[t] - keep[t] > ln[best] - keep[best]:
                    best = t
            keep[best] += align
            left -= align
    if reg_keep is not None:
        keep = [min(k, reg_keep) for k in keep]
    return keep


@pytest.mark.parametrize("reg_keep", KEEPS, ids=["keep-unset", "keep-0", "keep-64", "keep-640"])
@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("n", NS)
def test_windowed_layout(engine, monkeypatch, n, W, reg_keep):
    if reg_keep is not None:
        monkeypatch.setenv("GSPARSE_REG_KEEP", str(reg_keep))
    plain = engine.er_reg_layout(n, 8, True)
    lay = engine.er_reg_layout_w(n, 8, W, True)
    assert (lay["threads"], lay["G"], lay["T"]) == (512, 2, 8)
    T, ln = lay["T"], lay["len"]
    want = windowed_keeps(ln, W, reg_keep)
    whole = all(k % 64 == 0 for k in want)
    # a window is laid out exactly where every prefix is a whole number of wave-slots
    assert lay["W"] == (W if whole else 0)
    if lay["W"] == 0:
        assert {k: v for k, v in lay.items() if k not in ("W", "wbase")} == plain
        assert lay["wbase"] == [0] * T
        return
    assert lay["keep"] == want
    spans = []
    for t in range(T):
        keep, lb, wb = lay["keep"][t], lay["lbase"][t], lay["wbase"][t]
        assert keep % 64 == 0 and 0 <= keep <= ln[t], (t, keep)  # whole wave-slots, inside the chunk
        assert wb % 64 == 0, (t, wb)
        spans += [(lb, lb + keep), (wb, wb + W * 64)]
    # prefixes and windows: disjoint, below the zero slot; after it the scratch slot, the
    # diagonal slots, the chain sums / tail rows and the chunk table
    spans.sort()
    assert spans[0][0] >= 0 and spans[-1][1] <= lay["zslot"] < 0x8000
    for (_, e0), (s1, _) in zip(spans, spans[1:]):
        assert e0 <= s1
    assert lay["zslot"] == sum(lay["keep"]) + T * W * 64
    assert lay["dsl"] == 512
    assert lay["lds_bytes"] == 8 * (lay["zslot"] + 2 + 512 + 6 * 32 * T + 2 * 16) <= LDS


def test_window_zero_is_the_plain_layout(engine):
    for n in NS:
        lay = engine.er_reg_layout_w(n, 8, 0, True)
        assert lay["W"] == 0
        assert {k: v for k, v in lay.items() if k not in ("W", "wbase")} == engine.er_reg_layout(n, 8, True)


def test_roman_windowed_keeps_pinned(engine):
    """Roman-empire size, 8 ddot threads: 12 / 16 KB of windows out of the prefixes."""
    l3 = engine.er_reg_layout_w(22662, 8, 3, True)
    assert l3["W"] == 3 and sorted(l3["keep"], reverse=True) == [2112] * 7 + [2048]
    l4 = engine.er_reg_layout_w(22662, 8, 4, True)
    assert l4["W"] == 4 and sorted(l4["keep"], reverse=True) == [2048] * 7 + [1984]


@pytest.mark.parametrize("threads", [3, 16])
@pytest.mark.parametrize("n", [12000, 22662])
def test_other_geometries_have_no_window(engine, monkeypatch, n, threads):
    """4 threads per chain (3 ddot threads) and 1 (16): W = 0 whatever is asked."""
    monkeypatch.setenv("GSPARSE_REG_KEEP", "640")
    plain = engine.er_reg_layout(n, threads, True)
    for W in (3, 4):
        lay = engine.er_reg_layout_w(n, threads, W, True)
        if plain is None:
            assert lay is None
            continue
        assert lay["G"] in (1, 4) and lay["W"] == 0
        assert {k: v for k, v in lay.items() if k not in ("W", "wbase")} == plain


def test_weighted_form_has_no_window(engine, monkeypatch):
    monkeypatch.setenv("GSPARSE_REG_KEEP", "640")
    assert engine.er_reg_layout_w(12000, 8, 3, False)["W"] == 0
