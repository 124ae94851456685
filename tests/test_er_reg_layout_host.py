"""Where the register-resident CG (ApproxER mode 5) keeps p: the host layout function
(gs_er_reg_layout -> reg_layout, csrc/gs_cg.hpp), no GPU.

Every chunk keeps a prefix of keep rows in LDS, in whole wave-slots of 32 G rows; the
kernels' immediate-offset fast path, the p codes of the ELL copy and the chunk table all
follow this one function, so its invariants are pinned here.  The
expected keeps restate the rule by hand (`parent_keeps`: capacity shared in proportion
to the chunk lengths, rounded down to wave-slots, the remainder handed out one wave-slot
at a time to the chunk with the most rows outside LDS) and the Roman-size values are the
ones the kernels ran with before the layout left regres_run.

The LDS-resident rows of a chunk are a prefix: there are no staggered windows and so no
stagger rule to assert.
"""

import os
import subprocess

import pytest

from conftest import PKG

LIB = os.path.join(PKG, "gsparse", "libgsparse.so")
LDS = 160 * 1024
NS = (2000, 12000, 22662)
TS = (1, 3, 8, 16)
# the one-wave (256-thread) form holds at most 88 rows per thread: one or three chunks
# of 22,662 rows do not fit either form
NO_MODE5 = {(22662, 1), (22662, 3)}


@pytest.fixture
def layout(monkeypatch):
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    for name in list(os.environ):
        if name.startswith(("GSPARSE_CG_", "GSPARSE_RES_", "GSPARSE_REG_")):
            monkeypatch.delenv(name)
    from gsparse import engine

    return engine.er_reg_layout


def chunks(n, threads):
    """make_chunks (OpenBLAS's split of a length-n ddot)."""
    if n <= 10000 or threads <= 1:
        return [0], [n]
    a, ln, lo, rem = [], [], 0, n
    for t in range(threads, 0, -1):
        if rem <= 0:
            break
        w = (rem + t - 1) // t
        a.append(lo)
        ln.append(w)
        lo += w
        rem -= w
    return a, ln


def parent_keeps(ln, G, threads, unit, reg_keep=None):
    T = len(ln)
    dsl = 2 * threads if threads == 256 else threads if unit else 0
    cap = (LDS - (6 * 32 * T + 2 * 16 + 2 + dsl) * 8) // 8
    tot, align = sum(ln), 32 * G
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
    return keep, dsl


@pytest.mark.parametrize("unit", [True, False], ids=["unit", "weighted"])
@pytest.mark.parametrize("reg_keep", [None, 0, 64, 640])
@pytest.mark.parametrize("threads", TS)
@pytest.mark.parametrize("n", NS)
def test_layout_invariants(layout, monkeypatch, n, threads, reg_keep, unit):
    if reg_keep is not None:
        monkeypatch.setenv("GSPARSE_REG_KEEP", str(reg_keep))
    lay = layout(n, threads, unit)
    if (n, threads) in NO_MODE5:
        assert lay is None
        return
    a, ln = chunks(n, threads)
    T, G = lay["T"], lay["G"]
    assert (lay["start"], lay["len"]) == (a, ln) and T == len(a)
    assert lay["threads"] in (256, 512) and 32 * T * G <= lay["threads"]
    assert G in (1, 2, 4, 8) and (G == 8 or 32 * T * 2 * G > lay["threads"])
    rows = max((l & ~31) >> 5 for l in ln)
    assert (rows + G - 1) // G <= lay["R"] <= (44 if lay["threads"] == 512 else 88)
    spans = []
    for t in range(T):
        keep, lb = lay["keep"][t], lay["lbase"][t]
        # whole wave-slots, inside the chunk (a chunk that fits is kept whole; a forced
        # GSPARSE_REG_KEEP is taken as given: the per-lane p codes cover a partial slot)
        assert keep % (32 * G) == 0 or keep == ln[t] or keep == reg_keep, (t, keep)
        assert 0 <= keep <= ln[t], (t, keep)
        spans.append((lb, lb + keep))
    # LDS bases: disjoint ranges below the zero slot
    spans.sort()
    assert spans[0][0] >= 0 and spans[-1][1] <= lay["zslot"]
    for (_, e0), (s1, _) in zip(spans, spans[1:]):
        assert e0 <= s1
    assert lay["zslot"] == sum(lay["keep"]) < 0x8000  # p codes are 15-bit LDS slots
    # p, zero + scratch slot, diagonal slots, 6 x 32 T chain sums / tail rows, chunk table
    want, dsl = parent_keeps(ln, G, lay["threads"], unit, reg_keep)
    assert lay["dsl"] == dsl
    assert lay["lds_bytes"] == 8 * (lay["zslot"] + 2 + dsl + 6 * 32 * T + 2 * 16) <= LDS
    # the keeps the kernels ran with before the layout left regres_run
    assert lay["keep"] == want


def test_roman_keeps_pinned(layout):
    """Roman-empire size, 8 ddot threads: 18,368 of the 22,662 rows of p in LDS."""
    lay = layout(22662, 8, True)
    assert (lay["threads"], lay["G"], lay["R"], lay["T"]) == (512, 2, 44, 8)
    assert sorted(lay["keep"], reverse=True) == [2304] * 7 + [2240]
    lay16 = layout(22662, 16, True)
    assert (lay16["threads"], lay16["G"], lay16["R"], lay16["T"]) == (512, 1, 44, 16)


def test_narrow_form_and_bad_arguments(layout, monkeypatch):
    monkeypatch.setenv("GSPARSE_REG_NT", "256")
    lay = layout(12000, 8, True)
    assert lay["threads"] == 256 and lay["G"] == 1 and lay["dsl"] == 512
    assert layout(0x8000, 8, True) is None  # p codes hold 15-bit rows
    from gsparse import _lib

    assert _lib.lib().gs_er_reg_layout(-1, 8, 1, None) != 0
