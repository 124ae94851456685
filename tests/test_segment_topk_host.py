"""Segmented top-k (gs_segment_topk): the ABI entry and the per-node rule, no GPU.

`segment_topk_rule` is the NumPy restatement the GPU tests compare the kernels
with (tests/test_gpu_segment_topk.py imports it): sort each segment's keys, take
the k-th largest t, compare gt (keys above t) and eq (keys equal to t).  Here it
is checked against the host restatement of the reference's loops,
selection.degree_aware_mask: a column the rule guarantees is never one the
reference drops.
"""

import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT, load_golden

HEADER = os.path.join(ROOT, "include", "gsparse.h")
LIB = os.path.join(PKG, "gsparse", "libgsparse.so")


def order_keys(x):
    """gs_topk.hip's order_key: uint64 keys ordered as np.sort orders the scores,
    -0.0 == +0.0, every NaN the one largest key."""
    x = np.array(x, dtype=np.float64)
    x[x == 0] = 0.0
    b = x.view(np.uint64)
    neg = (b >> np.uint64(63)) != 0
    key = np.where(neg, ~b, b | np.uint64(1 << 63))
    key[np.isnan(x)] = ~np.uint64(0)
    return key


def segment_topk_rule(scores, src, num_nodes, k):
    """(mask, status, n_guaranteed, n_ambiguous) by the per-node rule."""
    src = np.asarray(src, dtype=np.int64)
    E = len(src)
    scores = np.asarray(scores, dtype=np.float64)[:E]
    keys = order_keys(scores)
    order = np.argsort(src, kind="stable")
    bounds = np.searchsorted(src[order], np.arange(num_nodes + 1))
    mask = np.zeros(E, dtype=bool)
    status = np.zeros(num_nodes, dtype=np.uint8)
    for u in range(num_nodes):
        cols = order[bounds[u]:bounds[u + 1]]
        d = len(cols)
        if d == 0:
            continue
        if d <= k:
            mask[cols] = True
            status[u] = 1
            continue
        ks = np.sort(keys[cols])
        t = ks[d - k]
        gt, eq = int((ks > t).sum()), int((ks == t).sum())
        if gt + eq != k or np.isnan(scores[cols]).any():
            status[u] = 2
        else:
            mask[cols[keys[cols] >= t]] = True
            status[u] = 1
    return mask, status, int(mask.sum()), int((status == 2).sum())


# ---- 1. ABI ------------------------------------------------------------------
def test_header_declares_segment_topk():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bgs_segment_topk\s*\(", text)
    for name in ["GS_SEGK_EMPTY", "GS_SEGK_ALL", "GS_SEGK_SHORT", "GS_SEGK_LDS", "GS_SEGK_STREAM",
                 "GS_SEGK_CLASSES"]:
        assert name in text
    assert re.search(r"#define\s+GS_API_VERSION\s+3\b", text)


def test_library_exports_and_binds_segment_topk():
    from gsparse import _lib

    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"\bT gs_segment_topk\b", out)
    assert "gs_segment_topk" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["gs_segment_topk"]
    assert len(args) == 17  # the handle + the 16 arguments after it in gsparse.h
    L = _lib.lib(LIB)
    assert L.gs_segment_topk.argtypes == args


def test_engine_and_selection_expose_the_feature():
    import inspect

    from gsparse import engine, selection

    assert callable(engine.Engine.segment_topk)
    assert engine.Engine.SEGK_CLASSES == ("empty", "all", "short", "lds", "stream")
    assert "info" in inspect.signature(selection.degree_aware_mask_device).parameters


# ---- 2. the rule ---------------------------------------------------------------
def test_order_keys_order_and_specials():
    x = np.array([-np.inf, -2.5, -1e-300, -0.0, 0.0, 5e-324, 1.0, np.inf, np.nan])
    k = order_keys(x)
    assert k[3] == k[4]
    assert (np.diff(k[[0, 1, 2, 3, 5, 6, 7, 8]].astype(object)) > 0).all()
    assert k[8] == np.uint64(0xFFFFFFFFFFFFFFFF)
    assert order_keys(np.array([-np.nan]))[0] == k[8]


def test_rule_on_hand_made_segments():
    #        node 0: unique top 2     node 1: tie at the cut   node 2: d <= k   node 3: -
    src = np.array([0, 0, 0, 1, 1, 1, 2, 2, 0])
    sc = np.array([3.0, 1.0, 2.0, 5.0, 4.0, 4.0, 7.0, 7.0, 0.5])
    mask, status, ng, na = segment_topk_rule(sc, src, 4, 2)
    assert status.tolist() == [1, 2, 1, 0]
    assert mask.tolist() == [True, False, True, False, False, False, True, True, False]
    assert (ng, na) == (4, 1)
    # a tie block wholly above the cut and one wholly below it are decided
    src = np.zeros(5, dtype=np.int64)
    m, s, _, _ = segment_topk_rule(np.array([9.0, 9.0, 1.0, 1.0, 5.0]), src, 1, 3)
    assert s[0] == 1 and m.tolist() == [True, True, False, False, True]
    # -0.0 and +0.0 are one key: they tie at the cut
    m, s, _, _ = segment_topk_rule(np.array([-0.0, 0.0, 1.0]), np.zeros(3, dtype=np.int64), 1, 2)
    assert s[0] == 2 and not m.any()
    # a NaN makes a node with d > k ambiguous, never one with d <= k
    m, s, _, _ = segment_topk_rule(np.array([np.nan, 1.0, 2.0]), np.zeros(3, dtype=np.int64), 1, 2)
    assert s[0] == 2
    m, s, _, _ = segment_topk_rule(np.array([np.nan, 1.0, 2.0]), np.zeros(3, dtype=np.int64), 1, 3)
    assert s[0] == 1 and m.all()


@pytest.mark.parametrize("name", ["rmat10", "karate_test", "cora_like"])
@pytest.mark.parametrize("k", [2, 3, 5])
def test_rule_never_guarantees_a_column_the_reference_drops(name, k):
    """Every guaranteed column is in selection.degree_aware_mask's result (the
    reference's loops restated), the decided nodes' budgets are met, and with
    the ambiguous nodes resolved by the reference's own call phase 1 is the
    reference's phase 1."""
    from gsparse.selection import degree_aware_mask

    g = load_golden(name)
    ei, n = g["edge_index"], int(g["num_nodes"])
    E = ei.shape[1]
    for metric in ["jaccard", "degree", "approx_er"]:
        sc = g[f"scores_{metric}"]
        mask, status, ng, na = segment_topk_rule(sc, ei[0], n, k)
        deg = np.bincount(ei[0], minlength=n)
        assert ng == int(np.minimum(deg, k)[status == 1].sum())
        assert ((status == 0) == (deg == 0)).all()
        for r in [0.2, 0.5, 0.8]:
            host = degree_aware_mask(sc, ei, n, E, r, k)
            assert not (mask & ~host).any(), (metric, r)
        # r -> 0: the host result is phase 1 alone
        phase1 = degree_aware_mask(sc, ei, n, E, 1e-9, k)
        full = mask.copy()
        for u in np.nonzero(status == 2)[0]:
            inc = np.nonzero(ei[0] == u)[0]
            full[inc[np.argsort(sc[inc])[-k:]]] = True
        assert np.array_equal(full, phase1), metric
