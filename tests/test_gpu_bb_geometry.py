"""The metric backbone at the one size boundary its geometry has (65,536 nodes), tied to
gs_bb_geometry: what the staged entry points report is what bb_geometry says, on both
sides of the line, and the masks agree with each other and with the oracle.

The graph: a ring of 65,536 nodes plus two random chords per node, both directions of
every pair listed as columns, one weight per pair, uniform in [0.5, 6.5) (with
[0.5, 1.5) the local lower bounds keep every column and no source is left to search;
with this range 56,624 rows have open columns after the certificates, before and after
the backbone unit was split).  Run (a) has n = 65,536 (16
landmarks, one source per workgroup); run (b) has the same columns and n = 65,537 --
one isolated node flips the size class (48 landmarks spread over the GPU, 16 sources
per workgroup, degree relabeling as before) and nothing else.  A gs_pair_distances
call on the same context between two runs of (a) borrows the search slabs: the record
of their idle state has to survive a foreign user.
"""

from __future__ import annotations

import os

import numpy as np
import pytest

import gsparse_oracle as O

pytestmark = pytest.mark.gpu

N0 = 65536


def _graph():
    rng = np.random.default_rng(65536)
    u = np.arange(N0, dtype=np.int64)
    a = np.concatenate([u, u, u])
    b = np.concatenate([(u + 1) % N0, (u + rng.integers(2, N0 - 1, N0)) % N0,
                        (u + rng.integers(2, N0 - 1, N0)) % N0])
    w = rng.uniform(0.5, 6.5, a.size)
    ei = np.stack([np.concatenate([a, b]), np.concatenate([b, a])])
    return np.ascontiguousarray(ei), np.ascontiguousarray(np.concatenate([w, w]))


def _staged(stages, ei, n, w):
    """One rank's staged run: (K, nsrc after the certificates, nbatch, keep mask)."""
    K = stages.begin(ei, n, w, 1e-9, 0, 1)
    stages.certify(0, 1)
    state = np.zeros(ei.shape[1], dtype=np.uint8)
    stages.state_io(state, out=True)
    nsrc = int(np.unique(ei[0][state == 0]).size)
    nbatch = stages.plan()
    stages.search(0, nbatch, 0, 1)
    keep, _ = stages.finish()
    return K, nsrc, nbatch, keep[: ei.shape[1]].astype(bool)


def test_backbone_across_the_size_line_matches_its_geometry(monkeypatch):
    from gsparse._lib import Context
    from gsparse.engine import bb_geometry
    from gsparse.metric_backbone import BackboneStages, pair_distances

    for name in list(os.environ):  # the defaults are what is tested
        if name.startswith("GSPARSE_BB_"):
            monkeypatch.delenv(name)
    ei, w = _graph()
    ctx = Context(0)
    stages = BackboneStages(ctx)
    masks = {}
    for run, n, K_want, S_want in (("a", N0, 16, 1), ("b", N0 + 1, 48, 16)):
        K, nsrc, nbatch, keep = _staged(stages, ei, n, w)
        geo = bb_geometry(n, nsrc, 1, 0)
        print(f"run ({run}): n={n} K={K} nsrc={nsrc} nbatch={nbatch} geometry={geo}")
        assert K == K_want == geo["K"]
        assert nsrc > 16, nsrc  # the searches have work: the comparison below is not vacuous
        assert geo["S"] == S_want
        assert nbatch == geo["nbatch"] == -(-nsrc // S_want)
        masks[run] = keep
    assert np.array_equal(masks["a"], masks["b"])
    # 256 seeded source rows: every column of theirs against the oracle's per-row Dijkstra
    rows = np.unique(np.random.default_rng(256).choice(N0, 256, replace=False))
    ref, decided = O.metric_backbone_rows(ei, N0, w, rows, threads=max(1, min(16, os.cpu_count() or 1)))
    assert decided.sum() >= 4 * rows.size  # a row has its two ring columns and two chords at least
    bad = np.flatnonzero(decided & (masks["a"] != ref))
    assert bad.size == 0, (bad.size, int(decided.sum()))
    # a foreign user of the slabs: hop counts on a 1,000-node ring, then run (a) again
    r = np.arange(1000, dtype=np.int64)
    ring = np.stack([np.concatenate([r, (r + 1) % 1000]), np.concatenate([(r + 1) % 1000, r])])
    q = np.stack([np.zeros(999, dtype=np.int64), r[1:]], axis=1)
    hops = pair_distances(ring, 1000, None, q, ctx=ctx)
    assert np.array_equal(hops, np.minimum(r[1:], 1000 - r[1:]).astype(np.float64))
    again = _staged(stages, ei, N0, w)[3]
    assert np.array_equal(again, masks["a"])
