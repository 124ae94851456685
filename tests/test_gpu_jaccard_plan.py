"""The symmetric Jaccard's kept plan (csrc/gs_jac_plan.hip): calls repeated on the same
rows, count mode on a plan that ratio mode built, part calls between whole-graph calls
and a second graph on the same context -- with the hash classes on their side streams
or all on the context stream (GSPARSE_JAC_CONCURRENT=0), and with the bitmap rows in one
batch or one batch per row (GSPARSE_JAC_BMROWS=1).  Every result bit for bit the oracle's."""

import numpy as np
import pytest

import gsparse_oracle as O
from conftest import bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gs():
    import gsparse

    return gsparse


def _oracle_counts(ip, ix, jac):
    """|N(u) ∩ N(v)| per CSR entry, recovered from the oracle's ratio c / (d_u + d_v - c):
    c = J (d_u + d_v) / (1 + J) rounded, accepted only if it gives the oracle's ratio back
    bit for bit (the ratio is strictly increasing in c, in steps far above an ulp at
    these degrees, so that c is the one the oracle divided).  O.jaccard_counts, the
    A @ A of the count-share tests, needs 33 s and 13 GB for this graph (its hubs' leaves
    pair up 1.5e9 times), three times over with O.jaccard_part_counts: too much for a
    test that runs with every suite."""
    deg = np.diff(ip)
    s = (deg[O.csr_rows(ip)] + deg[ix]).astype(np.float64)
    c = np.rint(jac * s / (1.0 + jac))
    uni = s - c
    with np.errstate(divide="ignore", invalid="ignore"):
        back = np.where(uni > 0.0, c / uni, 0.0)
    assert bits_equal(back, jac)
    return c


def _oracle_part_counts(ip, ix, counts, part, nparts):
    """O.jaccard_part_counts on the counts above: the owner entries of the part's rows."""
    R, _ = O.jaccard_shares(ip, ix, nparts)
    rows, deg = O.csr_rows(ip), np.diff(ip)
    own = (deg[rows] > deg[ix]) | ((deg[rows] == deg[ix]) & (rows <= ix))
    return counts[own & (rows >= R[part]) & (rows < R[part + 1])].astype(np.uint32)


@pytest.fixture(scope="module")
def ref():
    """The 60,000-node hub graph of test_jaccard_quotient_tables_vs_oracle with its
    oracle results, and the plain hub graph (the same n) as a second graph."""
    from test_gpu_parity import _hub_graph, _quotient_graph

    ei, n = _quotient_graph("hub60k")
    ip, ix, d = O.canonical_csr(ei, n)
    deg = np.diff(ip)
    for lo, hi in [(32, 1024), (1024, 4096), (4096, 8192), (8192, 16384)]:
        assert ((deg > lo) & (deg <= hi)).any(), (lo, hi)
    assert (deg > 16384).sum() >= 2  # two bitmap rows: two batches with GSPARSE_JAC_BMROWS=1
    ei2, n2 = _hub_graph()
    assert n2 == n
    ip2, ix2, d2 = O.canonical_csr(ei2, n2)
    assert len(ix2) != len(ix)
    jac = O.jaccard(ip, ix)
    counts = _oracle_counts(ip, ix, jac)
    # the recovery agrees with the A @ A oracles where those are cheap
    from gsparse import graphs

    sip, six, _ = O.canonical_csr(graphs.rmat(12, 8, seed=5), 1 << 12)
    small = _oracle_counts(sip, six, O.jaccard(sip, six))
    assert np.array_equal(small, O.jaccard_counts(sip, six))
    assert all(np.array_equal(_oracle_part_counts(sip, six, small, p, 2), O.jaccard_part_counts(sip, six, p, 2))
               for p in range(2))
    return {
        "n": n, "csr": (ip, ix, d), "jaccard": jac, "counts": counts,
        "part_counts": [_oracle_part_counts(ip, ix, counts, p, 2) for p in range(2)],
        "csr2": (ip2, ix2, d2), "jaccard2": O.jaccard(ip2, ix2),
    }


@pytest.mark.parametrize("bmrows", [None, "1"])
@pytest.mark.parametrize("concurrent", [None, "0"])
def test_kept_plan_sequence(gs, ref, monkeypatch, concurrent, bmrows):
    from gsparse._lib import Context

    if concurrent is not None:
        monkeypatch.setenv("GSPARSE_JAC_CONCURRENT", concurrent)
    if bmrows is not None:
        monkeypatch.setenv("GSPARSE_JAC_BMROWS", bmrows)
    n, whole = ref["n"], ref["jaccard"]
    ctx = Context()
    ctx.set_graph_csr(n, *ref["csr"])
    e = gs.engine.Engine(ctx)
    assert e.symmetric
    # 1. twice on the same rows: the second call runs from the kept plan
    assert bits_equal(e.jaccard(), whole)
    assert bits_equal(e.jaccard(), whole)
    # 2. count mode on the plan that ratio mode built
    assert bits_equal(e.common_neighbors(), ref["counts"])
    # 3. the key changes with every call: parts between whole-graph calls
    parts = [e.jaccard_part(0, 2), e.jaccard_part(1, 2)]
    again = e.jaccard_part(0, 2)
    assert bits_equal(e.jaccard(), whole)
    assert bits_equal(again, parts[0])
    assert bits_equal(parts[0] + parts[1], whole)
    assert np.array_equal((parts[0] != 0).astype(int) + (parts[1] != 0), (whole != 0).astype(int))
    # 4. the parts' raw counts, then the whole again
    for p in range(2):
        assert np.array_equal(e.jaccard_part_counts(p, 2), ref["part_counts"][p]), p
    assert bits_equal(e.jaccard(), whole)
    # 5. a different graph with the same n on the same context
    ctx.set_graph_csr(n, *ref["csr2"])
    e2 = gs.engine.Engine(ctx)
    assert e2.nnz != e.nnz
    assert bits_equal(e2.jaccard(), ref["jaccard2"])
    assert bits_equal(e2.jaccard(), ref["jaccard2"])
    ctx.close()
