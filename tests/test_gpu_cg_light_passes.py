"""Register-resident CG (ApproxER mode 5), two threads per chain: the window kernel's p
update in one sweep (the p_old of the last 12 slots and of the tail row requested from the
global slot ahead of the sweep, slots past the prefix before them in groups, the prefix LDS
to LDS), bit for bit against the oracle's C CG with the iteration counts.  The plain
two-per-chain kernel, the other geometries and the weighted form share its lambdas and are
run beside it.

n = 12,000 fits LDS whole (24 row slots, 28 tail rows per chunk), so GSPARSE_REG_KEEP decides
how many slots lie past the prefix: unset none (what is requested ahead is never used), 0 all
24 (the 12 requested ahead and the grouped remainder both run), 64 / 640 all but one / ten.
Window unset / 0 / 3 picks the window or the plain kernel.  The "tails" graph adds, in chunk
1, edges between tail rows and (i) a chain row past every prefix the cases run, (ii) a row of
the next chunk, and (iii) makes one tail row long (more than 8 entries, neighbours of both
kinds).  n = 11,776 has no tail row, n = 12,024 has 31 per chunk.
"""

import os

import numpy as np
import pytest
import torch

import gsparse_oracle as O
from conftest import bits_equal

pytestmark = pytest.mark.gpu

N = 12000
ITERS = 20
KEEPS = (None, 0, 64, 640)
WINDOWS = (None, 0, 3)


def layout_w(n, threads, keep, W):
    """engine.er_reg_layout_w under GSPARSE_REG_KEEP = keep (None: unset)."""
    from gsparse import engine

    old = os.environ.pop("GSPARSE_REG_KEEP", None)
    try:
        if keep is not None:
            os.environ["GSPARSE_REG_KEEP"] = str(keep)
        return engine.er_reg_layout_w(n, threads, W, True)
    finally:
        os.environ.pop("GSPARSE_REG_KEEP", None)
        if old is not None:
            os.environ["GSPARSE_REG_KEEP"] = old


def tail_edges():
    """Edges at the tail rows of chunk 1, placed from the layout (the same rows for every
    GSPARSE_REG_KEEP the cases run: a chunk's rows do not depend on it)."""
    lay = layout_w(N, 8, 640, 3)
    assert lay["W"] == 3 and lay["keep"][1] == 640
    for keep in (0, 64):
        other = layout_w(N, 8, keep, 3)
        assert other["start"] == lay["start"] and other["len"] == lay["len"] and other["keep"][1] == keep
    a, ln, nxt = lay["start"][1], lay["len"][1], lay["start"][2]
    n32 = ln & ~31
    assert ln - n32 == 28 and nxt == a + ln
    chain = a + 640 + 64 * 3 + 5  # a chain row of the fourth wave-slot past the longest prefix
    assert chain < a + n32
    ex = [(a + n32 + 2, chain), (a + n32 + 9, nxt + 10)]
    long_row = a + n32 + 5
    ex += [(long_row, a + n32 - 40 - k) for k in range(6)]  # chain rows of its own chunk
    ex += [(long_row, nxt + 100 + k) for k in range(6)]      # rows of the next chunk
    return np.array(ex, dtype=np.int64).T, long_row


@pytest.fixture(scope="module")
def graphs12k():
    from gsparse import graphs

    ei = graphs.roman_like(N, 17500, seed=3)
    ex, long_row = tail_edges()
    out = {}
    for name, e in (("plain", O.coalesce(ei, N)),
                    ("tails", O.coalesce(np.concatenate([ei, ex], axis=1), N)),
                    # every 7th edge doubled: multiplicity-2 entries, the weighted form
                    ("weighted", np.concatenate([ei, ei[:, ::7]], axis=1))):
        ip, ix, d = O.canonical_csr(e, N)
        out[name] = (e, ip, ix, d, {})
    ip = out["tails"][1]
    assert ip[long_row + 1] - ip[long_row] > 8  # with the diagonal: more than 8 entries
    return out


def reference(g, threads, n=N, iters=ITERS):
    e, ip, ix, d, refs = g
    if (threads, iters) not in refs:
        refs[(threads, iters)] = O.approx_er(ip, ix, d, n, epsilon=0.9, max_cg_iters=iters, impl="c",
                                             blas_threads=threads)
    return refs[(threads, iters)]


def run(e, n, threads, iters=ITERS):
    import gsparse as gs

    sp_ = gs.GraphSparsifier(gs.Data(edge_index=torch.from_numpy(e), num_nodes=n), "cpu")
    er = sp_._engine.approx_er(epsilon=0.9, max_cg_iters=iters, blas_threads=threads)
    return er, sp_._engine.er_iterations(), sp_._engine.er_reg_window()


def set_env(monkeypatch, keep, window):
    monkeypatch.setenv("GSPARSE_CG_MODE", "5")
    for name in ("GSPARSE_REG_KEEP", "GSPARSE_REG_WINDOW", "GSPARSE_CG_SLOTS"):
        monkeypatch.delenv(name, raising=False)
    if keep is not None:
        monkeypatch.setenv("GSPARSE_REG_KEEP", str(keep))
    if window is not None:
        monkeypatch.setenv("GSPARSE_REG_WINDOW", str(window))


def ident(v):
    return "unset" if v is None else str(v)


@pytest.mark.parametrize("window", WINDOWS, ids=["win-" + ident(w) for w in WINDOWS])
@pytest.mark.parametrize("keep", KEEPS, ids=["keep-" + ident(k) for k in KEEPS])
@pytest.mark.parametrize("graph", ["plain", "tails"])
def test_sweep_vs_oracle(graphs12k, graph, keep, window, monkeypatch):
    set_env(monkeypatch, keep, window)
    e = graphs12k[graph][0]
    er, it, st = run(e, N, 8)
    print(graph, keep, window, st)
    if window == 3 and keep is not None:
        assert st["W"] == 3  # the window kernel ran
    if window == 0:
        assert st["W"] == 0
    assert np.all(it == ITERS), (int(it.min()), int(it.max()))
    assert bits_equal(er, reference(graphs12k[graph], 8))


@pytest.mark.parametrize("window", [0, 3])
@pytest.mark.parametrize("keep", [None, 0, 640], ids=["keep-unset", "keep-0", "keep-640"])
@pytest.mark.parametrize("n", [11776, 12024])
def test_tail_row_counts(n, keep, window, monkeypatch):
    """No tail row at all (8 chunks of 1,472 rows) and 31 per chunk."""
    from gsparse import graphs

    lay = layout_w(n, 8, keep, 0)
    assert all(ln - (ln & ~31) == (0 if n == 11776 else 31) for ln in lay["len"][:8])
    e = O.coalesce(graphs.roman_like(n, int(n * 17500 / 12000), seed=3), n)
    ip, ix, d = O.canonical_csr(e, n)
    set_env(monkeypatch, keep, window)
    er, it, st = run(e, n, 8)
    assert np.all(it == ITERS), (int(it.min()), int(it.max()))
    assert bits_equal(er, reference((e, ip, ix, d, _REFS.setdefault(n, {})), 8, n=n))


_REFS = {}


def test_bench_instantiation(monkeypatch):
    """Roman-empire size at T = 8: 44 row slots, the default window choice."""
    from gsparse import graphs

    n = 22_662
    e = O.coalesce(graphs.roman_like(), n)
    ip, ix, d = O.canonical_csr(e, n)
    set_env(monkeypatch, None, None)
    er, it, st = run(e, n, 8)
    print(st)
    assert st["W"] == 3
    assert np.all(it == ITERS), (int(it.min()), int(it.max()))
    assert bits_equal(er, O.approx_er(ip, ix, d, n, epsilon=0.9, max_cg_iters=ITERS, impl="c", blas_threads=8))


@pytest.mark.parametrize("threads", [3, 16])
def test_other_geometries(graphs12k, threads, monkeypatch):
    """Four threads per chain and one: the forms that share the kernel's lambdas."""
    set_env(monkeypatch, 640, None)
    e = graphs12k["tails"][0]
    er, it, st = run(e, N, threads)
    assert st["W"] == 0
    assert np.all(it == ITERS), (int(it.min()), int(it.max()))
    assert bits_equal(er, reference(graphs12k["tails"], threads))


@pytest.mark.parametrize("keep", [None, 640], ids=["keep-unset", "keep-640"])
def test_weighted_form(graphs12k, keep, monkeypatch):
    """Two threads per chain, weights in the ELL: the two-pass p update as before."""
    set_env(monkeypatch, keep, None)
    e = graphs12k["weighted"][0]
    er, it, st = run(e, N, 8)
    assert st["W"] == 0
    assert np.all(it == ITERS), (int(it.min()), int(it.max()))
    assert bits_equal(er, reference(graphs12k["weighted"], 8))
