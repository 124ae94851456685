"""Register-resident CG (ApproxER mode 5), two threads per chain: the rotating LDS window
of p rows past the prefix (k_cg_regwide<WIN>, GSPARSE_REG_WINDOW), bit for bit against
the oracle's C CG, and what the engine records about its choice against a NumPy
restatement of the coding rule (reg_window_model.py).

n = 12,000 fits LDS whole, so GSPARSE_REG_KEEP pushes rows past the prefix.  The cases
run on roman_like(12000, 17500, seed=3) and on that graph plus edges the window must not
serve, placed from the layout function for every GSPARSE_REG_KEEP the cases run:
  * from a row past the prefix to the rows two wave-slots below and above in its chunk;
  * from a row of the chunk before to a row past the prefix;
  * between a chunk's tail row and a chain row past the prefix (both directions);
  * a long row in the first wave-slot past the prefix and one in the last inside it, with
    window-eligible and global neighbours among the entries beyond the ELL's 8.
The model classifies each of them and the test asserts the class before it runs.
"""

import os

import numpy as np
import pytest
import torch

import gsparse_oracle as O
import reg_window_model as M
from conftest import bits_equal

pytestmark = pytest.mark.gpu

N = 12000
ITERS = 20
KEEPS = (0, 64, 640)
WINDOWS = (0, 3, 4, None)


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


def placed(keep):
    """The rows of the added structures for GSPARSE_REG_KEEP = keep, in chunk 1."""
    lay = layout_w(N, 8, keep, 3)
    assert lay["W"] == 3 and lay["keep"][1] == keep and lay["keep"] == layout_w(N, 8, keep, 4)["keep"]
    a, ln = lay["start"][1], lay["len"][1]
    n32 = ln & ~31
    assert keep + 64 * 8 < n32 < ln
    far = a + keep + 64 * 3 + 5  # a row of the fourth wave-slot past the prefix
    d = {
        "far": far, "below": far - 128, "above": far + 128,
        "other": a - 100 - (keep // 64), "target": a + keep + 70,  # a chain row of chunk 0
        "tail": a + n32 + 3, "chain": a + n32 - 40,
        "long_out": a + keep + 3 + (keep // 64),  # first wave-slot past the prefix
    }
    if keep:
        d["long_in"] = a + keep - 20  # last wave-slot inside it
    return d


def added_edges():
    ex = []
    for keep in KEEPS:
        d = placed(keep)
        ex += [(d["far"], d["below"]), (d["far"], d["above"]), (d["other"], d["target"]), (d["tail"], d["chain"])]
        # next wave-slot (window-eligible) and three wave-slots up (global), high columns:
        # the last of them are the entries beyond the ELL's 8
        ex += [(d["long_out"], d["long_out"] + 64 + k) for k in range(6)]
        ex += [(d["long_out"], d["long_out"] + 192 + k) for k in range(6)]
        if keep:
            ex += [(d["long_in"], d["long_in"] + 64 + k) for k in range(6)]
            ex += [(d["long_in"], d["long_in"] + 256 + k) for k in range(6)]
    return np.array(ex, dtype=np.int64).T


@pytest.fixture(scope="module")
def graphs12k():
    from gsparse import graphs

    ei = graphs.roman_like(N, 17500, seed=3)
    out = {}
    for name, e in (("plain", O.coalesce(ei, N)),
                    ("added", O.coalesce(np.concatenate([ei, added_edges()], axis=1), N))):
        ip, ix, d = O.canonical_csr(e, N)
        out[name] = (e, ip, ix, d, {})
    return out


def reference(g, threads, iters=ITERS, n=N):
    e, ip, ix, d, refs = g
    if (threads, iters) not in refs:
        refs[(threads, iters)] = O.approx_er(ip, ix, d, n, epsilon=0.9, max_cg_iters=iters, impl="c",
                                             blas_threads=threads)
    return refs[(threads, iters)]


def run(e, n, threads, iters):
    import gsparse as gs

    sp_ = gs.GraphSparsifier(gs.Data(edge_index=torch.from_numpy(e), num_nodes=n), "cpu")
    er = sp_._engine.approx_er(epsilon=0.9, max_cg_iters=iters, blas_threads=threads)
    return er, sp_._engine.er_iterations(), sp_._engine.er_reg_window()


def expected_stats(ip, ix, n, threads, keep, window):
    """What the engine must record: the default window (3) is weighed when the variable is
    unset and used only if it leaves strictly fewer slow wave-slots; 3 / 4 are taken as
    given; 0 weighs nothing."""
    if window == 0:
        return {"W": 0, "slow_plain": -1, "slow_window": -1, "window_codes": 0}
    W = 3 if window is None else window
    lay = layout_w(n, threads, keep, W)
    if lay["W"] == 0:
        return {"W": 0, "slow_plain": -1, "slow_window": -1, "window_codes": 0}
    slow_p, _ = M.counts(ip, ix, n, layout_w(n, threads, keep, 0), 0)
    slow_w, codes = M.counts(ip, ix, n, lay, W)
    use = window is not None or slow_w < slow_p
    return {"W": W if use else 0, "slow_plain": slow_p, "slow_window": slow_w, "window_codes": codes if use else 0}


def set_env(monkeypatch, keep, window):
    monkeypatch.setenv("GSPARSE_CG_MODE", "5")
    for name in ("GSPARSE_REG_KEEP", "GSPARSE_REG_WINDOW", "GSPARSE_CG_SLOTS"):
        monkeypatch.delenv(name, raising=False)
    if keep is not None:
        monkeypatch.setenv("GSPARSE_REG_KEEP", str(keep))
    if window is not None:
        monkeypatch.setenv("GSPARSE_REG_WINDOW", str(window))


def test_added_edges_are_global(graphs12k):
    """The model's verdict on the added structures: none of them is a window code."""
    _, ip, ix, _, _ = graphs12k["added"]
    for keep in KEEPS:
        d = placed(keep)
        for W in (3, 4):
            look = M.entry_classes(ip, ix, N, layout_w(N, 8, keep, W), W)
            for i, c in (("far", "below"), ("far", "above"), ("below", "far"), ("above", "far"),
                         ("other", "target"), ("tail", "chain"), ("chain", "tail")):
                assert look(d[i], d[c])[0] == M.GLOBAL, (keep, W, i, c)
            for row, far in (("long_out", 192),) + ((("long_in", 256),) if keep else ()):
                near = [look(d[row], d[row] + 64 + k) for k in range(6)]
                glob = [look(d[row], d[row] + far + k) for k in range(6)]
                assert all(c == M.WINDOW for c, _ in near) and all(c == M.GLOBAL for c, _ in glob), (keep, W, row)
                # both kinds among the overflow entries (places 8 and up)
                assert any(p >= 8 for _, p in near) and all(p >= 8 for _, p in glob), (keep, W, row, near)


@pytest.mark.parametrize("window", WINDOWS, ids=["win-0", "win-3", "win-4", "win-unset"])
@pytest.mark.parametrize("keep", KEEPS, ids=["keep-0", "keep-64", "keep-640"])
@pytest.mark.parametrize("graph", ["plain", "added"])
def test_window_vs_oracle(graphs12k, graph, keep, window, monkeypatch):
    set_env(monkeypatch, keep, window)
    e, ip, ix, _, _ = graphs12k[graph]
    er, it, st = run(e, N, 8, ITERS)
    print(graph, keep, window, st)
    assert st == expected_stats(ip, ix, N, 8, keep, window)
    assert np.all(it == ITERS), (int(it.min()), int(it.max()))
    assert bits_equal(er, reference(graphs12k[graph], 8))


@pytest.mark.parametrize("keep", [0, 640], ids=["keep-0", "keep-640"])
def test_window_columns_in_turn(graphs12k, keep, monkeypatch):
    """7 workgroups: each solves many columns in turn, the pass's prologue (the first two
    own rows, slot 0 of a chunk without a prefix) runs again for every column."""
    set_env(monkeypatch, keep, 3)
    monkeypatch.setenv("GSPARSE_CG_SLOTS", "7")
    e = graphs12k["added"][0]
    er, it, st = run(e, N, 8, ITERS)
    assert st["W"] == 3
    assert np.all(it == ITERS), (int(it.min()), int(it.max()))
    assert bits_equal(er, reference(graphs12k["added"], 8))


@pytest.mark.parametrize("threads", [3, 16])
def test_other_geometries_ignore_the_knob(graphs12k, threads, monkeypatch):
    """4 threads per chain and 1: no window kernel, GSPARSE_REG_WINDOW=4 changes nothing."""
    set_env(monkeypatch, 640, 4)
    e = graphs12k["added"][0]
    er, it, st = run(e, N, threads, ITERS)
    assert st["W"] == 0
    assert np.all(it == ITERS), (int(it.min()), int(it.max()))
    assert bits_equal(er, reference(graphs12k["added"], threads))


N2 = 18600  # the smallest size here that overflows LDS by itself (44 row slots)


def random_graph(n, m, seed):
    rng = np.random.default_rng(seed)
    u, v = rng.integers(0, n, m), rng.integers(0, n, m)
    ok = u != v
    e = np.stack([np.concatenate([u[ok], v[ok]]), np.concatenate([v[ok], u[ok]])]).astype(np.int64)
    return O.coalesce(e, n)


@pytest.mark.parametrize("kind", ["roman", "random"])
def test_window_chosen_per_graph(kind, monkeypatch):
    """GSPARSE_REG_WINDOW unset: a window for the band graph, none for a uniformly random
    one of the same size (every wave-slot is slow either way)."""
    from gsparse import graphs

    m = int(N2 * 32_927 / 22_662)
    e = O.coalesce(graphs.roman_like(N2, m, seed=0), N2) if kind == "roman" else random_graph(N2, m, 5)
    ip, ix, d = O.canonical_csr(e, N2)
    set_env(monkeypatch, None, None)
    er, it, st = run(e, N2, 8, 2)
    print(kind, st)
    assert st == expected_stats(ip, ix, N2, 8, None, None)
    assert st["W"] == (3 if kind == "roman" else 0)
    ref = O.approx_er(ip, ix, d, N2, epsilon=0.9, max_cg_iters=2, impl="c", blas_threads=8)
    assert np.all(it == 2)
    assert bits_equal(er, ref)


@pytest.mark.parametrize("window", [3, 4])
def test_roman_counts(window, monkeypatch):
    """Roman-empire size: the recorded slow wave-slots, plain and windowed, and the window
    codes equal the model's own count."""
    from gsparse import graphs

    n = 22_662
    e = O.coalesce(graphs.roman_like(), n)
    ip, ix, d = O.canonical_csr(e, n)
    set_env(monkeypatch, None, window)
    er, it, st = run(e, n, 8, 1)
    want = expected_stats(ip, ix, n, 8, None, window)
    print(window, st, want)
    assert st == want and st["W"] == window
    assert st["slow_window"] < st["slow_plain"]
    assert bits_equal(er, O.approx_er(ip, ix, d, n, epsilon=0.9, max_cg_iters=1, impl="c", blas_threads=8))
