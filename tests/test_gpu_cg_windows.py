"""Register-resident CG (ApproxER mode 5): the slots whose p rows live outside LDS, the
edges of the LDS-resident prefixes and long rows next to them, bit for bit against the
oracle's C CG.

The graph is roman_like(12000, 17500, seed=3) plus rows with 10 extra neighbours each
(rows longer than the ELL's 8 entries: the overflow fold), placed from the host layout
function (engine.er_reg_layout) for every (ddot threads, GSPARSE_REG_KEEP) the cases
run, never guessed:
  * rows h, h + 32, h + 64, h + 128 of one chunk with 10 lower-indexed extra neighbours --
    the same lane's consecutive slots at 1, 2 and 4 threads per chain, the diagonal among
    the overflow entries -- and a second set with 10 higher-indexed ones;
  * a long row in the last slot inside a chunk's LDS-resident prefix and one in the first
    slot after it;
  * a long row within 28 rows of a chunk boundary, on each side.
blas_threads 3 / 8 / 16 give (threads per chain, row slots) = (4, 32), (2, 24), (1, 24).
"""

import os

import numpy as np
import pytest
import torch

import gsparse_oracle as O
from conftest import bits_equal

pytestmark = pytest.mark.gpu

N = 12000
THREADS = (3, 8, 16)
KEEPS = (None, 0, 64, 640)
GEOMETRY = {3: (4, 32), 8: (2, 24), 16: (1, 24)}
ITERS = 20


def layout_with(threads, keep):
    """engine.er_reg_layout under GSPARSE_REG_KEEP = keep (None: unset)."""
    from gsparse import engine

    old = os.environ.pop("GSPARSE_REG_KEEP", None)
    try:
        if keep is not None:
            os.environ["GSPARSE_REG_KEEP"] = str(keep)
        return engine.er_reg_layout(N, threads, True)
    finally:
        os.environ.pop("GSPARSE_REG_KEEP", None)
        if old is not None:
            os.environ["GSPARSE_REG_KEEP"] = old


def special_rows():
    """{row: "lo" | "hi"}: the long rows and the side their extra neighbours lie on."""
    lays = {(t, k): layout_with(t, k) for t in THREADS for k in KEEPS}
    for (t, _), lay in lays.items():
        assert lay is not None and lay["threads"] == 512 and (lay["G"], lay["R"]) == GEOMETRY[t]

    def one_chunk(h):  # rows h .. h + 128 inside one chunk at every thread count
        for t in THREADS:
            lay = lays[(t, None)]
            c = max(i for i, s in enumerate(lay["start"]) if s <= h)
            if h + 128 >= lay["start"][c] + lay["len"][c]:
                return False
        return True

    rows = {}
    h_lo = next(h for h in range(4100, N) if one_chunk(h))
    h_hi = next(h for h in range(8300, N) if one_chunk(h))
    for d in (0, 32, 64, 128):
        rows[h_lo + d] = "lo"
        rows[h_hi + d] = "hi"
    for (t, _), lay in lays.items():
        c = 1  # a chunk with a chunk before and after it
        edge = lay["start"][c] + lay["keep"][c]  # first row after the LDS-resident prefix
        if edge < lay["start"][c] + lay["len"][c]:
            rows.setdefault(edge - 1, "lo")  # last slot inside (keep 0: the chunk before)
            rows.setdefault(edge, "hi")      # first slot after
        b = lay["start"][2]
        rows.setdefault(b - 20, "hi")  # gathers across the boundary
        rows.setdefault(b + 20, "lo")
    return rows


@pytest.fixture(scope="module")
def windows_er():
    from gsparse import graphs

    ei = graphs.roman_like(N, 17500, seed=3)
    rng = np.random.default_rng(23)
    extra = []
    for row, side in sorted(special_rows().items()):
        pool = np.arange(max(0, row - 3000), row) if side == "lo" else np.arange(row + 1, min(N, row + 3000))
        have = set(ei[1][ei[0] == row].tolist()) | set(ei[0][ei[1] == row].tolist())
        pool = np.array([v for v in pool.tolist() if v not in have])
        extra += [(row, int(v)) for v in rng.choice(pool, 10, replace=False)]
    ex = np.array(extra, dtype=np.int64).T
    e = O.coalesce(np.concatenate([ei, ex], axis=1), N)
    ip, ix, d = O.canonical_csr(e, N)
    assert int(np.diff(ip).max()) >= 12  # the long rows are there (entries beyond the ELL's 8)
    ref = {t: O.approx_er(ip, ix, d, N, epsilon=0.9, max_cg_iters=ITERS, impl="c", blas_threads=t)
           for t in THREADS}
    return e, ref


def run(gs, e, threads):
    sp_ = gs.GraphSparsifier(gs.Data(edge_index=torch.from_numpy(e), num_nodes=N), "cpu")
    er = sp_._engine.approx_er(epsilon=0.9, max_cg_iters=ITERS, blas_threads=threads)
    return er, sp_._engine.er_iterations()


@pytest.mark.parametrize("keep", KEEPS, ids=["keep-unset", "keep-0", "keep-64", "keep-640"])
@pytest.mark.parametrize("threads", THREADS)
def test_windows_vs_oracle(windows_er, threads, keep, monkeypatch):
    import gsparse as gs

    monkeypatch.setenv("GSPARSE_CG_MODE", "5")
    monkeypatch.delenv("GSPARSE_REG_KEEP", raising=False)
    if keep is not None:
        monkeypatch.setenv("GSPARSE_REG_KEEP", str(keep))
    e, ref = windows_er
    er, it = run(gs, e, threads)
    assert np.all(it == ITERS), (int(it.min()), int(it.max()))
    assert bits_equal(er, ref[threads])


def test_windows_columns_in_turn(windows_er, monkeypatch):
    """7 workgroups: each solves many columns in turn (the per-column setup and the first
    slot's own-p request run again for every column)."""
    import gsparse as gs

    monkeypatch.setenv("GSPARSE_CG_MODE", "5")
    monkeypatch.setenv("GSPARSE_CG_SLOTS", "7")
    monkeypatch.setenv("GSPARSE_REG_KEEP", "640")
    e, ref = windows_er
    er, it = run(gs, e, 8)
    assert np.all(it == ITERS), (int(it.min()), int(it.max()))
    assert bits_equal(er, ref[8])
