"""The device normal stream (csrc/gs_rng.hip, gs_ziggurat.hpp) against NumPy's
Generator(PCG64).standard_normal beyond seed 42: every (graph, k, seed) case of
stream_cases.py, the host-RNG path, the three parse block sizes, column slices, the
draw-count cache and the drop-in path.

Everything is compared on Z = er_z(...) (n x k), bit for bit, with the oracle's CG on
NumPy's own stream (stream_cases.reference): eight iterations, so Z depends on every
normal and on the sign of every R column, which the scores cannot see.

Not reached: k_zig_link_seq, the chained link for blocks whose exit depends on the entry
offset -- it needs two parse chains that stay unmerged across a whole block, which no
stream of testable length produces."""

import numpy as np
import pytest

import gsparse_oracle as O
import stream_cases as SC
from conftest import bits_equal, load_golden

pytestmark = pytest.mark.gpu

TWO_SEEDS = (7, 2 ** 63 + 5)


def engine(name):
    """A fresh context holding golden `name` (no draw-count cache from another test)."""
    from gsparse._lib import Context
    from gsparse.engine import Engine

    n, ip, ix, d, _ = SC.graph(name)
    ctx = Context(0)
    ctx.set_graph_csr(n, ip, ix, d)
    return Engine(ctx)


def run(eng, case, seed, cols=None, host=False):
    """prepare -> project (device stream or NumPy's, streamed) -> 8 CG iterations;
    (Z[:, c0:c1], its[c0:c1])."""
    k = case[1]
    c0, c1 = cols if cols is not None else (0, k)
    assert eng.er_prepare(k) == SC.graph(case[0])[4]
    project = eng.er_project_host if host else eng.er_project_device
    project(np.random.default_rng(seed), k, cols=cols)
    eng.er_solve(c0, c1, SC.MAXITER, SC.RTOL, 1)
    return eng.er_z(c0, c1), eng.er_iterations()[c0:c1]


def first_bad(got, ref):
    """Where two Z blocks first differ, for the assertion message: (row, column)."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if got.shape != ref.shape:
        return got.shape, ref.shape
    bad = np.argwhere(got.view(np.uint64) != ref.view(np.uint64))
    return tuple(bad[0]) if len(bad) else None


def check(got, case, seed, cols=None):
    z, its = got
    Z, ito = SC.reference(case, seed)
    c0, c1 = cols if cols is not None else (0, case[1])
    assert np.array_equal(its, ito[c0:c1]), (its, ito[c0:c1])
    assert bits_equal(z, Z[:, c0:c1]), first_bad(z, Z[:, c0:c1])


def small_chunks(monkeypatch, case, rows=3501):
    """The host path's row chunk cut to `rows` R rows: the large case streams three."""
    from gsparse import engine as E

    monkeypatch.setattr(E, "_ROW_CHUNK_BYTES", 8 * case[1] * rows)
    m = SC.graph(case[0])[4]
    assert -(-m // rows) >= 3


@pytest.mark.parametrize("seed", SC.SEEDS, ids=SC.seed_id)
@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_device_stream_matches_numpy(case, seed):
    check(run(engine(case[0]), case, seed), case, seed)


@pytest.mark.parametrize("seed", SC.SEEDS, ids=SC.seed_id)
@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_host_stream_matches_numpy(case, seed, monkeypatch):
    """rng_mode="host": NumPy draws R, gs_er_project_rows_cols folds it row chunk by row
    chunk (three chunks for the large case, the later ones from the Y the earlier left)."""
    if case == SC.LARGE:
        small_chunks(monkeypatch, case)
    check(run(engine(case[0]), case, seed, host=True), case, seed)


@pytest.mark.parametrize("seed", TWO_SEEDS, ids=SC.seed_id)
@pytest.mark.parametrize("block", ["512", "1024"])
@pytest.mark.parametrize("case", (SC.LARGE,) + SC.AROUND_1024, ids=SC.case_id)
def test_parse_block_sizes(case, block, seed, monkeypatch):
    """GSPARSE_ZIG_BLOCK = 512 / 1024 (1024 is what m * k >= 2^29 runs): emit spans of
    2 / 1 parse blocks instead of 4, the same Z as unset and as NumPy's."""
    eng = engine(case[0])
    unset = run(eng, case, seed)
    check(unset, case, seed)
    monkeypatch.setenv("GSPARSE_ZIG_BLOCK", block)
    got = run(eng, case, seed)
    check(got, case, seed)
    assert bits_equal(got[0], unset[0])
    # and on a context that never parsed this stream with 256-draw blocks
    check(run(engine(case[0]), case, seed), case, seed)


def slices(k):
    from gsparse.engine import er_split

    b = er_split(k, 2)
    return [(0, 1), (k - 1, k), (1, k), (63, 129), (b[0], b[1]), (b[1], b[2])]


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("seed", TWO_SEEDS, ids=SC.seed_id)
@pytest.mark.parametrize("cols", slices(SC.LARGE[1]), ids=lambda c: f"cols{c[0]}-{c[1]}")
def test_column_slices(cols, seed, host, monkeypatch):
    """cols = (c0, c1), a rank's JL columns: every normal is parsed, R[:, c0:c1] alone is
    stored and projected, and only those columns can be solved and read."""
    from gsparse._lib import GsparseError

    case, k = SC.LARGE, SC.LARGE[1]
    c0, c1 = cols
    assert 0 <= c0 < c1 <= k
    if host:
        small_chunks(monkeypatch, case)
    eng = engine(case[0])
    check(run(eng, case, seed, cols=cols, host=host), case, seed, cols)
    outside = c0 - 1 if c0 > 0 else c1
    with pytest.raises(GsparseError, match="not all solved"):
        eng.er_z(outside, outside + 1)
    with pytest.raises(GsparseError, match="not all solved"):
        eng.er_z(0, k)
    with pytest.raises(GsparseError, match="not projected"):
        eng.er_solve(outside, outside + 1, SC.MAXITER, SC.RTOL, 1)
    # the refused calls left the solved slice as it was
    assert bits_equal(eng.er_z(c0, c1), SC.reference(case, seed)[0][:, c0:c1])


@pytest.mark.parametrize("case", [SC.LARGE, ("karate_test", 14)], ids=SC.case_id)
def test_draw_count_cache(case, monkeypatch):
    """One context: a repeated stream skips the "enough draws?" check (zig_key); another
    seed of the same length, the first seed again and another block size must not reuse
    what was cached for a different stream."""
    A, B = 12345, 1
    eng = engine(case[0])
    first = run(eng, case, A)
    check(first, case, A)
    again = run(eng, case, A)
    check(again, case, A)
    assert bits_equal(first[0], again[0])
    check(run(eng, case, B), case, B)
    check(run(eng, case, A), case, A)
    monkeypatch.setenv("GSPARSE_ZIG_BLOCK", "1024")
    check(run(eng, case, A), case, A)
    monkeypatch.delenv("GSPARSE_ZIG_BLOCK")
    check(run(eng, case, A), case, A)


def test_projection_state_checks():
    from gsparse._lib import GsparseError

    case, seed = ("karate_test", 14), 0
    k = case[1]
    eng = engine(case[0])
    eng.er_prepare(k)
    eng.er_project_device(np.random.default_rng(seed), k, cols=(2, 9))
    with pytest.raises(GsparseError, match="projection already started"):
        eng.er_project_device(np.random.default_rng(seed), k, cols=(2, 9))
    for c0, c1 in ((0, k), (1, 9), (2, 10), (9, 10)):
        with pytest.raises(GsparseError, match="not projected"):
            eng.er_solve(c0, c1, SC.MAXITER, SC.RTOL, 1)
    with pytest.raises(ValueError):
        eng.er_solve(5, 5, SC.MAXITER, SC.RTOL, 1)
    eng.er_solve(2, 9, SC.MAXITER, SC.RTOL, 1)
    check((eng.er_z(2, 9), eng.er_iterations()[2:9]), case, seed, (2, 9))
    # a new prepare starts over: the whole width, another seed
    check(run(eng, case, 1), case, 1)


@pytest.mark.parametrize("seed", [0, 12345, 2 ** 63 + 5], ids=SC.seed_id)
@pytest.mark.parametrize("name", ["karate_test", "roman2000"])
def test_drop_in_approx_er_other_seeds(name, seed):
    """Engine.approx_er with the device stream == the oracle's, at the reference's own
    k = jl_dim(n, 0.9) and 500 iterations."""
    g = load_golden(name)
    n, ip, ix, d = int(g["num_nodes"]), g["indptr"], g["indices"], g["data"]
    ref = O.approx_er(ip, ix, d, n, epsilon=0.9, seed=seed, impl="c", blas_threads=1)
    got = engine(name).approx_er(epsilon=0.9, seed=seed, blas_threads=1, rng_mode="device")
    assert bits_equal(got, ref), float(np.max(np.abs(got - ref) / np.abs(ref)))
