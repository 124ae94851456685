"""The symmetric Jaccard's rules without a GPU: csrc/gs_jac.hpp's row classes, task
counts, quotient-table parameters, hash, slot encoding and bucket match, compiled for
the host by tools/jac_host_check.cpp, against the NumPy restatement below."""

import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LIGHT, GIANT, TASK_MIN, MAX_ENT = 32, 16384, 65536, 1024
TABLE = {-1: 0, 0: 2048, 1: 8192, 2: 16384, 3: 32768, 4: 0}
MUL24 = 0x9E3779


# ---- the restatement ----------------------------------------------------------------
def np_class(d):
    return -1 if d <= LIGHT else 0 if d <= 1024 else 1 if d <= 4096 else 2 if d <= 8192 else \
        3 if d <= GIANT else 4


def np_probes(k, du):
    return max(16 * TABLE[k], 8 * du, TASK_MIN)


def np_tasks(k, du, w):
    if k < 0 or w == 0:
        return 0
    t = np_probes(k, du)
    return min(max(-(-w // t), -(-du // MAX_ENT)), du)


def np_qparams(n, C):
    """(hmask, qb, rmask, dmax), or None when fewer than 4 distance bits are left."""
    b = 1
    while b < 31 and (1 << b) < n:
        b += 1
    bb = (C // 8).bit_length() - 1
    b = max(b, bb)
    qb = b - bb
    if 16 - qb < 4:
        return None
    return (1 << b) - 1, qb, (1 << qb) - 1, min((1 << (16 - qb)) - 2, C // 8 - 1)


def np_hash(x, hmask):
    return (((x.astype(np.uint64) & 0xFFFFFF) * MUL24) & 0xFFFFFFFF & hmask).astype(np.uint32)


def np_table(ids, C, qp):
    """Sequential insert into buckets of 8: the ids placed, and whether one could not be."""
    hmask, qb, rmask, dmax = qp
    nb = C // 8
    fill = np.zeros(nb, dtype=np.int64)
    placed, ovf = set(), False
    for x, h in zip(ids.tolist(), np_hash(ids, hmask).tolist()):
        home = h >> qb
        for d in range(dmax + 1):
            bkt = (home + d) & (nb - 1)
            if fill[bkt] < 8:
                fill[bkt] += 1
                placed.add(x)
                break
        else:
            ovf = True
    return placed, ovf


# ---- the header compiled for the host -------------------------------------------------
@pytest.fixture(scope="module")
def jac_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("jac")
    exe = str(d / "jac_check")
    src = os.path.join(ROOT, "tools", "jac_host_check.cpp")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O2", src, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("hipcc host build unavailable: " + r.stderr[-300:])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, check=True, text=True)
        return [[int(v) for v in line.split()] for line in out.stdout.splitlines()]

    run.dir = d
    return run


def _rule_cases():
    cases = []
    for edge in (LIGHT, 1024, 4096, 8192, GIANT):
        for du in (edge - 1, edge, edge + 1, edge + 2):
            t = np_probes(np_class(du), du)
            # no work, one probe, around one and several tasks' worth, and far more work than
            # du tasks hold (the nt <= du cap)
            for w in (0, 1, t - 1, t, t + 1, 3 * t - 1, 3 * t, 3 * t + 1, 2 * du * t + 1):
                cases.append((du, w))
    return cases


def test_class_and_task_rules(jac_check):
    cases = _rule_cases()
    path = str(jac_check.dir / "rules.bin")
    np.array(cases, dtype=np.int64).tofile(path)
    got = jac_check("rules", path)
    assert len(got) == len(cases)
    floor_binds = cap_binds = 0
    for (du, w), (k, t, nt) in zip(cases, got):
        assert (k, t, nt) == (np_class(du), np_probes(np_class(du), du), np_tasks(np_class(du), du, w)), (du, w)
        if k >= 0 and w:
            floor_binds += -(-w // t) < -(-du // MAX_ENT) and nt == -(-du // MAX_ENT)
            cap_binds += -(-w // t) > du and nt == du
    assert floor_binds and cap_binds
    # the classes on either side of every boundary
    assert [np_class(d) for d in (32, 33, 1024, 1025, 4096, 4097, 8192, 8193, 16384, 16385)] == \
        [-1, 0, 0, 1, 1, 2, 2, 3, 3, 4]


QN = [1, 2 ** 11, 2 ** 12 + 1, 60000, 3_000_000, 2 ** 22, 2 ** 23, 2 ** 23 + 1, 2 ** 24, 2 ** 24 + 1,
      2 ** 31 - 1]


@pytest.mark.parametrize("C", [16384, 32768])
def test_qparams(jac_check, C):
    got = jac_check("qparams", C, *QN)
    for n, (ok, hmask, qb, rmask, dmax) in zip(QN, got):
        want = np_qparams(n, C)
        assert bool(ok) == (want is not None), n
        # ids of b bits leave 16 - (b - log2(C / 8)) distance bits: 4 at 2^23 (C = 16384) / 2^24
        assert bool(ok) == (n <= (2 ** 23 if C == 16384 else 2 ** 24)), n
        if want is not None:
            assert (hmask, qb, rmask, dmax) == want, n
            assert hmask + 1 >= n and 16 - qb >= 4 and ((dmax + 1) << qb) + rmask < 2 ** 16


@pytest.mark.parametrize("n", [60000, 3_000_000])
@pytest.mark.parametrize("C", [16384, 32768])
def test_hash_is_a_bijection_and_slots_decode(jac_check, C, n):
    hmask, qb, rmask, dmax = np_qparams(n, C)
    path = str(jac_check.dir / f"hash_{C}_{n}.bin")
    jac_check("hash", C, n, path)
    got = np.fromfile(path, dtype=np.uint32).reshape(n, 2)
    x = np.arange(n, dtype=np.int64)
    h = np_hash(x, hmask)
    assert np.array_equal(got[:, 0], h)
    assert np.unique(h).size == n  # no two ids below n collide
    # (home bucket, distance, remainder) gives h back: the slot holds d + 1 and the remainder
    slot = got[:, 1].astype(np.int64)
    assert slot.min() > 0 and slot.max() < 2 ** 16
    d = (slot >> qb) - 1
    assert np.array_equal(d, x % (dmax + 1))
    nb = C // 8
    bucket = ((h.astype(np.int64) >> qb) + d) & (nb - 1)  # where the insert puts it
    home = (bucket - d) & (nb - 1)
    assert hmask + 1 == nb << qb  # every hash bit is in (home, remainder)
    assert np.array_equal((home << qb) | (slot & rmask), h.astype(np.int64))


@pytest.mark.parametrize("cut", [None, 0, 1])
@pytest.mark.parametrize("C,n,count", [(16384, 60000, 4096), (16384, 60000, 12000), (32768, 60000, 16384),
                                       (32768, 3_000_000, 16384), (16384, 3_000_000, 12000)])
def test_table_round_trip(jac_check, C, n, count, cut):
    rng = np.random.default_rng(C + n + count)
    ids = rng.choice(n, count, replace=False).astype(np.int32)
    others = np.setdiff1d(np.arange(n, dtype=np.int32), ids)
    qs = np.concatenate([ids, others if n <= 60000 else rng.choice(others, 20000, replace=False)])
    hmask, qb, rmask, dmax = np_qparams(n, C)
    if cut is not None:
        dmax = min(dmax, cut)
    placed, ovf = np_table(ids, C, (hmask, qb, rmask, dmax))
    pi, pq = str(jac_check.dir / "ids.bin"), str(jac_check.dir / "qs.bin")
    ids.tofile(pi)
    qs.tofile(pq)
    got = jac_check("table", C, n, -1 if cut is None else cut, pi, pq)
    assert got[0][0] == int(ovf)
    found = np.array([g[0] for g in got[1:]], dtype=bool)
    want = np.fromiter((int(q) in placed for q in qs.tolist()), dtype=bool, count=qs.size)
    assert np.array_equal(found, want)  # every id placed is found, no other id is
    if cut is None:
        assert not ovf and len(placed) == count
    if cut == 0 and count >= 12000:
        assert ovf  # the dense tables do overflow with the distance cut to 0
