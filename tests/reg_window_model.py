"""NumPy restatement of how the register-resident CG (ApproxER mode 5, two threads per
chain) codes the entries of L_reg's ELL copy -- csrc/gs_cg_reg.hip's p_code -- for the
tests of the p window (test_er_reg_window_host.py, test_gpu_cg_reg_window.py).  Written
from the rule, not from the library: it takes a layout (engine.er_reg_layout_w) and the
graph and says, per entry (i -> c) of L_reg, where the kernel finds p_c:

  DIAG    the diagonal entry (the owner thread's diagonal slot);
  PREFIX  c lies in its chunk's LDS-resident prefix;
  WINDOW  c is a chain row past the prefix of i's own chunk, i is a chain row too, and
          their wave-slots (offset in the chunk // 64) differ by at most one;
  GLOBAL  everything else: another chunk's row past its prefix, a row two or more
          wave-slots away, a tail row (offset >= len & ~31) at either end.

A wave-slot is slow when one of its chain rows has a GLOBAL code among the first 8
entries of its row (entries in ascending column order, the diagonal among them).
"""

import numpy as np

DIAG, PREFIX, WINDOW, GLOBAL = 0, 1, 2, 3


def lreg_pattern(ip, ix, n):
    """(rows, cols, pos): the entries of L_reg = D - A + 1e-6 I of a loop-free graph in
    CSR order, pos the entry's place in its row."""
    rows = np.concatenate([np.repeat(np.arange(n, dtype=np.int64), np.diff(ip)), np.arange(n, dtype=np.int64)])
    cols = np.concatenate([np.asarray(ix, dtype=np.int64), np.arange(n, dtype=np.int64)])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    first = np.searchsorted(rows, np.arange(n))
    return rows, cols, np.arange(len(rows)) - first[rows]


def classify(rows, cols, lay, W):
    """The class of every entry under the layout `lay` with a window of W wave-slots."""
    start = np.asarray(lay["start"], dtype=np.int64)
    ln = np.asarray(lay["len"], dtype=np.int64)
    keep = np.asarray(lay["keep"], dtype=np.int64)
    slot = 32 * lay["G"]
    n32 = ln & ~np.int64(31)
    ti = np.searchsorted(start, rows, side="right") - 1
    tc = np.searchsorted(start, cols, side="right") - 1
    oi, oc = rows - start[ti], cols - start[tc]
    prefix = oc < keep[tc]
    near = np.abs(oc // slot - oi // slot) <= 1
    window = (W > 0) & ~prefix & (ti == tc) & (oc < n32[tc]) & (oi < n32[ti]) & near
    cls = np.where(rows == cols, DIAG, np.where(prefix, PREFIX, np.where(window, WINDOW, GLOBAL)))
    return cls, ti, oi


def counts(ip, ix, n, lay, W):
    """(slow wave-slots, window codes) of the graph under the layout."""
    rows, cols, pos = lreg_pattern(ip, ix, n)
    cls, ti, oi = classify(rows, cols, lay, W)
    ln = np.asarray(lay["len"], dtype=np.int64)
    slot = 32 * lay["G"]
    slow = (cls == GLOBAL) & (pos < 8) & (oi < (ln & ~np.int64(31))[ti])
    slots = np.unique(ti[slow] * (1 << 20) + oi[slow] // slot)
    return int(len(slots)), int(np.count_nonzero(cls == WINDOW))


def entry_classes(ip, ix, n, lay, W):
    """{(i, c): (class, place in row i)} lookup for single entries."""
    rows, cols, pos = lreg_pattern(ip, ix, n)
    cls, _, _ = classify(rows, cols, lay, W)
    key = rows * n + cols

    def look(i, c):
        at = np.searchsorted(key, i * n + c)
        assert at < len(key) and key[at] == i * n + c, (i, c)
        return int(cls[at]), int(pos[at])

    return look
