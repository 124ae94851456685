"""Symmetric random baseline -- drop-in for ``src/sparsification/random.py``.

The result is defined by NumPy: ``np.unique(keys, return_inverse=True)`` over the
undirected keys, ``default_rng(seed).random`` and ``np.argsort`` (random.py:14-52).
It is computed on the device: gs_undirected_ids (a radix sort of (key, column)
pairs, head flags, a scan, a scatter) gives ``inverse_idx``, gs_pcg64_doubles the
PCG64 double stream, gs_random_mask the select of the ``n_keep`` highest scores and
the gather ``keep_undir[inverse_idx]`` -- all bit for bit NumPy's values.

``RandomBaseline`` is the resident form: ids and scores are built once and stay on
the device, a sweep over retention rates uploads nothing.  ``precompute_random_scores``
and ``random_sparsify`` keep the reference's signatures and types.

The reference's own NumPy lines are the host form.  They run when the input is
outside the device contract (an id outside ``[0, num_nodes)``, an empty graph, ...:
NumPy then decides, errors included), when no device context can be made
(``GsparseUnavailable``), when ``GSPARSE_RANDOM=host`` asks for them, and -- the
argsort alone -- for a cut whose tie block np.argsort's unstable order decides
(``tie_break="numpy"``, the default; ``"stable"`` keeps the device's stable rule).
``last_selection["path"]`` says which form ran ("device" or "host").
"""

import os

import numpy as np

from ._args import on_device, to_host
from .data import Data

# what the last precompute_random_scores / random_sparsify call did: path ("device" or
# "host") and, after a device select, cut / beyond / tied / ambiguous
last_selection: dict = {}

_ENGINES: dict = {}


def _record(info: dict):
    last_selection.clear()
    last_selection.update(info)


def _host_precompute_random_scores(data: Data, seed: int = 42):
    """Reproducible symmetric random score per undirected edge (random.py:14-33)."""
    ei = data.edge_index.cpu().numpy()
    src, dst = ei[0], ei[1]
    n = data.num_nodes
    u = np.minimum(src, dst)
    v = np.maximum(src, dst)
    keys = u.astype(np.int64) * (n + 1) + v.astype(np.int64)
    _, inverse_idx = np.unique(keys, return_inverse=True)
    n_undirected = int(inverse_idx.max()) + 1
    rng = np.random.default_rng(seed)
    undirected_scores = rng.random(n_undirected)
    return undirected_scores, inverse_idx


def _host_random_sparsify(data: Data, undirected_scores, inverse_idx, retention_ratio: float,
                          device: str) -> Data:
    """Keep the top fraction of undirected edges by random score (random.py:36-52)."""
    if retention_ratio == 1.0:
        return data.clone()
    n_undirected = len(undirected_scores)
    n_keep = max(1, int(n_undirected * retention_ratio))
    keep_undir = np.zeros(n_undirected, dtype=bool)
    keep_undir[np.argsort(undirected_scores)[-n_keep:]] = True
    mask = keep_undir[inverse_idx]
    sparse = data.clone()
    sparse.edge_index = data.edge_index[:, mask].to(device)
    return sparse


def _tie_break(tie_break):
    tb = tie_break or os.environ.get("GSPARSE_TIE_BREAK", "numpy")
    if tb not in ("numpy", "stable"):
        raise ValueError(f"tie_break must be 'numpy' or 'stable', got {tb!r}")
    return tb


def _engine(data: Data, gpu):
    """The Engine of the random baseline's context on device ``gpu`` (default: the device
    of a CUDA ``edge_index``, else the package's default device), or None when the host
    form is asked for or no context can be made.  One context per device is kept for the
    process: it holds only scratch (sort buffers, staging), never a caller's arrays."""
    if os.environ.get("GSPARSE_RANDOM", "device") == "host":
        return None
    from ._lib import Context, GsparseUnavailable, default_device
    from .engine import Engine

    ei = data.edge_index
    if gpu is None and getattr(ei, "is_cuda", False):
        gpu = ei.device.index
    try:
        dev = default_device() if gpu is None else int(gpu)
        if dev not in _ENGINES:
            _ENGINES[dev] = Engine(Context(dev))
        return _ENGINES[dev]
    except GsparseUnavailable:
        return None


def _select_info(path, cut, beyond, tied, n_keep):
    need = n_keep - beyond
    return {"path": path, "cut": cut, "beyond": beyond, "tied": tied, "need": need,
            "ambiguous": 0 < need < tied}


def _host_keep_mask(undirected_scores, inverse_idx, n_keep):
    """random.py:47-49, the reference's own calls."""
    keep_undir = np.zeros(len(undirected_scores), dtype=bool)
    keep_undir[np.argsort(undirected_scores)[-n_keep:]] = True
    return keep_undir[inverse_idx]


class RandomBaseline:
    """The symmetric random baseline of one graph, resident on the device.

    Builds ``inverse_idx`` (the undirected-edge id of every ``edge_index`` column) and
    the ``default_rng(seed)`` score of every undirected edge once and keeps both on the
    device; a CUDA ``edge_index`` on that device is read in place.  ``mask`` /
    ``sparsify`` / ``sweep`` then select per retention rate without any upload.  Masks of
    one handle nest: the edges kept at a smaller ratio are kept at every larger one.

    Args:
        data: ``Data`` with ``edge_index`` [2, E] and ``num_nodes``.
        seed: seed of ``np.random.default_rng`` (random.py:31).
        gpu: device ordinal (default: ``edge_index``'s device, else the package default).
        tie_break: "numpy" (default: an ambiguous cut is resolved by the reference's own
            ``np.argsort`` call) or "stable" (the device's ``kind='stable'`` rule).

    ``path`` is "device" or "host" (the reference's NumPy lines: see the module
    docstring); ``last_selection`` records the last mask's ``path``, ``cut``, ``beyond``,
    ``tied`` and ``ambiguous``."""

    def __init__(self, data: Data, seed: int = 42, gpu=None, tie_break=None):
        self.data = data
        self.seed = seed
        self.tie_break = _tie_break(tie_break)
        self.num_edges = int(data.edge_index.size(1))
        self.last_selection: dict = {}
        self._scores = self._inverse = None    # host copies (np.ndarray), made on first access
        self._d_scores = self._d_inverse = None  # device tensors
        self._eng = _engine(data, gpu)
        if self._eng is not None and self._build_device():
            self.path = "device"
            return
        self._eng = None
        self.path = "host"
        self._scores, self._inverse = _host_precompute_random_scores(data, seed)
        self.n_undirected = len(self._scores)

    def _build_device(self) -> bool:
        import torch

        eng, ei = self._eng, self.data.edge_index
        try:
            n = int(self.data.num_nodes)
        except (TypeError, ValueError):
            return False
        dev = torch.device("cuda", eng.ctx.device)
        if on_device(ei, eng.ctx.device):
            src, dst = ei[0], ei[1]
        else:
            e = ei.detach().cpu().numpy()
            if e.dtype.kind not in "iu" or e.dtype == np.uint64:
                return False
            src, dst = e[0], e[1]
        inv = torch.empty(self.num_edges, dtype=torch.int64, device=dev)
        inv, cnt, status = eng.undirected_ids(src, dst, n, out=inv)
        if status != 0:
            return False
        self._d_inverse = inv
        self.n_undirected = cnt
        self._d_scores = eng.pcg64_doubles(np.random.default_rng(self.seed), 0, cnt,
                                           out=torch.empty(cnt, dtype=torch.float64, device=dev))
        return True

    @property
    def undirected_scores(self) -> np.ndarray:
        """float64[n_undirected]: ``default_rng(seed).random(n_undirected)``."""
        if self._scores is None:
            self._scores = self._d_scores.cpu().numpy()
        return self._scores

    @property
    def inverse_idx(self) -> np.ndarray:
        """int64[E]: the undirected-edge id of every ``edge_index`` column."""
        if self._inverse is None:
            self._inverse = self._d_inverse.cpu().numpy()
        return self._inverse

    def _n_keep(self, retention_ratio: float) -> int:
        return max(1, int(self.n_undirected * retention_ratio))

    def mask(self, retention_ratio: float):
        """bool[E] on ``edge_index``'s device: the columns ``random_sparsify`` keeps."""
        import torch

        ei = self.data.edge_index
        if retention_ratio == 1.0:
            self.last_selection = {"path": self.path}
            return torch.ones(self.num_edges, dtype=torch.bool, device=ei.device)
        n_keep = self._n_keep(retention_ratio)
        if self._eng is None:
            self.last_selection = {"path": "host"}
            m = _host_keep_mask(self._scores, self._inverse, n_keep)
            return torch.from_numpy(m).to(ei.device)
        eng = self._eng
        out = None
        if on_device(ei, eng.ctx.device):
            out = torch.empty(self.num_edges, dtype=torch.bool, device=ei.device)
        m, cut, beyond, tied = eng.random_mask(self._d_scores, self._d_inverse, n_keep,
                                               self.num_edges, out=out)
        info = _select_info("device", cut, beyond, tied, n_keep)
        if info["ambiguous"] and self.tie_break == "numpy":
            # np.argsort's unstable order decides inside the tie block: make that call
            info["path"] = "host"
            m = _host_keep_mask(self.undirected_scores, self.inverse_idx, n_keep)
        self.last_selection = info
        if isinstance(m, np.ndarray):
            m = torch.from_numpy(m).to(ei.device)
        return m

    def sparsify(self, retention_ratio: float, device: str) -> Data:
        """``random_sparsify(data, scores, inverse, retention_ratio, device)``."""
        if retention_ratio == 1.0:
            self.last_selection = {"path": self.path}
            return self.data.clone()
        mask = self.mask(retention_ratio)
        sparse = self.data.clone()
        sparse.edge_index = self.data.edge_index[:, mask].to(device)
        return sparse

    def sweep(self, retention_ratios, device: str) -> list:
        """One sparsified ``Data`` per retention rate, from the resident ids and scores."""
        return [self.sparsify(r, device) for r in retention_ratios]


def precompute_random_scores(data: Data, seed: int = 42):
    """Reproducible symmetric random score per undirected edge (random.py:14-33):
    ``(undirected_scores, inverse_idx)`` as NumPy arrays, built on the device."""
    rb = RandomBaseline(data, seed)
    _record({"path": rb.path})
    return rb.undirected_scores, rb.inverse_idx


def _device_arrays(undirected_scores, inverse_idx, num_edges):
    """The caller's arrays in the form gs_random_mask takes, or None where only NumPy's
    own indexing rules can say what they mean."""
    s = undirected_scores
    if not getattr(s, "is_cuda", False):
        s = np.asarray(s)
        if s.ndim != 1 or s.dtype != np.float64 or len(s) < 1 or np.isnan(s).any():
            return None  # NaN: np.argsort's order among NaNs and the device keys may differ
    elif s.dim() != 1 or str(s.dtype) != "torch.float64" or s.numel() < 1 or bool(s.isnan().any()):
        return None
    inv = inverse_idx
    if not getattr(inv, "is_cuda", False):
        inv = np.asarray(inv)
        if inv.ndim != 1 or inv.dtype.kind not in "iu" or inv.dtype == np.uint64:
            return None
        inv = inv.astype(np.int64, copy=False)
    elif inv.dim() != 1 or str(inv.dtype) != "torch.int64":
        return None
    if len(inv) != num_edges:
        return None
    return s, inv


def random_sparsify(data: Data, undirected_scores, inverse_idx, retention_ratio: float,
                    device: str, tie_break=None) -> Data:
    """Keep the top fraction of undirected edges by random score (random.py:36-52).

    The arrays are uploaded as given (nothing is cached between calls; use
    ``RandomBaseline`` for a sweep) and gs_random_mask selects and gathers."""
    tb = _tie_break(tie_break)
    if retention_ratio == 1.0:
        _record({"path": "host"})
        return data.clone()
    eng = _engine(data, None)
    E = int(data.edge_index.size(1))
    arrays = _device_arrays(undirected_scores, inverse_idx, E) if eng is not None else None
    if arrays is None:
        _record({"path": "host"})
        return _host_random_sparsify(data, undirected_scores, inverse_idx, retention_ratio, device)
    import torch

    s, inv = arrays
    n_keep = max(1, int(len(s) * retention_ratio))
    ei = data.edge_index
    out = torch.empty(E, dtype=torch.bool, device=ei.device) if on_device(ei, eng.ctx.device) else None
    mask, cut, beyond, tied = eng.random_mask(s, inv, n_keep, E, out=out)
    info = _select_info("device", cut, beyond, tied, n_keep)
    if info["ambiguous"] and tb == "numpy":
        _record(dict(info, path="host"))
        return _host_random_sparsify(data, to_host(undirected_scores), to_host(inverse_idx),
                                     retention_ratio, device)
    _record(info)
    if isinstance(mask, np.ndarray):
        mask = torch.from_numpy(mask).to(ei.device)
    sparse = data.clone()
    sparse.edge_index = ei[:, mask].to(device)
    return sparse
