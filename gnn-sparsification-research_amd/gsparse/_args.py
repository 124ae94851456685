"""How an array reaches libgsparse: the one place that decides pointer side, dtype and size.

The library takes a raw pointer and a GS_HOST / GS_DEVICE flag and trusts both: a wrong
flag, a buffer of another dtype, a short or a strided one is an out-of-bounds access on
the device, not an exception.  So every array handed to ``Context.call`` passes through
``inp`` (the library reads it) or ``out`` (the library writes it) first:

* NumPy arrays, CPU tensors and sequences are host buffers; a CUDA tensor is a device
  buffer and must live on the context's device (ValueError).
* An input is made contiguous (a copy where needed; keep the returned array alive for
  the call).  Its dtype is converted on the sides ``cast`` names, else a TypeError.
* An output is the caller's own buffer, never a copy: a wrong dtype is a TypeError, a
  strided or a short one a ValueError (``short`` names another exception where NumPy's
  own IndexError is mimicked).  Without a buffer a fresh host array is made.
"""

from __future__ import annotations

import numpy as np

from ._lib import GS_DEVICE, GS_HOST


def is_tensor(a) -> bool:
    return hasattr(a, "is_cuda") and hasattr(a, "data_ptr")


def on_device(a, device: int) -> bool:
    """Whether ``a`` is a CUDA tensor on device ordinal ``device``."""
    return is_tensor(a) and a.is_cuda and a.device.index == device


def to_host(a):
    """A CUDA tensor's values as a NumPy array; anything else as it is."""
    return a.cpu().numpy() if is_tensor(a) and a.is_cuda else a


def dtype_of(a):
    """The NumPy dtype of an array's or a tensor's elements (None where NumPy has none)."""
    if isinstance(a, np.ndarray):
        return a.dtype
    try:
        return np.dtype(str(a.dtype).rpartition(".")[2])
    except TypeError:
        return None


def _dtypes(dtype):
    return tuple(np.dtype(d) for d in (dtype if isinstance(dtype, tuple) else (dtype,)))


def _side(a, device: int, name: str) -> int:
    if not (is_tensor(a) and a.is_cuda):
        return GS_HOST
    if a.device.index != device:
        raise ValueError(f"{name} is on {a.device}, the context drives cuda:{device}")
    return GS_DEVICE


def inp(a, dtype, name: str, device: int, count: int | None = None, cast: str = "host",
        short=ValueError):
    """An array the library reads: ``(contiguous array to keep alive, loc)``.

    ``dtype``: the element type, or a tuple of accepted ones (the first is what a
    conversion gives), or None to keep the array's own.  ``cast``: "both" converts a
    wrong dtype on either side, "host" only host data (a CUDA tensor of another dtype is
    a TypeError), "never" refuses it on both.  Fewer than ``count`` elements: ``short``."""
    dts = None if dtype is None else _dtypes(dtype)
    loc = _side(a, device, name)
    if loc == GS_HOST:
        a = a.detach().numpy() if is_tensor(a) else np.asarray(a)
    wrong = dts is not None and dtype_of(a) not in dts
    if wrong and (cast == "never" or (cast == "host" and loc == GS_DEVICE)):
        raise TypeError(f"{name} must be {' or '.join(d.name for d in dts)}, got {a.dtype}")
    if loc == GS_HOST:
        a = np.ascontiguousarray(a, dtype=dts[0] if wrong else None)
    else:
        if wrong:
            import torch

            a = a.to(getattr(torch, dts[0].name))
        a = a.contiguous()
    if count is not None and size(a) < count:
        raise short(f"{name} holds {size(a)} < {count} values")
    return a, loc


def out(buf, dtype, count: int, name: str, device: int, fresh=np.empty, short=ValueError):
    """A buffer the library writes ``count`` elements into: ``(buffer, loc)``.  ``buf``
    None: ``fresh(count, dtype)`` on the host; else the caller's array or tensor itself."""
    dts = _dtypes(dtype)
    if buf is None:
        return fresh(count, dtype=dts[0]), GS_HOST
    if not (is_tensor(buf) or isinstance(buf, np.ndarray)) or dtype_of(buf) not in dts:
        raise TypeError(f"{name} must be a {' or '.join(d.name for d in dts)} array or tensor, "
                        f"got {getattr(buf, 'dtype', type(buf).__name__)}")
    if not (buf.is_contiguous() if is_tensor(buf) else buf.flags.c_contiguous):
        raise ValueError(f"{name} must be contiguous")
    if size(buf) < count:
        raise short(f"{name} holds {size(buf)} values, the library writes {count}")
    return buf, _side(buf, device, name)


def size(a) -> int:
    """Elements of an array or a tensor."""
    return a.size if isinstance(a, np.ndarray) else a.numel()


def pair(src, dst, device: int, cast: str = "both"):
    """The int64 ``src`` / ``dst`` ids of E columns, both on one side:
    ``(src, dst, E, loc)``."""
    src, loc = inp(src, np.int64, "src", device, cast=cast)
    dst, dloc = inp(dst, np.int64, "dst", device, cast=cast)
    if loc != dloc:
        raise ValueError("src and dst must both be numpy arrays or both CUDA tensors")
    E = int(src.shape[0])
    if int(dst.shape[0]) != E:
        raise ValueError(f"src holds {E} ids, dst {int(dst.shape[0])}")
    return src, dst, E, loc


def mask_out(buf, count: int, device: int, name: str = "out"):
    """A keep mask of ``count`` bytes: the caller's uint8/bool buffer (ValueError for any
    other) or a zeroed host array of max(count, 1) bytes."""
    try:
        return out(buf, (np.uint8, np.bool_), max(count, 1) if buf is None else count, name,
                   device, fresh=np.zeros)
    except TypeError as e:
        raise ValueError(str(e)) from None


def alloc(count: int, dtype, like):
    """A zeroed host array, or an uninitialised tensor on ``like``'s device when ``like``
    (a value ``inp`` returned) is a CUDA tensor: a result that lives where the ids do."""
    if not (is_tensor(like) and like.is_cuda):
        return np.zeros(count, dtype=dtype)
    import torch

    return torch.empty(count, dtype=getattr(torch, np.dtype(dtype).name), device=like.device)


def as_bool(mask):
    """A uint8 mask array or tensor viewed as bool."""
    if isinstance(mask, np.ndarray):
        return mask.view(bool)
    import torch

    return mask.view(torch.bool)


def pcg64_words(rng: np.random.Generator):
    """(state_hi, state_lo, inc_hi, inc_lo) of a Generator(PCG64)."""
    st = rng.bit_generator.state
    if st.get("bit_generator") != "PCG64":
        raise NotImplementedError("the device stream supports the PCG64 bit generator")
    if st.get("has_uint32"):
        raise NotImplementedError("PCG64 state with a buffered uint32")
    s, inc = int(st["state"]["state"]), int(st["state"]["inc"])
    m64 = (1 << 64) - 1
    return s >> 64, s & m64, inc >> 64, inc & m64
