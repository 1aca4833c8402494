"""Host side of every ragged audio entry point: the F0 trackers, the stress conditions, WORLD synthesis, pitch shift
and ``RaggedResampler``.  A ragged batch is rows packed back to back in a 1-D tensor or padded in a 2-D one; here it
becomes lengths and offsets (``row_layout``), the int64 arrays and the zeroed plan a C row plan fills (``plan_arrays``, ``plan_meta``;
every such plan opens with offset and length), and that plan with its device copy (``device_plan``).  Also what those
callers share around it: the refusal of anything but float32 device audio (``check_waves``), host pointers for ctypes
(``host_ptrs``), per-call scratch (``workspace``) and the roots of the LDS transforms of ``csrc/dsp.h`` (``fft_roots``,
``real_split_roots``)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


def host_ptrs(*arrays) -> list:
    """Addresses of host arrays for a ctypes call (None stays None: NULL)."""
    return [None if a is None else a.ctypes.data for a in arrays]


def i64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int64).reshape(-1)


def packed_offsets(lengths) -> np.ndarray:
    """Start of each row when rows of ``lengths`` lie back to back: the exclusive prefix sum, int64."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    return np.cumsum(lengths, dtype=np.int64) - lengths


def row_layout(x, lengths=None, *, whole_by_default: bool = False):
    """``(lengths, offsets)`` of the rows of ``x`` as lists of int, offsets in elements from ``x``'s first.

    1-D ``x``: rows packed back to back; ``lengths`` is required unless ``whole_by_default``, which reads a missing
    one as a single row of all of ``x``; their sum may stay below ``x.numel()`` (trailing slack).
    2-D ``x``: one padded row per ``x[r]``, at ``r * x.stride(0)``; ``lengths`` defaults to the width.
    ``ValueError`` on a negative length, a length above the width, a count other than the number of 2-D rows, or a
    sum above ``x.numel()``."""
    if x.dim() == 2:
        B, width = int(x.shape[0]), int(x.shape[1])
        lengths = [width] * B if lengths is None else [int(n) for n in lengths]
        if len(lengths) != B:
            raise ValueError(f"ragged rows: {len(lengths)} lengths for {B} padded rows")
        if any(n > width for n in lengths):
            raise ValueError("ragged rows: a row length exceeds the padded width")
        offsets = [r * int(x.stride(0)) for r in range(B)]
    elif x.dim() == 1:
        if lengths is None:
            if not whole_by_default:
                raise ValueError("ragged rows: packed rows need their lengths")
            lengths = [int(x.numel())]
        lengths = [int(n) for n in lengths]
        offsets = packed_offsets(lengths).tolist()
        if sum(lengths) > x.numel():
            raise ValueError("ragged rows: packed row lengths exceed the input")
    else:
        raise ValueError("ragged rows: a 1-D packed or a 2-D padded tensor is expected")
    if any(n < 0 for n in lengths):
        raise ValueError("ragged rows: a row length is negative")
    return lengths, offsets


def check_waves(x, who: str) -> None:
    """``RuntimeError`` in ``who``'s name unless ``x`` is float32 device audio, 1-D or 2-D with contiguous rows."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() not in (1, 2) or \
            (x.numel() > 0 and x.stride(-1) != 1):
        raise RuntimeError(f"{who} (HIP) needs contiguous-row float32 device audio; no CPU fallback exists")


def plan_meta(fields_fn: str, R: int) -> np.ndarray:
    """The zeroed ``(max(R, 1), fields_fn())`` int64 plan that a C row plan of R rows fills."""
    return np.zeros((max(int(R), 1), getattr(_lib.load(), fields_fn)()), np.int64)


def plan_arrays(fields_fn: str, lengths, offsets, mismatch: str):
    """``(R, lengths, offsets, meta)`` for a C row plan: int64 arrays (packed when ``offsets`` is None) and the zeroed
    plan.  ``ValueError(mismatch)`` unless there is one offset per row."""
    lengths = i64(lengths)
    R = int(lengths.size)
    offsets = packed_offsets(lengths) if offsets is None else i64(offsets)
    if offsets.size != R:
        raise ValueError(mismatch)
    return R, lengths, offsets, plan_meta(fields_fn, R)


def device_plan(x, lengths, plan, who: str) -> dict:
    """``plan(lengths, offsets)`` (a dict with the host plan as ``meta``) of ``x`` in one of the three layouts (one 1-D
    wave, packed rows with ``lengths``, padded rows), with its device copy as ``meta_d``."""
    check_waves(x, who)
    pl = plan(*row_layout(x, lengths, whole_by_default=True))
    pl["meta_d"] = torch.from_numpy(pl["meta"]).to(x.device)
    return pl


def workspace(n_bytes, device) -> torch.Tensor:
    """Scratch of a call: a fresh allocation every time (never empty, so it has a data pointer)."""
    return torch.empty((max(int(n_bytes), 1),), dtype=torch.uint8, device=device)


def fft_roots(C: int) -> np.ndarray:
    """The C-th roots of unity with the forward sign, exp(-2 pi i m / C) for m < C: float64, shape (C, 2)."""
    m = np.arange(C, dtype=np.float64)
    return np.stack([np.cos(2 * np.pi * m / C), -np.sin(2 * np.pi * m / C)], axis=1)


def real_split_roots(C: int) -> np.ndarray:
    """exp(-2 pi i k / 2C) for k <= C (a packed C-point transform -> the real 2C-point one): float64, (C + 1, 2)."""
    k = np.arange(C + 1, dtype=np.float64)
    return np.stack([np.cos(np.pi * k / C), -np.sin(np.pi * k / C)], axis=1)
