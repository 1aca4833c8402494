"""Host side of every ragged audio entry point: the F0 trackers, the stress conditions, WORLD synthesis and CheapTrick,
pitch shift, ``RaggedResampler``, the noise, the stimuli and the room responses.  A ragged batch is rows packed back to
back in a 1-D tensor or padded in a 2-D one; here it becomes lengths and offsets (``row_layout``), the int64 arrays and
the zeroed plan a C row plan fills (``plan_arrays``, ``plan_meta``; every such plan opens with offset and length), and
that plan with its device copy (``device_plan``; ``to_device`` for a plan that also has a ``params`` table).  Also what
those callers share around it: the refusal of anything but a GPU device (``gpu_device``), but float32 device audio
(``check_waves``) or but a contiguous device tensor of a dtype (``check_device_tensor``), one value per row from a
number or a sequence (``per_row``), where a plan's rows end (``plan_extent``) and the output made or checked for them
(``plan_output``), recordings or tracks as one packed batch (``PackedRecordings``, ``pack_tracks``), host pointers for
ctypes (``host_ptrs``), per-call scratch (``workspace``) and the roots of the LDS transforms of ``csrc/dsp.h``
(``fft_roots``, ``real_split_roots``)."""
from __future__ import annotations

import hashlib

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


def gpu_device(device, who: str) -> torch.device:
    """``device`` as a ``torch.device``; ``RuntimeError`` in ``who``'s name unless it is a GPU."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{who} (HIP) needs a GPU device, got {device}; no CPU fallback exists")
    return device


def check_device_tensor(t, who: str, dtype=torch.float32) -> None:
    """``RuntimeError`` in ``who``'s name unless ``t`` is a contiguous device tensor of ``dtype``."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"{who} (HIP) needs a contiguous {str(dtype).replace('torch.', '')} device tensor; "
                           "no CPU fallback exists")


def per_row(value, R: int, what: str, dtype=np.int64) -> np.ndarray:
    """One value per row as a ``dtype`` array: a number serves every row, a sequence must have exactly ``R`` values,
    else ``ValueError(what)``."""
    if np.ndim(value) == 0:
        return np.full(int(R), value, dtype)
    values = np.ascontiguousarray(value, dtype=dtype).reshape(-1)
    if values.size != R:
        raise ValueError(what)
    return values


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


def to_device(pl: dict, device) -> dict:
    """The plan with the device copies of its two tables (``meta_d``, ``params_d``), made once per device."""
    device = torch.device(device)
    if "meta_d" not in pl or pl["meta_d"].device != device:
        pl["meta_d"] = torch.from_numpy(pl["meta"]).to(device)
        pl["params_d"] = torch.from_numpy(pl["params"]).to(device)
    return pl


def plan_extent(pl: dict) -> int:
    """Where the last row of a plan (``rows``, ``offsets``, ``lengths``) ends in its output."""
    return int(np.max(pl["offsets"] + pl["lengths"])) if pl["rows"] else 0


def plan_output(pl: dict, out, device, who: str, short: str = "the output is shorter than the plan's rows"):
    """The output of a plan's rows: a zeroed float32 tensor of the plan's extent (never empty) on ``device``, or ``out``
    itself: ``RuntimeError`` unless it is a contiguous float32 device tensor, ``ValueError`` if the rows do not fit."""
    if out is None:
        return torch.zeros((max(plan_extent(pl), 1),), dtype=torch.float32, device=device)
    check_device_tensor(out, who)
    if out.numel() < plan_extent(pl):
        raise ValueError(f"{who}: {short}")
    return out


class PackedRecordings:
    """K recordings (1-D float arrays of any length >= 1, taken as they are) as one ragged batch on the host: the
    float32 arrays, ``lengths`` and ``offsets`` (lists), ``packed`` (back to back) and ``key``, the sha1 of lengths and
    samples that names the set's device tables.  ``ValueError(empty)`` for no recording or an empty one."""

    def __init__(self, recordings, empty: str):
        self._items = [np.ascontiguousarray(np.asarray(h, dtype=np.float32).reshape(-1)) for h in recordings]
        if not self._items or any(h.size < 1 for h in self._items):
            raise ValueError(empty)
        self.lengths = [int(h.size) for h in self._items]
        self.offsets = packed_offsets(self.lengths).tolist()
        self.packed = np.concatenate(self._items)
        self.key = hashlib.sha1(np.asarray(self.lengths, np.int64).tobytes() + self.packed.tobytes()).hexdigest()

    def __len__(self):
        return len(self._items)


def pack_tracks(tracks, device):
    """``(packed, offsets, lengths)`` of R tracks (tensors or arrays, flattened) as float32 on ``device``: back to
    back in one tensor that a trailing zero keeps from being empty."""
    def track(t):
        if isinstance(t, torch.Tensor):
            return t.detach().reshape(-1).to(device, torch.float32)
        return torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=np.float32).reshape(-1))).to(device)

    rows = [track(t) for t in tracks]
    lengths = [int(t.numel()) for t in rows]
    tail = torch.zeros(1, dtype=torch.float32, device=rows[0].device if rows else device)
    return torch.cat(rows + [tail]), packed_offsets(lengths).tolist(), lengths


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
