"""Host-side layout of a ragged batch: rows packed back to back in a 1-D tensor or padded in a 2-D one, as lengths and
offsets.  Everything that takes such a batch reads it through here: ``RaggedResampler``, the pitch-shift ``Plan``, and
the F0 trackers through ``f0_tracker._RaggedTracker`` (``PraatACTracker``, ``WorldDioTracker``), whose C row plans then
open with exactly these two numbers per row (offset, length)."""
from __future__ import annotations

import numpy as np


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
