"""Additive noise at an SNR on the device (``csrc/noise.hip``): seeded white noise, white noise coloured by a bank of
one-pole sections (pink, brown, or a custom colour), a recorded bed looped, and the mix at a signal-to-noise ratio with
the notebooks' peak rule.  It is the degradation the reference leaves to its users (its
Utils/noise_robustness_evaluation.ipynb is a stub and its README asks for "your own noise augmentation").  There is no
CPU path.  ``tests/noise_ref.py`` is the float64 restatement that pins every stage.

Every function takes or makes a ragged batch the way the stress conditions do: rows packed back to back in a 1-D tensor
with ``lengths``, or padded in a 2-D one.  A row's result is bit-identical whether the row is made alone, packed at an
odd offset or padded, and depends on its own seed, not on its position in the batch; a stage's launch count does not
depend on the rows.  Rows of length 0 are valid.

Conventions: sample ``j`` of a seeded row is ``z(seed, j)``, Philox4x32-10 keyed by the seed with counter ``j`` and
Box-Muller of its first two words in float32 (``world.synthesize``'s drawn noise); a coloured row runs ``warmup``
samples that are not written, so sample ``i`` is generated sample ``warmup + i``; the SNR is over the whole row,
silence included."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, ops
from .ragged import (PackedRecordings, check_device_tensor, check_waves, gpu_device, host_ptrs, i64, per_row,
                     plan_arrays, plan_extent, plan_output, row_layout, to_device, workspace)

MAX_SECTIONS = 8
NOISE_COLOURS = ("white", "pink", "brown")
STAT_KEYS = ("peak", "rms_signal", "rms_noise", "scale")           # of the mix at an SNR; stimuli.finish's too
BROWN_CORNER_HZ = 20.0
# d0, d1 and the (pole, gain) sections of the pink filter: a pole-zero fit of 1 / sqrt(f) whose poles are fixed in z, so
# the response follows -3 dB / octave from sr / 2000 to sr / 2.2 within 0.059 dB peak to peak at any rate
_PINK = (0.5362, 0.115926, ((0.99886, 0.0555179), (0.99332, 0.0750759), (0.96900, 0.1538520), (0.86650, 0.3104856),
                            (0.55000, 0.5329522), (-0.7616, -0.0168980)))


def colour_sections(colour, sr):
    """``(d0, d1, [(a, b), ...])`` in float64 of a colour: ``y[j] = d0 w[j] + d1 w[j - 1] + sum_k s_k[j]`` with
    ``s_k[j] = a_k s_k[j - 1] + b_k w[j]``.  ``colour``: a name in ``NOISE_COLOURS`` (``"brown"`` is one leaky
    integrator with its corner at 20 Hz) or a dict ``{"d0", "d1", "sections"}`` of the same shape.  ``ValueError`` for an
    unknown name, more than 8 sections, a non-finite coefficient or a pole with ``|a| >= 1``."""
    sr = float(sr)
    if not (math.isfinite(sr) and sr > 0.0):
        raise ValueError(f"noise: sr must be positive and finite, got {sr!r}")
    if isinstance(colour, str):
        if colour not in NOISE_COLOURS:
            raise ValueError(f"noise colour {colour!r} is not one of {NOISE_COLOURS}")
        if colour == "white":
            d0, d1, sections = 1.0, 0.0, []
        elif colour == "pink":
            d0, d1, sections = _PINK[0], _PINK[1], list(_PINK[2])
        else:
            d0, d1, sections = 0.0, 0.0, [(math.exp(-2.0 * math.pi * BROWN_CORNER_HZ / sr), 1.0)]
    elif isinstance(colour, dict):
        d0, d1 = float(colour.get("d0", 0.0)), float(colour.get("d1", 0.0))
        sections = [(float(a), float(b)) for a, b in colour.get("sections", ())]
    else:
        raise ValueError("noise: a colour is a name in NOISE_COLOURS or a dict {'d0', 'd1', 'sections'}")
    if len(sections) > MAX_SECTIONS:
        raise ValueError(f"noise: a colour has at most {MAX_SECTIONS} sections, got {len(sections)}")
    if not all(math.isfinite(v) for v in (d0, d1, *(c for s in sections for c in s))):
        raise ValueError("noise: a colour's coefficients must be finite")
    if any(not abs(a) < 1.0 for a, _ in sections):
        raise ValueError("noise: a section's pole must lie inside the unit circle (|a| < 1)")
    return d0, d1, sections


def row_seeds(seed, R: int) -> np.ndarray:
    """One int64 seed per row: ``seed + r`` for an int, the values themselves for a sequence of R."""
    if np.ndim(seed) == 0:
        base = int(seed)
        seeds = [base + r for r in range(R)]
    else:
        seeds = [int(s) for s in seed]
        if len(seeds) != R:
            raise ValueError("noise: one seed per row")
    return np.asarray([((s + 2 ** 63) % 2 ** 64) - 2 ** 63 for s in seeds], dtype=np.int64).reshape(-1)


def plan_rows(lengths, offsets=None, warmup=0, seeds=0, white_offsets=None, colour="white", sr=24000) -> dict:
    """``pe_noise_plan`` (host only): the row plan, the colour table and the constants.  ``offsets``: where each row
    lies in the output (default: packed); ``warmup``: an int or one per row; ``white_offsets``: where each row's given
    ``warmup + n`` white samples lie (default: drawn in the kernel)."""
    d0, d1, sections = colour_sections(colour, sr)
    lib = _lib.load()
    R, n, off, meta = plan_arrays("pe_noise_plan_fields", lengths, offsets, "noise plan: one offset per row")
    if np.any(n < 0):
        raise ValueError("noise plan: a row length is negative")
    one_each = "noise plan: one warm-up and one white offset per row"
    warm, woff = per_row(warmup, R, one_each), per_row(-1 if white_offsets is None else white_offsets, R, one_each)
    if np.any(warm < 0):
        raise ValueError("noise plan: a warm-up is negative")
    seed = row_seeds(seeds, R)
    coeffs = np.asarray([d0, d1] + [c for s in sections for c in s], np.float64)
    params = np.zeros(lib.pe_noise_param_fields(), np.float64)
    consts, totals = np.zeros(4, np.int64), np.zeros(2, np.int64)
    status = lib.pe_noise_plan(R, *host_ptrs(n, off, warm, seed, woff, coeffs), len(sections),
                               *host_ptrs(consts, meta, params, totals))
    if status == -1:
        raise ValueError("noise plan: pe_noise_plan refused a row or the colour (PE_E_ARG)")
    _lib.check(status, "pe_noise_plan")
    return dict(rows=R, lengths=n, offsets=off, warmup=warm, seeds=seed, white_offsets=woff, meta=meta, params=params,
                piece=int(consts[0]), stat_fields=int(consts[2]), bed_fields=int(consts[3]), n_samples=int(totals[0]),
                n_pieces=int(totals[1]), sections=len(sections))


def _ws(pl, device):
    n_bytes = _lib.load().pe_noise_workspace_bytes(pl["n_pieces"])
    return workspace(n_bytes, device), n_bytes


# -------------------------------------------------------------------------------------------------------------- stages
def white(lengths, seeds=0, device="cuda", offsets=None, warmup=0, out=None) -> torch.Tensor:
    """``pe_noise_white``: standard normals, row r from its own seed (``seeds``: an int, row r takes ``seeds + r``, or
    one per row).  Rows packed back to back, or at ``offsets`` of ``out``.  ``warmup``: the first sample's index in the
    row's stream.  One launch."""
    device = gpu_device(out.device if isinstance(out, torch.Tensor) else device, "noise")
    pl = to_device(plan_rows(lengths, offsets, warmup, seeds), device)
    y = plan_output(pl, out, device, "noise.white")
    with torch.cuda.device(device):
        ops._call("pe_noise_white", pl["meta_d"].data_ptr(), pl["meta"].ctypes.data, pl["rows"], y.data_ptr(),
                  _lib.stream_ptr())
    return y if out is not None else y[:plan_extent(pl)]


def coloured(lengths, colour, sr, seeds=None, white=None, warmup=4096, offsets=None, device="cuda", out=None):
    """``pe_noise_colour``: noise of a colour (``colour_sections``), row r either drawn from its seed (``seeds``, as
    ``white`` takes them; default 0) or filtered from given white noise (``white``: a packed float32 device tensor of
    ``warmup + n`` samples per row, back to back).  Each row runs ``warmup`` samples first, which lets the slow poles
    settle, and writes the ``n`` that follow.  Double arithmetic, rounded once to float32.  Three launches."""
    if white is not None and seeds is not None:
        raise ValueError("noise.coloured: seeds or white, not both")
    n = i64(lengths)
    woff = None
    if white is not None:
        check_device_tensor(white, "noise.coloured")
        device = white.device
        gen = n + per_row(warmup, n.size, "noise plan: one warm-up and one white offset per row")
        woff = np.cumsum(gen) - gen
        if int(np.sum(gen)) > white.numel():
            raise ValueError("noise.coloured: the white input needs warmup + n samples per row")
    device = gpu_device(out.device if isinstance(out, torch.Tensor) else device, "noise")
    pl = to_device(plan_rows(n, offsets, warmup, 0 if seeds is None else seeds, woff, colour, sr), device)
    y = plan_output(pl, out, device, "noise.coloured")
    ws, n_bytes = _ws(pl, device)
    with torch.cuda.device(device):
        ops._call("pe_noise_colour", pl["meta_d"].data_ptr(), pl["meta"].ctypes.data, pl["params_d"].data_ptr(),
                  pl["params"].ctypes.data, _lib.ptr(white), 0 if white is None else white.numel(), pl["rows"],
                  y.data_ptr(), ws.data_ptr(), n_bytes, _lib.stream_ptr())
    return y if out is not None else y[:plan_extent(pl)]


class NoiseSet(PackedRecordings):
    """K recorded noise beds (1-D float arrays of any length >= 1, taken as they are) as one ragged batch
    (``recordings``, ``lengths``, ``offsets``, ``packed``, ``key``), kept on the device once per set and device."""

    def __init__(self, recordings, device="cuda"):
        super().__init__(recordings, "NoiseSet: at least one recording, each of at least one sample")
        self.recordings = self._items
        self.device = torch.device(device)

    def audio(self, device=None) -> torch.Tensor:
        """The recordings back to back on the device."""
        device = gpu_device(self.device if device is None else device, "noise")
        return _lib.device_table(("noise_bed", self.key), device, lambda: self.packed)


def bed(noise_set: NoiseSet, lengths, index=0, start=0, offsets=None, device=None, out=None) -> torch.Tensor:
    """``pe_noise_bed``: row r is recording ``index[r]`` of the set looped from its sample ``start[r]`` (an int serves
    every row): ``out[i] = bed[(start + i) mod L]``.  ``ValueError`` for an index outside the set or a start outside the
    recording.  One launch."""
    if not isinstance(noise_set, NoiseSet):
        raise ValueError("noise.bed: a NoiseSet is expected")
    device = gpu_device(out.device if isinstance(out, torch.Tensor) else
                        (noise_set.device if device is None else device), "noise")
    pl = plan_rows(lengths, offsets)
    R = pl["rows"]
    one_each = "noise.bed: one index and one start per row"
    index, start = per_row(index, R, one_each).tolist(), per_row(start, R, one_each).tolist()
    if any(k < 0 or k >= len(noise_set) for k in index):
        raise ValueError("noise.bed: an index lies outside the set")
    if any(s < 0 or s >= noise_set.lengths[k] for k, s in zip(index, start)):
        raise ValueError("noise.bed: a start lies outside its recording")
    beds = np.zeros((max(R, 1), pl["bed_fields"]), np.int64)
    for r, (k, s) in enumerate(zip(index, start)):
        beds[r] = (noise_set.offsets[k], noise_set.lengths[k], s)
    to_device(pl, device)
    y = plan_output(pl, out, device, "noise.bed")
    audio = noise_set.audio(device)
    beds_d = torch.from_numpy(beds).to(device)
    with torch.cuda.device(device):
        ops._call("pe_noise_bed", pl["meta_d"].data_ptr(), pl["meta"].ctypes.data, audio.data_ptr(), audio.numel(),
                  beds_d.data_ptr(), beds.ctypes.data, R, y.data_ptr(), _lib.stream_ptr())
    return y if out is not None else y[:plan_extent(pl)]


def mix_at_snr(x, noise, snr_db, lengths=None, peak_normalize: bool = True, return_stats: bool = False):
    """``pe_noise_mix``: ``y = x + float32(noise * scale)`` with ``scale = float32((rms_s / 10^(snr_db / 20)) /
    rms_n)``, both rms in double over the row's float32 samples (the timbre notebook's mix); a row whose signal or noise
    is silent is a copy with ``scale = 0``.  ``peak_normalize``: then ``y / float32(peak + 1e-6)`` where ``peak = max|y|
    > 0.99`` (the notebooks' ``_normalize``).  ``x`` and ``noise`` share one layout (packed with ``lengths``, or padded);
    ``snr_db``: a number or one per row.  The result is dense of ``x``'s shape, zero outside the rows.
    ``return_stats``: also the ``(rows, 4)`` float64 ``STAT_KEYS`` on the device.  Five launches, four without the peak
    rule: the mix of ``csrc/snr_mix.h``, which ``stimuli.finish`` runs in place under its fade."""
    check_waves(x, "mix_at_snr")
    check_waves(noise, "mix_at_snr")
    if tuple(noise.shape) != tuple(x.shape) or noise.device != x.device:
        raise ValueError("mix_at_snr: x and noise share one shape and device")
    x, noise = x.contiguous(), noise.contiguous()
    row_lengths, offsets = row_layout(x, lengths, whole_by_default=True)
    pl = to_device(plan_rows(row_lengths, offsets), x.device)
    R = pl["rows"]
    snr = per_row(snr_db, R, "mix_at_snr: one snr_db per row", np.float64)
    if not np.all(np.isfinite(snr)):
        raise ValueError("mix_at_snr: snr_db must be finite")
    y = torch.zeros(tuple(x.shape), dtype=torch.float32, device=x.device)
    stats = torch.zeros((max(R, 1), pl["stat_fields"]), dtype=torch.float64, device=x.device)
    if R and pl["n_samples"]:
        snr_d = torch.from_numpy(snr).to(x.device)
        ws, n_bytes = _ws(pl, x.device)
        with torch.cuda.device(x.device):
            ops._call("pe_noise_mix", x.data_ptr(), noise.data_ptr(), pl["meta_d"].data_ptr(), pl["meta"].ctypes.data,
                      snr_d.data_ptr(), snr.ctypes.data, int(bool(peak_normalize)), R, y.data_ptr(), stats.data_ptr(),
                      ws.data_ptr(), n_bytes, _lib.stream_ptr())
    return (y, stats[:R]) if return_stats else y
