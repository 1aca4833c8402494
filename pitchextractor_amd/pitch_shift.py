"""On-device pitch shifting: ``librosa.effects.pitch_shift(y, sr=sr, n_steps=s, res_type=...)`` with librosa 0.10's
defaults, as the reference's synthetic-data generator calls it (meldataset.py:324-517).

STFT (n_fft 2048, hop 512, periodic Hann, centre zero padding) -> phase vocoder at ``rate = 2**(-s/12)`` -> iSTFT to
``round(N / rate)`` samples -> resampy's band-limited sinc interpolation from ``sr / rate`` back to ``sr`` -> fixed to
N samples (at ``n_steps = 0`` the two rates are equal and the stretched signal is copied, as librosa's ``resample``
returns its input then).  Four HIP stages (``csrc/pitch_shift.hip``); there is no CPU path.  The resampling filters are resampy's
``kaiser_best`` / ``kaiser_fast`` rebuilt from their published parameters (not from resampy's data files, which are not
available here): parity with librosa / resampy is unpinned, see DESIGN.md.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, ops
from .ragged import host_ptrs, plan_arrays

N_FFT, HOP = 2048, 512
N_BINS = N_FFT // 2 + 1
TABLE_PRECISION = 512                                     # resampy: 2 ** 9 table entries per zero crossing
# res_type -> (zero crossings, rolloff, Kaiser beta)
RES_TYPES = {"kaiser_best": (64, 0.9475937167399596, 14.769656459379492),
             "kaiser_fast": (16, 0.85, 8.555041594543659)}
MAX_SEMITONES = 24.0


# --------------------------------------------------------------------------- host-side lengths (no device needed)
def stretch_rate(n_steps: float) -> float:
    """2 ** (-s / 12) at the step the plan sees: ``Plan`` hands ``n_steps`` over as float32, so every length below
    is formed from the rounded step too (0.35 or 7.3 are not float32 numbers; M, int(M r) and the column count
    differ at some lengths otherwise)."""
    return 2.0 ** (-float(np.float32(n_steps)) / 12)


def stft_frames(n: int) -> int:
    return 1 + int(n) // HOP


def stretched_columns(n: int, n_steps: float) -> int:
    """len(np.arange(0, frames, rate)): columns of the phase vocoder's output."""
    return int(math.ceil(stft_frames(n) / stretch_rate(n_steps)))


def stretched_len(n: int, n_steps: float) -> int:
    """M = int(round(N / rate)): length of the time-stretched signal."""
    return int(round(int(n) / stretch_rate(n_steps)))


def resample_ratio(n_steps: float, sr: int) -> float:
    return float(sr) / (float(sr) / stretch_rate(n_steps))


def resampled_len(n: int, n_steps: float, sr: int) -> int:
    """int(M * r): samples resampy produces; the output is zero from there to N."""
    return int(stretched_len(n, n_steps) * resample_ratio(n_steps, sr))


def check_res_type(res_type: str) -> str:
    if res_type not in RES_TYPES:
        raise ValueError(f"pitch shift resample_type {res_type!r} is not supported on the HIP path: use one of "
                         f"{sorted(RES_TYPES)}")
    return res_type


def resample_filter(res_type: str = "kaiser_best") -> np.ndarray:
    """float64 right wing of resampy's windowed-sinc filter: kaiser(2n+1, beta)[n:] * rolloff * sinc(rolloff * t),
    t = linspace(0, zeros, n + 1), n = zeros * 512."""
    zeros, rolloff, beta = RES_TYPES[check_res_type(res_type)]
    n = zeros * TABLE_PRECISION
    return np.kaiser(2 * n + 1, beta)[n:] * rolloff * np.sinc(rolloff * np.linspace(0, zeros, num=n + 1))


# --------------------------------------------------------------------------- batch layout
class Plan:
    """Host layout of a ragged batch (``pe_pitch_shift_plan``): per-row int64 fields, (rate, ratio) pairs and the
    workspace sizes {frames, columns, stretched samples, output samples}."""

    def __init__(self, lengths, n_steps, x_offsets=None, out_start=None, out_len=None, out_rows=None,
                 out_stride=None, *, sr: int, res_type: str = "kaiser_best"):
        self.res_type = check_res_type(res_type)
        mismatch = "pitch shift plan: per-row arrays differ in length"
        R, lengths, self.x_offsets, self.meta = plan_arrays("pe_pitch_shift_plan_fields", lengths, x_offsets, mismatch)
        self.n_rows = R
        self.lengths = lengths
        self.n_steps = np.ascontiguousarray(n_steps, dtype=np.float32).reshape(-1)
        self.out_start = np.zeros(R, np.int64) if out_start is None else np.ascontiguousarray(out_start, np.int64)
        self.out_len = lengths.copy() if out_len is None else np.ascontiguousarray(out_len, np.int64)
        self.out_rows = np.arange(R, dtype=np.int64) if out_rows is None else np.ascontiguousarray(out_rows, np.int64)
        self.out_stride = int(self.out_len.max(initial=0) if out_stride is None else out_stride)
        if not (self.n_steps.size == self.out_start.size == self.out_len.size == self.out_rows.size == R):
            raise ValueError(mismatch)
        self.ratios = np.zeros((max(R, 1), 2), np.float64)
        self.totals = np.zeros(4, np.int64)
        _lib.check(_lib.load().pe_pitch_shift_plan(
            R, *host_ptrs(self.lengths, self.n_steps, self.x_offsets, self.out_start, self.out_len, self.out_rows),
            self.out_stride, int(sr), N_FFT, HOP, list(RES_TYPES).index(self.res_type),
            *host_ptrs(self.meta, self.ratios, self.totals)), "pe_pitch_shift_plan")
        self.n_frames, self.n_cols, self.n_stretched, self.n_out = (int(v) for v in self.totals)


class PitchShifter:
    """``table``: the device copy of a resampling filter; ``run`` executes the four stages for a ``Plan``."""

    def table(self, res_type, device):
        def build():                                      # the filter's right wing, then its forward differences
            w = resample_filter(res_type)
            d = np.zeros_like(w)
            d[:-1] = np.diff(w)
            return np.concatenate([w, d])
        return _lib.device_table(("resampy", res_type), device, build)

    def run(self, plan: Plan, waves, gains, out, noise=None, keep=False, spec=None):
        """waves: flat float32 device audio addressed by the plan's x offsets; gains (R,) float32 device; out: float32
        device tensor addressed by out_row * out_stride + i.  ``spec`` replaces the STFT stage's output (tests).
        Returns the intermediate buffers when ``keep``."""
        dev = out.device
        for name, t in (("waves", waves), ("gains", gains), ("out", out), ("noise", noise), ("spec", spec)):
            if t is not None and (not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous()):
                raise RuntimeError(f"pitch shift: {name} must be a contiguous float32 device tensor (no CPU path)")
        if plan.n_rows == 0 or plan.n_out == 0:
            return {} if keep else None
        if gains.numel() != plan.n_rows:
            raise ValueError("pitch shift: one gain per row")
        if noise is not None and noise.numel() != plan.n_out:
            raise ValueError("pitch shift: noise must hold one value per output sample")
        need = int((plan.out_rows * plan.out_stride + plan.out_len).max(initial=0))
        if out.numel() < need or waves.numel() < int((plan.x_offsets + plan.lengths).max(initial=0)):
            raise ValueError("pitch shift: input or output buffer smaller than the plan addresses")
        meta = torch.from_numpy(plan.meta).to(dev, non_blocking=False)
        ratios = torch.from_numpy(plan.ratios).to(dev, non_blocking=False)
        R = plan.n_rows
        if spec is None:
            spec = torch.empty((plan.n_frames, N_BINS, 2), dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                ops._call("pe_pitch_shift_stft", waves.data_ptr(), meta.data_ptr(), R, plan.n_frames, spec.data_ptr(),
                          _lib.stream_ptr(), work=float(plan.n_frames * (N_FFT + 2 * N_BINS) * 4))
        elif spec.numel() != plan.n_frames * N_BINS * 2:
            raise ValueError("pitch shift: spec does not match the plan")
        cols = torch.empty((plan.n_cols, N_BINS, 2), dtype=torch.float32, device=dev)
        frames = torch.empty((plan.n_cols, N_FFT), dtype=torch.float32, device=dev)
        stretched = torch.empty((plan.n_stretched,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ops._call("pe_pitch_shift_vocoder", spec.data_ptr(), meta.data_ptr(), ratios.data_ptr(), R, plan.n_cols,
                      cols.data_ptr(), _lib.stream_ptr(), work=float(plan.n_cols * N_BINS * 8 * 3))
            ops._call("pe_pitch_shift_istft", cols.data_ptr(), meta.data_ptr(), R, plan.n_cols, plan.n_stretched,
                      frames.data_ptr(), stretched.data_ptr(), _lib.stream_ptr(),
                      work=float(plan.n_cols * (N_BINS * 8 + N_FFT * 8) + plan.n_stretched * 4 * 5))
            ops._call("pe_pitch_shift_resample", stretched.data_ptr(), meta.data_ptr(), ratios.data_ptr(),
                      self.table(plan.res_type, dev).data_ptr(), list(RES_TYPES).index(plan.res_type),
                      gains.data_ptr(), _lib.ptr(noise), R, plan.n_out, out.data_ptr(), _lib.stream_ptr(),
                      work=float(plan.n_out * 8))
        if keep:
            return {"spec": torch.view_as_complex(spec), "cols": torch.view_as_complex(cols), "frames": frames,
                    "stretched": stretched, "meta": plan.meta, "ratios": plan.ratios}
        return None


_SHIFTER = PitchShifter()


def pitch_shift(y: torch.Tensor, *, sr: int, n_steps: float, res_type: str = "kaiser_best") -> torch.Tensor:
    """librosa's signature on a 1-D float32 device tensor; returns a tensor of the same length."""
    if y.dim() != 1:
        raise ValueError("pitch_shift expects a 1-D waveform; use pitch_shift_ragged for batches")
    y = y.contiguous()
    out = torch.empty_like(y)
    plan = Plan([y.numel()], [n_steps], sr=sr, res_type=res_type)
    _SHIFTER.run(plan, y, torch.ones(1, dtype=torch.float32, device=y.device), out)
    return out


def pitch_shift_ragged(waves: torch.Tensor, offsets, lengths, n_steps, gains: torch.Tensor, out: torch.Tensor,
                       out_rows=None, out_start=None, out_len=None, *, sr: int, res_type: str = "kaiser_best",
                       noise: torch.Tensor | None = None) -> torch.Tensor:
    """Ragged batch.  ``waves``: flat float32 device audio, row r at ``offsets[r]`` with ``lengths[r]`` samples (host
    sequences), shifted by ``n_steps[r]`` and scaled by ``gains[r]``; output samples ``[out_start[r], out_start[r] +
    out_len[r])`` of row r (default: all of them) go to ``out[out_rows[r], :out_len[r]]`` of the 2-D ``out``, plus
    ``noise`` (flat, the windows back to back) when given.  Returns ``out``."""
    if out.dim() != 2:
        raise ValueError("out must be 2-D (rows, samples)")
    plan = Plan(lengths, n_steps, offsets, out_start, out_len, out_rows, out.stride(0), sr=sr, res_type=res_type)
    if out.stride(1) != 1:
        raise ValueError("out rows must be contiguous")
    _SHIFTER.run(plan, waves.contiguous(), gains.to(out.device, torch.float32).contiguous(), out, noise)
    return out
