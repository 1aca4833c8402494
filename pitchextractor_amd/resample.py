"""On-device resampler: ``torchaudio.functional.resample(x, orig, new)`` with its defaults
(sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), as the reference uses it at
meldataset.py:621-627.  (B, N) or (N,) float32 device audio in, ceil(new*N/orig) samples out."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib, ops
from .mel import _tracked
from .ragged import check_waves, row_layout


class _ResampleOfWave(torch.autograd.Function):
    """The forward launch as it is, with ``ops.resample_backward`` (csrc/resample.hip) behind it.  The operator is
    linear: only the input's shape is kept.  ``run(wave)`` is the untracked call."""

    @staticmethod
    def forward(ctx, wave, resampler, run):
        ctx.resampler, ctx.shape = resampler, tuple(wave.shape)
        return run(wave)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        single = len(ctx.shape) == 1
        grad = ops.resample_backward(ctx.resampler, grad_out.unsqueeze(0) if single else grad_out, ctx.shape[-1])
        return (grad[0] if single else grad), None, None


class _RaggedResampleOfWave(torch.autograd.Function):
    """``RaggedResampler``'s launch with ``ops.resample_ragged_backward`` behind it; the gradient comes in the layout of
    the input (packed or padded rows).  ``out_lengths`` carries no graph."""

    @staticmethod
    def forward(ctx, x, resampler, run, rates, lengths):
        ctx.resampler, ctx.shape, ctx.rates, ctx.lengths = resampler, tuple(x.shape), rates, lengths
        y, out_lengths = run(x)
        ctx.mark_non_differentiable(out_lengths)
        return y, out_lengths

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y, _grad_lengths):
        grad = ops.resample_ragged_backward(ctx.resampler, grad_y, ctx.rates, ctx.lengths,
                                            packed=len(ctx.shape) == 1, width=ctx.shape[-1])
        return grad, None, None, None, None


class Resampler:
    """``resampler(wave)``: (N,) or (B, N) float32 device audio at ``orig_freq`` -> ``out_len(N)`` samples at
    ``new_freq``.  Differentiable with respect to the wave: when grad is enabled and the wave requires grad, the same
    values come from the same launch with a ``grad_fn`` (``ops.resample_backward``, once differentiable); otherwise
    nothing is recorded."""

    def __init__(self, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.lowpass_filter_width, self.rolloff = int(lowpass_filter_width), float(rolloff)
        g = math.gcd(self.orig_freq, self.new_freq)
        self._orig, self._new = self.orig_freq // g, self.new_freq // g
        self._plan, self._device = None, None

    def out_len(self, n_in: int) -> int:
        return -(-int(n_in) * self._new // self._orig)

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_plan"], st["_device"] = None, None
        return st

    def _get_plan(self, device):
        if self._plan is None or self._device != device:
            handle = C.c_void_p()
            with torch.cuda.device(device):
                _lib.check(_lib.load().pe_resample_plan_create(C.byref(handle), self.orig_freq, self.new_freq,
                                                               self.lowpass_filter_width, self.rolloff),
                           "pe_resample_plan_create")
            self._plan, self._device = handle, device
        return self._plan

    def __call__(self, wave: torch.Tensor) -> torch.Tensor:
        if not wave.is_cuda or wave.dtype != torch.float32:
            raise RuntimeError("Resampler (HIP) needs float32 device audio; no CPU fallback exists")
        if self.orig_freq == self.new_freq:
            return wave
        if _tracked(wave):
            return _ResampleOfWave.apply(wave, self, self._resample)
        return self._resample(wave)

    def _resample(self, wave: torch.Tensor) -> torch.Tensor:
        single = wave.dim() == 1
        x = wave.unsqueeze(0) if single else wave
        if x.stride(-1) != 1:
            x = x.contiguous()
        n_out = self.out_len(x.shape[1])
        y = torch.empty((x.shape[0], n_out), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            ops._call("pe_resample_forward", self._get_plan(x.device), x.data_ptr(), x.shape[0], x.shape[1], x.stride(0),
                      y.data_ptr(), y.stride(0), n_out, _lib.stream_ptr())
        return y[0] if single else y


class RaggedResampler:
    """Rows at mixed source rates to one target rate in ONE launch (``pe_resample_ragged_forward``).  Row r equals
    ``Resampler(rates[r], target_sr)`` on that row alone, bit for bit; a row already at the target is copied.  One
    plan is cached per set of source rates and device.  Differentiable with respect to ``x`` as ``Resampler`` is
    (``ops.resample_ragged_backward``, one launch, the gradient in ``x``'s own layout); ``out_lengths`` carries no
    graph."""

    def __init__(self, target_sr: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
        self.target_sr = int(target_sr)
        self.lowpass_filter_width, self.rolloff = int(lowpass_filter_width), float(rolloff)
        self._plans = {}

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_plans"] = {}
        return st

    def out_len(self, rate: int, n: int) -> int:
        rate = int(rate)
        if rate == self.target_sr:
            return int(n)
        g = math.gcd(rate, self.target_sr)
        return -(-int(n) * (self.target_sr // g) // (rate // g))

    def _get_plan(self, rates: tuple, device):
        key = (rates, device)
        if key not in self._plans:
            handle = C.c_void_p()
            arr = (C.c_int * len(rates))(*rates)
            with torch.cuda.device(device):
                _lib.check(_lib.load().pe_resample_ragged_plan_create(C.byref(handle), arr, len(rates), self.target_sr,
                                                                      self.lowpass_filter_width, self.rolloff),
                           "pe_resample_ragged_plan_create")
            self._plans[key] = handle
        return self._plans[key]

    def __call__(self, x: torch.Tensor, rates, lengths=None, y_width: int | None = None):
        """``x``: (B, N) padded rows (``lengths`` per row, default N) or a flat (N,) tensor of rows packed back to
        back (``lengths`` required).  ``rates``, ``lengths``: host sequences.  Returns ``(y (B, y_width),
        out_lengths int32 (B,) device)``; ``y_width`` defaults to the longest output and each row is zero past its
        own output."""
        check_waves(x, "RaggedResampler")
        rates = [int(r) for r in rates]
        lengths, offsets = row_layout(x, lengths)
        B = len(rates)
        if len(lengths) != B:
            raise ValueError("one rate per row")
        if _tracked(x):                                      # the same call below, with the backward behind it
            return _RaggedResampleOfWave.apply(x, self, lambda w: self(w, rates, lengths, y_width), rates, lengths)
        distinct = tuple(sorted(set(rates)))
        index = {r: k for k, r in enumerate(distinct)}
        ridx = [index[r] for r in rates]
        out_lengths = [self.out_len(r, n) for r, n in zip(rates, lengths)]
        if y_width is None:
            y_width = max(out_lengths, default=0)
        # one pinned staging buffer per dtype: n_in, rate index and output lengths (int32), offsets (int64)
        host32 = torch.tensor(lengths + ridx + out_lengths, dtype=torch.int32).pin_memory()
        host64 = torch.tensor(offsets, dtype=torch.int64).pin_memory()
        dev32 = host32.to(x.device, non_blocking=True)
        dev64 = host64.to(x.device, non_blocking=True)
        y = torch.empty((B, int(y_width)), dtype=torch.float32, device=x.device)
        if B and y_width:                                    # (an empty y has no data pointer)
            with torch.cuda.device(x.device):
                ops._call("pe_resample_ragged_forward", self._get_plan(distinct, x.device), x.data_ptr(),
                          dev64.data_ptr(), dev32.data_ptr(), dev32[B:].data_ptr(), host32[:B].data_ptr(),
                          host32[B:2 * B].data_ptr(), B, y.data_ptr(), y.stride(0), int(y_width), _lib.stream_ptr())
        return y, dev32[2 * B:]
