"""WORLD vocoder synthesis on the GPU: ``pyworld.synthesize(f0, sp, ap, fs, frame_period)`` (WORLD's ``Synthesis``) and
the vowel generator the reference builds on it (Utils/synthetic.py).

The time base -- where the glottal pulses fall -- is a sequential float64 recurrence (a running phase wrapped at 2 pi)
whose rounding decides a pulse's sample wherever a period is a whole number of samples, so it runs here on the host
(``time_base``), in WORLD's order of operations.  The device gets the finished pulse table and does the heavy part:
one minimum-phase impulse response of ``fft_size`` samples per pulse and their overlap-add (``csrc/world_synth.hip``);
there is no CPU path.  Two stated deviations from WORLD: pulse p's aperiodic noise is ``noise[index[p] : index[p] +
noise_size[p]]`` of a caller-given array of standard normals, or drawn in the kernel from Philox keyed by ``(seed,
sample)`` (WORLD draws from a process-global xorshift stream), and the per-pulse arithmetic is float32.  pyworld is not
available here: parity with its binary is unpinned, the yardstick is a float64 restatement of the published algorithm
(``tests/world_ref.py``), see DESIGN.md.  Opt-in, the time base runs on the device as well (``time_base_device``,
``tables="device"``, ``time_base="device"``; ``csrc/world_time_base.hip``): the phase as an exact 128-bit integer in
turns of 2^-64, which no order of addition can change, pinned bit for bit by ``tests/world_time_base_ref.py`` (DESIGN.md
section 30).

Also WORLD's CheapTrick (``pyworld.cheaptrick``), the spectral envelope of a recording (``cheaptrick``,
``cheaptrick_ragged``, ``csrc/cheaptrick.hip``), and analysis / resynthesis on top of both (``resynthesize``,
``resynthesize_ragged``): the envelope of a recording through ``Synthesis`` on a chosen F0 curve, returned with the
curve it was synthesized from (``label_curve``), which is exact by construction.  Stated deviations of CheapTrick:
float32 per-frame arithmetic, the two ``randn`` safeguards dropped or replaced by their scale, and the linear smoothing
as a sum over the covered bins instead of a cumulative-sum difference.  Parity with pyworld's binary is unpinned here
too; the yardstick is ``tests/cheaptrick_ref.py``.

And WORLD's D4C (``pyworld.d4c``), the band aperiodicity of a recording (``d4c``, ``d4c_ragged``, ``csrc/d4c.hip``),
which ``resynthesize(..., ap="d4c")`` hands to the synthesizer in place of a constant template.  Stated deviations:
float32 per-frame arithmetic with the smoothing sums accumulated in double, the window's ``randn`` dropped (a silent
window is unvoiced), the linear smoothing as for CheapTrick.  Unpinned as well; the yardstick is ``tests/d4c_ref.py``
(DESIGN.md section 24).

And voice transforms between analysis and synthesis (``VoiceTransform``, ``warp_envelopes``, ``resynthesize(...,
transform=)``, ``csrc/world_warp.hip``): the envelope read along a warped frequency axis (formant ratio), the frames at
another rate (tempo), a spectral tilt, and the aperiodicity scaled (breath).  The synthesizer is still driven by the
curve the item is labelled with, so the label stays exact; ``time_warp_curve`` brings a curve to the output time axis.
The yardstick is ``tests/world_warp_ref.py``.
"""
from __future__ import annotations

import hashlib
import math
import random
from dataclasses import dataclass
from typing import NamedTuple, Tuple

import numpy as np
import torch

from . import _lib, ops
from .ragged import (check_device_tensor, check_waves, fft_roots, host_ptrs, i64, pack_tracks, plan_meta,
                     row_layout)

FFT_SIZES = (512, 1024, 2048)
WORKSPACE_BYTES = 256 << 20                                 # responses of one launch; more rows go to further launches
UNVOICED_F0 = 500.0                                         # WORLD's pulse rate for unvoiced stretches

DEFAULT_VOWELS = (
    {"label": "ah", "formants": ((730.0, 90.0, 1.0), (1090.0, 110.0, 0.6), (2440.0, 150.0, 0.4))},
    {"label": "ih", "formants": ((390.0, 80.0, 1.0), (1990.0, 120.0, 0.6), (2550.0, 160.0, 0.4))},
    {"label": "uh", "formants": ((440.0, 70.0, 1.0), (1020.0, 90.0, 0.6), (2240.0, 150.0, 0.4))},
)


def check_fft_size(fft_size) -> int:
    if int(fft_size) not in FFT_SIZES:
        raise ValueError(f"WORLD synthesis fft_size {fft_size!r} is not supported on the HIP path: use one of "
                         f"{list(FFT_SIZES)}")
    return int(fft_size)


# --------------------------------------------------------------------------- host side: lengths and the time base
def output_length(n_frames: int, fs, frame_period_ms: float) -> int:
    """WORLD's y_length = int(f0_length * frame_period * fs / 1000)."""
    return int(int(n_frames) * frame_period_ms * fs / 1000)


def lowest_f0(fs, fft_size: int) -> float:
    return fs / fft_size + 1.0


class PulseTable(NamedTuple):
    index: np.ndarray                          # int64 (P,) sample of each pulse, strictly increasing
    shift: np.ndarray                          # float64 (P,) fractional delay in seconds, 0 <= shift * fs <= 1
    vuv: np.ndarray                            # bool (P,) voicing at the pulse's sample
    noise_size: np.ndarray                     # int64 (P,) samples to the next pulse, 0 for the last


def time_base(f0, fs, frame_period_ms: float, fft_size: int) -> PulseTable:
    """WORLD's GetTimeBase + GetPulseLocationsForTimeBase, numpy float64 in WORLD's order: frames below ``lowest_f0``
    are unvoiced; F0 and voicing get one extrapolated frame and are interpolated linearly to the sample times; the
    phase is the running sum of 2 pi f0 / fs (500 Hz where unvoiced), wrapped with fmod; a pulse sits wherever the
    wrapped phase drops by more than pi, its fractional position from the two samples around the wrap."""
    f0 = np.asarray(f0, dtype=np.float64).reshape(-1)
    L = f0.shape[0]
    if L < 2:
        raise ValueError("WORLD synthesis needs at least two frames")
    if not np.all(np.isfinite(f0)):
        raise ValueError("WORLD synthesis: f0 must be finite")
    fp = frame_period_ms / 1000.0
    n = output_length(L, fs, frame_period_ms)
    coarse_f0 = np.where(f0 >= lowest_f0(fs, fft_size), f0, 0.0)
    coarse_vuv = (coarse_f0 != 0.0).astype(np.float64)
    coarse_f0 = np.append(coarse_f0, 2 * coarse_f0[L - 1] - coarse_f0[L - 2])
    coarse_vuv = np.append(coarse_vuv, 2 * coarse_vuv[L - 1] - coarse_vuv[L - 2])
    coarse_t = np.arange(L + 1) * fp
    t = np.arange(n) / fs
    vuv = np.interp(t, coarse_t, coarse_vuv) > 0.5
    f0i = np.where(vuv, np.interp(t, coarse_t, coarse_f0), UNVOICED_F0)
    total = np.cumsum(2 * np.pi * f0i / fs)
    wrap = np.fmod(total, 2 * np.pi)
    index = np.flatnonzero(np.abs(wrap[1:] - wrap[:-1]) > np.pi).astype(np.int64)
    y1 = wrap[index] - 2 * np.pi
    y2 = wrap[index + 1]
    shift = (-y1 / (y2 - y1)) / fs
    noise_size = np.zeros_like(index)
    noise_size[:-1] = np.diff(index)
    return PulseTable(index, shift, vuv[index], noise_size)


# --------------------------------------------------------------------------- the time base on the device
TIME_BASE_MODES = ("host", "device")


def check_time_base_mode(mode) -> str:
    if mode not in TIME_BASE_MODES:
        raise ValueError(f"WORLD time base {mode!r} is not a mode: use one of {list(TIME_BASE_MODES)}")
    return mode


def no_table() -> PulseTable:
    """The empty table a request carries when the device computes the time base."""
    return PulseTable(np.zeros(0, np.int64), np.zeros(0, np.float64), np.zeros(0, bool), np.zeros(0, np.int64))


def coarse_curves(f0, fs, fft_size: int):
    """The extended coarse curves of ``time_base_device``, built as ``time_base`` builds them: F0 with the frames below
    ``lowest_f0`` at 0 and the voicing as 0 / 1, each with one extrapolated frame -- the F0's clamped at 0 from below
    (the one deviation: WORLD's goes negative after a steep final fall and runs the phase backwards)."""
    f0 = np.asarray(f0, dtype=np.float64).reshape(-1)
    L = f0.shape[0]
    if L < 2:
        raise ValueError("WORLD synthesis needs at least two frames")
    if not np.all(np.isfinite(f0)):
        raise ValueError("WORLD synthesis: f0 must be finite")
    cf = np.where(f0 >= lowest_f0(fs, fft_size), f0, 0.0)
    cv = (cf != 0.0).astype(np.float64)
    cf = np.append(cf, max(2 * cf[L - 1] - cf[L - 2], 0.0))
    cv = np.append(cv, 2 * cv[L - 1] - cv[L - 2])
    if not max(float(cf.max()), UNVOICED_F0) < fs / 2.0:
        raise ValueError("WORLD time base: F0 (and the unvoiced 500 Hz) must stay below half the sample rate")
    return cf, cv


class TimeBasePlan:
    """Host layout of a ragged batch of curves for ``pe_world_time_base`` (``pe_world_time_base_plan``, no device call):
    the packed extended coarse curves, the per-row int64 fields and the totals {pieces, pulse slots, samples}."""

    def __init__(self, f0s, fs, frame_period_ms: float, fft_size: int):
        curves = [coarse_curves(f, fs, fft_size) for f in f0s]
        R = self.n_rows = len(curves)
        self.fs, self.frame_period_ms = float(fs), float(frame_period_ms)
        self.n_frames = _i64([c[0].size - 1 for c in curves], R)
        cat = lambda k: np.ascontiguousarray(np.concatenate([c[k] for c in curves]) if R else np.zeros(1))  # noqa: E731
        self.cf, self.cv = cat(0), cat(1)
        self.meta = plan_meta("pe_world_time_base_plan_fields", R)
        self.totals = np.zeros(3, np.int64)
        _lib.check(_lib.load().pe_world_time_base_plan(
            R, *host_ptrs(self.n_frames, self.cf, self.cv), self.fs, self.frame_period_ms,
            *host_ptrs(self.meta, self.totals)), "pe_world_time_base_plan")
        self.n_pieces, self.n_slots, self.n_samples = (int(v) for v in self.totals)
        self.samples = self.meta[:R, 1].copy()
        self.sample_offsets = self.meta[:R, 0].copy()
        self.slot_offsets = self.meta[:R, 6].copy()
        self.capacity = self.meta[:R, 7].copy()


class DevicePulseTables(NamedTuple):
    """The pulse tables of a ragged batch on the device (``time_base_device``).  Row r's pulses are the first
    ``counts[r]`` of the slots from ``slot_offsets[r]`` on (its capacity: up to ``slot_offsets[r + 1]``) of the flat
    ``index`` / ``shift`` / ``vuv``; the slots beyond them are not written.  ``index``, ``shift``, ``vuv``, ``counts``
    and ``status`` are views of ``buffer``, so ``host`` copies the batch in one piece."""
    index: torch.Tensor                        # int64 (slots,) sample of each pulse
    shift: torch.Tensor                        # float64 (slots,) fractional delay in seconds
    vuv: torch.Tensor                          # uint8 (slots,) voicing at the pulse's sample
    counts: torch.Tensor                       # int64 (R,) pulses of each row, on the device
    slot_offsets: np.ndarray                   # int64 (R + 1,) host: first slot of each row, and the slot total
    status: torch.Tensor                       # int32 (2,) nonzero first word: a pulse fell outside its row's slots
    buffer: torch.Tensor                       # uint8: the one allocation the others are views of

    def host(self):
        """One device-to-host copy for the whole batch; a list of ``PulseTable`` with ``noise_size`` filled."""
        raw = self.buffer.cpu().numpy()
        S, R = int(self.slot_offsets[-1]), int(self.counts.numel())
        index = raw[:8 * S].view(np.int64)
        shift = raw[8 * S:16 * S].view(np.float64)
        counts = raw[16 * S:16 * S + 8 * R].view(np.int64)
        status = raw[16 * S + 8 * R:16 * S + 8 * R + 8].view(np.int32)
        vuv = raw[16 * S + 8 * R + 8:16 * S + 8 * R + 8 + S]
        if int(status[0]) != 0:
            raise _lib.HipLibraryError("pe_world_time_base: a pulse fell outside its row's slots (foreign plan)")
        tables = []
        for r in range(R):
            a, c = int(self.slot_offsets[r]), int(counts[r])
            if c < 0 or a + c > int(self.slot_offsets[r + 1]):
                raise _lib.HipLibraryError("pe_world_time_base: a row's pulse count exceeds its slots")
            idx = index[a:a + c].copy()
            noise_size = np.zeros_like(idx)
            noise_size[:-1] = np.diff(idx)
            tables.append(PulseTable(idx, shift[a:a + c].copy(), vuv[a:a + c].astype(bool), noise_size))
        return tables


def time_base_buffer(n_slots: int, n_rows: int, device) -> torch.Tensor:
    """The zeroed byte buffer ``DevicePulseTables`` is laid out in: index, shift, counts, status, vuv."""
    return torch.zeros((16 * n_slots + 8 * n_rows + 8 + n_slots,), dtype=torch.uint8, device=device)


def time_base_device(f0s, fs, frame_period_ms: float, fft_size: int, device, *, buffer: torch.Tensor | None = None,
                     hooks: bool = False, stages: int = 7, workspace: torch.Tensor | None = None):
    """``time_base`` for a ragged batch of host curves on the device (``csrc/world_time_base.hip``), with the phase as
    an exact integer in turns of 2^-64 instead of a float64 running sum: the same pulses as ``time_base`` wherever a
    pulse has a phase margin, shifts within the host's own accumulated rounding, and the same bits whatever the batch
    around a row (the definition: DESIGN.md section 30, ``tests/world_time_base_ref.py``).  One deviation: the
    extrapolated last frame of the F0 is clamped at 0.  Returns ``DevicePulseTables``; with ``hooks`` also a dict of
    the per-sample ``f0i`` (float64), ``lo`` (uint64 as int64 bits) and ``hi`` (int64) of every row back to back, and
    the plan.  ``buffer``: a ``time_base_buffer`` of the caller's to write into.  There is no CPU path."""
    from .ragged import gpu_device, workspace as scratch
    device = gpu_device(device, "WORLD time base")
    plan = TimeBasePlan([_host_f0(f) for f in f0s], fs, frame_period_ms, check_fft_size(fft_size))
    R, S = plan.n_rows, plan.n_slots
    slot_offsets = np.concatenate([plan.slot_offsets, [S]]).astype(np.int64)
    if buffer is None:
        buffer = time_base_buffer(S, R, device)
    check_device_tensor(buffer, "WORLD time base", torch.uint8)
    if buffer.numel() != 16 * S + 8 * R + 8 + S:
        raise ValueError("WORLD time base: the buffer is not the plan's size")
    a, b, c = 16 * S, 16 * S + 8 * R, 16 * S + 8 * R + 8
    tables = DevicePulseTables(buffer[:8 * S].view(torch.int64), buffer[8 * S:a].view(torch.float64), buffer[c:],
                               buffer[a:b].view(torch.int64), slot_offsets, buffer[b:c].view(torch.int32), buffer)
    hook = None
    if hooks:
        N = max(plan.n_samples, 1)
        hook = {"f0i": torch.zeros(N, dtype=torch.float64, device=device),
                "lo": torch.zeros(N, dtype=torch.int64, device=device),
                "hi": torch.zeros(N, dtype=torch.int64, device=device), "plan": plan}
    if R:
        up = lambda x: torch.from_numpy(x).to(device)  # noqa: E731
        meta_d, cf_d, cv_d = up(plan.meta), up(plan.cf), up(plan.cv)
        n_bytes = _lib.load().pe_world_time_base_workspace_bytes(plan.n_pieces)
        ws = scratch(n_bytes, device) if workspace is None else workspace
        with torch.cuda.device(device):
            ops._call("pe_world_time_base", cf_d.data_ptr(), cv_d.data_ptr(), meta_d.data_ptr(), plan.meta.ctypes.data,
                      R, plan.fs, plan.frame_period_ms, int(stages), _lib.ptr(tables.index), _lib.ptr(tables.shift),
                      _lib.ptr(tables.vuv), _lib.ptr(tables.counts), _lib.ptr(tables.status),
                      _lib.ptr(hook and hook["f0i"]), _lib.ptr(hook and hook["lo"]), _lib.ptr(hook and hook["hi"]),
                      ws.data_ptr(), ws.numel(), _lib.stream_ptr(), work=float(plan.n_samples * 16))
    return (tables, hook) if hooks else tables


def _tables_of(tables, f0s, fs, frame_period, fft_size, device):
    """``tables`` as a list of pulse tables: the string ``"device"`` is one device time base for all rows and one copy
    back; ``None`` the host's ``time_base`` row by row."""
    if isinstance(tables, str):
        if tables != "device":
            raise ValueError(f"WORLD synthesis: tables {tables!r} is neither a list of pulse tables nor 'device'")
        return time_base_device(f0s, fs, frame_period, fft_size, device).host() if len(f0s) else []
    if tables is None:
        return [time_base(f, fs, frame_period, fft_size) for f in f0s]
    return tables


def dc_remover(fft_size: int) -> np.ndarray:
    """WORLD's GetDCRemover: a Hann-like window over both halves, normalised to remove a unit sum."""
    half = fft_size // 2
    w = np.zeros(fft_size)
    w[:half] = 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(half) + 1.0) / (1.0 + fft_size))
    w[fft_size - 1 - np.arange(half)] = w[:half]
    return w / (2 * w[:half].sum())


def noise_seed(curve) -> int:
    """Seed of a generated item's aperiodic noise: 8 bytes of a digest of the curve, so that neither ``random`` nor
    ``np.random`` is consumed for it."""
    data = np.ascontiguousarray(curve, dtype=np.float64).tobytes()
    return int.from_bytes(hashlib.blake2b(data, digest_size=8).digest(), "little")


# --------------------------------------------------------------------------- batch layout
def _i64(a, n=None):
    a = i64(a)
    if n is not None and a.size != n:
        raise ValueError("WORLD plan: per-row arrays differ in length")
    return a


class Plan:
    """Host layout of a ragged batch (``pe_world_plan``): per-row int64 fields, the planned pulses and the workspace
    sizes {planned pulses, output samples}.  ``tables``: one ``PulseTable`` (or (index, shift, vuv, ...)) per row."""

    def __init__(self, n_frames, tables, sp_offsets, sp_strides, ap_offsets=None, ap_strides=None, noise_offsets=None,
                 seeds=None, out_start=None, out_len=None, out_rows=None, out_stride=None, *, fs, frame_period_ms,
                 fft_size, f0s=None):
        self.n_frames = _i64(n_frames)
        R = self.n_rows = self.n_frames.size
        self.meta = plan_meta("pe_world_plan_fields", R)
        self.fs, self.frame_period_ms, self.fft_size = fs, float(frame_period_ms), int(fft_size)
        if len(tables) != R:
            raise ValueError("WORLD plan: one pulse table per row")
        self.pulse_cnt = _i64([len(t[0]) for t in tables], R)
        cat = lambda k, dt: np.ascontiguousarray(  # noqa: E731
            np.concatenate([np.asarray(t[k]).reshape(-1) for t in tables]) if R else np.zeros(0), dtype=dt)
        self.index, self.shift, self.vuv = cat(0, np.int64), cat(1, np.float64), cat(2, np.uint8)
        self.y_len = _i64([output_length(n, fs, self.frame_period_ms) for n in self.n_frames], R)
        self.sp_offsets, self.sp_strides = _i64(sp_offsets, R), _i64(sp_strides, R)
        self.ap_offsets = np.full(R, -1, np.int64) if ap_offsets is None else _i64(ap_offsets, R)
        self.ap_strides = np.zeros(R, np.int64) if ap_strides is None else _i64(ap_strides, R)
        self.noise_offsets = np.full(R, -1, np.int64) if noise_offsets is None else _i64(noise_offsets, R)
        self.seeds = (np.zeros(R, np.int64) if seeds is None else
                      np.array([int(s) & (2 ** 64 - 1) for s in seeds], dtype=np.uint64).view(np.int64))
        self.out_start = np.zeros(R, np.int64) if out_start is None else _i64(out_start, R)
        self.out_len = self.y_len - self.out_start if out_len is None else _i64(out_len, R)
        self.out_rows = np.arange(R, dtype=np.int64) if out_rows is None else _i64(out_rows, R)
        self.out_stride = int(self.out_len.max(initial=0) if out_stride is None else out_stride)
        if self.seeds.size != R:
            raise ValueError("WORLD plan: per-row arrays differ in length")
        f0 = None
        if f0s is not None:
            f0 = np.ascontiguousarray(np.concatenate([np.asarray(f, np.float64).reshape(-1) for f in f0s])
                                      if R else np.zeros(0))
            if f0.size != int(self.n_frames.sum()):
                raise ValueError("WORLD plan: f0 curves do not match the frame counts")
        P = max(int(self.index.size), 1)
        self.pulses = np.zeros((P, 6), np.int64)
        self.pulse_f = np.zeros((P, 2), np.float64)
        self.totals = np.zeros(2, np.int64)
        _lib.check(_lib.load().pe_world_plan(
            R, *host_ptrs(self.n_frames, f0, self.pulse_cnt, self.index, self.shift, self.vuv, self.sp_offsets,
                          self.sp_strides, self.ap_offsets, self.ap_strides, self.noise_offsets, self.seeds,
                          self.out_start, self.out_len, self.out_rows),
            self.out_stride, float(fs), self.frame_period_ms, self.fft_size,
            *host_ptrs(self.meta, self.pulses, self.pulse_f, self.totals)), "pe_world_plan")
        self.n_pulses, self.n_out = (int(v) for v in self.totals)
        self.pulses, self.pulse_f = self.pulses[:max(self.n_pulses, 1)], self.pulse_f[:max(self.n_pulses, 1)]


class WorldSynth:
    """``table``: the device copy of the transform's roots of unity and the DC remover; ``run`` executes the two
    stages for a ``Plan``."""

    def table(self, fft_size, device):
        return _lib.device_table(("world", int(fft_size)), device,
                                 lambda: np.concatenate([fft_roots(fft_size).reshape(-1), dc_remover(fft_size)]))

    def run(self, plan: Plan, sp, ap, gains, out, noise=None, out_noise=None, keep=False):
        """sp / ap / noise: flat float32 device tensors addressed by the plan's offsets (ap, noise optional); gains
        (R,) float32 device; out: float32 device tensor addressed by out_row * out_stride + i; out_noise: the output
        windows' additive noise back to back.  Returns the responses when ``keep``."""
        dev = out.device
        for name, t in (("sp", sp), ("ap", ap), ("gains", gains), ("out", out), ("noise", noise),
                        ("out_noise", out_noise)):
            if t is not None and (not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous()):
                raise RuntimeError(f"WORLD synthesis: {name} must be a contiguous float32 device tensor (no CPU path)")
        if plan.n_rows == 0 or plan.n_out == 0:
            return {} if keep else None
        N, R = plan.fft_size, plan.n_rows
        bins = N // 2 + 1
        if gains.numel() != R:
            raise ValueError("WORLD synthesis: one gain per row")
        if out_noise is not None and out_noise.numel() != plan.n_out:
            raise ValueError("WORLD synthesis: out_noise must hold one value per output sample")
        if out.numel() < int((plan.out_rows * plan.out_stride + plan.out_len).max(initial=0)):
            raise ValueError("WORLD synthesis: output buffer smaller than the plan addresses")
        if sp.numel() < int((plan.sp_offsets + (plan.n_frames - 1) * plan.sp_strides).max(initial=0)) + bins:
            raise ValueError("WORLD synthesis: sp smaller than the plan addresses")
        has_ap = plan.ap_offsets >= 0
        if has_ap.any() and (ap is None or ap.numel() < int(
                (plan.ap_offsets + (plan.n_frames - 1) * plan.ap_strides)[has_ap].max()) + bins):
            raise ValueError("WORLD synthesis: ap smaller than the plan addresses")
        has_noise = plan.noise_offsets >= 0
        if has_noise.any() and (noise is None or noise.numel() < int((plan.noise_offsets + plan.y_len)[has_noise].max())):
            raise ValueError("WORLD synthesis: noise must hold one value per sample of the row")
        meta = torch.from_numpy(plan.meta).to(dev)
        pulses = torch.from_numpy(plan.pulses).to(dev)
        pulse_f = torch.from_numpy(plan.pulse_f).to(dev)
        resp = torch.empty((plan.n_pulses, N), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ops._call("pe_world_responses", sp.data_ptr(), _lib.ptr(ap), _lib.ptr(noise), meta.data_ptr(),
                      pulses.data_ptr(), pulse_f.data_ptr(), self.table(N, dev).data_ptr(), R, plan.n_pulses, N,
                      resp.data_ptr(), _lib.stream_ptr(), work=float(plan.n_pulses * (N * 4 + 4 * bins * 4)))
            ops._call("pe_world_overlap_add", resp.data_ptr(), meta.data_ptr(), pulses.data_ptr(), gains.data_ptr(),
                      _lib.ptr(out_noise), R, plan.n_out, N, out.data_ptr(), _lib.stream_ptr(),
                      work=float(plan.n_out * 8))
        if keep:
            return {"responses": resp, "meta": plan.meta, "pulses": plan.pulses, "pulse_f": plan.pulse_f}
        return None


_SYNTH = WorldSynth()


def _device_f32(name, t):
    if t is not None and (not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32):
        raise RuntimeError(f"WORLD synthesis: {name} must be a contiguous float32 device tensor (no CPU path)")
    return None if t is None else t.contiguous()


def _host_f0(f0):
    if torch.is_tensor(f0):
        f0 = f0.detach().cpu().numpy()
    return np.asarray(f0, dtype=np.float64).reshape(-1)


def world_synthesize_ragged(f0s, sp, sp_offsets, sp_strides, gains: torch.Tensor, out: torch.Tensor, out_rows=None,
                            out_start=None, out_len=None, *, fs, frame_period: float, fft_size: int, ap=None,
                            ap_offsets=None, ap_strides=None, tables=None, noise=None, noise_offsets=None, seeds=None,
                            out_noise=None) -> torch.Tensor:
    """Ragged batch.  Row r has the host curve ``f0s[r]`` (``tables[r]`` its pulse table; computed here when not
    given: by ``time_base`` on the host, or with ``tables="device"`` by one ``time_base_device`` for all rows and one
    copy back, after which the host plan runs unchanged); frame f of its envelope is the ``fft_size // 2 + 1`` floats of the flat float32 device tensor ``sp`` at
    ``sp_offsets[r] + f * sp_strides[r]`` (stride 0: one template for every frame), ``ap`` likewise (``ap_offsets[r] <
    0`` or no ``ap``: zeros).  The row's aperiodic noise is ``noise`` at ``noise_offsets[r]`` (one standard normal per
    sample of the row) or, without it, drawn on the device from ``seeds[r]``.  Samples ``[out_start[r], out_start[r] +
    out_len[r])`` of row r (default: all) times ``gains[r]`` go to ``out[out_rows[r], :out_len[r]]`` of the 2-D
    ``out``, plus ``out_noise`` (flat, the windows back to back) when given.  Rows whose responses would not fit one
    256 MiB workspace run in several launches.  Returns ``out``."""
    if out.dim() != 2:
        raise ValueError("out must be 2-D (rows, samples)")
    if out.stride(1) != 1:
        raise ValueError("out rows must be contiguous")
    fft_size = check_fft_size(fft_size)
    sp, ap, noise, out_noise = (_device_f32(n, t) for n, t in (("sp", sp), ("ap", ap), ("noise", noise),
                                                              ("out_noise", out_noise)))
    f0s = [_host_f0(f) for f in f0s]
    R = len(f0s)
    tables = _tables_of(tables, f0s, fs, frame_period, fft_size, out.device)
    n_frames = [f.size for f in f0s]
    y_len = np.array([output_length(n, fs, frame_period) for n in n_frames], dtype=np.int64)
    out_start = np.zeros(R, np.int64) if out_start is None else _i64(out_start, R)
    out_len = y_len - out_start if out_len is None else _i64(out_len, R)
    out_rows = np.arange(R, dtype=np.int64) if out_rows is None else _i64(out_rows, R)
    gains = gains.to(out.device, torch.float32).contiguous()
    # rows per launch: the planned pulses' responses stay within the workspace
    half = fft_size // 2
    planned = [int(np.searchsorted(t[0], out_start[r] + out_len[r] - 1 + half, "left") -
                   np.searchsorted(t[0], out_start[r] - half, "left")) if out_len[r] > 0 else 0
               for r, t in enumerate(tables)]
    limit = WORKSPACE_BYTES // (4 * fft_size)
    groups, cur, used = [], [], 0
    for r in range(R):
        if cur and used + planned[r] > limit:
            groups.append(cur)
            cur, used = [], 0
        cur.append(r)
        used += planned[r]
    if cur:
        groups.append(cur)
    pick = lambda a, g, dflt=None: dflt if a is None else [a[r] for r in g]  # noqa: E731
    n_off = np.concatenate([[0], np.cumsum(out_len)])
    for g in groups:
        plan = Plan(pick(n_frames, g), pick(tables, g), pick(sp_offsets, g), pick(sp_strides, g),
                    pick(ap_offsets, g) if ap is not None else None, pick(ap_strides, g) if ap is not None else None,
                    pick(noise_offsets, g) if noise is not None else None, pick(seeds, g), out_start[g], out_len[g],
                    out_rows[g], out.stride(0), fs=fs, frame_period_ms=frame_period, fft_size=fft_size,
                    f0s=pick(f0s, g))
        _SYNTH.run(plan, sp, ap, gains[g[0]:g[-1] + 1], out, noise,
                   None if out_noise is None else out_noise[int(n_off[g[0]]):int(n_off[g[-1] + 1])])
    return out


def world_synthesize(f0, sp: torch.Tensor, ap: torch.Tensor | None = None, fs=24000, frame_period: float = 5.0, *,
                     noise: torch.Tensor | None = None, seed: int = 0, time_base: str = "host") -> torch.Tensor:
    """pyworld's ``synthesize(f0, sp, ap, fs, frame_period)`` on the device.  ``f0``: host curve (a tensor is brought
    to the host); ``sp`` / ``ap``: float32 device tensors ``(len(f0), fft_size / 2 + 1)``, or one ``(fft_size / 2 +
    1,)`` template for every frame; ``ap=None`` is all zeros.  ``noise``: one standard normal per output sample (device
    float32) for the aperiodic part; drawn on the device from ``seed`` when not given.  ``time_base``: ``"host"`` (the
    float64 recurrence of the module's ``time_base``) or ``"device"`` (``time_base_device``).  Returns a 1-D float32
    device tensor of ``int(len(f0) * frame_period * fs / 1000)`` samples."""
    tables = "device" if check_time_base_mode(time_base) == "device" else None
    f0 = _host_f0(f0)
    sp = _device_f32("sp", sp)
    ap = _device_f32("ap", ap)
    noise = _device_f32("noise", noise)
    bins = sp.shape[-1]
    fft_size = check_fft_size(2 * (bins - 1))
    for name, t in (("sp", sp), ("ap", ap)):
        if t is not None and not ((t.dim() == 1 and t.shape[0] == bins) or
                                  (t.dim() == 2 and tuple(t.shape) == (f0.size, bins))):
            raise ValueError(f"world_synthesize: {name} must be (len(f0), {bins}) or ({bins},)")
    n = output_length(f0.size, fs, frame_period)
    if noise is not None and noise.numel() != n:
        raise ValueError("world_synthesize: noise must hold one value per output sample")
    out = torch.zeros((1, max(n, 1)), dtype=torch.float32, device=sp.device)
    stride = lambda t: [bins if t.dim() == 2 else 0]  # noqa: E731
    world_synthesize_ragged([f0], sp.reshape(-1), [0], stride(sp), torch.ones(1), out, fs=fs,
                            frame_period=frame_period, fft_size=fft_size,
                            ap=None if ap is None else ap.reshape(-1), ap_offsets=None if ap is None else [0],
                            ap_strides=None if ap is None else stride(ap),
                            noise=None if noise is None else noise.reshape(-1),
                            noise_offsets=None if noise is None else [0], seeds=[seed], tables=tables)
    return out[0, :n]


# --------------------------------------------------------------------------- CheapTrick: the envelope of a recording
CHEAPTRICK_Q1 = -0.15
CHEAPTRICK_F0_FLOOR = 71.0


def cheaptrick_fft_size(fs, f0_floor: float = CHEAPTRICK_F0_FLOOR) -> int:
    """WORLD's GetFFTSizeForCheapTrick: 2^(1 + floor(log2(3 fs / f0_floor + 1)))."""
    return 2 ** (1 + int(math.log(3.0 * fs / f0_floor + 1.0) / math.log(2.0)))


def cheaptrick_floor(fs, fft_size: int) -> float:
    """The lowest F0 a transform of ``fft_size`` analyses as itself; frames at or below it are analysed at 500 Hz."""
    return 3.0 * fs / (fft_size - 3.0)


class Envelopes(NamedTuple):
    """What ``cheaptrick_ragged`` and ``d4c_ragged`` return: frame ``first[r] + q`` of row r is the ``bins`` floats of
    the flat float32 device tensor ``sp`` (the envelopes, or D4C's aperiodicities) at ``offsets[r] + q * strides[r]``,
    for ``q < counts[r]``."""
    sp: torch.Tensor
    offsets: np.ndarray
    strides: np.ndarray
    first: np.ndarray
    counts: np.ndarray
    fft_size: int

    def row(self, r: int) -> torch.Tensor:
        bins = self.fft_size // 2 + 1
        return self.sp.as_strided((int(self.counts[r]), bins), (int(self.strides[r]), 1), int(self.offsets[r]))

    def frame0_offsets(self) -> np.ndarray:
        """Where frame 0 of each row lies (or would lie), for ``world_synthesize_ragged``'s ``sp_offsets``."""
        return self.offsets - self.first * self.strides


class _FrameRows(NamedTuple):
    """What a frame analysis takes from the rows alone, whichever analysis it is: where the rows lie in ``x``, their F0
    curves packed on the device (``f0``) with each row's offset and length in it, and the frames asked for."""
    n: int
    offsets: np.ndarray
    lengths: np.ndarray
    f0: torch.Tensor
    f0_off: np.ndarray
    f0_len: np.ndarray
    first: np.ndarray
    counts: np.ndarray


def _frame_rows(who, x, lengths, f0s, frames) -> _FrameRows:
    """``cheaptrick_ragged`` and ``d4c_ragged`` build this from their arguments, or take the one that
    ``resynthesize_ragged`` built for both (``_rows``, which then stands for ``lengths``, ``f0s`` and ``frames``): the
    envelope and the aperiodicity of a resynthesis are of the same frames by construction, with one upload of the F0."""
    check_waves(x, who)
    lengths, offsets = row_layout(x, lengths, whole_by_default=True)
    R = len(lengths)
    f0s = list(f0s)
    if len(f0s) != R:
        raise ValueError(f"{who}: one F0 curve per row")
    f0_d, f0_off, f0_len = pack_tracks(f0s, x.device)
    first = np.zeros(R, np.int64) if frames is None else _i64([fr[0] for fr in frames], R)
    counts = _i64(f0_len, R) - first if frames is None else _i64([fr[1] for fr in frames], R)
    return _FrameRows(R, i64(offsets), i64(lengths), f0_d, i64(f0_off), i64(f0_len), first, counts)


def _frame_plan(who, plan_fn, rows: _FrameRows, device, out, out_offsets, out_strides, fft_size, config, n_totals=1):
    """``rows`` and where their frames go, through the C plan ``plan_fn`` (``config``: its arguments between
    ``out_stride`` and ``meta``).  Returns ``(meta, totals, out, Envelopes)`` with ``out`` made on ``device``, or
    checked against what the plan addresses."""
    R, first, counts = rows.n, rows.first, rows.counts
    bins = fft_size // 2 + 1
    strides = np.full(R, bins, np.int64) if out_strides is None else _i64(out_strides, R)
    if out_offsets is None:
        out_offsets = np.cumsum(counts * strides) - counts * strides
    out_offsets = _i64(out_offsets, R)
    meta = plan_meta(plan_fn + "_fields", R)
    totals = np.zeros(n_totals, np.int64)
    _lib.check(getattr(_lib.load(), plan_fn)(
        R, *host_ptrs(rows.offsets, rows.lengths, rows.f0_off, rows.f0_len, first, counts, out_offsets, strides),
        *config, *host_ptrs(meta, totals)), plan_fn)
    need = int((out_offsets + np.maximum(counts - 1, 0) * strides + bins)[counts > 0].max(initial=0))
    if out is None:
        out = torch.empty((max(need, 1),), dtype=torch.float32, device=device)
    else:
        check_device_tensor(out, who)
        if out.numel() < need:
            raise ValueError(f"{who}: the output is smaller than the plan addresses")
    return meta, totals, out, Envelopes(out, out_offsets, strides, first, counts, fft_size)


def cheaptrick_ragged(x: torch.Tensor, lengths, f0s, fs, frame_period: float = 5.0, *, q1: float = CHEAPTRICK_Q1,
                      f0_floor: float = CHEAPTRICK_F0_FLOOR, fft_size: int | None = None, frames=None,
                      out: torch.Tensor | None = None, out_offsets=None, out_strides=None,
                      _rows: _FrameRows | None = None) -> Envelopes:
    """WORLD's CheapTrick for a ragged batch, one launch.  ``x``: float32 device audio, rows packed back to back (1-D,
    with ``lengths``) or padded (2-D; ``lengths`` defaults to the width).  ``f0s``: one F0 curve per row at
    ``frame_period`` (ms) spacing, 0 = unvoiced (tensors or arrays; brought to the device as float32).  ``frames``: per
    row ``(first_frame, n_frames)`` to analyse only those (default: every frame of the curve).  ``out``: a flat float32
    device tensor to write into, at ``out_offsets[r] + q * out_strides[r]`` (default: the rows' frames back to back in a
    new tensor).  There is no CPU path."""
    check_waves(x, "CheapTrick")
    fft_size = check_fft_size(cheaptrick_fft_size(fs, f0_floor) if fft_size is None else fft_size)
    bins = fft_size // 2 + 1
    rows = _frame_rows("CheapTrick", x, lengths, f0s, frames) if _rows is None else _rows
    R, f0_d = rows.n, rows.f0
    meta, totals, out, env = _frame_plan(
        "CheapTrick", "pe_cheaptrick_plan", rows, x.device, out, out_offsets, out_strides, fft_size,
        (float(fs), float(frame_period), float(f0_floor), fft_size))
    if R and int(totals[0]):
        meta_d = torch.from_numpy(meta).to(x.device)
        with torch.cuda.device(x.device):
            ops._call("pe_cheaptrick", x.data_ptr(), f0_d.data_ptr(), meta_d.data_ptr(), meta.ctypes.data,
                      _SYNTH.table(fft_size, x.device).data_ptr(), R, float(fs), float(frame_period), float(q1),
                      float(f0_floor), fft_size, out.data_ptr(), _lib.stream_ptr(),
                      work=float(int(totals[0]) * (bins * 4 + 3 * fft_size * 4)))
    return env


def cheaptrick(x: torch.Tensor, f0, fs, frame_period: float = 5.0, *, q1: float = CHEAPTRICK_Q1,
               f0_floor: float = CHEAPTRICK_F0_FLOOR, fft_size: int | None = None) -> torch.Tensor:
    """pyworld's ``cheaptrick(x, f0, t, fs)`` on the device for ``t = arange(len(f0)) * frame_period`` ms: ``x`` a 1-D
    float32 device wave, ``f0`` its curve (0 = unvoiced).  Returns the ``(len(f0), fft_size / 2 + 1)`` float32 power
    envelope; ``fft_size`` defaults to WORLD's for ``f0_floor``."""
    if not torch.is_tensor(x) or x.dim() != 1:
        raise RuntimeError("CheapTrick (HIP) needs a 1-D float32 device wave; no CPU fallback exists")
    env = cheaptrick_ragged(x, None, [f0], fs, frame_period, q1=q1, f0_floor=f0_floor, fft_size=fft_size)
    return env.row(0)


# --------------------------------------------------------------------------- D4C: the band aperiodicity of a recording
D4C_THRESHOLD = 0.85


def _d4c_table(n_d: int, n_l: int, device) -> torch.Tensor:
    """The N_d-th roots of unity, then the N_l-th (LoveTrain's transform), as ``pe_d4c_bands`` reads them."""
    return _lib.device_table(("d4c", n_d, n_l), device,
                             lambda: np.concatenate([fft_roots(n_d).reshape(-1), fft_roots(n_l).reshape(-1)]))


def d4c_ragged(x: torch.Tensor, lengths, f0s, fs, frame_period: float = 5.0, *, threshold: float = D4C_THRESHOLD,
               fft_size: int | None = None, frames=None, out: torch.Tensor | None = None, out_offsets=None,
               out_strides=None, return_bands: bool = False, _rows: _FrameRows | None = None):
    """WORLD's D4C for a ragged batch, two launches (the band analysis, then its expansion to bins).  The arguments are
    ``cheaptrick_ragged``'s, and so is the layout returned: an ``Envelopes`` whose ``sp`` holds the aperiodicity, ``bins
    = fft_size / 2 + 1`` floats in (0, 1] per frame (``fft_size`` defaults to CheapTrick's for ``fs``).  ``threshold``:
    LoveTrain's; a frame with ``a0 <= threshold`` is all ``1 - 1e-12``.  With ``return_bands`` also the ``(frames, 1 +
    bands)`` float32 device tensor of the analysed frames in row order: ``a0``, then the bands' coarse aperiodicity in
    dB (NaN where the frame has the unvoiced verdict).  There is no CPU path."""
    check_waves(x, "D4C")
    fft_size = check_fft_size(cheaptrick_fft_size(fs) if fft_size is None else fft_size)
    threshold = float(threshold)
    if not math.isfinite(threshold):
        raise ValueError("D4C: threshold must be finite")
    rows = _frame_rows("D4C", x, lengths, f0s, frames) if _rows is None else _rows
    R, f0_d = rows.n, rows.f0
    meta, totals, out, env = _frame_plan("D4C", "pe_d4c_plan", rows, x.device, out, out_offsets, out_strides, fft_size,
                                         (float(fs), float(frame_period), fft_size), n_totals=5)
    n_frames, n_d, n_l, n_bands, _ = (int(v) for v in totals)
    bands = torch.empty((max(n_frames, 1), 1 + n_bands), dtype=torch.float32, device=x.device)
    if R and n_frames:
        meta_d = torch.from_numpy(meta).to(x.device)
        with torch.cuda.device(x.device):
            ops._call("pe_d4c_bands", x.data_ptr(), f0_d.data_ptr(), meta_d.data_ptr(), meta.ctypes.data,
                      _d4c_table(n_d, n_l, x.device).data_ptr(), R, float(fs), float(frame_period), threshold,
                      fft_size, bands.data_ptr(), _lib.stream_ptr(), work=float(n_frames * 8 * n_d * 4))
            ops._call("pe_d4c_expand", bands.data_ptr(), meta_d.data_ptr(), meta.ctypes.data, R, float(fs), fft_size,
                      out.data_ptr(), _lib.stream_ptr(), work=float(n_frames * (fft_size // 2 + 1) * 4))
    return (env, bands[:n_frames]) if return_bands else env


def d4c(x: torch.Tensor, f0, fs, frame_period: float = 5.0, *, threshold: float = D4C_THRESHOLD,
        fft_size: int | None = None) -> torch.Tensor:
    """pyworld's ``d4c(x, f0, t, fs)`` on the device for ``t = arange(len(f0)) * frame_period`` ms: ``x`` a 1-D float32
    device wave, ``f0`` its curve (0 = unvoiced).  Returns the ``(len(f0), fft_size / 2 + 1)`` float32 aperiodicity;
    ``fft_size`` defaults to CheapTrick's for ``fs``."""
    if not torch.is_tensor(x) or x.dim() != 1:
        raise RuntimeError("D4C (HIP) needs a 1-D float32 device wave; no CPU fallback exists")
    return d4c_ragged(x, None, [f0], fs, frame_period, threshold=threshold, fft_size=fft_size).row(0)


def label_curve(new_f0, fs, fft_size: int) -> np.ndarray:
    """The curve a resynthesized item is labelled with: ``new_f0`` (float64) with every frame the synthesizer does not
    voice (``new_f0 <= lowest_f0(fs, fft_size)``) set to 0.  The synthesizer is driven with this curve."""
    f0 = _host_f0(new_f0).copy()
    f0[~(f0 > lowest_f0(fs, fft_size))] = 0.0
    return f0


# --------------------------------------------------------------------------- voice transforms in the WORLD domain
class VoiceTransform(NamedTuple):
    """What a resynthesis changes about the speaker, none of which touches the label: ``formant`` scales the formant
    frequencies (the VTLP factor alpha of Jaitly & Hinton 2013, within [0.5, 2]; the map is linear up to ``f_hi`` Hz or
    ``f_hi / formant``, whichever is lower, and runs straight to Nyquist from there), ``rate`` the speed the frames are
    read at (1.25: a quarter faster and shorter), ``tilt`` adds that many dB per octave to the envelope around 1 kHz,
    ``breath`` that many dB to the aperiodicity.  The defaults are the identity."""
    formant: float = 1.0
    rate: float = 1.0
    tilt: float = 0.0
    breath: float = 0.0
    f_hi: float = 4800.0


def warped_length(n: int, rate: float) -> int:
    """Samples of an ``n``-sample recording read at ``rate``."""
    return int(round(int(n) / float(rate)))


def warped_frames(n: int, hop: int, rate: float) -> int:
    """Frames (one per ``hop``, the first at sample 0) of an ``n``-sample recording read at ``rate``."""
    return 1 + warped_length(n, rate) // int(hop)


def source_positions(n_frames: int, rate: float, src_frames: int) -> np.ndarray:
    """Where output frame g reads the source, in source frames (float64): ``min(g * rate, src_frames - 1)``."""
    return np.minimum(np.arange(int(n_frames), dtype=np.float64) * float(rate), float(max(int(src_frames) - 1, 0)))


def time_warp_curve(base_f0, positions) -> np.ndarray:
    """The curve ``base_f0`` (0 = unvoiced) at the source ``positions``, host float64: linear in Hz between two voiced
    frames; where either neighbour is unvoiced, the value of the nearer one (the earlier on a tie), so that no value is
    an average with 0."""
    base = _host_f0(base_f0)
    pos = np.asarray(positions, dtype=np.float64).reshape(-1)
    if base.size == 0 or pos.size == 0:
        return np.zeros(pos.size)
    i = np.clip(np.floor(pos).astype(np.int64), 0, base.size - 1)
    j = np.minimum(i + 1, base.size - 1)
    t = np.clip(pos - i, 0.0, 1.0)
    a, b = base[i], base[j]
    return np.where((a > 0) & (b > 0), a + t * (b - a), np.where(t <= 0.5, a, b))


def warp_envelopes(env: Envelopes, ap, positions, transforms, fs, *, first=None, out: torch.Tensor | None = None,
                   out_offsets=None, out_strides=None):
    """The frames of ``env`` (``cheaptrick_ragged``'s result) read at ``positions`` under ``transforms``, one launch
    (``csrc/world_warp.hip``).  ``positions[r]``: float64 source-frame positions of row r's output frames, on the axis
    ``env.first`` counts on, each within the frames ``env`` holds; ``transforms[r]``: a ``VoiceTransform`` (``None``:
    the identity; ``rate`` is not read here: it is in the positions).  ``ap``: ``None``, one ``(bins,)`` float32 device
    template for every row and frame, or an ``Envelopes`` of the same frames (``d4c_ragged``'s).  ``first[r]``: the
    output frame ``positions[r][0]`` stands for (default 0); ``out`` / ``out_offsets`` / ``out_strides`` as for
    ``cheaptrick_ragged``.  Returns ``(Envelopes, ap_out)``: the warped envelopes, and the warped aperiodicity as a flat
    tensor in the same layout (``None`` without ``ap``).  There is no CPU path."""
    check_device_tensor(env.sp, "WORLD warp")
    fft_size = check_fft_size(env.fft_size)
    bins = fft_size // 2 + 1
    src_counts = _i64(env.counts)
    R = src_counts.size
    positions = [np.asarray(p, dtype=np.float64).reshape(-1) for p in positions]
    transforms = [VoiceTransform() if t is None else VoiceTransform(*t) for t in transforms]
    if len(positions) != R or len(transforms) != R:
        raise ValueError("WORLD warp: one position array and one transform per row")
    counts = _i64([p.size for p in positions], R)
    rel = np.concatenate([p - float(env.first[r]) for r, p in enumerate(positions)]) if R else np.zeros(0)
    if not np.all(np.isfinite(rel)):
        raise ValueError("WORLD warp: positions must be finite")
    whole = np.floor(rel)
    frac = (rel - whole).astype(np.float32)
    whole[frac >= 1.0] += 1.0                                   # a fraction that float32 rounds up to 1
    frac[frac >= 1.0] = 0.0
    pos_frame = np.ascontiguousarray(np.clip(whole, -1.0, 2.0 ** 31 - 1), dtype=np.int32)
    params = np.ascontiguousarray([[t.formant, t.f_hi, t.tilt, t.breath] for t in transforms],
                                  dtype=np.float32).reshape(R, 4)
    ap_t = ap_off = ap_str = None
    if isinstance(ap, Envelopes):
        if ap.fft_size != fft_size or not np.array_equal(ap.first, env.first) or \
                not np.array_equal(ap.counts, env.counts):
            raise ValueError("WORLD warp: ap must hold the frames env holds")
        ap_t, ap_off, ap_str = ap.sp, _i64(ap.offsets, R), _i64(ap.strides, R)
    elif ap is not None:
        if not torch.is_tensor(ap) or tuple(ap.shape) != (bins,):
            raise ValueError(f"WORLD warp: ap must be one ({bins},) template or an Envelopes")
        ap_t, ap_off, ap_str = ap, np.zeros(R, np.int64), np.zeros(R, np.int64)
    if ap_t is not None:
        check_device_tensor(ap_t, "WORLD warp")
    strides = np.full(R, bins, np.int64) if out_strides is None else _i64(out_strides, R)
    out_offsets = _i64(np.cumsum(counts * strides) - counts * strides if out_offsets is None else out_offsets, R)
    first = np.zeros(R, np.int64) if first is None else _i64(first, R)
    meta = plan_meta("pe_world_warp_plan_fields", R)
    totals = np.zeros(1, np.int64)
    _lib.check(_lib.load().pe_world_warp_plan(
        R, *host_ptrs(src_counts, _i64(env.offsets, R), _i64(env.strides, R), ap_off, ap_str, counts, out_offsets,
                      strides, pos_frame, frac, params), float(fs), fft_size, *host_ptrs(meta, totals)),
        "pe_world_warp_plan")
    live = counts > 0
    last = np.maximum(src_counts - 1, 0)
    if env.sp.numel() < int((_i64(env.offsets) + last * _i64(env.strides) + bins)[live].max(initial=0)):
        raise ValueError("WORLD warp: env.sp is smaller than its layout addresses")
    if ap_t is not None and ap_t.numel() < int((ap_off + last * ap_str + bins)[live].max(initial=0)):
        raise ValueError("WORLD warp: ap is smaller than its layout addresses")
    need = int((out_offsets + np.maximum(counts - 1, 0) * strides + bins)[live].max(initial=0))
    if out is None:
        out = torch.empty((max(need, 1),), dtype=torch.float32, device=env.sp.device)
    else:
        check_device_tensor(out, "WORLD warp")
        if out.numel() < need:
            raise ValueError("WORLD warp: the output is smaller than the plan addresses")
    ap_out = None if ap_t is None else torch.empty_like(out)
    if R and int(totals[0]):
        dev = env.sp.device
        up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
        meta_d, pos_d, frac_d, params_d = up(meta), up(pos_frame), up(frac), up(params)
        with torch.cuda.device(dev):
            ops._call("pe_world_warp", env.sp.data_ptr(), _lib.ptr(ap_t), meta_d.data_ptr(), meta.ctypes.data,
                      pos_d.data_ptr(), frac_d.data_ptr(), params_d.data_ptr(), R, float(fs), fft_size,
                      out.data_ptr(), _lib.ptr(ap_out), _lib.stream_ptr(),
                      work=float(int(totals[0]) * bins * 4 * (3 if ap_t is None else 6)))
    return Envelopes(out, out_offsets, strides, first, counts, fft_size), ap_out


def _resynthesize_warped(x, lengths, f0s, new_f0s, fs, frame_period, transforms, positions, *, ap, seeds, noise,
                         noise_offsets, gains, out, out_rows, out_start, out_len, out_noise, tables, q1, f0_floor,
                         fft_size, d4c_threshold):
    """``resynthesize_ragged`` with ``transforms``: the analyses run on the source frames, ``warp_envelopes`` brings
    them to the output frames, and the synthesizer reads those in place."""
    check_waves(x, "WORLD resynthesis")
    R = len(row_layout(x, lengths, whole_by_default=True)[0])
    fft_size = check_fft_size(cheaptrick_fft_size(fs, f0_floor) if fft_size is None else fft_size)
    bins = fft_size // 2 + 1
    labels = [label_curve(f, fs, fft_size) for f in new_f0s]
    f0s = list(f0s)
    transforms = [VoiceTransform() if t is None else VoiceTransform(*t) for t in transforms]
    if len(f0s) != R or len(labels) != R or len(transforms) != R:
        raise ValueError("WORLD resynthesis: one F0 curve, one new curve and one transform per row")
    for t in transforms:
        if not (math.isfinite(t.rate) and 0.25 <= t.rate <= 4.0):
            raise ValueError("WORLD resynthesis: a transform's rate must lie in [0.25, 4]")
    src_frames = np.array([len(f) for f in f0s], np.int64)
    n_frames = np.array([b.size for b in labels], np.int64)
    if positions is None:
        positions = [source_positions(n_frames[r], transforms[r].rate, src_frames[r]) for r in range(R)]
    positions = [np.asarray(p, dtype=np.float64).reshape(-1) for p in positions]
    if len(positions) != R or any(p.size != n for p, n in zip(positions, n_frames)):
        raise ValueError("WORLD resynthesis: one source position per frame of the new curve")
    if any(n > 0 and s < 1 for n, s in zip(n_frames, src_frames)):
        raise ValueError("WORLD resynthesis: a row with output frames needs source frames")
    estimate = isinstance(ap, str)
    if estimate and ap != "d4c":
        raise ValueError(f"WORLD resynthesis: ap {ap!r} is not a mode; the one estimator is 'd4c'")
    if ap is not None and not estimate and tuple(ap.shape) != (bins,):
        raise ValueError(f"WORLD resynthesis: ap must be one ({bins},) template")
    y_len = np.array([output_length(n, fs, frame_period) for n in n_frames], np.int64)
    out_start = np.zeros(R, np.int64) if out_start is None else _i64(out_start, R)
    out_len = y_len - out_start if out_len is None else _i64(out_len, R)
    if out is None:
        out = torch.zeros((max(R, 1), max(int(out_len.max(initial=0)), 1)), dtype=torch.float32, device=x.device)
    # the output frames the planned pulses read, as without transforms ...
    per_frame = frame_period * fs / 1000.0
    lo = np.clip(np.floor((out_start - fft_size // 2) / per_frame).astype(np.int64) - 1, 0, n_frames)
    hi = np.clip(np.ceil((out_start + out_len + fft_size // 2) / per_frame).astype(np.int64) + 2, 0, n_frames)
    hi = np.where(out_len > 0, hi, lo)
    # ... and the source frames those read: floor / ceil of their positions, and one frame either side
    s_lo, s_hi = np.zeros(R, np.int64), np.zeros(R, np.int64)
    for r in range(R):
        if hi[r] > lo[r]:
            p = positions[r][lo[r]:hi[r]]
            s_lo[r] = min(max(int(math.floor(p.min())) - 1, 0), src_frames[r])
            s_hi[r] = min(max(int(math.ceil(p.max())) + 2, 0), src_frames[r])
    rows = _frame_rows("CheapTrick", x, lengths, f0s, list(zip(s_lo, s_hi - s_lo)))
    env = cheaptrick_ragged(x, lengths, f0s, fs, frame_period, q1=q1, f0_floor=f0_floor, fft_size=fft_size, _rows=rows)
    if estimate:
        ap = d4c_ragged(x, lengths, f0s, fs, frame_period, threshold=d4c_threshold, fft_size=fft_size, _rows=rows)
    base = np.cumsum(n_frames * bins) - n_frames * bins          # each row's output frame 0, whole rows laid out
    sp = torch.empty((max(int((n_frames * bins).sum()), 1),), dtype=torch.float32, device=x.device)
    warped, ap = warp_envelopes(env, ap, [p[a:b] for p, a, b in zip(positions, lo, hi)], transforms, fs, first=lo,
                                out=sp, out_offsets=base + lo * bins)
    ap_offsets = ap_strides = None
    if ap is not None:
        ap_offsets, ap_strides = warped.frame0_offsets(), warped.strides
    world_synthesize_ragged(labels, warped.sp, warped.frame0_offsets(), warped.strides,
                            torch.ones(R) if gains is None else gains, out, out_rows, out_start, out_len, fs=fs,
                            frame_period=frame_period, fft_size=fft_size, ap=ap, ap_offsets=ap_offsets,
                            ap_strides=ap_strides, tables=tables, noise=noise, noise_offsets=noise_offsets,
                            seeds=seeds, out_noise=out_noise)
    return out, labels


def resynthesize_ragged(x: torch.Tensor, lengths, f0s, new_f0s, fs, frame_period: float, *, ap=None, seeds=None,
                        noise=None, noise_offsets=None, gains=None, out: torch.Tensor | None = None, out_rows=None,
                        out_start=None, out_len=None, out_noise=None, tables=None, q1: float = CHEAPTRICK_Q1,
                        f0_floor: float = CHEAPTRICK_F0_FLOOR, fft_size: int | None = None,
                        d4c_threshold: float = D4C_THRESHOLD, transforms=None, positions=None):
    """Analysis / resynthesis of a ragged batch: the envelope of row r of ``x`` under ``f0s[r]``
    (``cheaptrick_ragged``), then ``world_synthesize_ragged`` driven by ``label_curve(new_f0s[r])`` reading that
    envelope in place.  ``ap``: ``None``, one ``(bins,)`` float32 device template for every row and frame, or the
    string ``"d4c"``: the recording's own aperiodicity (``d4c_ragged`` with ``d4c_threshold`` on the frames CheapTrick
    analyses, into a buffer of the same layout that the synthesizer reads in place).  With
    windows (``out_start`` / ``out_len``) only the frames their pulses read are analysed: the samples of the window -+
    ``fft_size / 2``, and one frame either side for the synthesizer's frame interpolation.  The other arguments are
    ``world_synthesize_ragged``'s. Returns ``(out, labels)``, ``labels[r]`` the float64 label curve of row r.

    ``transforms``: one ``VoiceTransform`` (or ``None``: the identity) per row changes the speaker and leaves the label
    exact (``warp_envelopes``).  ``new_f0s[r]`` is then on the output time axis, one value per output frame, and output
    frame g reads the source at ``positions[r][g]`` frames (default ``min(g * rate, len(f0s[r]) - 1)``); only the
    source frames the window's output frames read are analysed.  Without ``transforms`` nothing of this runs."""
    if transforms is not None:
        return _resynthesize_warped(x, lengths, f0s, new_f0s, fs, frame_period, transforms, positions, ap=ap,
                                    seeds=seeds, noise=noise, noise_offsets=noise_offsets, gains=gains, out=out,
                                    out_rows=out_rows, out_start=out_start, out_len=out_len, out_noise=out_noise,
                                    tables=tables, q1=q1, f0_floor=f0_floor, fft_size=fft_size,
                                    d4c_threshold=d4c_threshold)
    check_waves(x, "WORLD resynthesis")
    R = len(row_layout(x, lengths, whole_by_default=True)[0])
    fft_size = check_fft_size(cheaptrick_fft_size(fs, f0_floor) if fft_size is None else fft_size)
    bins = fft_size // 2 + 1
    labels = [label_curve(f, fs, fft_size) for f in new_f0s]
    f0s = list(f0s)
    if len(f0s) != R or len(labels) != R or any(len(a) != b.size for a, b in zip(f0s, labels)):
        raise ValueError("WORLD resynthesis: one F0 curve and one new curve of the same length per row")
    estimate = isinstance(ap, str)
    if estimate and ap != "d4c":
        raise ValueError(f"WORLD resynthesis: ap {ap!r} is not a mode; the one estimator is 'd4c'")
    if ap is not None and not estimate and tuple(ap.shape) != (bins,):
        raise ValueError(f"WORLD resynthesis: ap must be one ({bins},) template")
    n_frames = np.array([b.size for b in labels], np.int64)
    y_len = np.array([output_length(n, fs, frame_period) for n in n_frames], np.int64)
    out_start = np.zeros(R, np.int64) if out_start is None else _i64(out_start, R)
    out_len = y_len - out_start if out_len is None else _i64(out_len, R)
    if out is None:
        out = torch.zeros((max(R, 1), max(int(out_len.max(initial=0)), 1)), dtype=torch.float32, device=x.device)
    # frames the planned pulses read: pulse samples in [start - N/2, start + len - 2 + N/2], frames floor / ceil of each
    per_frame = frame_period * fs / 1000.0
    lo = np.clip(np.floor((out_start - fft_size // 2) / per_frame).astype(np.int64) - 1, 0, n_frames)
    hi = np.clip(np.ceil((out_start + out_len + fft_size // 2) / per_frame).astype(np.int64) + 2, 0, n_frames)
    hi = np.where(out_len > 0, hi, lo)
    base = np.cumsum(n_frames * bins) - n_frames * bins          # each row's frame 0, whole rows laid out
    sp = torch.empty((max(int((n_frames * bins).sum()), 1),), dtype=torch.float32, device=x.device)
    rows = _frame_rows("CheapTrick", x, lengths, f0s, list(zip(lo, hi - lo)))    # once, for both analyses
    env = cheaptrick_ragged(x, lengths, f0s, fs, frame_period, q1=q1, f0_floor=f0_floor, fft_size=fft_size, out=sp,
                            out_offsets=base + lo * bins, _rows=rows)
    ap_offsets = ap_strides = None if ap is None else [0] * R
    if estimate:
        ap = d4c_ragged(x, lengths, f0s, fs, frame_period, threshold=d4c_threshold, fft_size=fft_size,
                        out=torch.empty_like(sp), out_offsets=base + lo * bins, _rows=rows).sp
        ap_offsets, ap_strides = env.frame0_offsets(), env.strides
    world_synthesize_ragged(labels, env.sp, env.frame0_offsets(), env.strides,
                            torch.ones(R) if gains is None else gains, out, out_rows, out_start, out_len, fs=fs,
                            frame_period=frame_period, fft_size=fft_size, ap=ap, ap_offsets=ap_offsets,
                            ap_strides=ap_strides,
                            tables=tables, noise=noise, noise_offsets=noise_offsets, seeds=seeds, out_noise=out_noise)
    return out, labels


def resynthesize(x: torch.Tensor, f0, new_f0, fs, frame_period: float = 5.0, *, ap=None, seed: int = 0,
                 noise: torch.Tensor | None = None, q1: float = CHEAPTRICK_Q1, f0_floor: float = CHEAPTRICK_F0_FLOOR,
                 fft_size: int | None = None, d4c_threshold: float = D4C_THRESHOLD,
                 transform: VoiceTransform | None = None, time_base: str = "host"):
    """The recording ``x`` (1-D float32 device wave with the curve ``f0``) resynthesized on ``new_f0``: its CheapTrick
    envelope through WORLD's ``Synthesis``, with no aperiodicity (``ap=None``), one ``(bins,)`` template, or the
    recording's own as D4C estimates it (``ap="d4c"``, ``d4c_threshold``).  Returns ``(audio, label)``: the 1-D float32 device wave of
    ``int(len(f0) * frame_period * fs / 1000)`` samples and the float64 host curve it was synthesized from
    (``label_curve``), exact by construction.  With ``transform`` (a ``VoiceTransform``) the speaker changes as well:
    ``new_f0`` then has one value per output frame (``time_warp_curve`` brings a curve there), and the wave has
    ``int(len(new_f0) * frame_period * fs / 1000)`` samples.  ``time_base``: ``"host"`` or ``"device"``, where the
    pulse positions are computed (``time_base_device``)."""
    tables = "device" if check_time_base_mode(time_base) == "device" else None
    if not torch.is_tensor(x) or x.dim() != 1:
        raise RuntimeError("WORLD resynthesis (HIP) needs a 1-D float32 device wave; no CPU fallback exists")
    n = output_length(len(_host_f0(new_f0)), fs, frame_period)
    if noise is not None and noise.numel() != n:
        raise ValueError("resynthesize: noise must hold one value per output sample")
    out, labels = resynthesize_ragged(x, None, [f0], [new_f0], fs, frame_period, ap=ap, seeds=[seed],
                                      noise=None if noise is None else noise.reshape(-1),
                                      noise_offsets=None if noise is None else [0], q1=q1, f0_floor=f0_floor,
                                      fft_size=fft_size, d4c_threshold=d4c_threshold, tables=tables,
                                      transforms=None if transform is None else [transform])
    return out[0, :n], labels[0]


# --------------------------------------------------------------------------- the reference's vowel generator
def formant_templates(profiles, fs, fft_size: int):
    """Utils/synthetic.py:122-147: one spectral envelope per profile, a sum of Gaussians floored at 1e-3."""
    freq_axis = np.linspace(0, fs / 2, fft_size // 2 + 1)
    templates = []
    for profile in profiles:
        formants = profile.get("formants", [])
        if not formants:
            continue
        envelope = np.zeros_like(freq_axis)
        for formant in formants:
            if len(formant) < 2:
                continue
            freq, bandwidth = float(formant[0]), float(formant[1])
            amplitude = float(formant[2]) if len(formant) > 2 else 1.0
            if bandwidth <= 0:
                bandwidth = 60.0
            envelope += amplitude * np.exp(-0.5 * ((freq_axis - freq) / (bandwidth / 2.0)) ** 2)
        templates.append(np.maximum(envelope, 1e-3).astype(np.float64))
    if not templates:
        raise ValueError("No valid vowel templates provided for WORLD synthesis")
    return templates


@dataclass
class ModulationConfig:
    vibrato_probability: float = 0.6
    vibrato_semitones: float = 0.35
    vibrato_rate_range: Tuple[float, float] = (4.0, 7.0)
    max_segments: int = 4


class WorldDraw(NamedTuple):
    curve: np.ndarray                          # float64 (L,) the drawn F0 curve, one value per hop
    template: int
    gain: float
    noise: np.ndarray | None                   # float64 (n,) additive noise of the whole utterance
    table: PulseTable


class WorldGenerator:
    """The host half of the reference's ``WorldSynthesizer`` (Utils/synthetic.py:71-220): the same configuration, the
    same validation, and ``draw`` consuming ``random`` and ``np.random`` exactly as ``generate`` does.  The synthesis
    itself is left to the device (``world_synthesize_ragged``)."""

    def __init__(self, sample_rate, hop_length, fft_size=None, config=None):
        self.sample_rate, self.hop_length = int(sample_rate), int(hop_length)
        self.fft_size = check_fft_size(int(fft_size or 1024))
        cfg = dict(config or {})
        duration_cfg = cfg.get("duration", {}) or {}
        self.min_duration = float(duration_cfg.get("min", 0.5))
        self.max_duration = float(duration_cfg.get("max", 1.8))
        if self.max_duration <= 0:
            raise ValueError("Synthetic duration must be positive")
        pitch_range = cfg.get("pitch_range", [110.0, 320.0])
        if len(pitch_range) != 2:
            raise ValueError("pitch_range must contain two values")
        self.pitch_min, self.pitch_max = float(min(pitch_range)), float(max(pitch_range))
        noise_db_cfg = cfg.get("noise_db", -60.0)
        self.noise_db = None if noise_db_cfg is None else float(noise_db_cfg)
        gain_cfg = cfg.get("gain_db_range", [-18.0, -6.0])
        if isinstance(gain_cfg, (int, float)):
            gain_cfg = [gain_cfg, gain_cfg]
        if len(gain_cfg) != 2:
            raise ValueError("gain_db_range must provide two values")
        gain_min, gain_max = float(gain_cfg[0]), float(gain_cfg[1])
        if gain_min > gain_max:
            gain_min, gain_max = gain_max, gain_min
        self.gain_db_range = (gain_min, gain_max)
        # where the pulse tables are computed: "host" (draw() calls time_base) or "device" (draw() leaves the table
        # empty and the device stage computes the batch's tables at once); no draw depends on it
        self.time_base = check_time_base_mode(cfg.get("time_base", "host"))
        self.modulation = ModulationConfig(**(cfg.get("modulation", {}) or {}))
        self.templates = formant_templates(cfg.get("vowel_profiles") or DEFAULT_VOWELS, self.sample_rate,
                                           self.fft_size)
        self.frame_period = 1000.0 * self.hop_length / self.sample_rate
        table = np.stack(self.templates).astype(np.float32)
        self._table_key = ("world_templates", self.fft_size, hashlib.blake2b(table.tobytes(), digest_size=8).hexdigest())
        self._table = table

    def device_templates(self, device) -> torch.Tensor:
        """The templates as one float32 device table (T, fft_size / 2 + 1), copied once per device."""
        return _lib.device_table(self._table_key, device, lambda: self._table)

    def _sample_duration(self) -> float:
        if self.max_duration <= self.min_duration:
            return max(self.max_duration, 0.1)
        return random.uniform(self.min_duration, self.max_duration)

    def _sample_f0_curve(self, num_frames: int) -> np.ndarray:
        base = random.uniform(self.pitch_min, self.pitch_max)
        curve = np.full(num_frames, base, dtype=np.float64)
        num_segments = random.randint(1, max(1, int(self.modulation.max_segments)))
        if num_segments > 1 and num_frames > 2:
            available = max(1, num_frames - 1)
            positions = sorted(random.sample(range(1, available), min(num_segments - 1, available - 1)))
            positions = [0] + positions + [num_frames - 1]
            values = [random.uniform(self.pitch_min, self.pitch_max) for _ in range(len(positions))]
            for i in range(len(positions) - 1):
                start, end = positions[i], positions[i + 1]
                if end <= start:
                    continue
                curve[start:end + 1] = np.linspace(values[i], values[i + 1], end - start + 1)
        if random.random() < self.modulation.vibrato_probability:
            depth = max(float(self.modulation.vibrato_semitones), 0.0)
            if depth > 0:
                rate = random.uniform(*self.modulation.vibrato_rate_range)
                t = np.arange(num_frames, dtype=np.float64) * (self.frame_period / 1000.0)
                curve *= 2.0 ** (np.sin(2.0 * math.pi * rate * t) * (depth / 12.0))
        return curve

    def draw(self) -> WorldDraw:
        duration = self._sample_duration()
        num_frames = max(2, int(np.ceil((duration * 1000.0) / self.frame_period)))
        template = random.choice(range(len(self.templates)))
        curve = self._sample_f0_curve(num_frames)
        gain = float(10.0 ** (random.uniform(*self.gain_db_range) / 20.0))
        n = output_length(num_frames, self.sample_rate, self.frame_period)
        noise = None
        if self.noise_db is not None:
            noise_gain = float(10.0 ** (self.noise_db / 20.0))
            if noise_gain > 0:
                noise = np.random.normal(scale=noise_gain, size=(n,))
        return WorldDraw(curve, template, gain, noise, no_table() if self.time_base == "device" else
                         time_base(curve, self.sample_rate, self.frame_period, self.fft_size))
