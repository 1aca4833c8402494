"""The oracle of the device time base (``world.time_base_device``, ``csrc/world_time_base.hip``): WORLD's GetTimeBase +
GetPulseLocationsForTimeBase with the phase as an exact integer, restated twice -- a plain Python-``int`` loop over the
samples (``time_base_int``) and a vectorised numpy form with ``uint64`` words and explicit carries
(``time_base_vec``) -- which must agree exactly, and with the kernels bit for bit.

For a row of ``L >= 2`` finite frames ``f0``, ``fs``, ``frame_period_ms`` and ``fft_size``, with ``fp =
frame_period_ms / 1000`` and ``n = world.output_length(L, fs, frame_period_ms)``, everything float64 without contraction:

  coarse curves   ``cf = where(f0 >= lowest_f0, f0, 0)``, ``cv = (cf != 0)``; both get one extrapolated frame ``2 a[L-1]
                  - a[L-2]``; the extrapolated ``cf[L]`` is clamped at 0 from below (the one stated deviation from
                  ``world.time_base``: without it a voiced last frame below half its predecessor runs the phase
                  backwards inside the last frame period).  ``ValueError`` unless every value of the extended ``cf``,
                  and 500, is below ``fs / 2``.
  per sample i    ``t = i / fs``, ``ct[j] = j * fp``; ``j = clip(floor(t / fp), 0, L - 1)`` corrected by comparisons so
                  that ``ct[j] <= t < ct[j + 1]`` and clipped again; ``interp(c) = ((c[j+1] - c[j]) / (ct[j+1] - ct[j]))
                  * (t - ct[j]) + c[j]``; ``vuv_i = interp(cv) > 0.5``; ``f0i = interp(cf) if vuv_i else 500``.
  increment       ``inc_i = rint(ldexp(f0i / fs, 64))``, an unsigned 64-bit integer below 2^63 (ties to even).
  phase           ``T_i = sum of inc_k for k <= i`` exactly; ``hi_i = T_i >> 64``, ``lo_i = T_i mod 2^64``.
  pulses          sample ``i`` in ``[0, n - 2]`` carries pulse number ``hi_i`` iff ``hi_(i+1) == hi_i + 1``; the row has
                  ``hi_(n-1)`` pulses.
  delay           ``x = float(2^64 - lo_i) / float(inc_(i+1))`` (both conversions to nearest even, IEEE division), in
                  (0, 1]; ``shift = x / fs``.  ``vuv[p] = vuv_i``; ``noise_size`` from ``np.diff`` of the indices.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from pitchextractor_amd.world import PulseTable, lowest_f0, output_length

UNVOICED_F0 = 500.0
PIECE = 4096
TWO64 = 1 << 64


class Trace(NamedTuple):
    """A row's table and what the kernels' test hooks show: per-sample ``f0i`` (float64), ``lo`` (uint64), ``hi``
    (int64), and the pulse count."""
    table: PulseTable
    f0i: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    count: int


def coarse_curves(f0, fs, frame_period_ms, fft_size):
    """``(cf_ext, cv_ext)``: float64 arrays of ``L + 1`` values each."""
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
    if not (max(float(cf.max()), UNVOICED_F0) < fs / 2.0):
        raise ValueError("WORLD time base: F0 must stay below half the sample rate")
    return cf, cv


def capacity(cf_ext, n, fs) -> int:
    """The plan's pulse slots of a row: ``floor(n * max(cf_ext, 500) / fs) + 1``."""
    return int(math.floor(float(n) * max(float(np.max(cf_ext)), UNVOICED_F0) / float(fs))) + 1


def _finish(index, shift, vuv, f0i, lo, hi, n):
    index = np.asarray(index, dtype=np.int64)
    noise_size = np.zeros_like(index)
    noise_size[:-1] = np.diff(index)
    table = PulseTable(index, np.asarray(shift, dtype=np.float64), np.asarray(vuv, dtype=bool), noise_size)
    return Trace(table, f0i, lo, hi, int(hi[n - 1]) if n > 0 else 0)


def time_base_int(f0, fs, frame_period_ms, fft_size) -> Trace:
    """The definition as a loop over the samples: Python floats (IEEE double) and Python ints."""
    cf, cv = (a.tolist() for a in coarse_curves(f0, fs, frame_period_ms, fft_size))
    L = len(cf) - 1
    fp = frame_period_ms / 1000.0
    fs_f = float(fs)
    n = output_length(L, fs, frame_period_ms)
    incs, vuvs, f0is = [], [], []
    for i in range(n):
        t = i / fs_f
        j = min(max(int(math.floor(t / fp)), 0), L - 1)
        while j > 0 and j * fp > t:
            j -= 1
        while j < L - 1 and (j + 1) * fp <= t:
            j += 1
        x0, x1 = j * fp, (j + 1) * fp
        v = ((cv[j + 1] - cv[j]) / (x1 - x0)) * (t - x0) + cv[j]
        voiced = v > 0.5
        f = ((cf[j + 1] - cf[j]) / (x1 - x0)) * (t - x0) + cf[j] if voiced else UNVOICED_F0
        incs.append(round(math.ldexp(f / fs_f, 64)))                 # Python's round: exact, ties to even, as rint
        vuvs.append(voiced)
        f0is.append(f)
    total, los, his = 0, [], []
    for inc in incs:
        total += inc
        los.append(total % TWO64)
        his.append(total >> 64)
    index, shift, vuv = [], [], []
    for i in range(n - 1):
        if his[i + 1] == his[i] + 1:
            assert his[i] == len(index)
            x = float(TWO64 - los[i]) / float(incs[i + 1])
            index.append(i)
            shift.append(x / fs_f)
            vuv.append(vuvs[i])
    return _finish(index, shift, vuv, np.array(f0is, dtype=np.float64), np.array(los, dtype=np.uint64),
                   np.array(his, dtype=np.int64), n)


def time_base_vec(f0, fs, frame_period_ms, fft_size) -> Trace:
    """The definition vectorised: numpy float64, and uint64 words with explicit carries for the phase."""
    cf, cv = coarse_curves(f0, fs, frame_period_ms, fft_size)
    L = cf.shape[0] - 1
    fp = frame_period_ms / 1000.0
    fs_f = float(fs)
    n = output_length(L, fs, frame_period_ms)
    t = np.arange(n, dtype=np.float64) / fs_f
    j = np.clip(np.floor(t / fp).astype(np.int64), 0, L - 1)
    for _ in range(4):
        j = np.where((j > 0) & (j * fp > t), j - 1, j)
    for _ in range(4):
        j = np.where((j < L - 1) & ((j + 1) * fp <= t), j + 1, j)
    x0, x1 = j * fp, (j + 1) * fp
    interp = lambda c: ((c[j + 1] - c[j]) / (x1 - x0)) * (t - x0) + c[j]  # noqa: E731
    voiced = interp(cv) > 0.5
    f0i = np.where(voiced, interp(cf), UNVOICED_F0)
    inc = np.rint(np.ldexp(f0i / fs_f, 64)).astype(np.uint64)
    with np.errstate(over="ignore"):
        lo = np.cumsum(inc, dtype=np.uint64)                         # wraps modulo 2^64
    carry = lo < inc                                                 # the addition of inc_i passed 2^64
    hi = np.cumsum(carry.astype(np.int64))
    index = np.flatnonzero(carry[1:]).astype(np.int64)               # hi_(i+1) == hi_i + 1
    rest = np.where(lo[index] == 0, float(TWO64), (np.uint64(0) - lo[index]).astype(np.float64)) if index.size else \
        np.zeros(0)
    shift = (rest / inc[index + 1].astype(np.float64)) / fs_f
    return _finish(index, shift, voiced[index], f0i, lo, hi, n)


def table_of(f0, fs, frame_period_ms, fft_size) -> PulseTable:
    """The restatement's ``PulseTable``: a drop-in for ``world.time_base``."""
    return time_base_vec(f0, fs, frame_period_ms, fft_size).table


# --------------------------------------------------------------------------- the test curves
CONFIGS = (                                                          # fs, fft_size, frame_period_ms
    (24000, 1024, 12.5), (16000, 1024, 5.0), (48000, 2048, 10.0), (22050, 1024, 1000.0 * 256 / 22050),
    (8000, 512, 10.0))


def margin_curves(L: int, seed: int = 0):
    """Curves whose pulses keep a phase margin (no period is a whole number of samples for long): a glide, a vibrato
    with jitter, voiced / unvoiced / voiced, and one with trailing unvoiced frames."""
    rng = np.random.RandomState(seed)
    k = np.arange(L, dtype=np.float64)
    glide = 111.3 + (287.9 - 111.3) * k / (L - 1)
    vibrato = 203.7 * 2.0 ** (0.5 / 12.0 * np.sin(2 * np.pi * 5.3 * k / 97.0)) + rng.uniform(-0.7, 0.7, L)
    vuv = 151.9 + 40.0 * np.sin(2 * np.pi * k / 61.0) + rng.uniform(-0.5, 0.5, L)
    vuv[L // 3: L // 3 + max(L // 7, 1)] = 0.0
    trailing = 263.1 + 30.0 * np.cos(2 * np.pi * k / 43.0) + rng.uniform(-0.5, 0.5, L)
    trailing[-max(L // 9, 3):] = 0.0
    return {"glide": glide, "vibrato": vibrato, "vuv": vuv, "trailing": trailing}
