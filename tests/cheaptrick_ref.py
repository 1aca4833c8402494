"""float64 restatement of WORLD's CheapTrick (Morise, Speech Communication 2015; ``cheaptrick.cpp``, what pyworld calls
``cheaptrick``), written from the published algorithm for testing ``pitchextractor_amd.world.cheaptrick`` and
``csrc/cheaptrick.hip``.  pyworld is not available here: parity with its binary is unpinned.  Stated
deviations, shared with the kernel: the two ``randn`` safeguard terms are dropped (1e-12 in the window) or replaced by
their scale (``+ 2^-52`` after the linear smoothing), and the linear smoothing is the sum over the covered bins plus the
two partial edge bins (``smooth_interval``) instead of WORLD's difference of two interpolated points of a cumulative sum
(``smooth_cumulative``, kept here as the literal formulation the first is tested against).  ``fp32=True`` is the same
formulation with every array, transform and sum in float32 / complex64 -- the yardstick for what the device's float32
arithmetic may cost.  The frame's sample origin and window length are float64 in both variants, as on the device."""
from __future__ import annotations

import math

import numpy as np
import scipy.fft

DEFAULT_F0 = 500.0
EPS = 2.0 ** -52


def f0_floor_of(fs, fft_size):
    return 3.0 * fs / (fft_size - 3.0)


def default_fft_size(fs, f0_floor=71.0):
    return 2 ** (1 + int(math.log(3.0 * fs / f0_floor + 1) / math.log(2.0)))


def frame_window(x, fs, f0, position, ft=np.float64):
    """The F0-adaptive Hann-like window at ``position`` seconds, applied: sum w^2 = 1, zero DC."""
    half = int(1.5 * fs / f0 + 0.5)
    origin = int(position * fs + 0.001 + 0.5)
    i = np.arange(-half, half + 1)
    seg = np.asarray(x, dtype=ft)[np.clip(origin + i, 0, len(x) - 1)]
    w = ft(0.5) * np.cos(ft(np.pi) * (i.astype(ft) * ft(f0 / (1.5 * fs)))).astype(ft) + ft(0.5)
    w = (w / np.sqrt(np.sum(w * w, dtype=ft))).astype(ft)
    coef = np.sum(seg * w, dtype=ft) / np.sum(w, dtype=ft)
    return (seg * w - w * coef).astype(ft)


def power_spectrum(wave, fft_size, fp32=False):
    if fp32:
        X = scipy.fft.rfft(np.asarray(wave, dtype=np.float32), fft_size)
        return (X.real * X.real + X.imag * X.imag).astype(np.float32)
    return np.abs(np.fft.rfft(wave, fft_size)) ** 2


def dc_correction(P, fs, f0, fft_size):
    """P[k] += P interpolated at f0 - k delta for every k with k delta <= f0."""
    ft = P.dtype.type
    K = min(int(f0 / (fs / fft_size)), fft_size // 2 - 1)
    k = np.arange(K + 1)
    pos = ft(f0 * fft_size / fs) - k.astype(ft)
    base = np.floor(pos).astype(np.int64)
    frac = (pos - base).astype(ft)
    out = P.copy()
    out[:K + 1] = P[:K + 1] + (P[base] + (P[base + 1] - P[base]) * frac)
    return out


def _mirror(j, fft_size):
    j = np.abs(j)
    return np.where(j > fft_size // 2, fft_size - j, j)


def smooth_interval(P, fs, f0, fft_size):
    """Mean over [f - w/2, f + w/2], w = 2 f0 / 3, of the piecewise-constant spectrum holding P[k] on [(k - 1/2) delta,
    (k + 1/2) delta), mirrored at 0 and fs/2.  In cell units the interval is [k + 1/2 - h, k + 1/2 + h) with h = f0 N /
    (3 fs): the two partial weights do not depend on k."""
    ft = P.dtype.type
    H = fft_size // 2
    h = ft(f0 * fft_size / (3.0 * fs))
    hi = int(math.floor(h))
    hf = ft(h - ft(hi))
    lo_down = hf > ft(0.5)                                       # the lower edge falls one cell further down
    ka_off = -hi - (1 if lo_down else 0)
    wa = ft(1.0) - (ft(1.5) - hf if lo_down else ft(0.5) - hf)
    up = hf >= ft(0.5)
    kb_off = hi + (1 if up else 0)
    wb = hf - ft(0.5) if up else ft(0.5) + hf
    k = np.arange(H + 1)
    if ka_off == kb_off:                                         # h < 1/2: the interval lies inside one cell
        return (ft(2.0) * h * P[_mirror(k + ka_off, fft_size)] / (ft(2.0) * h)).astype(ft)
    s = wa * P[_mirror(k + ka_off, fft_size)]
    if kb_off - ka_off > 1:
        whole = k[:, None] + np.arange(ka_off + 1, kb_off)[None, :]
        s = s + np.sum(P[_mirror(whole, fft_size)], axis=1, dtype=ft)
    s = s + wb * P[_mirror(k + kb_off, fft_size)]
    return (s / (ft(2.0) * h)).astype(ft)


def smooth_cumulative(P, fs, f0, fft_size):
    """WORLD's LinearSmoothing, literally: the mirrored spectrum's cumulative sum, interpolated at f -+ w/2."""
    H = fft_size // 2
    width = f0 * 2.0 / 3.0
    delta = fs / fft_size
    boundary = int(width * fft_size / fs) + 1
    j = np.arange(H + 2 * boundary + 1) - boundary
    segment = np.cumsum(P[_mirror(j, fft_size)] * delta)
    origin = -(boundary - 0.5) * delta

    def interp(xi):
        pos = (xi - origin) / delta
        base = np.floor(pos).astype(np.int64)
        return segment[base] + (segment[base + 1] - segment[base]) * (pos - base)

    axis = np.arange(H + 1) / fft_size * fs - width / 2.0
    return (interp(axis + width) - interp(axis)) / width


def lifter(fs, f0, fft_size, q1):
    i = np.arange(1, fft_size // 2 + 1)
    x = f0 * i / fs
    out = np.ones(fft_size // 2 + 1)
    out[1:] = np.sin(np.pi * x) / (np.pi * x) * ((1.0 - 2.0 * q1) + 2.0 * q1 * np.cos(2.0 * np.pi * x))
    return out


def smoothing_with_recovery(Q, fs, f0, fft_size, q1, fp32=False):
    ft = np.float32 if fp32 else np.float64
    H = fft_size // 2
    logq = np.log(Q).astype(ft)
    full = np.concatenate([logq, logq[H - 1:0:-1]])
    lift = lifter(fs, f0, fft_size, q1).astype(ft)
    if fp32:
        c = scipy.fft.fft(full.astype(np.complex64)).real[:H + 1].astype(ft) * lift / ft(fft_size)
        env = scipy.fft.fft(np.concatenate([c, c[H - 1:0:-1]]).astype(np.complex64)).real[:H + 1]
    else:
        c = np.fft.fft(full).real[:H + 1] * lift / fft_size
        env = np.fft.fft(np.concatenate([c, c[H - 1:0:-1]])).real[:H + 1]
    return np.exp(env.astype(ft))


def used_f0(f0, fs, fft_size):
    return DEFAULT_F0 if not f0 > f0_floor_of(fs, fft_size) else float(f0)


def frame(x, fs, f0, position, fft_size, q1=-0.15, fp32=False, smooth=True):
    """One frame's envelope (fft_size / 2 + 1,); ``smooth=False``: the windowed periodogram of the same frame."""
    ft = np.float32 if fp32 else np.float64
    f0 = used_f0(f0, fs, fft_size)
    P = power_spectrum(frame_window(x, fs, f0, position, ft), fft_size, fp32)
    if not smooth:
        return P
    P = dc_correction(P, fs, f0, fft_size)
    Q = smooth_interval(P, fs, f0, fft_size) + ft(EPS)
    return smoothing_with_recovery(Q, fs, f0, fft_size, q1, fp32)


def cheaptrick(x, f0, fs, frame_period_ms=5.0, q1=-0.15, f0_floor=71.0, fft_size=None, fp32=False, first_frame=0,
               n_frames=None):
    """(frames, fft_size / 2 + 1): frame f at f * frame_period_ms, ``f0`` float32-rounded as the device reads it."""
    fft_size = default_fft_size(fs, f0_floor) if fft_size is None else int(fft_size)
    f0 = np.asarray(f0, dtype=np.float32).astype(np.float64).reshape(-1)
    n_frames = f0.size - first_frame if n_frames is None else n_frames
    out = np.empty((n_frames, fft_size // 2 + 1), np.float32 if fp32 else np.float64)
    for q in range(n_frames):
        f = first_frame + q
        out[q] = frame(x, fs, f0[f], f * (frame_period_ms / 1000.0), fft_size, q1, fp32)
    return out
