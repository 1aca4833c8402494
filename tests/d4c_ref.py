"""float64 restatement of WORLD's D4C (Morise, Speech Communication 84, 2016; ``d4c.cpp``, what pyworld calls ``d4c``),
written from the published algorithm for testing ``pitchextractor_amd.world.d4c`` and ``csrc/d4c.hip``.  pyworld is not
available here: parity with its binary is unpinned.  Stated deviations, shared with the kernel:
the window's ``randn * 1e-12`` is dropped; a LoveTrain frame whose denominator is 0 has ``a0 = 0``; a frame whose
smoothed power is not positive in every bin takes the unvoiced verdict; a band whose group delay is all zero reads 0
dB and ``coarse`` is floored at -200 dB; the linear smoothing is the interval sum of ``tests/cheaptrick_ref.py`` at a
general width.  ``fp32=True`` is the same formulation with every array, transform and sum in float32 / complex64 -- the
yardstick for what the device's float32 arithmetic may cost.  Sample origins, window lengths and per-frame constants
are float64 in both variants, as on the device."""
from __future__ import annotations

import math

import numpy as np
import scipy.fft

from tests import cheaptrick_ref as ct

FLOOR_F0 = 47.0
LOWEST_F0 = 40.0
INTERVAL = 3000.0
UPPER_LIMIT = 15000.0
SAFE = 1e-12
THRESHOLD = 0.85
COARSE_FLOOR = -200.0


def _pow2_above(v):
    return 2 ** (1 + int(math.floor(math.log2(v))))


def constants(fs):
    """N_d, N_l, bands, L (the Nuttall window's points) of a sample rate; ``ValueError`` where the kernel refuses."""
    if fs / 2.0 <= 7900.0:
        raise ValueError("D4C: the LoveTrain band (7900 Hz) does not fit below fs / 2")
    c = {"N_d": _pow2_above(4.0 * fs / FLOOR_F0 + 1.0), "N_l": _pow2_above(3.0 * fs / LOWEST_F0 + 1.0),
         "bands": int(min(UPPER_LIMIT, fs / 2.0 - INTERVAL) / INTERVAL)}
    c["L"] = 2 * int(INTERVAL * c["N_d"] / fs) + 1
    if c["N_d"] > 4096 or c["N_l"] > 4096 or c["bands"] > 5:
        raise ValueError("D4C: transform sizes above 4096 or more than 5 bands are not supported")
    return c


def matlab_round(v):
    return int(v + 0.5) if v > 0 else int(v - 0.5)


def nuttall(L, ft=np.float64):
    u = (np.arange(L).astype(ft) / ft(L - 1)).astype(ft)
    pi = ft(np.pi)
    return (ft(0.355768) - ft(0.487396) * np.cos(ft(2) * pi * u) + ft(0.144232) * np.cos(ft(4) * pi * u) -
            ft(0.012604) * np.cos(ft(6) * pi * u)).astype(ft)


def windowed(x, fs, f0, position, ratio, blackman, ft=np.float64):
    """WORLD's GetWindowedWaveform without its randn: (2 half + 1,) samples."""
    half = matlab_round(ratio * fs / f0 / 2.0)
    origin = matlab_round(position * fs + 0.001)
    i = np.arange(-half, half + 1)
    seg = np.asarray(x, dtype=ft)[np.clip(origin + i, 0, len(x) - 1)]
    a = (i.astype(ft) * ft(2.0 * f0 / (ratio * fs))).astype(ft)
    pi = ft(np.pi)
    if blackman:
        w = ft(0.08) * np.cos(ft(2) * pi * a) + ft(0.5) * np.cos(pi * a) + ft(0.42)
    else:
        w = ft(0.5) * np.cos(pi * a) + ft(0.5)
    w = w.astype(ft)
    xw = (seg * w).astype(ft)
    coef = np.sum(xw, dtype=ft) / np.sum(w, dtype=ft)
    return (xw - w * coef).astype(ft)


def _rfft(wave, n, fp32):
    if fp32:
        return scipy.fft.rfft(np.asarray(wave, dtype=np.float32), n)
    return np.fft.rfft(np.asarray(wave, dtype=np.float64), n)


def _power(X, ft):
    return (X.real.astype(ft) ** 2 + X.imag.astype(ft) ** 2).astype(ft)


def love_train(x, fs, F0, position, N_l, fp32=False):
    """a0 of a frame: the share of [100, 4000] Hz in [100, 7900] Hz; 0 where F0 <= 0 or the denominator is 0."""
    ft = np.float32 if fp32 else np.float64
    if not F0 > 0:
        return 0.0
    f0 = min(max(float(F0), LOWEST_F0), fs * (0.5 - 1.0 / N_l))
    wave = windowed(x, fs, f0, position, 3.0, True, ft)[:N_l]
    P = _power(_rfft(wave, N_l, fp32), ft)
    b0, b1, b2 = (int(math.ceil(v * N_l / fs)) for v in (100.0, 4000.0, 7900.0))
    P[:b0] = 0
    C = np.cumsum(P, dtype=ft)
    return float(C[b1] / C[b2]) if C[b2] > 0 else 0.0


def smooth(P, h, N):
    """Mean of P over [k + 1/2 - h, k + 1/2 + h) in cells (cell j holds P[mirror(j)] on [j, j + 1)) for k <= N / 2:
    ``cheaptrick_ref.smooth_interval`` at a half width of h bins."""
    ft = P.dtype.type
    H = N // 2
    h = ft(h)
    hi = int(math.floor(h))
    hf = ft(h - ft(hi))
    lo_down = hf > ft(0.5)
    ka_off = -hi - (1 if lo_down else 0)
    wa = ft(1.0) - (ft(1.5) - hf if lo_down else ft(0.5) - hf)
    up = hf >= ft(0.5)
    kb_off = hi + (1 if up else 0)
    wb = hf - ft(0.5) if up else ft(0.5) + hf
    k = np.arange(H + 1)
    if ka_off == kb_off:
        return (ft(2.0) * h * P[ct._mirror(k + ka_off, N)] / (ft(2.0) * h)).astype(ft)
    s = wa * P[ct._mirror(k + ka_off, N)]
    if kb_off - ka_off > 1:
        whole = k[:, None] + np.arange(ka_off + 1, kb_off)[None, :]
        s = s + np.sum(P[ct._mirror(whole, N)], axis=1, dtype=ft)
    s = s + wb * P[ct._mirror(k + kb_off, N)]
    return (s / (ft(2.0) * h)).astype(ft)


def centroid(x, fs, f0, position, N, fp32=False):
    ft = np.float32 if fp32 else np.float64
    w = windowed(x, fs, f0, position, 4.0, True, ft)[:N]
    ss = np.sum(w * w, dtype=ft)
    w = (w * (ft(1.0) / np.sqrt(ss))).astype(ft) if ss > 0 else np.zeros_like(w)
    X = _rfft(w, N, fp32)
    Y = _rfft((w * (np.arange(w.size) + 1).astype(ft)).astype(ft), N, fp32)
    return (X.real.astype(ft) * Y.real.astype(ft) + X.imag.astype(ft) * Y.imag.astype(ft)).astype(ft)


def smoothed_power(x, fs, f0, position, N, fp32=False):
    ft = np.float32 if fp32 else np.float64
    P = _power(_rfft(windowed(x, fs, f0, position, 4.0, False, ft)[:N], N, fp32), ft)
    P = ct.dc_correction(P, fs, f0, N)
    return smooth(P, f0 * N / (2.0 * fs), N)


def static_group_delay(x, fs, f0, position, N, fp32=False):
    """(group delay, smoothed power): the zero-power rule reads the second."""
    power = smoothed_power(x, fs, f0, position, N, fp32)
    cen = centroid(x, fs, f0, position - 0.25 / f0, N, fp32) + centroid(x, fs, f0, position + 0.25 / f0, N, fp32)
    cen = ct.dc_correction(cen, fs, f0, N)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = cen / power
    g = smooth(g, f0 * N / (4.0 * fs), N)
    return g - smooth(g, f0 * N / (2.0 * fs), N), power


def coarse_aperiodicity(g, fs, N, bands, L, fp32=False):
    """Per band: the Nuttall-windowed group delay's power spectrum, sorted ascending and summed; 10 log10 of
    S[N / 2 - round(8 N / L) - 1] / S[N / 2]."""
    ft = np.float32 if fp32 else np.float64
    win = nuttall(L, ft)
    hl = L // 2
    bw = matlab_round(8.0 * N / L)
    out = np.zeros(bands)
    for i in range(bands):
        centre = int(INTERVAL * (i + 1) * N / fs)
        seg = (g[centre - hl:centre + hl + 1].astype(ft) * win).astype(ft)
        S = np.cumsum(np.sort(_power(_rfft(seg, N, fp32), ft)), dtype=ft)
        if S[N // 2] > 0:
            with np.errstate(divide="ignore"):
                out[i] = max(float(ft(10.0) * np.log10(S[N // 2 - bw - 1] / S[N // 2])), COARSE_FLOOR)
    return out


def frame(x, fs, F0, position, threshold=THRESHOLD, fp32=False, c=None):
    """(a0, coarse (bands,), power_min): ``coarse`` is NaN for a frame with the unvoiced verdict; ``power_min`` is the
    smallest bin of the smoothed power where the band analysis ran (else NaN)."""
    c = constants(fs) if c is None else c
    ft = np.float32 if fp32 else np.float64
    nan = np.full(c["bands"], np.nan)
    a0 = love_train(x, fs, F0, position, c["N_l"], fp32)
    if not F0 > 0 or a0 <= ft(threshold):
        return a0, nan, np.nan
    N = c["N_d"]
    f0 = min(max(float(F0), FLOOR_F0), fs * (0.5 - 1.0 / N))
    g, power = static_group_delay(x, fs, f0, position, N, fp32)
    if not np.all(power > 0):
        return a0, nan, float(np.min(power))
    coarse = coarse_aperiodicity(g, fs, N, c["bands"], c["L"], fp32)
    rev = (ft(F0) - ft(100.0)) / ft(50.0)
    return a0, np.minimum(0.0, (coarse.astype(ft) + rev).astype(np.float64)), float(np.min(power))


def expand(coarse, fs, fft_size, fp32=False):
    """One frame's band values (NaN: unvoiced) at the fft_size / 2 + 1 bins: linear in dB between the knots."""
    ft = np.float32 if fp32 else np.float64
    bins = fft_size // 2 + 1
    if np.isnan(coarse[0]):
        return np.full(bins, ft(1.0 - SAFE), ft)
    bands = len(coarse)
    xs = np.concatenate([[0.0], INTERVAL * (np.arange(bands) + 1), [fs / 2.0]]).astype(ft)
    ys = np.concatenate([[-60.0], coarse, [-SAFE]]).astype(ft)
    fr = (np.arange(bins) * fs / fft_size).astype(ft)
    seg = np.minimum((fr / ft(INTERVAL)).astype(np.int64), bands)
    db = ((ys[seg + 1] - ys[seg]) / (xs[seg + 1] - xs[seg]) * (fr - xs[seg]) + ys[seg]).astype(ft)
    db = np.minimum(db, ft(0.0))                                 # no knot lies above 0: rounding alone would
    return np.power(ft(10.0), db / ft(20.0)).astype(ft)


def d4c(x, f0, fs, frame_period_ms=5.0, threshold=THRESHOLD, fft_size=None, fp32=False, first_frame=0, n_frames=None):
    """``(ap (frames, fft_size / 2 + 1), bands (frames, 1 + bands) = {a0, coarse}, power_min (frames,))``: frame f at
    f * frame_period_ms, ``f0`` float32-rounded as the device reads it."""
    c = constants(fs)
    fft_size = ct.default_fft_size(fs) if fft_size is None else int(fft_size)
    f0 = np.asarray(f0, dtype=np.float32).astype(np.float64).reshape(-1)
    n_frames = f0.size - first_frame if n_frames is None else n_frames
    ft = np.float32 if fp32 else np.float64
    ap = np.empty((n_frames, fft_size // 2 + 1), ft)
    band = np.empty((n_frames, 1 + c["bands"]))
    pmin = np.empty(n_frames)
    for q in range(n_frames):
        f = first_frame + q
        a0, coarse, pmin[q] = frame(x, fs, f0[f], f * (frame_period_ms / 1000.0), threshold, fp32, c)
        band[q, 0], band[q, 1:] = a0, coarse
        ap[q] = expand(coarse, fs, fft_size, fp32)
    return ap, band, pmin
