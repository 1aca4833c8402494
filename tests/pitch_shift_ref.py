"""float64 restatement of ``librosa.effects.pitch_shift`` (librosa 0.10 defaults, resampy 0.4 ``kaiser_best`` /
``kaiser_fast``) written from the published algorithm, for testing the HIP stages; parity with librosa itself is
unpinned.  ``fp32=True`` mimics librosa's own arithmetic on float32 input instead: a complex64 STFT and a
float32 running phase in the phase vocoder -- the yardstick for what finite precision costs on ill-conditioned bins."""
from __future__ import annotations

import numpy as np

from pitchextractor_amd.pitch_shift import (HOP, N_FFT, RES_TYPES, resample_filter, resample_ratio, stretch_rate,
                                            stretched_len, TABLE_PRECISION)

N_BINS = N_FFT // 2 + 1


def window():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)       # periodic Hann


def stft(y, fp32=False):
    """(frames, 1025): centre=True with zero padding of n_fft // 2, 1 + N // hop frames.  ``fp32``: the transform
    itself in float32 arithmetic (numpy's single-precision FFT), so bins far below the frame's rounding level carry
    rounding-noise phases as any float32 FFT gives them."""
    if fp32:
        y = np.asarray(y, dtype=np.float32)
        pad = np.zeros(y.shape[0] + N_FFT, np.float32)
        pad[N_FFT // 2:N_FFT // 2 + y.shape[0]] = y
        idx = np.arange(1 + y.shape[0] // HOP)[:, None] * HOP + np.arange(N_FFT)[None, :]
        return np.fft.rfft(pad[idx] * window().astype(np.float32)[None, :], axis=1).astype(np.complex64)
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    frames = 1 + n // HOP
    pad = np.zeros(n + N_FFT)
    pad[N_FFT // 2:N_FFT // 2 + n] = y
    idx = np.arange(frames)[:, None] * HOP + np.arange(N_FFT)[None, :]
    return np.fft.rfft(pad[idx] * window()[None, :], axis=1)


def phase_vocoder(D, rate, fp32=False):
    """librosa.phase_vocoder(D.T, rate, hop_length=512).T for D (frames, 1025)."""
    steps = np.arange(0, D.shape[0], rate, dtype=np.float64)
    Dp = np.concatenate([D, np.zeros((2, D.shape[1]), D.dtype)])
    adv = HOP * np.fft.rfftfreq(N_FFT, d=1.0 / (2 * np.pi))
    phase = np.angle(D[0])                                    # float32 for a complex64 spectrum
    out = np.zeros((steps.size, D.shape[1]), np.complex64 if fp32 else np.complex128)
    for t, s in enumerate(steps):
        i = int(s)
        a = np.mod(s, 1.0)
        c0, c1 = Dp[i], Dp[i + 1]
        mag = (1.0 - a) * np.abs(c0) + a * np.abs(c1)
        out[t] = mag * (np.cos(phase) + 1j * np.sin(phase))
        dp = np.angle(c1) - np.angle(c0) - adv
        dp = dp - 2.0 * np.pi * np.round(dp / (2.0 * np.pi))
        phase += adv + dp
    return out


def istft(S, length, fp32=False):
    """librosa.istft(S.T, hop 512, centre, length=length) for S (columns, 1025)."""
    dt = np.float32 if fp32 else np.float64
    n_frames = min(S.shape[0], int(np.ceil((length + N_FFT) / HOP)))
    w = window()
    fr = (np.fft.irfft(S[:n_frames], n=N_FFT, axis=1) * w[None, :]).astype(dt)
    total = N_FFT + HOP * (n_frames - 1)
    y = np.zeros(total, dt)
    wss = np.zeros(total, dt)
    for t in range(n_frames):
        y[t * HOP:t * HOP + N_FFT] += fr[t]
        wss[t * HOP:t * HOP + N_FFT] += (w * w).astype(dt)
    out = np.zeros(length, dt)
    ws = np.zeros(length, dt)
    body, wbody = y[N_FFT // 2:N_FFT // 2 + length], wss[N_FFT // 2:N_FFT // 2 + length]
    out[:body.size], ws[:wbody.size] = body, wbody
    nz = ws > np.finfo(dt).tiny
    out[nz] /= ws[nz]
    return out


def filter_tables(res_type, ratio):
    W = resample_filter(res_type)
    if ratio < 1:
        W = ratio * W
    return W, np.diff(W, append=W[-1])


def resample(x, ratio, res_type="kaiser_best"):
    """resampy.resample(x, sr_orig, sr_new) with sr_new / sr_orig = ratio: int(len(x) * ratio) samples.  At ratio 1
    the input comes back unfiltered, as librosa.resample returns it when orig_sr == target_sr (n_steps = 0)."""
    x = np.asarray(x, dtype=np.float64)
    if ratio == 1.0:
        return x.copy()
    W, dW = filter_tables(res_type, ratio)
    nwin = W.size
    scale = min(1.0, ratio)
    step = int(scale * TABLE_PRECISION)
    n_out = int(x.size * ratio)
    T = np.arange(n_out) / ratio
    n = T.astype(np.int64)
    y = np.zeros(n_out)
    frac = scale * (T - n)
    for sgn, fr, lim in ((-1, frac, n + 1), (1, scale - frac, x.size - n - 1)):
        idx = fr * TABLE_PRECISION
        off = idx.astype(np.int64)
        eta = idx - off
        cnt = np.minimum(lim, (nwin - off) // step)
        for a in range(int(cnt.max(initial=0))):
            m = a < cnt
            w = off[m] + a * step
            src = n[m] - a if sgn < 0 else n[m] + 1 + a
            y[m] += (W[w] + eta[m] * dW[w]) * x[src]
    return y


def resample_at(x, ratio, res_type, j):
    """``resample(x, ratio, res_type)[j]`` for an array of output indices ``j < int(len(x) * ratio)``, each output
    summed tap by tap on its own: for slices of rows too long to resample whole."""
    x = np.asarray(x, dtype=np.float64)
    j = np.asarray(j, dtype=np.int64)
    if ratio == 1.0:
        return x[j]
    W, dW = filter_tables(res_type, ratio)
    scale = min(1.0, ratio)
    step = int(scale * TABLE_PRECISION)
    y = np.zeros(j.size)
    for q, jj in enumerate(j):
        T = float(jj) / ratio
        n = int(T)
        frac = scale * (T - n)
        idx = frac * TABLE_PRECISION
        off = int(idx)
        a = np.arange(max(0, min(n + 1, (W.size - off) // step)))
        left = np.dot(W[off + a * step] + (idx - off) * dW[off + a * step], x[n - a])
        idx = (scale - frac) * TABLE_PRECISION
        off = int(idx)
        a = np.arange(max(0, min(x.size - n - 1, (W.size - off) // step)))
        y[q] = left + np.dot(W[off + a * step] + (idx - off) * dW[off + a * step], x[n + 1 + a])
    return y


# --------------------------------------------------------------------------- what the kernels read (plan coverage)
def resampler_reads(j, ratio, M, res_type):
    """(lo, hi): the stretched samples lo .. hi (inclusive; lo > hi: none) that ps_resample_kernel's two tap loops
    read for output indices ``j``, from the kernel's own off, step, i_max and k_max; the one sample j at ratio 1."""
    j = np.asarray(j, dtype=np.int64)
    if ratio == 1.0:
        return j.copy(), j.copy()
    nwin = RES_TYPES[res_type][0] * TABLE_PRECISION + 1
    scale = min(1.0, ratio)
    step = int(scale * TABLE_PRECISION)
    T = j.astype(np.float64) / ratio
    n = T.astype(np.int64)
    frac = scale * (T - n)
    off = (frac * TABLE_PRECISION).astype(np.int64)
    i_max = np.minimum(n + 1, (nwin - off) // step)
    off = ((scale - frac) * TABLE_PRECISION).astype(np.int64)
    k_max = np.minimum(M - n - 1, (nwin - off) // step)
    return n + 1 - np.maximum(i_max, 0), n + np.maximum(k_max, 0)


def ola_reads(s, n_ola):
    """(t_lo, t_hi): the frames t_lo .. t_hi (inclusive; t_lo > t_hi: none) that ps_ola_kernel sums into stretched
    samples ``s``."""
    p = np.asarray(s, dtype=np.int64) + N_FFT // 2
    t_lo = np.where(p < N_FFT, 0, (p - N_FFT) // HOP + 1)
    t_hi = np.minimum(n_ola - 1, p // HOP)
    past = p >= N_FFT + HOP * (n_ola - 1)
    return np.where(past, 1, t_lo), np.where(past, 0, t_hi)


def vocoder_last_frame(c_hi, rate):
    """The last input frame that output columns 0 .. c_hi - 1 of ps_vocoder_kernel read."""
    return int(float(c_hi - 1) * rate) + 1


# --------------------------------------------------------------------------- shared test signals
def three_sines(n, sr=24000):
    t = np.arange(n) / sr
    return sum(a * np.sin(2 * np.pi * f * t + p)
               for a, f, p in ((0.3, 180.0, 0.1), (0.2, 523.0, 1.0), (0.1, 1710.0, 2.0))).astype(np.float32)


def silence_then_signal(n_silent=8192, n_signal=12000):
    """Exact zeros, then the three-sine signal: the spectra of the first frames are digital silence."""
    return np.concatenate([np.zeros(n_silent, np.float32), three_sines(n_signal)])


SILENCE_FLOOR, SILENCE_WIDE_FLOOR = 1e-3, 1e-4              # masks of the silence tests, as shares of the largest bin


def loud_cells(want, floor):
    """(mask, onset, share) of a vocoder reference ``want`` (columns, bins): the cells whose magnitude exceeds
    ``floor`` of the largest, the first column that is not exact silence, and the share of the cells at and after
    that column which the mask keeps."""
    mag = np.abs(want)
    mask = mag > floor * mag.max()
    onset = int(np.argmax(mag.max(axis=1) > 0))
    return mask, onset, float(mask[onset:].mean())


def pitch_shift(y, sr, n_steps, res_type="kaiser_best", fp32=False):
    y = np.asarray(y)
    N = y.shape[0]
    rate = stretch_rate(n_steps)
    stretched = istft(phase_vocoder(stft(y, fp32), rate, fp32), stretched_len(N, n_steps), fp32)
    shifted = resample(stretched, resample_ratio(n_steps, sr), res_type)
    out = np.zeros(N)
    k = min(N, shifted.size)
    out[:k] = shifted[:k]
    return out.astype(np.float32) if fp32 else out
