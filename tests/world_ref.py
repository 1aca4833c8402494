"""float64 restatement of WORLD's ``Synthesis`` (what pyworld 0.3.x calls ``synthesize``), written from the published
algorithm for testing ``pitchextractor_amd.world`` and ``csrc/world_synth.hip``; parity with the pyworld binary is
unpinned.  Two stated deviations: pulse p's aperiodic noise is ``noise[index[p] : index[p] + noise_size]``
of a caller-given array of standard normals (WORLD draws from a process-global xorshift stream), and ``fp32=True``
does the per-pulse transforms, log / exp and sums in float32 / complex64 (``scipy.fft`` keeps single precision) -- the
yardstick for what the device's float32 arithmetic may cost.  The time base is float64 in both variants."""
from __future__ import annotations

import math

import numpy as np
import scipy.fft

VOWELS = {"ah": ((730.0, 90.0, 1.0), (1090.0, 110.0, 0.6), (2440.0, 150.0, 0.4)),
          "ih": ((390.0, 80.0, 1.0), (1990.0, 120.0, 0.6), (2550.0, 160.0, 0.4)),
          "uh": ((440.0, 70.0, 1.0), (1020.0, 90.0, 0.6), (2240.0, 150.0, 0.4))}
MIN_MARGIN = 1e-6           # rad: closest a phase sample may come to a wrap before rounding could move a pulse


def envelope(label, fs, fft_size):
    """The generator's formant template: a sum of Gaussians floored at 1e-3 (Utils/synthetic.py:122-147)."""
    freq = np.linspace(0, fs / 2, fft_size // 2 + 1)
    env = np.zeros_like(freq)
    for f, bw, amp in VOWELS[label]:
        env += amp * np.exp(-0.5 * ((freq - f) / (bw / 2.0)) ** 2)
    return np.maximum(env, 1e-3)


def output_length(n_frames, fs, frame_period_ms):
    return int(n_frames * frame_period_ms * fs / 1000)


def time_base(f0, fs, frame_period_ms, fft_size, check_margin=False):
    """(index, shift, vuv at the pulses, noise_size, smallest wrap margin).  The phase sum is a plain sequential
    float64 loop.  ``check_margin``: assert that no crossing has a phase sample within MIN_MARGIN of the wrap."""
    f0 = np.asarray(f0, dtype=np.float64)
    L = f0.shape[0]
    fp = frame_period_ms / 1000.0
    n = output_length(L, fs, frame_period_ms)
    lowest = fs / fft_size + 1.0
    cf0 = [x if x >= lowest else 0.0 for x in f0.tolist()]
    cvuv = [1.0 if x != 0.0 else 0.0 for x in cf0]
    cf0.append(2 * cf0[L - 1] - cf0[L - 2])
    cvuv.append(2 * cvuv[L - 1] - cvuv[L - 2])
    ct = [i * fp for i in range(L + 1)]
    t = np.array([i / fs for i in range(n)], dtype=np.float64)
    f0i = np.interp(t, ct, cf0)
    vuv = np.interp(t, ct, cvuv) > 0.5
    two_pi = 2 * math.pi
    wrap = np.empty(n)
    total = 0.0
    for i in range(n):
        total += two_pi * (f0i[i] if vuv[i] else 500.0) / fs
        wrap[i] = math.fmod(total, two_pi)
    index, shift = [], []
    margin = math.inf
    for i in range(n - 1):
        if abs(wrap[i + 1] - wrap[i]) > math.pi:
            y1, y2 = wrap[i] - two_pi, wrap[i + 1]
            index.append(i)
            shift.append((-y1 / (y2 - y1)) / fs)
            margin = min(margin, abs(y1), abs(y2))
    if check_margin:
        assert margin >= MIN_MARGIN, margin
    index = np.array(index, dtype=np.int64)
    P = index.size
    noise_size = np.array([index[min(P - 1, p + 1)] - index[p] for p in range(P)], dtype=np.int64)
    return index, np.array(shift), vuv[index], noise_size, margin


def _ffts(fp32):
    if fp32:
        c = lambda x: np.asarray(x, dtype=np.complex64)  # noqa: E731
        return (lambda x: scipy.fft.fft(c(x)), lambda x: scipy.fft.ifft(c(x)),
                lambda x: scipy.fft.rfft(np.asarray(x, dtype=np.float32)),
                lambda x, n: scipy.fft.irfft(c(x), n))
    return np.fft.fft, np.fft.ifft, np.fft.rfft, np.fft.irfft


def minphase(log_amp, fp32=False):
    """log_amp: N/2+1 half log-amplitudes -> the N/2+1 bins of the minimum-phase spectrum with that amplitude."""
    fft, ifft, _, _ = _ffts(fp32)
    half = log_amp.shape[0] - 1
    N = 2 * half
    full = np.concatenate([log_amp, log_amp[half - 1:0:-1]])
    c = np.real(ifft(full))
    c[1:half] *= 2
    c[half + 1:] = 0
    return np.exp(fft(c))[:half + 1]


def dc_remover(N):
    half = N // 2
    w = np.zeros(N)
    w[:half] = 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(half) + 1.0) / (1.0 + N))
    w[N - 1 - np.arange(half)] = w[:half]
    return w / (2 * w[:half].sum())


def _frames(table, pos, L):
    lo, hi = min(L - 1, int(math.floor(pos))), min(L - 1, int(math.ceil(pos)))
    frac = pos - math.floor(pos)
    if table.ndim == 1:
        return table
    return table[lo] if lo == hi else (1 - frac) * table[lo] + frac * table[hi]


def responses(n_frames, sp, ap, fs, frame_period_ms, index, shift, vuv, noise_size, noise, fp32=False):
    """(P, N) per-pulse responses, already divided by N.  sp / ap: (L, N/2+1) or one (N/2+1,) template; ap None is
    all zeros."""
    ft = np.float32 if fp32 else np.float64
    sp = np.abs(np.asarray(sp, dtype=ft))
    N = 2 * (sp.shape[-1] - 1)
    half = N // 2
    ap = np.zeros(sp.shape[-1], ft) if ap is None else np.asarray(ap, dtype=ft)
    ap2 = np.clip(ap, ft(0.001), ft(0.999999999999)) ** 2
    fp = frame_period_ms / 1000.0
    _, _, rfft, irfft = _ffts(fp32)
    dcr = dc_remover(N).astype(ft)
    k = np.arange(half + 1)
    out = np.zeros((len(index), N), ft)
    noise = np.asarray(noise, dtype=ft)
    for p in range(len(index)):
        pos = (index[p] / fs) / fp
        S, A = _frames(sp, pos, n_frames), _frames(ap2, pos, n_frames)
        voiced = bool(vuv[p])
        ns = int(noise_size[p])
        per = np.zeros(N, ft)
        if voiced and not A[0] > 0.999:
            H = minphase(np.log(S * (1 - A) + ft(1e-12)) / 2, fp32)
            ramp = np.exp(-1j * (2 * np.pi * (shift[p] * fs) / N * k))
            H = H * (ramp.astype(np.complex64) if fp32 else ramp)
            per = np.fft.fftshift(irfft(H, N) * N).astype(ft)
            dc = per[half:].sum(dtype=ft)
            per[:half] = 0
            per = per - dc * dcr
        z = np.zeros(N, ft)
        if ns > 0:
            seg = noise[index[p]:index[p] + ns]
            z[:ns] = seg - seg.mean(dtype=ft)
        Ha = minphase(np.log(S * A) / 2 if voiced else np.log(S) / 2, fp32)
        apd = np.fft.fftshift(irfft(Ha * rfft(z), N) * N).astype(ft)
        out[p] = (per * ft(math.sqrt(ns)) + apd) / N
    return out


def overlap_add(resp, index, n):
    N = resp.shape[1]
    y = np.zeros(n, resp.dtype)
    for p, i in enumerate(index):
        off = int(i) - N // 2 + 1
        lo, hi = max(0, -off), min(N, n - off)
        if hi > lo:
            y[off + lo:off + hi] += resp[p, lo:hi]
    return y


def synthesize(f0, sp, ap, fs, frame_period_ms, noise, fp32=False, table=None):
    """The waveform (float64, or float32 arithmetic with ``fp32``); ``table``: a ready (index, shift, vuv,
    noise_size) instead of this module's own time base."""
    f0 = np.asarray(f0, dtype=np.float64)
    sp = np.asarray(sp)
    N = 2 * (sp.shape[-1] - 1)
    index, shift, vuv, noise_size = (time_base(f0, fs, frame_period_ms, N)[:4] if table is None else table)
    resp = responses(f0.shape[0], sp, ap, fs, frame_period_ms, index, shift, vuv, noise_size, noise, fp32)
    return overlap_add(resp, index, output_length(f0.shape[0], fs, frame_period_ms))


# --------------------------------------------------------------------------- the rows the tests share
FS, HOP, FFT = 24000, 300, 1024
FRAME_PERIOD = 1000.0 * HOP / FS


def rows():
    """name -> (f0 (L,), sp (L, 513) or (513,), ap or None): curves whose every phase wrap keeps a margin of at
    least MIN_MARGIN, so that the pulse table does not hang on the last bit of the phase sum."""
    ah, ih = envelope("ah", FS, FFT), envelope("ih", FS, FFT)
    t = np.arange(40) * (FRAME_PERIOD / 1000.0)
    glide = np.linspace(110.0, 320.0, 40) * 2.0 ** (np.sin(2 * np.pi * 5.0 * t) * (0.4 / 12.0))
    w = np.linspace(0.0, 1.0, 24)[:, None]
    return {
        "two": (np.full(2, 97.3), ah, None),
        "glide_vib": (glide, ah, None),
        "hi": (np.full(30, 1093.0), ih, None),
        "morph": (np.full(24, 173.3), (1 - w) * ah[None, :] + w * ih[None, :], np.full((24, FFT // 2 + 1), 0.3)),
        "gap": (np.concatenate([np.full(12, 150.3), np.zeros(8), np.full(12, 233.1)]), ah, None),
    }
