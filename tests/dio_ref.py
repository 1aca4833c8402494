"""float64 numpy restatement of the DIO + StoneMask tracker (csrc/f0_dio.hip): WORLD's ``dio`` and ``stonemask`` with
pyworld's defaults (speed 1: no decimation), written from the published algorithm (Morise et al. 2009; WORLD).  pyworld
is not available to the tests: parity with its binary is unpinned and this file is the oracle.  ``dtype=np.float32``
runs every signal-path operation in float32 (host-side constants, frame times and sample positions stay float64, as on
the device); its deviation from the float64 run is the yardstick the kernels are held to.

Conventions fixed here (DESIGN.md "F0 tracking: DIO + StoneMask"):
 * ``round`` is half away from zero (WORLD's matlab_round);
 * frames = (int)(1000 n / sr / frame_period) + 1, t[i] = i * frame_period / 1000, also for n = 0 (one frame);
 * the band signal is the linear convolution of x - mean (zero outside the row) with the low-cut filter (centred) and
   the band's Nuttall window, read ``2 * half_average_length`` samples late: what WORLD's single zero-padded FFT gives.
   The float64 run convolves the whole row; the float32 run does overlap-save in blocks, as the device;
 * a fine edge is the integer i + 1 and the fraction x[i] / (x[i] - x[i + 1]) in (0, 1]; an interval's value is
   sr / (integer difference + fraction difference), its location (in samples, doubled) integer sum + fraction sum;
 * interpolation at a frame picks the segment k = clamp(#locations <= t, 1, intervals - 1) and extrapolates linearly
   from the end segments (WORLD's interp1 / histc);
 * "too few events": a band needs at least 3 intervals (4 edges) of every kind (WORLD: ``intervals - 2 > 0``);
 * the best band is the first one with the lowest score; a row of at most voice_range_minimum frames is all unvoiced;
 * StoneMask reads sample clamp(round((t + k / sr) sr) - 1, 0, n - 1) and evaluates the Blackman window at
   (round(..) - 1) / sr - t (WORLD's one-based index); the window half-length is computed in float64 from the
   contour's (float32 on the device) F0.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import scipy.fft

from tests import f0_track_ref as S

DEFAULTS = dict(f0_floor=71.0, f0_ceil=800.0, channels_in_octave=2.0, allowed_range=0.1)
NUTTALL = (0.355768, 0.487396, 0.144232, 0.012604)
REJECTED = 100000.0
KINDS = 4


def round_half_away(v: float) -> float:
    return -math.floor(-v + 0.5) if v < 0 else math.floor(v + 0.5)


class Consts:
    def __init__(self, sr, hop, **config):
        cfg = {**DEFAULTS, **{k: v for k, v in config.items() if k in DEFAULTS}}
        self.sr, self.hop = int(sr), int(hop)
        self.f0_floor, self.f0_ceil = float(cfg["f0_floor"]), float(cfg["f0_ceil"])
        self.channels, self.allowed = float(cfg["channels_in_octave"]), float(cfg["allowed_range"])
        self.frame_period = self.hop * 1000.0 / self.sr
        self.bands = 1 + int(math.log2(self.f0_ceil / self.f0_floor) * self.channels)
        self.boundary = [self.f0_floor * 2.0 ** ((b + 1) / self.channels) for b in range(self.bands)]
        self.half = [int(round_half_away(self.sr / bd / 2.0)) for bd in self.boundary]
        self.cut = int(round_half_away(self.sr / 50.0))
        self.vrm = int(0.5 + 1000.0 / self.frame_period / self.f0_floor) * 2 + 1
        self.taps = 2 * self.cut + 4 * self.half[0]
        self.nfft = 1024
        while self.nfft < 2 * self.taps:
            self.nfft *= 2
        self.step = self.nfft - self.taps + 1
        self.lead = self.cut + 2 * self.half[0] - 1


def frame_count(n, c: Consts) -> int:
    return int(1000.0 * n / c.sr / c.frame_period) + 1


def frame_times(n, c: Consts) -> np.ndarray:
    return np.arange(frame_count(n, c), dtype=np.float64) * c.frame_period / 1000.0


def low_cut_filter(c: Consts) -> np.ndarray:
    """2 cut + 1 taps centred on tap ``cut``: a negated, sum-normalised Hann shape plus a unit impulse."""
    N = 2 * c.cut + 1
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1, N + 1, dtype=np.float64) / (N + 1))
    f = -w / np.sum(w)
    f[c.cut] += 1.0
    return f


def nuttall(length: int) -> np.ndarray:
    t = np.arange(length, dtype=np.float64) / (length - 1.0)
    a = NUTTALL
    return a[0] - a[1] * np.cos(2 * np.pi * t) + a[2] * np.cos(4 * np.pi * t) - a[3] * np.cos(6 * np.pi * t)


def combined_filter(c: Consts, b: int) -> tuple[np.ndarray, int]:
    """(taps g, delay D): band[i] = sum_m g[m] y[i + D - m]."""
    return np.convolve(low_cut_filter(c), nuttall(4 * c.half[b])), 2 * c.half[b] + c.cut


def centred(x, dtype):
    x = np.asarray(x, np.float32)
    if x.size == 0:
        return x.astype(dtype)
    mean = np.sum(x.astype(np.float64)) / x.size
    return x.astype(np.float64) - mean if dtype == np.float64 else x - np.float32(mean)


def band_signals(x, c: Consts, dtype=np.float64) -> np.ndarray:
    """(bands, n)."""
    y = centred(x, dtype)
    n = y.size
    out = np.zeros((c.bands, n), dtype)
    if n == 0:
        return out
    if dtype == np.float64:
        for b in range(c.bands):
            g, D = combined_filter(c, b)
            L = scipy.fft.next_fast_len(n + g.size)
            full = scipy.fft.irfft(scipy.fft.rfft(y, L) * scipy.fft.rfft(g, L), L)
            out[b] = full[D:D + n]
        return out
    # float32: overlap-save in blocks of nfft with filter spectra built in float64, as on the device
    blocks = -(-n // c.step)
    pad = np.zeros(c.lead + blocks * c.step + c.nfft, np.float32)
    pad[c.lead:c.lead + n] = y
    idx = (np.arange(blocks) * c.step)[:, None] + np.arange(c.nfft)[None, :]
    spec = scipy.fft.rfft(pad[idx], axis=1)
    assert spec.dtype == np.complex64
    D0 = 2 * c.half[0] + c.cut
    for b in range(c.bands):
        g, D = combined_filter(c, b)
        gd = np.zeros(c.nfft)
        gd[D0 - D:D0 - D + g.size] = g
        G = np.fft.rfft(gd).astype(np.complex64)
        w = scipy.fft.irfft(spec * G[None, :], c.nfft, axis=1)
        assert w.dtype == np.float32
        out[b] = w[:, c.taps - 1:c.taps - 1 + c.step].reshape(-1)[:n]
    return out


def events(sig, dtype=np.float64):
    """Per band and kind (signal, negation, first difference, negated difference): (idx int64, frac dtype)."""
    out = []
    for y in np.asarray(sig, dtype):
        d = y[1:] - y[:-1]
        kinds = []
        for v in (y, -y, d, -d):
            if v.size < 2:
                kinds.append((np.zeros(0, np.int64), np.zeros(0, dtype)))
                continue
            a, b = v[:-1], v[1:]
            i = np.nonzero((0 < a) & (b <= 0))[0]
            kinds.append((i + 1, (a[i] / (a[i] - b[i])).astype(dtype)))
        out.append(kinds)
    return out


def interval_track(idx, frac, xs2, sr, dtype):
    """One interval track interpolated at the doubled sample positions xs2 (float64)."""
    dt = np.dtype(dtype).type
    fsum = (frac[:-1] + frac[1:]).astype(dtype)
    loc2 = (idx[:-1] + idx[1:]).astype(np.float64) + fsum.astype(np.float64)
    M = loc2.size
    k = np.clip(np.searchsorted(loc2, xs2, side="right"), 1, M - 1)
    a = k - 1
    i0, i1, i2 = idx[a], idx[a + 1], idx[a + 2]
    f0, f1, f2 = frac[a], frac[a + 1], frac[a + 2]
    va = dt(sr) / ((i1 - i0).astype(dtype) + (f1 - f0))
    vb = dt(sr) / ((i2 - i1).astype(dtype) + (f2 - f1))
    sa, sb = fsum[a], fsum[a + 1]
    num = (xs2 - (i0 + i1).astype(np.float64)) - sa.astype(np.float64)
    den = (i2 - i0).astype(np.float64) + (sb.astype(np.float64) - sa.astype(np.float64))
    s = num.astype(dtype) / den.astype(dtype)
    return (va + s * (vb - va)).astype(dtype)


def candidates(ev, n, c: Consts, dtype=np.float64):
    """dict(cand (bands, frames), score, best, best_band, raw_mean, raw_score)."""
    dt = np.dtype(dtype).type
    t = frame_times(n, c)
    xs2 = 2.0 * (t * float(c.sr))
    T = t.size
    cand, score = np.zeros((c.bands, T), dtype), np.full((c.bands, T), dt(REJECTED), dtype)
    raw_mean, raw_score = np.full((c.bands, T), np.nan), np.full((c.bands, T), np.nan)
    for b in range(c.bands):
        if any(idx.size < 4 for idx, _ in ev[b]):
            continue
        v = [interval_track(idx, frac, xs2, c.sr, dtype) for idx, frac in ev[b]]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            mean = (((v[0] + v[1]) + v[2]) + v[3]) / dt(4)
            d = [vk - mean for vk in v]
            spread = np.sqrt((((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]) / dt(3))
        bd = dt(np.float32(c.boundary[b])) if dtype == np.float32 else dt(c.boundary[b])
        out = (mean > bd) | (mean < bd / dt(2)) | (mean > dt(c.f0_ceil)) | (mean < dt(c.f0_floor)) | np.isnan(spread)
        cand[b] = np.where(out, dt(0), mean)
        score[b] = np.where(out, dt(REJECTED), spread)
        raw_mean[b], raw_score[b] = mean, spread
    best_band = np.argmin(score, axis=0) if T else np.zeros(0, np.int64)       # first lowest
    best = cand[best_band, np.arange(T)]
    return dict(cand=cand, score=score, best=best, best_band=best_band.astype(np.int32), raw_mean=raw_mean,
                raw_score=raw_score)


def select_best(current, past, cand_col, allowed, dt, margins=None):
    ref = (current * dt(3) - past) / dt(2)
    err = np.abs(ref - cand_col)
    j = int(np.argmin(err))                                               # first smallest
    best = cand_col[j]
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.abs(dt(1) - best / ref)
    if margins is not None:
        margins.append(abs(float(q) - float(allowed)))
    return dt(0) if q > allowed else best


def fix_contour(best, cand, c: Consts, dtype=np.float64, margins=None):
    """FixF0Contour: (step1, step2, step3, step4), each (frames,)."""
    dt = np.dtype(dtype).type
    best, cand = np.asarray(best, dtype), np.asarray(cand, dtype)
    T, vrm, ar = best.size, c.vrm, dt(c.allowed)
    z = np.zeros(T, dtype)
    if T <= vrm:
        return z, z.copy(), z.copy(), z.copy()
    base = np.zeros(T, dtype)
    base[vrm:T - vrm] = best[vrm:T - vrm]
    s1 = np.zeros(T, dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.abs((base[vrm:] - base[vrm - 1:-1]) / (dt(1e-12) + base[vrm:]))
    s1[vrm:] = np.where(q < ar, base[vrm:], dt(0))
    if margins is not None:
        live = base[vrm:] > 0
        margins.extend(np.abs(q[live].astype(np.float64) - float(ar)).tolist())
    centre = (vrm - 1) // 2
    s2 = s1.copy()
    zero = (s1 == 0).astype(np.int64)
    win = np.convolve(zero, np.ones(vrm, np.int64), mode="same")
    inner = np.zeros(T, bool)
    inner[centre:T - centre] = True
    s2[inner & (win > 0)] = 0
    s3 = s2.copy()
    for i in range(1, T):
        if not (s2[i] == 0 and s2[i - 1] != 0):
            continue
        for j in range(i - 1, T - 1):
            if j > i - 1 and s2[j + 1] == 0 and s2[j] != 0:
                break
            s3[j + 1] = select_best(s3[j], s3[j - 1], cand[:, j + 1], ar, dt, margins)
            if s3[j + 1] == 0:
                break
    s4 = s3.copy()
    for i in range(T - 1, 0, -1):
        if not (s2[i - 1] == 0 and s2[i] != 0):
            continue
        for j in range(i, 1, -1):
            if j < i and s2[j - 1] == 0 and s2[j] != 0:
                break
            s4[j - 1] = select_best(s4[j], s4[j + 1], cand[:, j - 1], ar, dt, margins)
            if s4[j - 1] == 0:
                break
    return s1, s2, s3, s4


def _fix_f0(main, diff, N, sr, f, harmonics, dt, discrete=None):
    num = den = dt(0)
    for h in range(harmonics):
        u = float(f) * N / float(sr) * (h + 1)
        idx = int(math.floor(u + 0.5))
        if discrete is not None:
            discrete.append(abs(u - math.floor(u) - 0.5) / u)
        m, d = main[idx], diff[idx]
        nm = m.real * d.imag - m.imag * d.real
        pw = m.real * m.real + m.imag * m.imag
        inst = dt(0) if pw == 0 else dt(idx) * dt(sr) / dt(N) + nm / pw * dt(sr) / dt(2) / dt(np.pi)
        amp = np.sqrt(pw)
        num = num + amp * inst
        den = den + amp * dt(h + 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return num / den


def stonemask(x, f0, c: Consts, dtype=np.float64, margins=None, discrete=None):
    dt = np.dtype(dtype).type
    x = np.asarray(x, np.float32).astype(dtype)
    f0 = np.asarray(f0, dtype)
    n, sr = x.size, c.sr
    out = np.zeros(f0.size, dtype)
    for i in np.nonzero(f0 > 0)[0]:
        f = f0[i]
        if f <= dt(40) or f > dt(sr) / dt(12) or n == 0:
            continue
        t = float(i) * c.frame_period / 1000.0
        half = int(1.5 * sr / float(f) + 1.0)
        if discrete is not None:
            v = 1.5 * sr / float(f) + 1.0
            discrete.append(min(v - math.floor(v), math.ceil(v) - v) / v)
        length = 2 * half + 1
        N = 2 ** (2 + int(math.floor(math.log2(length))))
        pos = (t + np.arange(-half, half + 1, dtype=np.float64) / sr) * sr
        raw = np.where(pos < 0, -np.floor(-pos + 0.5), np.floor(pos + 0.5))
        u = (((raw - 1.0) / sr - t) / (length / float(sr))).astype(dtype)
        w = dt(0.42) + dt(0.5) * np.cos(dt(2 * np.pi) * u) + dt(0.08) * np.cos(dt(4 * np.pi) * u)
        wp = np.concatenate([[dt(0)], w, [dt(0)]]).astype(dtype)
        dw = -(wp[2:] - wp[:-2]) / dt(2)
        seg = x[np.clip(raw.astype(np.int64) - 1, 0, n - 1)]
        main = scipy.fft.rfft(seg * w, N)
        diff = scipy.fft.rfft(seg * dw, N)
        r = dt(0)
        first = _fix_f0(main, diff, N, sr, f, 2, dt, discrete)
        if margins is not None and first > 0:
            margins.append(abs(float(first) / float(f) - 2.0))
        if first > 0 and not first > f * dt(2):
            nh = min(int(float(sr) / 2.0 / float(first)), 6)
            r = _fix_f0(main, diff, N, sr, first, nh, dt, discrete)
        if margins is not None:
            margins.append(abs(abs(float(r) - float(f)) / float(f) - 0.2))
        if not abs(r - f) <= f * dt(0.2):
            r = f
        out[i] = r
    return out


def track(y, sr, hop, dtype=np.float64, stonemask_on=True, **config):
    """Every stage of the tracker on one wave."""
    c = Consts(sr, hop, **config)
    y = np.asarray(y, np.float32)
    sig = band_signals(y, c, dtype)
    ev = events(sig, dtype)
    cd = candidates(ev, y.size, c, dtype)
    jumps, sm, disc = [], [], []
    steps = fix_contour(cd["best"], cd["cand"], c, dtype, jumps)
    dio = steps[3]
    refined = stonemask(y, dio.astype(np.float32), c, dtype, sm, disc) if stonemask_on else dio
    # range tests that decide the contour: the chosen band's, and any range-rejected candidate that would have won
    T = cd["best"].size
    rng = []
    for b in range(c.bands):
        m, s = cd["raw_mean"][b].astype(np.float64), cd["raw_score"][b].astype(np.float64)
        chosen = (cd["best_band"] == b) & (cd["score"][b] < REJECTED)
        rival = (cd["score"][b] >= REJECTED) & np.isfinite(s) & (s < cd["score"][cd["best_band"], np.arange(T)])
        for thr in (c.boundary[b], c.boundary[b] / 2.0, c.f0_ceil, c.f0_floor):
            with np.errstate(invalid="ignore"):
                rng.extend(np.abs(m[chosen | rival] / thr - 1.0).tolist())
    margin = dict(range=min(rng, default=np.inf), jump=min(jumps, default=np.inf), stonemask=min(sm, default=np.inf),
                  discrete=min(disc, default=np.inf))
    return dict(consts=c, bands=sig, events=ev, counts=np.array([[k[0].size for k in b] for b in ev], np.int32),
                cand=cd["cand"], score=cd["score"], best=cd["best"], best_band=cd["best_band"], steps=steps,
                dio=np.asarray(dio, np.float32), f0=np.asarray(refined, np.float32), times=frame_times(y.size, c),
                margin=margin)


# --------------------------------------------------------------------------- comparison helpers and test inputs
cents = S.cents
GPU_CONFIGS = [(16000, 160), (24000, 300), (48000, 480)]


def voiced_glide(seconds, f_a, f_b, sr, seed):
    """A glide voiced from its first to its last sample (no lead-in): StoneMask's index clamp runs at both ends."""
    return S.glide_signal(seconds, f_a, f_b, sr, seed=seed, lead=0.0)[0]


# Glides cross every band boundary, and a frame that lands within a cent of one is no margin input: the durations below
# were picked so that, on the float64 run, no deciding range test comes closer than 3e-3 (relative) to its threshold at
# this rate (tests/test_f0_dio_cpu.py asserts the condition itself).
_DOWN_GLIDE_SECONDS = {16000: 1.4, 24000: 1.75, 48000: 1.4}


def margin_inputs(sr):
    out = [voiced_glide(1.2, 75.0, 780.0, sr, 11), voiced_glide(_DOWN_GLIDE_SECONDS.get(sr, 1.4), 420.0, 95.0, sr, 12)]
    if sr == 48000:
        out.append(long_input(sr))
    return out


LONG_F0 = 640.0


def long_input(sr):
    """20 s: a float32 absolute event position would show here (0.06 samples at 10^6 are 14 cents at 640 Hz).  StoneMask
    picks its window length (int)(1.5 sr / f0 + 1) and its bins round(f N / sr h) from the DIO contour, so over 2000
    frames a contour that moves at all crosses one of those steps in some frame, where the float32 and the float64
    run then differ by a window, not by rounding.  The long row is therefore a steady tone whose steps are far away:
    ``margin["discrete"]`` (asserted against this row's own yardstick in tests/test_f0_dio_cpu.py)."""
    return S.glide_signal(20.0, LONG_F0, LONG_F0, sr, seed=8, lead=0.0)[0]


def vibrato_input(sr):
    """Vibrato with digital-silence gaps: the events inside the gaps are rounding noise, so no margin guarantee."""
    return S.vibrato_signal(2.0, 140.0, sr, seed=7, gaps=((0.35, 0.45), (0.7, 0.75)))[0]


def natural_inputs(sr):
    return [vibrato_input(sr)] + S.natural_inputs(sr)


def short_inputs(sr):
    return [np.zeros(0, np.float32), (0.1 * np.sin(np.arange(100) * 0.3)).astype(np.float32),
            np.full(int(0.5 * sr), 0.1, np.float32)]




def cast_events(ev, dtype):
    return [[(i, f.astype(dtype)) for i, f in kinds] for kinds in ev]


def stage_run(y, a, dtype=np.float32):
    """Every stage in ``dtype`` on the float64 result ``a`` of the stage before it, cast to ``dtype``: what the stage
    tests feed the device."""
    c = a["consts"]
    y = np.asarray(y, np.float32)
    ev = events(a["bands"].astype(dtype), dtype)
    cd = candidates(cast_events(a["events"], dtype), y.size, c, dtype)
    steps = fix_contour(a["best"].astype(dtype), a["cand"].astype(dtype), c, dtype)
    return dict(bands=band_signals(y, c, dtype), events=ev,
                counts=np.array([[k[0].size for k in b] for b in ev], np.int32), cand=cd["cand"], score=cd["score"],
                best=cd["best"], best_band=cd["best_band"], steps=steps,
                f0=stonemask(y, a["dio"], c, dtype).astype(np.float32))


def contour_deviation(fa, fb):
    """(largest cents over frames voiced on both sides, frames whose voicing differs)."""
    fa, fb = np.asarray(fa, np.float64), np.asarray(fb, np.float64)
    both = (fa > 0) & (fb > 0)
    return (float(np.max(cents(fa[both], fb[both]))) if both.any() else 0.0,
            int(np.count_nonzero((fa > 0) != (fb > 0))))


def stage_deviation(a, b):
    """Deviation of the stage outputs ``b`` (``stage_run`` or the device) from the float64 run ``a``."""
    peak = max(float(np.max(np.abs(a["bands"]))) if a["bands"].size else 0.0, 1e-30)
    band = float(np.max(np.abs(a["bands"].astype(np.float64) - b["bands"]))) / peak if a["bands"].size else 0.0
    same_counts = bool(np.array_equal(a["counts"], b["counts"]))
    edge = 0.0
    if same_counts:
        for ka, kb in zip(a["events"], b["events"]):
            for (ia, fa), (ib, fb) in zip(ka, kb):
                if ia.size:
                    edge = max(edge, float(np.max(np.abs((ia - ib) + (fa.astype(np.float64) - fb)))))
    both = (a["cand"] > 0) & (b["cand"] > 0)
    cand_c = float(np.max(cents(a["cand"][both], b["cand"][both]))) if both.any() else 0.0
    sc = np.abs(a["score"].astype(np.float64) - b["score"])[both]
    # frames whose best band differs, and how far apart the two bands' float64 candidates are there
    T = a["best"].size
    differ = np.nonzero(np.asarray(a["best_band"]) != np.asarray(b["best_band"]))[0]
    band_gap = 0.0
    for t in differ:
        fa, fb = float(a["cand"][a["best_band"][t], t]), float(a["cand"][b["best_band"][t], t])
        band_gap = max(band_gap, float(cents(fa, fb)) if fa > 0 and fb > 0 else (0.0 if fa == fb else np.inf))
    sm_c, sm_flips = contour_deviation(a["f0"], b["f0"])
    return dict(band=band, same_counts=same_counts, edge=edge, cand_cents=cand_c,
                score=float(sc.max()) if sc.size else 0.0,
                cand_flips=int(np.count_nonzero((a["cand"] > 0) != (b["cand"] > 0))), best_band_differs=int(differ.size),
                best_band_gap=band_gap, stonemask_cents=sm_c, stonemask_flips=sm_flips, frames=T)


def config_margin_inputs(sr, inputs=None):
    """The margin inputs of a configuration: the rate's own (``margin_inputs``), or with ``inputs`` one glide voiced
    from end to end per entry (seconds, from Hz, to Hz, seed)."""
    if inputs is None:
        return margin_inputs(sr)
    return [voiced_glide(seconds, f_a, f_b, sr, seed) for seconds, f_a, f_b, seed in inputs]


def _pairs(waves, sr, hop, stonemask_on, config):
    cfg = dict(config)
    return tuple((track(y, sr, hop, stonemask_on=stonemask_on, **cfg),
                  track(y, sr, hop, dtype=np.float32, stonemask_on=stonemask_on, **cfg)) for y in waves)


@functools.lru_cache(maxsize=None)
def reference_pairs(sr, hop, stonemask_on=True, config=(), inputs=None):
    """(float64 run, float32 run) of the whole tracker for every margin input of one configuration.  ``config``: keys
    of ``DEFAULTS`` as a tuple of (key, value) pairs; ``inputs``: see ``config_margin_inputs``."""
    return _pairs(config_margin_inputs(sr, inputs), sr, hop, stonemask_on, config)


@functools.lru_cache(maxsize=None)
def natural_pairs(sr, hop, stonemask_on=True, config=(), inputs=None):
    """The natural inputs belong to the default batches: a configuration with its own ``inputs`` has none."""
    return _pairs(natural_inputs(sr) if inputs is None else [], sr, hop, stonemask_on, config)


@functools.lru_cache(maxsize=None)
def stage_pairs(sr, hop, config=(), inputs=None):
    """(float64 run, float32 stage run) for every margin and then every natural input."""
    ys = config_margin_inputs(sr, inputs) + (natural_inputs(sr) if inputs is None else [])
    refs = [a for a, _ in reference_pairs(sr, hop, True, config, inputs)] + \
        [a for a, _ in natural_pairs(sr, hop, True, config, inputs)]
    return tuple((a, stage_run(y, a)) for y, a in zip(ys, refs))


@functools.lru_cache(maxsize=None)
def config_yardstick(sr, hop, config=(), inputs=None):
    """float32-vs-float64 deviation of the restatement on ONE configuration's own inputs.  Stage figures (band signal
    error relative to the row's peak, fine edge in samples, candidate cents and score, StoneMask cents) come from
    ``stage_run``; the contour figures (``dio_cents``, ``cents``, and ``natural_*``) from the whole float32 run."""
    n_margin = len(config_margin_inputs(sr, inputs))
    st = [stage_deviation(a, b) for a, b in stage_pairs(sr, hop, config, inputs)]
    full = [(contour_deviation(a["dio"], b["dio"]), contour_deviation(a["f0"], b["f0"]))
            for a, b in reference_pairs(sr, hop, True, config, inputs)]
    nat = [(contour_deviation(a["dio"], b["dio"]), contour_deviation(a["f0"], b["f0"]))
           for a, b in natural_pairs(sr, hop, True, config, inputs)]
    m = st[:n_margin]
    return dict(band=max(d["band"] for d in st), edge=max(d["edge"] for d in m),
                cand_cents=max(d["cand_cents"] for d in m), score=max(d["score"] for d in m),
                stonemask_cents=max(d["stonemask_cents"] for d in m),
                dio_cents=max(d[0][0] for d in full), cents=max(d[1][0] for d in full),
                natural_dio_cents=max((d[0][0] for d in nat), default=0.0),
                natural_cents=max((d[1][0] for d in nat), default=0.0),
                stage_dev=st, full_flips=[(d[0][1], d[1][1]) for d in full],
                natural_flips=[(d[0][1], d[1][1]) for d in nat])


# Configurations off the defaults: (name, sr, hop, config, margin glides (seconds, from Hz, to Hz, seed)).  What each
# reaches is said in DESIGN.md "F0 tracking: DIO + StoneMask".  As with ``_DOWN_GLIDE_SECONDS`` the durations were picked
# per configuration so that, on the float64 run, no deciding test lands on its threshold (tests/test_f0_dio_cpu.py
# asserts the condition itself); ``allowed_0.5`` glides fast enough for a frame-to-frame change between 0.1 and 0.5.
_UP, _DOWN = (75.0, 780.0, 11), (420.0, 95.0, 12)
CONFIG_CASES = [
    ("sr8000", 8000, 80, (), ((1.0,) + _UP, (1.35,) + _DOWN)),
    ("sr22050", 22050, 256, (), ((1.4,) + _UP, (1.2,) + _DOWN)),
    ("sr44100", 44100, 512, (), ((1.2,) + _UP, (0.9,) + _DOWN)),
    ("one_band", 16000, 160, (("f0_floor", 200.0), ("f0_ceil", 250.0)),
     ((0.95, 190.0, 260.0, 11), (0.95, 260.0, 190.0, 12))),
    ("sixteen_bands", 16000, 160, (("channels_in_octave", 4.5),), ((1.2,) + _UP, (0.9,) + _DOWN)),
    ("wide", 24000, 300, (("f0_floor", 50.0), ("f0_ceil", 1000.0), ("channels_in_octave", 3.0)),
     ((1.05, 55.0, 950.0, 11), (1.0, 900.0, 60.0, 12))),
    ("narrow", 16000, 128, (("f0_floor", 120.0), ("f0_ceil", 400.0)), ((0.9,) + _UP, (1.0,) + _DOWN)),
    ("allowed_0.02", 16000, 160, (("allowed_range", 0.02),), ((1.1,) + _UP, (1.25,) + _DOWN)),
    ("allowed_0.5", 16000, 160, (("allowed_range", 0.5),), ((0.45,) + _UP, (0.45, 780.0, 75.0, 12))),
]
CASE_IDS = [c[0] for c in CONFIG_CASES]


def is_margin_input(res64, yard):
    """Every thresholded quantity of the float64 run is at least 1000x its own yardstick (cents, as a frequency ratio)
    away from its threshold: the range tests and the allowed_range jumps are tests on candidates (``cand_cents``),
    the 20 % and 2x tests on StoneMask's output (``stonemask_cents``).  Section lengths are integers: they differ only
    where a voicing decision does."""
    ratio = lambda c: 1000.0 * (2.0 ** (c / 1200.0) - 1.0)  # noqa: E731
    m = res64["margin"]
    return m["range"] >= ratio(yard["cand_cents"]) and m["jump"] >= ratio(yard["cand_cents"]) and \
        m["stonemask"] >= ratio(yard["stonemask_cents"])
