"""float64 numpy restatement of the F0 tracker (csrc/f0_track.hip): Boersma's autocorrelation method as published
(IFA Proceedings 17, 1993) and as Praat's "Sound: To Pitch (ac)" applies it.  Written from the algorithm, not from
any implementation; parity with Praat's binary is unpinned.  ``dtype=np.float32`` runs every signal-path operation
in float32 (the host-side constants stay float64, as on the device): its deviation from the float64 run is the
yardstick the kernel is held to.

Steps (numbers as in DESIGN.md "F0 tracking"):
 1. constants of (sr, hop, config): ``Consts``;
 2. frame count / first centre: ``frame_layout`` (float64, in this order of operations);
 3. whole-file mean and peak; 4. per-frame r[lag]; 5. candidates; 6. path: ``track`` / ``viterbi``.

The fixtures at the end (``reference_pairs``, ``natural_pairs``, ``config_yardstick``) are cached per (sr, hop, min_pitch,
seconds of the long row) and, for the cases off the defaults (``CONFIG_CASES``), per configuration and input set.
"""
from __future__ import annotations

import functools
import math

import numpy as np

DEFAULTS = dict(min_pitch=40.0, max_pitch=1100.0, silence_threshold=0.03, voicing_threshold=0.45, octave_cost=0.01,
                octave_jump_cost=1.0, voiced_unvoiced_cost=0.3)
N_CAND = 15
DEPTH_FIRST, DEPTH_REFINE = 30, 70
REFINE_H = (0.25, 0.25, 0.125, 0.125)          # fixed-count search: one parabolic step of half-width h per entry
SILENT_RATIO = 2.0 ** -20


class Consts:
    def __init__(self, sr, hop, **config):
        cfg = {**DEFAULTS, **config}
        self.sr, self.hop = int(sr), int(hop)
        self.min_pitch = float(cfg["min_pitch"])
        self.ceiling = min(float(cfg["max_pitch"]), 0.5 * self.sr)
        self.silence = float(cfg["silence_threshold"])
        self.voicing = float(cfg["voicing_threshold"])
        self.octave_cost = float(cfg["octave_cost"])
        self.octave_jump_cost = float(cfg["octave_jump_cost"])
        self.vuv_cost = float(cfg["voiced_unvoiced_cost"])
        self.nw = 2 * (int(math.floor(3.0 * self.sr / self.min_pitch)) // 2 - 1)
        self.hw = self.nw // 2
        self.nper = int(math.floor(self.sr / self.min_pitch))
        self.hper = self.nper // 2 + 1
        self.nfft = 1
        while self.nfft < 1.5 * self.nw:
            self.nfft *= 2
        self.maxlag = min(self.nw // 3 + 2, self.hw)          # lags 2 .. maxlag - 1 are searched
        self.dt = self.hop / float(self.sr)
        self.c = 0.01 / self.dt
        i = np.arange(1, self.nw + 1, dtype=np.float64)
        self.window = 0.5 - 0.5 * np.cos(2.0 * np.pi * i / (self.nw + 1))
        spec = np.fft.rfft(self.window, self.nfft)
        ac = np.fft.irfft(spec.real ** 2 + spec.imag ** 2, self.nfft)
        self.window_r = ac[:self.hw + 1] / ac[0]


def frame_layout(n_samples, c: Consts):
    """(frames, t1): float64, in exactly this order."""
    duration = float(n_samples) / float(c.sr)
    span = duration - 3.0 / c.min_pitch
    q = span / c.dt
    n = int(math.floor(q)) + 1
    n = max(n, 0)
    a = duration / 2.0
    b = float(n) * c.dt
    t1 = (a - b / 2.0) + c.dt / 2.0
    return n, t1


def frame_left_samples(n_frames, t1, c: Consts):
    """0-based index of the sample left of each frame centre (samples sit at (i + 0.5) / sr)."""
    f = np.arange(n_frames, dtype=np.float64)
    t = t1 + f * c.dt
    return np.floor(t * float(c.sr) - 0.5).astype(np.int64), t


def sinc_interp(r, rows, x, depth, hw):
    """Praat's NUM_interpolate_sinc on the symmetric r (r[row, |lag|], |lag| <= hw) at positions x (one per entry of
    rows): ``depth`` taps on either side, raised-cosine taper reaching zero one sample beyond them."""
    dt = r.dtype.type
    x = np.asarray(x, dtype=r.dtype)
    fl = np.floor(x)
    il = fl.astype(np.int64)
    frac = x - fl
    dep = np.minimum(depth, hw - il)
    k = np.arange(depth, dtype=np.int64)[None, :]
    live = k < dep[:, None]
    kf = k.astype(r.dtype)
    sign = np.where(k % 2 == 1, dt(-1), dt(1))
    out = np.zeros(x.shape, dtype=r.dtype)
    for right in (False, True):
        fr = (dt(1) - frac) if right else frac
        s0 = np.sin(dt(np.pi) * fr)[:, None]                           # each side from its own distance
        d = fr[:, None] + kf
        big = (fr + dep.astype(r.dtype))[:, None]
        ix = np.abs(il[:, None] + 1 + k) if right else np.abs(il[:, None] - k)
        ix = np.minimum(ix, hw)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = sign * s0 / (dt(np.pi) * d) * (dt(0.5) + dt(0.5) * np.cos(dt(np.pi) * (d / big)))
        w = np.where(live, w, dt(0))
        out = out + np.sum(r[rows[:, None], ix] * w, axis=1, dtype=r.dtype)
    exact = (frac == 0) | (dep <= 0)
    return np.where(exact, r[rows, np.minimum(il, hw)], out).astype(r.dtype)


def frame_correlations(x, c: Consts, dtype=np.float64):
    """Steps 3-4: (r (frames, hw + 1), intensity, silent flags, local peak, global peak)."""
    dt = np.dtype(dtype).type
    x = np.asarray(x, dtype=np.float32)
    n_frames, t1 = frame_layout(x.size, c)
    if dtype == np.float64:
        xm = x.astype(np.float64) - np.mean(x.astype(np.float64)) if x.size else x.astype(np.float64)
    else:
        xm = x - np.float32(np.mean(x.astype(np.float64))) if x.size else x
    gpeak = dt(np.max(np.abs(xm))) if x.size else dt(0)
    if n_frames == 0:
        z = np.zeros((0,), dtype)
        return np.zeros((0, c.hw + 1), dtype), z, np.zeros((0,), bool), z, gpeak
    left, _ = frame_left_samples(n_frames, t1, c)
    right = left + 1
    start = right - c.hw
    assert start.min() >= 0 and start.max() + c.nw <= x.size, "a window leaves the file"
    idx = start[:, None] + np.arange(c.nw)[None, :]
    frames = xm[idx]                                                   # (frames, nw)
    lmean = np.mean(frames[:, c.hw - c.nper:c.hw + c.nper], axis=1, dtype=dtype)
    lpeak = np.max(np.abs(frames[:, c.hw - c.hper:c.hw + c.hper] - lmean[:, None]), axis=1)
    silent = (gpeak == 0) | (lpeak < dt(SILENT_RATIO) * gpeak)
    with np.errstate(divide="ignore", invalid="ignore"):
        intensity = np.where(gpeak > 0, np.minimum(dt(1), lpeak / gpeak), dt(0)).astype(dtype)
    w = ((frames - lmean[:, None]) * c.window.astype(dtype)[None, :]).astype(dtype)
    spec = np.fft.rfft(w, c.nfft, axis=1)
    power = (spec.real * spec.real + spec.imag * spec.imag).astype(dtype)
    ac = np.fft.irfft(power, c.nfft, axis=1).astype(dtype)[:, :c.hw + 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = ac / (ac[:, :1] * c.window_r.astype(dtype)[None, :])
    r[:, 0] = 1
    r[silent] = 0
    return r.astype(dtype), intensity, silent, lpeak, gpeak


def candidates(x, c: Consts, dtype=np.float64, return_r=False):
    """Step 5: (cand_f (frames, 15), cand_s (frames, 15), cand_n (frames,)); voiced candidates in lag order."""
    dt = np.dtype(dtype).type
    r, intensity, silent, lpeak, gpeak = frame_correlations(x, c, dtype)
    T = r.shape[0]
    cand_f = np.zeros((T, N_CAND), dtype)
    cand_s = np.zeros((T, N_CAND), dtype)
    cand_n = np.ones((T,), np.int32)
    cand_s[:, 0] = dt(c.voicing) + np.maximum(dt(0), dt(2) - intensity / (dt(c.silence) / (dt(1) + dt(c.voicing))))
    info = dict(r=r, silent=silent, gap15=np.inf, thr_gap=np.inf, n_maxima=np.zeros((T,), np.int64))
    if T == 0:
        return (cand_f, cand_s, cand_n, info) if return_r else (cand_f, cand_s, cand_n)
    lags = np.arange(2, c.maxlag)
    mid, lo, hi = r[:, lags], r[:, lags - 1], r[:, lags + 1]
    is_max = (mid > dt(0.5) * dt(c.voicing)) & (mid > lo) & (mid >= hi) & ~silent[:, None]
    # distance of any local maximum of r from the candidate threshold (margin condition b)
    shape_max = (mid > lo) & (mid >= hi) & ~silent[:, None]
    if shape_max.any():
        info["thr_gap"] = float(np.min(np.abs(mid[shape_max].astype(np.float64) - 0.5 * c.voicing)))
    rows, cols = np.nonzero(is_max)                                    # row-major: lag order within a frame
    if rows.size:
        i = lags[cols]
        a, b, cc = r[rows, i - 1], r[rows, i], r[rows, i + 1]
        dr = dt(0.5) * (cc - a)
        d2r = (dt(2) * b - a) - cc
        x0 = i.astype(dtype) + dr / d2r
        s = sinc_interp(r, rows, x0, DEPTH_FIRST, c.hw)
        s = np.where(s > 1, dt(1) / s, s)
        score = s - dt(c.octave_cost) * np.log2(dt(c.min_pitch) / (dt(c.sr) / x0))
        keep = np.ones(rows.size, bool)
        counts = np.bincount(rows, minlength=T)
        info["n_maxima"] = counts                                      # local maxima above the threshold, per frame
        for t in np.nonzero(counts > N_CAND - 1)[0]:
            sel = np.nonzero(rows == t)[0]
            order = sorted(sel, key=lambda m: (-score[m], m))
            keep[order[N_CAND - 1:]] = False
            info["gap15"] = min(info["gap15"], float(score[order[N_CAND - 2]]) - float(score[order[N_CAND - 1]]))
        rows, i, xx = rows[keep], i[keep], x0[keep].astype(dtype)
        lo_x, hi_x = (i - 1).astype(dtype), (i + 1).astype(dtype)
        for h in REFINE_H:
            h = dt(h)
            ym = sinc_interp(r, rows, xx - h, DEPTH_REFINE, c.hw)
            y0 = sinc_interp(r, rows, xx, DEPTH_REFINE, c.hw)
            yp = sinc_interp(r, rows, xx + h, DEPTH_REFINE, c.hw)
            den = (dt(2) * y0 - ym) - yp
            with np.errstate(divide="ignore", invalid="ignore"):
                step = xx + dt(0.5) * h * (yp - ym) / den
            xx = np.where(den > 0, np.minimum(np.maximum(step, lo_x), hi_x), xx).astype(dtype)
        s = sinc_interp(r, rows, xx, DEPTH_REFINE, c.hw)
        s = np.where(s > 1, dt(1) / s, s)
        slot = np.zeros(rows.size, np.int64)
        first = np.r_[True, rows[1:] != rows[:-1]]
        pos = np.arange(rows.size)
        slot = pos - np.maximum.accumulate(np.where(first, pos, 0)) + 1
        cand_f[rows, slot] = dt(c.sr) / xx
        cand_s[rows, slot] = s
        cand_n = (1 + np.bincount(rows, minlength=T)).astype(np.int32)
    return (cand_f, cand_s, cand_n, info) if return_r else (cand_f, cand_s, cand_n)


def _local_and_voiced(cand_f, cand_s, cand_n, c: Consts):
    T = cand_f.shape[0]
    f = cand_f.astype(np.float64)
    s = cand_s.astype(np.float64)
    valid = np.arange(N_CAND)[None, :] < np.asarray(cand_n)[:, None]
    voiced = valid & (f > 0) & (f < c.ceiling)
    with np.errstate(divide="ignore", invalid="ignore"):
        local = np.where(voiced, s - c.octave_cost * np.log2(c.ceiling / np.where(voiced, f, 1.0)), s)
    local = np.where(valid, local, -np.inf)
    lf = np.where(voiced, np.log2(np.where(voiced, f, 1.0)), 0.0)
    assert local.shape == (T, N_CAND)
    return local, voiced, lf


def _transition(voiced_a, lf_a, voiced_b, lf_b, c: Consts):
    """cost[i, j] of going from candidate i (frame t - 1) to candidate j (frame t)."""
    both = voiced_a[:, None] & voiced_b[None, :]
    change = voiced_a[:, None] != voiced_b[None, :]
    return np.where(both, c.octave_jump_cost * c.c * np.abs(lf_a[:, None] - lf_b[None, :]),
                    np.where(change, c.vuv_cost * c.c, 0.0))


def viterbi(cand_f, cand_s, cand_n, c: Consts, return_margin=False):
    """Step 6 in float64: (path indices, f0).  With ``return_margin`` also the smallest amount by which the best
    path beats the best path forced through any other candidate of any single frame (max-marginals)."""
    T = cand_f.shape[0]
    if T == 0:
        out = (np.zeros((0,), np.int64), np.zeros((0,), np.float64))
        return out + (np.inf,) if return_margin else out
    local, voiced, lf = _local_and_voiced(cand_f, cand_s, cand_n, c)
    alpha = np.full((T, N_CAND), -np.inf)
    bp = np.zeros((T, N_CAND), np.int64)
    alpha[0] = local[0]
    for t in range(1, T):
        tot = alpha[t - 1][:, None] - _transition(voiced[t - 1], lf[t - 1], voiced[t], lf[t], c)
        bp[t] = np.argmax(tot, axis=0)                                 # first maximum = lowest index
        alpha[t] = tot[bp[t], np.arange(N_CAND)] + local[t]
    path = np.zeros((T,), np.int64)
    path[-1] = int(np.argmax(alpha[-1]))
    for t in range(T - 1, 0, -1):
        path[t - 1] = bp[t, path[t]]
    f = cand_f.astype(np.float64)[np.arange(T), path]
    f0 = np.where((f > 0) & (f < c.ceiling), f, 0.0)
    if not return_margin:
        return path, f0
    beta = np.zeros((T, N_CAND))
    for t in range(T - 2, -1, -1):
        tot = (beta[t + 1] + local[t + 1])[None, :] - _transition(voiced[t], lf[t], voiced[t + 1], lf[t + 1], c)
        beta[t] = np.max(tot, axis=1)
    marg = alpha + beta
    best = marg[np.arange(T), path]
    others = marg.copy()
    others[np.arange(T), path] = -np.inf
    gap = best - np.max(others, axis=1)
    gap = gap[np.isfinite(gap)]
    return path, f0, (float(gap.min()) if gap.size else np.inf)


def track(x, sr, hop, dtype=np.float64, **config):
    """The whole tracker on one wave: dict(f0, cand_f, cand_s, cand_n, path, times)."""
    c = Consts(sr, hop, **config)
    cand_f, cand_s, cand_n, info = candidates(x, c, dtype, return_r=True)
    path, f0, margin = viterbi(cand_f, cand_s, cand_n, c, return_margin=True)
    n, t1 = frame_layout(np.asarray(x).size, c)
    # relative distance of any candidate frequency from the ceiling (margin condition d): a candidate on the ceiling is
    # voiced or voiceless with the last bit, which moves its local score and every transition to it
    live = (np.arange(N_CAND)[None, :] < cand_n[:, None]) & (np.arange(N_CAND)[None, :] > 0)
    ceil_gap = float(np.min(np.abs(cand_f.astype(np.float64)[live] / c.ceiling - 1.0))) if live.any() else np.inf
    return dict(f0=f0.astype(np.float32), cand_f=cand_f, cand_s=cand_s, cand_n=cand_n, path=path,
                times=t1 + np.arange(n) * c.dt, margin=margin, consts=c, silent=info["silent"],
                gap15=info["gap15"], thr_gap=info["thr_gap"], ceil_gap=ceil_gap, r=info["r"], n_maxima=info["n_maxima"])


# --------------------------------------------------------------------------- comparison helpers
def cents(a, b):
    return 1200.0 * np.abs(np.log2(np.asarray(a, np.float64) / np.asarray(b, np.float64)))


def match_candidates(fa, sa, na, fb, sb, nb):
    """Candidate sets of one frame matched by frequency: (matched?, max cents, max strength difference)."""
    if na != nb:
        return False, np.inf, np.inf
    ds = abs(float(sa[0]) - float(sb[0]))
    if na == 1:
        return True, 0.0, ds
    ia, ib = np.argsort(fa[1:na]), np.argsort(fb[1:nb])
    a_f, b_f = np.asarray(fa[1:na], np.float64)[ia], np.asarray(fb[1:nb], np.float64)[ib]
    a_s, b_s = np.asarray(sa[1:na], np.float64)[ia], np.asarray(sb[1:nb], np.float64)[ib]
    return True, float(np.max(cents(a_f, b_f))), max(ds, float(np.max(np.abs(a_s - b_s))))


def deviation(res_a, res_b):
    """Largest candidate deviation between two runs: dict(cents, strength, set_mismatches, voicing_flips,
    contour_cents)."""
    T = res_a["cand_n"].shape[0]
    worst_c = worst_s = 0.0
    mism = 0
    for t in range(T):
        ok, dc, ds = match_candidates(res_a["cand_f"][t], res_a["cand_s"][t], int(res_a["cand_n"][t]),
                                      res_b["cand_f"][t], res_b["cand_s"][t], int(res_b["cand_n"][t]))
        if not ok:
            mism += 1
            continue
        worst_c, worst_s = max(worst_c, dc), max(worst_s, ds)
    fa, fb = np.asarray(res_a["f0"], np.float64), np.asarray(res_b["f0"], np.float64)
    flips = int(np.count_nonzero((fa > 0) != (fb > 0)))
    both = (fa > 0) & (fb > 0)
    cc = float(np.max(cents(fa[both], fb[both]))) if both.any() else 0.0
    return dict(cents=worst_c, strength=worst_s, set_mismatches=mism, voicing_flips=flips, contour_cents=cc, frames=T)


SAME_MAXIMUM_CENTS = 1.0


def set_deviation(res_a, res_b):
    """The selected candidate sets of two runs, frame by frame.  Two candidates are the same maximum of r when they lie
    within ``SAME_MAXIMUM_CENTS``: maxima of one frame are at least 2 lags apart, which at the longest lag searched
    (1201 samples at 48 kHz, min_pitch 40) is 2.9 cents, while a maximum moves by 1e-2 cents between float32 and
    float64.  The cent is argued from the lag grid alone, not fitted to a kernel.  dict(mismatches: frames whose counts differ or that hold a different maximum; cents / strength: largest
    deviation over the other frames)."""
    T = res_a["cand_n"].shape[0]
    mism, worst_c, worst_s = 0, 0.0, 0.0
    for t in range(T):
        ok, dc, ds = match_candidates(res_a["cand_f"][t], res_a["cand_s"][t], int(res_a["cand_n"][t]),
                                      res_b["cand_f"][t], res_b["cand_s"][t], int(res_b["cand_n"][t]))
        if not ok or dc > SAME_MAXIMUM_CENTS:
            mism += 1
            continue
        worst_c, worst_s = max(worst_c, dc), max(worst_s, ds)
    return dict(mismatches=mism, cents=worst_c, strength=worst_s, frames=T)


# --------------------------------------------------------------------------- test signals (shared by CPU and GPU tests)
def harmonic(f0_curve, sr, partials=(1.0, 0.5, 0.25), amplitude=0.5):
    """Sum of partials following ``f0_curve`` (Hz per sample), float32."""
    phase = np.cumsum(2.0 * np.pi * np.asarray(f0_curve, np.float64) / float(sr))
    y = sum(a * np.sin((k + 1) * phase) for k, a in enumerate(partials))
    return (amplitude * y / sum(abs(a) for a in partials)).astype(np.float32)


def glide_signal(seconds, f_a, f_b, sr, seed=0, lead=0.25, noise=1e-3, partials=(1.0, 0.5, 0.25)):
    """Near-silent lead-in, then a three-partial linear glide over a noise floor: (audio, f0 per sample, 0 in the
    lead-in)."""
    rng = np.random.default_rng(seed)
    n, n0 = int(seconds * sr), int(lead * sr)
    curve = np.zeros(n)
    curve[n0:] = np.linspace(f_a, f_b, n - n0)
    y = np.zeros(n, np.float32)
    y[n0:] = harmonic(curve[n0:], sr, partials)
    y += (noise * rng.standard_normal(n)).astype(np.float32)
    return y.astype(np.float32), curve


def vibrato_signal(seconds, f_centre, sr, seed=0, rate=5.5, depth_cents=60.0, gaps=((0.35, 0.45),), noise=1e-3):
    """Three-partial tone with a sinusoidal vibrato around a slow glide, digital-silence gaps (fractions of the
    length) and a noise floor outside them: (audio, f0 per sample with 0 in the gaps)."""
    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    t = np.arange(n) / float(sr)
    drift = np.linspace(0.0, 300.0, n)                                  # cents over the whole signal
    curve = f_centre * 2.0 ** ((drift + depth_cents * np.sin(2 * np.pi * rate * t)) / 1200.0)
    y = harmonic(curve, sr) + (noise * rng.standard_normal(n)).astype(np.float32)
    curve = curve.copy()
    for a, b in gaps:
        y[int(a * n):int(b * n)] = 0.0
        curve[int(a * n):int(b * n)] = 0.0
    return y.astype(np.float32), curve


def margin_inputs(sr, long_seconds=8.0):
    """The "margin" inputs of the GPU test at rate sr: signals whose float64 path is decided by a wide margin
    (asserted in the CPU test); the last one is ``long_seconds`` long."""
    specs = [(0.9, 80.0, 380.0), (2.0, 300.0, 120.0), (1.3, 200.0, 800.0)]
    out = [glide_signal(s, a, b, sr, seed=k)[0] for k, (s, a, b) in enumerate(specs)]
    out.append(vibrato_signal(long_seconds, 140.0, sr, seed=7, gaps=((0.35, 0.40), (0.7, 0.72)))[0])
    return out


def natural_inputs(sr):
    """Noise bursts and an onset in noise: inputs without a margin guarantee."""
    rng = np.random.default_rng(99)
    n = int(1.5 * sr)
    y = (0.02 * rng.standard_normal(n)).astype(np.float32)
    a, b = int(0.5 * sr), int(1.1 * sr)
    y[a:b] += harmonic(np.full(b - a, 180.0), sr)
    burst = (0.3 * rng.standard_normal(n)).astype(np.float32) * (np.arange(n) % (sr // 4) < sr // 16)
    tone, _ = glide_signal(1.5, 150.0, 250.0, sr, seed=5, noise=0.02)
    return [y, (tone + 0.2 * burst).astype(np.float32)]


# configurations of the GPU test: (sr, hop, min_pitch, seconds of the long margin input) -> FFT 2048 / 4096 / 8192 /
# 2048 / 1024
GPU_CONFIGS = [(16000, 160, 40.0, 8.0), (24000, 300, 40.0, 30.0), (48000, 480, 40.0, 8.0), (24000, 300, 75.0, 8.0),
               (16000, 160, 75.0, 8.0)]
SPILL_CONFIG = (16000, 80, 75.0, 30.0)                                # 6000 frames: back-pointers leave LDS


def yardstick(margin_results):
    """Largest float32-vs-float64 deviation of the restatement over (float64, float32) result pairs: (cents,
    strength, per-pair deviations)."""
    dev = [deviation(a, b) for a, b in margin_results]
    return max(d["cents"] for d in dev), max(d["strength"] for d in dev), dev


def is_margin_input(res64, strength_yardstick, cents_yardstick=None):
    """Conditions (a)-(c) of a margin input, on the float64 result; with ``cents_yardstick`` also (d): no candidate
    frequency of any frame within 1000x that yardstick (cents, as a frequency ratio) of the ceiling."""
    bound = 1000.0 * strength_yardstick
    ok = res64["margin"] >= bound and res64["thr_gap"] > bound and res64["gap15"] > bound
    if cents_yardstick is not None:
        ok = ok and res64["ceil_gap"] >= 1000.0 * (2.0 ** (cents_yardstick / 1200.0) - 1.0)
    return ok


def config_margin_inputs(sr, hop, min_pitch, long_seconds, inputs=None):
    """Margin inputs of one test configuration.  The spill configuration's small hop scales every transition cost up
    (c = 0.01 / time_step), which leaves the 0.9-s glide a path margin of only 2x the bound: it is left out there.
    ``inputs`` names an input set of the configuration cases (``CASE_INPUTS``) instead."""
    if inputs is not None:
        return CASE_INPUTS[inputs](sr)[0]
    waves = margin_inputs(sr, long_seconds)
    return waves[1:] if (sr, hop, min_pitch, long_seconds) == SPILL_CONFIG else waves


def _pairs(waves, sr, hop, min_pitch, config):
    cfg = dict(config, min_pitch=min_pitch)
    return tuple((track(y, sr, hop, **cfg), track(y, sr, hop, dtype=np.float32, **cfg)) for y in waves)


@functools.lru_cache(maxsize=None)
def reference_pairs(sr, hop, min_pitch, long_seconds, config=(), inputs=None):
    """(float64 result, float32 result) of the restatement for every margin input of one configuration.  ``config``:
    further keys of ``DEFAULTS`` as a tuple of (key, value) pairs."""
    return _pairs(config_margin_inputs(sr, hop, min_pitch, long_seconds, inputs), sr, hop, min_pitch, config)


@functools.lru_cache(maxsize=None)
def natural_pairs(sr, hop, min_pitch, config=(), inputs=None):
    return _pairs(natural_inputs(sr) if inputs is None else CASE_INPUTS[inputs](sr)[1], sr, hop, min_pitch, config)


@functools.lru_cache(maxsize=None)
def config_yardstick(sr, hop, min_pitch, long_seconds, config=(), inputs=None):
    """The yardsticks of ONE configuration: the deviation of the float32 run of the restatement from its float64 run
    on that configuration's own inputs, for exactly the quantities the GPU test asserts there.  ``cents`` / ``strength``:
    candidates of the margin inputs (also the bound of their contours, which are candidates); ``natural_cents``: the
    contour of the natural inputs (their weak candidates are not compared)."""
    margin = reference_pairs(sr, hop, min_pitch, long_seconds, config, inputs)
    cents_m, strength_m, _ = yardstick(margin) if margin else (0.0, 0.0, [])
    nat_pairs = natural_pairs(sr, hop, min_pitch, config, inputs)
    nat = [deviation(a, b)["contour_cents"] for a, b in nat_pairs]
    out = dict(cents=cents_m, strength=strength_m, natural_cents=max(nat, default=0.0))
    if inputs is not None:                                             # the selected sets of the natural rows
        sets = [set_deviation(a, b) for a, b in nat_pairs]
        out.update(natural_set_cents=max((d["cents"] for d in sets), default=0.0),
                   natural_set_strength=max((d["strength"] for d in sets), default=0.0))
    return out


# --------------------------------------------------------------------------- configurations off the defaults
def stepped_signal(segments, sr, gap=0.06, lead=0.05):
    """Steady three-partial tones (seconds, Hz, amplitude), each followed by ``gap`` seconds of digital silence (longer
    than a window at min_pitch 75, so no frame sees two tones) and no noise floor: every frame's maxima of r are those
    of one steady tone, which keeps them away from a threshold or a ceiling that a glide would sweep across."""
    parts = [np.zeros(int(lead * sr), np.float32)]
    for seconds, hz, amplitude in segments:
        parts.append(harmonic(np.full(int(seconds * sr), float(hz)), sr, amplitude=amplitude))
        parts.append(np.zeros(int(gap * sr), np.float32))
    return np.concatenate(parts).astype(np.float32)


def white_noise(seconds, sr, seed, amplitude=0.3):
    return (amplitude * np.random.default_rng(seed).standard_normal(int(seconds * sr))).astype(np.float32)


def weak_burst_signal(sr, seed=1, sigma=0.12):
    """Digital silence, 0.12 s of a 400 Hz tone in white noise (strength near 0.6), silence, a clean 150 Hz tone.  Under
    costs_a the burst gains more over its unvoiced candidate than two voicing changes cost at 0.14 and less than they
    would at 0.35, so the path says which factor the change was charged with."""
    rng = np.random.default_rng(seed)
    n = int(0.12 * sr)
    burst = harmonic(np.full(n, 400.0), sr, amplitude=0.3) + (sigma * rng.standard_normal(n)).astype(np.float32)
    z = lambda seconds: np.zeros(int(seconds * sr), np.float32)  # noqa: E731
    return np.concatenate([z(0.1), burst, z(0.1), harmonic(np.full(int(0.3 * sr), 150.0), sr), z(0.06)]).astype(np.float32)


def weak_fundamental_bursts(sr, hz=200.0, seconds=0.1):
    """Two 0.1-s bursts of a 200 Hz tone whose second partial dominates (0.2, 1, 0, 0.5), then a clean 150 Hz tone, all
    between digital silence.  Under max_pitch 300 the strongest maximum of a burst, 400 Hz, counts as voiceless, so the
    path enters and leaves it for nothing, while the slightly stronger 200 Hz candidate would pay two voicing changes:
    the burst comes out unvoiced.  A path that forgets the ceiling pays the changes either way and comes out at 200 Hz."""
    z = lambda s: np.zeros(int(s * sr), np.float32)  # noqa: E731
    burst = harmonic(np.full(int(seconds * sr), hz), sr, partials=(0.2, 1.0, 0.0, 0.5))
    return np.concatenate([z(0.1), burst, z(0.1), burst, z(0.1), harmonic(np.full(int(0.3 * sr), 150.0), sr),
                           z(0.06)]).astype(np.float32)


_GLIDES = ((0.9, 80.0, 380.0, 0), (1.0, 400.0, 150.0, 1), (1.3, 200.0, 800.0, 2))
_QUIET = ((0.4, 150.0, 0.5), (0.4, 200.0, 0.05), (0.4, 240.0, 0.001), (0.4, 180.0, 0.5))


def _glide_rows(sr, noise):
    return [glide_signal(s, a, b, sr, seed=k, noise=noise)[0] for s, a, b, k in _GLIDES]


# name -> sr -> (margin inputs, natural inputs).  "glides": an up-, a down- and a wide glide over the usual noise floor.
# "costs": two of the glides and the weak burst.  "ceiling": stepped tones on both sides of 300 Hz and the weak-fundamental bursts.  "quiet": at a low candidate
# threshold the maxima of a noise lead-in land anywhere, also on the threshold, so the glides come without a noise floor
# (their lead-in is digital silence), and a stepped row holds passages 20 and 54 dB under the peak.  "noise": white
# noise alone, two natural rows of unequal length (no margin exists in noise).
CASE_INPUTS = {
    "glides": lambda sr: (_glide_rows(sr, 1e-3), natural_inputs(sr)[:1]),
    "costs": lambda sr: (_glide_rows(sr, 1e-3)[:2] + [weak_burst_signal(sr)], natural_inputs(sr)[:1]),
    "ceiling": lambda sr: ([stepped_signal([(0.4, 150.0, 0.5), (0.4, 420.0, 0.5), (0.4, 220.0, 0.5), (0.4, 500.0, 0.5)], sr),
                            stepped_signal([(0.4, 350.0, 0.5), (0.4, 250.0, 0.5), (0.4, 520.0, 0.5)], sr),
                            weak_fundamental_bursts(sr)], natural_inputs(sr)[:1]),
    "quiet": lambda sr: (_glide_rows(sr, 0.0)[:2] + [stepped_signal(_QUIET, sr)], natural_inputs(sr)[:1]),
    "noise": lambda sr: ([], [white_noise(0.6, sr, seed=21), white_noise(0.25, sr, seed=22)]),
}

# (name, sr, hop, min_pitch, config, input set): what each reaches is said in DESIGN.md "F0 tracking"
CONFIG_CASES = [
    ("ceiling_300", 16000, 160, 75.0, (("max_pitch", 300.0),), "ceiling"),
    ("ceiling_nyquist", 16000, 160, 75.0, (("max_pitch", 20000.0),), "glides"),
    ("costs_a", 16000, 160, 75.0, (("octave_cost", 0.05), ("octave_jump_cost", 0.35), ("voiced_unvoiced_cost", 0.14)),
     "costs"),
    ("costs_zero", 16000, 160, 75.0, (("octave_cost", 0.0), ("octave_jump_cost", 0.0), ("voiced_unvoiced_cost", 0.0)),
     "glides"),
    ("thresholds_low", 16000, 160, 75.0, (("voicing_threshold", 0.2), ("silence_threshold", 0.09)), "quiet"),
    ("thresholds_high", 16000, 160, 75.0, (("voicing_threshold", 0.8), ("silence_threshold", 0.003)), "quiet"),
    ("maxima_48k", 48000, 480, 40.0, (("voicing_threshold", 0.01),), "noise"),
    ("maxima_16k", 16000, 160, 75.0, (("voicing_threshold", 0.01),), "noise"),
]
CASE_IDS = [c[0] for c in CONFIG_CASES]


def case_fixtures(case):
    """(margin waves, natural waves, margin pairs, natural pairs, yardstick) of one entry of ``CONFIG_CASES``.  A case
    has no long row: the fixtures' seconds argument is 0.0 there and only part of their cache key (the input set names
    the rows)."""
    _, sr, hop, min_pitch, config, inputs = case
    margin, natural = CASE_INPUTS[inputs](sr)
    return (margin, natural, reference_pairs(sr, hop, min_pitch, 0.0, config, inputs),
            natural_pairs(sr, hop, min_pitch, config, inputs), config_yardstick(sr, hop, min_pitch, 0.0, config, inputs))


def unvoiced_by_ceiling(res64):
    """Frames whose path takes a pitch candidate at or above the ceiling: unvoiced for that reason alone."""
    T = res64["path"].size
    chosen = res64["cand_f"].astype(np.float64)[np.arange(T), res64["path"]]
    return (res64["path"] > 0) & (chosen >= res64["consts"].ceiling)
