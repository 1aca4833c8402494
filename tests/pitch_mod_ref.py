"""float64 numpy restatement of the pitch-modulation kernels (csrc/pitch_mod.hip), written from the definition in
DESIGN.md "Pitch modulation": the direct sum over the filter table and the label rule.

``warp`` is the definition: ``y[i] = scale * sum_s W(scale |p - s|) x[s]`` in float64 for ``t0 < i < t1``, ``p = t0 +
tau(i - t0)``, ``scale = min(1, 1 / s)``, ``W`` the piecewise-linear read of ``pitch_shift.resample_filter`` at 512
entries per zero crossing; every other sample is the input's.  ``warp_f32`` is the same sum with the kernel's tap order
(the left wing from ``floor(p)`` down, then the right wing up) and a float32 accumulator; its deviation from ``warp`` is
the yardstick the kernel is held to.  ``labels`` is the label rule in float64."""
from __future__ import annotations

import numpy as np

from pitchextractor_amd import pitch_mod as PM
from pitchextractor_amd.pitch_shift import RES_TYPES, resample_filter

KP = 512


def _table(quality):
    win = resample_filter(quality)
    return win, np.append(np.diff(win), 0.0)


def positions(n, t0, t1, mod, sr):
    """(i, p, scale) of the warped samples ``t0 < i < min(t1, n)``: float64 source positions and cutoff scales."""
    i = np.arange(t0 + 1, min(t1, n), dtype=np.int64)
    tau, s = PM.time_map(mod, t1 - t0, (i - t0).astype(np.float64), sr)
    return i, float(t0) + tau, np.minimum(1.0, 1.0 / s)


def warp(x, t0, t1, mod, sr, quality="kaiser_fast"):
    """The definition in float64 -> float64 array of ``x``'s length."""
    x = np.asarray(x, dtype=np.float64)
    y = x.copy()
    if mod is None or mod.identity or x.size == 0:
        return y
    win, dwin = _table(quality)
    top = win.size - 1
    i, p, scale = positions(x.size, t0, t1, mod, sr)
    if i.size == 0:
        return y
    wing = int(np.ceil(RES_TYPES[quality][0] * 1.5)) + 1
    taps = np.floor(p).astype(np.int64)[:, None] + np.arange(-wing, wing + 2, dtype=np.int64)[None, :]
    xt = np.abs(p[:, None] - taps) * scale[:, None] * KP
    ok = (xt < top) & (taps >= 0) & (taps < x.size)
    off = np.where(ok, np.floor(xt), 0).astype(np.int64)
    w = np.where(ok, win[off] + (xt - off) * dwin[off], 0.0)
    y[i] = scale * np.sum(w * x[np.clip(taps, 0, x.size - 1)], axis=1)
    return y


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def warp_f32(x, t0, t1, mod, sr, quality="kaiser_fast"):
    """The kernel's arithmetic: positions in float64, the table read and the accumulation in float32, taps in the
    kernel's order -> float32 array."""
    x = np.asarray(x, dtype=np.float32)
    y = x.copy()
    if mod is None or mod.identity or x.size == 0:
        return y
    win, dwin = _table(quality)
    win32, dwin32 = win.astype(np.float32), np.append(np.diff(win), 0.0).astype(np.float32)
    top = float(win.size - 1)
    i, p, scale = positions(x.size, t0, t1, mod, sr)
    if i.size == 0:
        return y
    n0 = np.floor(p).astype(np.int64)
    frac = p - np.floor(p)
    sp = scale * KP
    v = np.zeros(i.size, np.float32)
    for start, sign, first in ((frac, -1, 0), (1.0 - frac, 1, 1)):
        for a in range(int(RES_TYPES[quality][0] * 1.5) + 1):
            xt = (start + float(a)) * sp
            live = xt < top
            if not live.any():
                break
            off = np.where(live, xt, 0.0).astype(np.int64)
            eta = (xt - off).astype(np.float32)
            w = _fma32(eta, dwin32[off], win32[off])
            s = n0 + first + sign * a
            src = np.where((s >= 0) & (s < x.size), x[np.clip(s, 0, x.size - 1)], np.float32(0))
            v = np.where(live, _fma32(w, src, v), v)
    y[i] = v * scale.astype(np.float32)
    return y


def labels(f0, sil, count, mod, hop, sr):
    """The label rule in float64: ``(f0 (float64), flags)`` of one row of ``W`` frames whose first ``count`` are kept,
    warped over ``T = (count - 1) hop``.  A voiced result is ``s * value`` (not yet rounded to float32)."""
    f0 = np.asarray(f0, dtype=np.float32)
    sil = np.asarray(sil, dtype=np.float32)
    out_f, out_q = f0.astype(np.float64), sil.copy()
    L = int(count)
    if mod is None or mod.identity or L < 2:
        return out_f, out_q
    tau, s = PM.time_map(mod, (L - 1) * hop, np.arange(L, dtype=np.float64) * hop, sr)
    pos = tau / float(hop)
    voiced = (f0[:L] > 0) & (sil[:L] == 0)
    for j in range(L):
        i = min(max(int(np.floor(pos[j])), 0), L - 1)
        k = min(i + 1, L - 1)
        t = min(max(pos[j] - i, 0.0), 1.0)
        if voiced[i] and voiced[k]:
            out_f[j], out_q[j] = s[j] * (float(f0[i]) + t * (float(f0[k]) - float(f0[i]))), 0.0
        else:
            pick = i if t <= 0.5 else k
            if voiced[pick]:
                out_f[j], out_q[j] = s[j] * float(f0[pick]), 0.0
            else:
                out_f[j], out_q[j] = float(f0[pick]), sil[pick]
    return out_f, out_q


def complex_tone(f0, sr, n, partials=10):
    """``partials`` equal-amplitude harmonics of ``f0`` Hz, peak below 1: float32."""
    t = np.arange(n, dtype=np.float64) / float(sr)
    y = sum(np.sin(2.0 * np.pi * (k + 1) * f0 * t + 0.3 * k) for k in range(partials))
    return (0.9 * y / np.max(np.abs(y))).astype(np.float32)


def rms_cents(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((1200.0 * np.log2(a / b)) ** 2)))


# the audio-and-label consistency case shared by the CPU and the GPU test: 1 s of a 220 Hz, 10-partial complex at
# 24 kHz and hop 300 (81 label frames, t1 = n), vibrato 0.03 at 6 Hz plus a ramp 0.06
CONSISTENCY = dict(sr=24000, hop=300, n=24000, f0=220.0, min_pitch=100.0,
                   mod=PM.Modulation(((0.03, 6.0, 0.7),), 0.06))


def consistency_scores(tracked, frame_times, new_labels, case=CONSISTENCY):
    """``(rms cents tracked vs new labels, rms cents old vs new labels)`` over the tracker's frames: the new labels
    (one per label frame, at ``j hop / sr``) are read linearly at the tracker's frame times."""
    tracked = np.asarray(tracked, np.float64)
    label_t = np.arange(len(new_labels), dtype=np.float64) * case["hop"] / case["sr"]
    at = np.asarray(frame_times, np.float64) - 0.5 / case["sr"]        # the tracker's samples sit at (i + 0.5) / sr
    new = np.interp(at, label_t, np.asarray(new_labels, np.float64))
    assert tracked.size == new.size and tracked.size > 0 and np.all(tracked > 0), "every tracked frame is voiced"
    return rms_cents(tracked, new), rms_cents(np.full(new.size, case["f0"]), new)
