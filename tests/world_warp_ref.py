"""Float64 restatement of the voice transforms of WORLD frames (csrc/world_warp.hip, ``world.warp_envelopes``) and of the
host conventions around them, with a float32 variant in the kernel's order of operations as the yardstick.

Conventions.  Output bin k sits at f = k fs / fft_size.  The frequency map (VTLP, Jaitly & Hinton 2013) is w(f) =
alpha f for f <= x0 = f_hi min(alpha, 1) / alpha and the straight line from (x0, alpha x0) to (fs / 2, fs / 2) above;
the output envelope at f is the source envelope at w^-1(f).  An output frame reads the source position i + frac (frac a
float32 in [0, 1), part of the input; frame i + 1 clamped to the last): ln sp is mixed linearly over the two frames, then
over the two source bins around w^-1(f); tilt_db_per_octave log2(max(f, 125) / 1000) dB are added (sp is a power) and
one exp taken.  ap: the same read in the linear domain, times 10^(breath_db / 20), clamped to [0, 1].  With alpha == 1,
no tilt and frac == 0 the frame's sp is a copy, and its ap when breath_db == 0 as well.

Inputs are what the kernel gets: float32 sp / ap, float32 alpha / f_hi / tilt / breath, float32 fractions.  The float64
restatement computes everything from them in float64; the float32 variant forms the map's four constants in float64,
rounds them, and works per bin in float32."""
import math

import numpy as np

LN_PER_DB = math.log(10.0) / 10.0


# --------------------------------------------------------------------------- the map, in Hz (float64)
def knee(alpha, f_hi):
    """(x0, y0): where the linear part of w ends, on the source and on the output axis."""
    x0 = f_hi * min(alpha, 1.0) / alpha
    return x0, alpha * x0


def w(f, alpha, f_hi, fs):
    f = np.asarray(f, dtype=np.float64)
    x0, y0 = knee(alpha, f_hi)
    return np.where(f <= x0, alpha * f, y0 + (f - x0) * (fs / 2.0 - y0) / (fs / 2.0 - x0))


def w_inv(f, alpha, f_hi, fs):
    f = np.asarray(f, dtype=np.float64)
    x0, y0 = knee(alpha, f_hi)
    return np.where(f <= y0, f / alpha, x0 + (f - y0) * (fs / 2.0 - x0) / (fs / 2.0 - y0))


# --------------------------------------------------------------------------- host conventions
def warped_frames(n, hop, rate):
    return 1 + int(round(n / rate)) // hop


def source_positions(n_frames, rate, src_frames, clamp=True):
    """Output frame g reads min(g * rate, src_frames - 1).  ``clamp=False`` restates a mistake (below)."""
    return np.array([min(g * rate, src_frames - 1) if clamp else g * rate for g in range(n_frames)], dtype=np.float64)


def time_warp_curve(base, positions):
    """Linear in Hz between two voiced frames; the nearer frame's value when either is unvoiced, ties to the earlier."""
    base = np.asarray(base, dtype=np.float64)
    out = np.zeros(len(positions))
    for g, p in enumerate(positions):
        i = min(int(math.floor(p)), base.size - 1)
        j = min(i + 1, base.size - 1)
        t = p - i
        if base[i] > 0 and base[j] > 0:
            out[g] = base[i] + t * (base[j] - base[i])
        else:
            out[g] = base[i] if t <= 0.5 else base[j]
    return out


def split_positions(positions):
    """(integer frame, float32 fraction in [0, 1)) of float64 positions; a fraction that float32 rounds up to 1 moves
    to the next frame."""
    p = np.asarray(positions, dtype=np.float64)
    whole = np.floor(p)
    frac = (p - whole).astype(np.float32)
    whole[frac >= 1.0] += 1
    frac[frac >= 1.0] = 0
    return whole.astype(np.int64), frac


# --------------------------------------------------------------------------- the transform of one row
def warp(sp, ap, positions, alpha=1.0, f_hi=4800.0, tilt=0.0, breath=0.0, *, fs, fp32=False, log_domain=True,
         invert=True):
    """sp (S, bins) float32 and ap likewise (or None) read at ``positions`` -> (sp_out, ap_out) of (len(positions),
    bins), float64 or (``fp32``) float32.  Three switches restate a mistake each, for the tests that must catch it:
    ``log_domain=False`` interpolates sp linearly, ``invert=False`` warps with alpha in place of 1 / alpha, and
    ``source_positions(clamp=False)`` runs past the last source frame (such positions are outside what ``warp``, like
    the plan, accepts)."""
    T = np.float32 if fp32 else np.float64
    sp = np.asarray(sp, dtype=np.float32)
    S, bins = sp.shape
    H = bins - 1
    fft_size = 2 * H
    alpha, f_hi, tilt, breath = (float(np.float32(v)) for v in (alpha, f_hi, tilt, breath))
    a = alpha if invert else 1.0 / alpha
    x0 = f_hi * min(a, 1.0) / a / (fs / fft_size)
    y0 = a * x0
    inv_alpha, y0c, x0c, slope = (T(v) for v in (1.0 / a, y0, x0, (H - x0) / (H - y0)))
    k = np.arange(bins).astype(T)
    u = np.where(k <= y0c, k * inv_alpha, x0c + (k - y0c) * slope).astype(T)
    k0 = np.clip(np.floor(u), 0, H - 1).astype(np.int64)
    t = np.clip(u - k0.astype(T), T(0), T(1)).astype(T)
    hz = k * T(fs / fft_size)
    tilt_ln = (T(tilt) * np.log2(np.maximum(hz, T(125)) / T(1000)).astype(T) * T(LN_PER_DB)).astype(T)
    gain = T(10.0) ** (T(breath) / T(20))
    whole, frac = split_positions(positions)
    if len(whole) and (whole.min() < 0 or (whole + frac).max() > S - 1):
        raise ValueError("a source position outside [0, src_frames - 1]")
    sp_out = np.zeros((len(whole), bins), T)
    ap_out = None if ap is None else np.zeros((len(whole), bins), T)
    for g, (i, fr) in enumerate(zip(whole, frac)):
        j = min(i + 1, S - 1)
        fr = T(0) if j == i else T(fr)
        same_axes = alpha == 1.0 and tilt == 0.0 and fr == 0
        if same_axes:
            sp_out[g] = sp[i]
        else:
            if log_domain:
                l = np.log(sp[i].astype(T))
                if fr != 0:
                    l = l + fr * (np.log(sp[j].astype(T)) - l)
            else:
                l = sp[i].astype(T)
                if fr != 0:
                    l = l + fr * (sp[j].astype(T) - l)
            v = l[k0] + t * (l[k0 + 1] - l[k0])
            if not log_domain:
                v = np.log(v)
            if tilt != 0.0:
                v = v + tilt_ln
            sp_out[g] = np.exp(v.astype(T))
        if ap is not None:
            if same_axes and breath == 0.0:
                ap_out[g] = ap[i]
            else:
                b = np.asarray(ap[i], dtype=np.float32).astype(T)
                if fr != 0:
                    b = b + fr * (np.asarray(ap[j], dtype=np.float32).astype(T) - b)
                ap_out[g] = np.clip((b[k0] + t * (b[k0 + 1] - b[k0])) * gain, T(0), T(1))
    return sp_out, ap_out
