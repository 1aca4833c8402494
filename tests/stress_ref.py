"""Float64 restatements of the stress conditions and melody metrics of ``pitchextractor_amd.stress`` /
``csrc/stress.hip``: the oracle of tests/test_stress_cpu.py (which holds them to numpy and scipy) and of
tests/test_stress_gpu.py.  Each states the float32 storage roundings the kernels make; everything else is float64
(the clipping threshold excepted: numpy itself computes it in float32, and so do the restatement and the kernel)."""
import math

import numpy as np

f32 = np.float32
BLOCK = 2048                                  # block step of the partitioned convolution


# --------------------------------------------------------------------------------------------------------------- rir
def rir(x, h):
    """``(y, peak, scaled)``: y[n] = sum_k h[k] x[n - k] for n < len(x) in float64, then y / (peak + 1e-6) if the
    peak exceeds 0.99."""
    x, h = np.asarray(x, np.float64), np.asarray(h, np.float64)
    if x.size == 0:
        return np.zeros(0), 0.0, False
    y = np.convolve(x, h)[:x.size]
    peak = float(np.max(np.abs(y)))
    scaled = peak > 0.99
    return (y / (peak + 1e-6) if scaled else y), peak, scaled


def rir_partitioned(x, h, dtype=np.float32, block=BLOCK):
    """The same convolution (before the normalisation) by uniformly partitioned overlap-save at ``block`` samples per
    step and transforms of ``2 * block``, with numpy's FFT in ``dtype``: the yardstick of the kernel, which does the
    same with its own float32 FFT.  Returns ``(y, dtype of the spectra)``."""
    x, h = np.asarray(x, dtype), np.asarray(h, dtype)
    n = x.size
    nb, parts = -(-n // block), -(-h.size // block)
    xp = np.zeros((nb + 1) * block, dtype)
    xp[block:block + n] = x                                        # block b reads samples [(b - 1) S, (b + 1) S)
    hp = np.zeros(parts * block, dtype)
    hp[:h.size] = h
    X = [np.fft.rfft(xp[b * block:(b + 2) * block]) for b in range(nb)]
    H = [np.fft.rfft(np.concatenate([hp[p * block:(p + 1) * block], np.zeros(block, dtype)])) for p in range(parts)]
    y = np.zeros(nb * block, dtype)
    for b in range(nb):
        acc = np.zeros(block + 1, X[0].dtype if X else np.complex64)
        for p in range(min(b + 1, parts)):
            acc = acc + X[b - p] * H[p]
        y[b * block:(b + 1) * block] = np.fft.irfft(acc, 2 * block)[block:]
    return y[:n], (X[0].dtype if X else None)


def decaying_rir(length, seed, t60_samples=None):
    """A seeded, exponentially decaying noise burst (no impulse responses ship), before ``prepare_rir``."""
    rng = np.random.default_rng(seed)
    t = np.arange(length, dtype=np.float64)
    tau = (t60_samples or max(length, 2)) / 6.9
    return (rng.standard_normal(length) * np.exp(-t / tau)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ biquads
def peaking_biquad(sr, freq, gain_db, Q):
    w0 = 2.0 * math.pi * freq / sr
    A = 10.0 ** (gain_db / 40.0)
    alpha = math.sin(w0) / (2.0 * Q)
    a0 = 1.0 + alpha / A
    b = np.array([1.0 + alpha * A, -2.0 * math.cos(w0), 1.0 - alpha * A]) / a0
    a = np.array([1.0, -2.0 * math.cos(w0) / a0, (1.0 - alpha / A) / a0])
    return b, a


def biquad_stage(x, b, a):
    """One stage: the direct recurrence in float64 (``a[0] == 1``), unclamped."""
    x = np.asarray(x, np.float64)
    y = np.zeros(x.size)
    x1 = x2 = y1 = y2 = 0.0
    b0, b1, b2, a1, a2 = float(b[0]), float(b[1]), float(b[2]), float(a[1]), float(a[2])
    for i in range(x.size):
        xi = float(x[i])
        v = b0 * xi + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        x2, x1, y2, y1 = x1, xi, y1, v
        y[i] = v
    return y


def microphone_eq(x, sr, curve):
    """The cascade: per stage the recurrence, one rounding to float32 (the stage's storage) and the clamp to [-1, 1],
    which is never fed back.  A stage whose b and a are equal is the identity."""
    y = np.asarray(x, np.float32)
    for stage in curve:
        b, a = peaking_biquad(sr, float(stage.get("freq", 1000.0)), float(stage.get("gain_db", 0.0)),
                              float(stage.get("Q", 0.707)))
        v = y.astype(np.float64) if np.array_equal(b, a) else biquad_stage(y, b, a)
        y = np.clip(v.astype(np.float32), f32(-1.0), f32(1.0))
    return y


# ----------------------------------------------------------------------------------------------------------- clipping
def quantile_f32(mag, q):
    """numpy 2's linear quantile of a float32 array at a Python float ``q``, operation by operation: q, the virtual
    index (N - 1) q, the weight g and the interpolation are all float32; ``hi - (hi - lo)(1 - g)`` when g >= 0.5, else
    ``lo + (hi - lo) g``."""
    s = np.sort(np.asarray(mag, np.float32))
    N = s.size
    v = f32(f32(N - 1) * f32(q))
    i = min(int(np.floor(v)), N - 1)
    g = f32(v - f32(np.floor(v)))
    lo, hi = s[i], s[min(i + 1, N - 1)]
    d = f32(hi - lo)
    return f32(hi - f32(d * f32(f32(1.0) - g))) if g >= f32(0.5) else f32(lo + f32(d * g))


def sample_clipping(x, percent):
    """``(y, thr)``; thr is None for a copy by ``percent <= 0``."""
    x = np.asarray(x, np.float32)
    if percent <= 0 or x.size == 0:
        return x.copy(), None
    thr = quantile_f32(np.abs(x), max(0.0, 1.0 - percent / 100.0))
    if thr <= 0:
        return x.copy(), thr
    return np.clip(x, -thr, thr), thr


# ---------------------------------------------------------------------------------------------------------------- agc
def agc_parameters(level_db, sr, target_rms):
    release = np.interp(level_db, [0.0, 10.0], [0.05, 0.4])
    depth_db = np.interp(level_db, [0.0, 10.0], [3.0, 18.0])
    return dict(attack_coeff=np.exp(-1.0 / (0.01 * sr)), release_coeff=np.exp(-1.0 / (release * sr)),
                max_gain=10 ** (depth_db / 20.0), target_rms=target_rms,
                smoothing=int(sr * np.interp(level_db, [0.0, 10.0], [0.01, 0.12])))


def agc_input(n, seed):
    """A leading silence, then bursts of amplitude 2.0, 2.0 and 0.2 with a long and a short silence between them: the
    follower attacks and releases, the gain reaches both of its bounds (the upper one in the leading silence), and the
    first onset drives the final clip."""
    rng = np.random.default_rng(seed)
    x = np.zeros(n, np.float32)
    edges = (np.array([0.04, 0.14, 0.7, 0.8, 0.86, 1.0]) * n).astype(int)
    for k, amp in ((0, 2.0), (2, 2.0), (4, 0.2)):
        m = edges[k + 1] - edges[k]
        x[edges[k]:edges[k + 1]] = (amp * rng.uniform(0.9, 1.0) * np.sin(2 * np.pi * 0.055 * np.arange(m) + 1.0))
    return x


def smooth_same(g, s):
    """``np.convolve(g, ones(s) / s, "same")`` as window sums in float64: out[i] = (1 / s) sum_{m < s} g[i + (s-1)//2 - m]."""
    g = np.asarray(g, np.float64)
    h = (s - 1) // 2
    pad = np.concatenate([np.zeros(s), g, np.zeros(s)])
    c = np.concatenate([[0.0], np.cumsum(pad)])                    # float32 gains: these sums are exact
    i = np.arange(g.size)
    return (c[i + h + s + 1] - c[i + h + 1]) / s


def agc_pumping(x, level_db, sr, target_rms=0.15, return_stages=False):
    x = np.asarray(x, np.float32)
    if level_db <= 0:
        return x.copy()
    p = agc_parameters(float(level_db), sr, target_rms)
    a, r, mg = float(p["attack_coeff"]), float(p["release_coeff"]), float(p["max_gain"])
    env, gains = 0.0, np.zeros(x.size, np.float32)
    lo = 1.0 / mg
    for i in range(x.size):
        rect = abs(float(x[i]))
        env = a * env + (1.0 - a) * rect if rect > env else r * env + (1.0 - r) * rect
        gains[i] = min(max(target_rms / (env + 1e-6), lo), mg)
    raw = gains
    s = p["smoothing"]
    if s > 1:
        if x.size < s:
            raise ValueError("row shorter than the smoothing length")
        gains = smooth_same(gains, s).astype(np.float32)
    y = np.clip((x * gains).astype(np.float32), f32(-1.0), f32(1.0))
    return (y, raw, gains, p) if return_stages else y


# ------------------------------------------------------------------------------------------------------------ metrics
def hz_to_cents(f0):
    return 1200.0 * np.log2(np.asarray(f0, np.float64) / 55.0)


def melody_metrics(reference, prediction, baseline=None, voicing_threshold_hz=10.0, return_diffs=False):
    """The notebooks' ``compute_metrics`` (float64 cents) plus ``VUV_flips`` of ``evaluate_pathology``."""
    reference, prediction = np.asarray(reference, np.float32), np.asarray(prediction, np.float32)
    n = min(reference.size, prediction.size)
    ref, pred = reference[:n], prediction[:n]
    rv, pv = ref > 0, pred.astype(np.float64) > voicing_threshold_hz
    voiced = int(np.count_nonzero(rv))
    out = dict(RPA=math.nan, RCA=math.nan, VUV=float(np.count_nonzero(rv == pv) / max(n, 1)), OctaveError=math.nan,
               VUV_flips=math.nan, n_voiced=voiced, n_frames=n)
    d = np.zeros(0)
    if voiced:
        d = hz_to_cents(np.maximum(pred[rv], f32(1e-5))) - hz_to_cents(ref[rv])
        circ = np.mod(d + 600.0, 1200.0) - 600.0
        octave = np.round(d / 1200.0)
        errors = (np.abs(d) > 50.0) & (octave != 0) & (np.abs(d - octave * 1200.0) <= 50.0)
        out.update(RPA=float(np.count_nonzero(np.abs(d) <= 50.0) / voiced),
                   RCA=float(np.count_nonzero(np.abs(circ) <= 50.0) / voiced),
                   OctaveError=float(np.count_nonzero(errors) / voiced))
    if baseline is not None:
        base = np.asarray(baseline, np.float32)
        m = min(base.size, prediction.size)
        if m:
            bv = base[:m].astype(np.float64) > voicing_threshold_hz
            cv = prediction[:m].astype(np.float64) > voicing_threshold_hz
            out["VUV_flips"] = float(np.count_nonzero(bv != cv) / m)
    return (out, d) if return_diffs else out


def boundary_margin_cents(d):
    """Distance of the cents differences from the nearest decision boundary of the metrics: +-50 cents around every
    multiple of 1200 (hits, octave errors, the circular distance) and the half octaves (where the octave number and the
    circular distance turn over)."""
    d = np.asarray(d, np.float64)
    if d.size == 0:
        return math.inf
    w = np.mod(d, 1200.0)
    dist = np.minimum.reduce([np.abs(w - 50.0), np.abs(w - 1150.0), np.abs(w - 600.0)])
    return float(np.min(dist))
