"""float64 / NumPy restatement of every stage of ``pitchextractor_amd.stimuli`` (``csrc/stimuli.hip``), after the
reference's Utils/dynamic_pitch_tools.py and the ``synthesize_timbre_waveform`` cell of
Utils/pitch_range_and_timbre_coverage.ipynb.  The phase is a sequential ``np.cumsum``, every rms is taken in float64 over
the float32 samples, the lag comes from ``np.correlate`` in float64.  tests/test_stimuli_cpu.py holds it against arrays
captured from the reference's own functions (tests/golden/make_stimuli_golden.py)."""
import math

import numpy as np

f32 = np.float32
FADE_TIME = 0.02
PIECE = 2048          # the scan piece of the kernels


def fade_samples(sr) -> int:
    return int(max(FADE_TIME * sr, 0))


def num_samples(duration, sr) -> int:
    return int(duration * sr)


# -------------------------------------------------------------------------------------------------------------- curves
def time_axis(duration, n) -> np.ndarray:
    return np.linspace(0.0, duration, n, endpoint=False, dtype=np.float64)


def glide_curve(duration, start_hz, end_hz, sr, n=None):
    """``(t, curve)`` in float64; ``n``: a sample count other than ``int(duration * sr)``."""
    t = time_axis(duration, num_samples(duration, sr) if n is None else n)
    return t, np.linspace(start_hz, end_hz, t.shape[0], dtype=np.float64)


def vibrato_curve(rate_hz, depth_cents, base_hz, duration, sr, n=None):
    t = time_axis(duration, num_samples(duration, sr) if n is None else n)
    modulation = np.sin(2.0 * np.pi * rate_hz * t)
    return t, base_hz * (2.0 ** ((depth_cents / 1200.0) * modulation))


def phase_of(curve, sr, blocked: int = 0) -> np.ndarray:
    """``cumsum(((2 pi) curve) / sr)``; ``blocked``: summed in pieces of that many samples with a carry instead."""
    omega = 2.0 * np.pi * np.asarray(curve).astype(np.float64) / float(sr)
    if not blocked:
        return np.cumsum(omega)
    out, carry = np.empty_like(omega), 0.0
    for lo in range(0, omega.size, blocked):
        part = np.cumsum(omega[lo:lo + blocked])
        out[lo:lo + blocked] = carry + part
        carry += part[-1]
    return out


def prefade(curve, sr, amplitude=0.8, blocked: int = 0) -> np.ndarray:
    """``float32(amplitude * sin(phase))``: the samples ahead of the fade."""
    return (amplitude * np.sin(phase_of(curve, sr, blocked))).astype(f32)


def tone_prefade(frequency, sr, duration, partials, n=None) -> np.ndarray:
    """The partial sum of ``synthesize_timbre_waveform`` in the profile's order, rounded to float32."""
    t = time_axis(duration, num_samples(duration, sr) if n is None else n)
    waveform = np.zeros_like(t, dtype=np.float64)
    for harmonic, amplitude in partials.items() if isinstance(partials, dict) else partials:
        if amplitude == 0:
            continue
        waveform += amplitude * np.sin(2.0 * math.pi * frequency * float(harmonic) * t)
    return waveform.astype(f32)


# -------------------------------------------------------------------------------------------------------------- finish
def fade_window(n, fade) -> np.ndarray:
    window = np.ones(n, dtype=np.float64)
    if fade <= 0:
        return window
    if n < fade:
        raise ValueError("a row is shorter than the fade")
    ramp = 0.5 - 0.5 * np.cos(np.linspace(0.0, np.pi, fade, dtype=np.float64))
    window[:fade] = ramp
    window[-fade:] = ramp[::-1]
    return window


def rms64(x) -> float:
    x = np.asarray(x, f32).astype(np.float64)
    return float(np.sqrt(np.mean(x * x))) if x.size else 0.0


def finish(x, sr, noise=None, snr_db=None, return_stages=False):
    """Fade, noise mix and peak normalisation of float32 samples.  Returns ``(y, stats)``, stats = ``{peak, rms_signal,
    rms_noise, scale}`` (scale 0: no mix); ``return_stages``: also ``(faded, mixed)``."""
    x = np.asarray(x, f32)
    faded = (x.astype(np.float64) * fade_window(x.size, fade_samples(sr))).astype(f32)
    rs, rn, scale = rms64(faded), 0.0, f32(0.0)
    mixed = faded
    if noise is not None:
        noise = np.asarray(noise, f32)
        rn = rms64(noise)
        if rs > 0 and rn > 0:
            scale = f32((rs / (10.0 ** (snr_db / 20.0))) / rn)
            mixed = faded + noise * scale                     # float32 product, float32 sum
    peak = float(np.max(np.abs(mixed))) if mixed.size else 0.0
    y = mixed / f32(peak + 1e-6) if peak > 0.99 else mixed
    stats = dict(peak=peak, rms_signal=rs, rms_noise=rn, scale=float(scale))
    return (y.astype(f32), stats, faded, mixed) if return_stages else (y.astype(f32), stats)


def synthesize_from_f0_curve(curve, sr, amplitude=0.8):
    return finish(prefade(curve, sr, amplitude), sr)[0]


def timbre_waveform(frequency, sr, duration, profile, noise=None):
    """``synthesize_timbre_waveform`` with the noise as an input: ``(y, stats)``."""
    x = tone_prefade(frequency, sr, duration, profile.get("partials", {1: 1.0}))
    snr = profile.get("snr_db")
    return finish(x, sr, noise if snr is not None else None, snr)


# ----------------------------------------------------------------------------------------------------------- reference
def frame_times(n, tstep, num_frames) -> np.ndarray:
    t32 = lambda i: f32(np.float64(i) * np.float64(tstep))  # noqa: E731
    duration = t32(n - 1)
    if n > 1:
        duration = duration + (t32(1) - t32(0))
    return np.linspace(0.0, duration, num=num_frames, endpoint=False, dtype=np.float64)


def sample_reference(n, tstep, curve32_at, num_frames) -> np.ndarray:
    """``sample_reference_f0`` frame by frame, as the kernel does it: ``curve32_at(j)`` is sample j of the curve rounded
    to float32, the time axis is ``float32(j * tstep)``."""
    tau = frame_times(n, tstep, num_frames)
    t32 = lambda j: float(f32(np.float64(j) * np.float64(tstep)))  # noqa: E731
    out = np.zeros(num_frames, f32)
    for k, x in enumerate(tau):
        if n == 1 or x >= t32(n - 1):
            out[k] = f32(curve32_at(n - 1))
            continue
        j = min(max(int(math.floor(x / tstep)), 0), n - 2)
        while j > 0 and t32(j) > x:
            j -= 1
        while j < n - 2 and t32(j + 1) <= x:
            j += 1
        x0, x1, y0, y1 = t32(j), t32(j + 1), float(f32(curve32_at(j))), float(f32(curve32_at(j + 1)))
        out[k] = f32(y0) if x == x0 else f32((y1 - y0) / (x1 - x0) * (x - x0) + y0)
    return out


def sample_reference_arrays(t32, curve32, num_frames) -> np.ndarray:
    """``sample_reference_f0`` on stored arrays (the reference's own lines)."""
    t32, curve32 = np.asarray(t32, f32), np.asarray(curve32, f32)
    if num_frames <= 0:
        return np.zeros((0,), f32)
    duration = t32[-1]
    if t32.size > 1:
        duration = duration + (t32[1] - t32[0])
    tau = np.linspace(0.0, duration, num=num_frames, endpoint=False, dtype=np.float64)
    return np.interp(tau, t32, curve32).astype(f32)


# ------------------------------------------------------------------------------------------------------------- metrics
def rms_cents(ref, pred) -> float:
    L = min(len(ref), len(pred))
    ref, pred = np.asarray(ref[:L], f32), np.asarray(pred[:L], f32)
    mask = ref > 0
    if L == 0 or not np.any(mask):
        return math.nan
    cents = lambda f: 1200.0 * np.log2(f.astype(np.float64) / 55.0)  # noqa: E731
    d = cents(np.maximum(pred[mask], f32(1e-5))) - cents(ref[mask])
    return float(np.sqrt(np.mean(d * d)))


def correlation(ref, pred):
    """The full cross-correlation of the mean-centred tracks in float64, or None when either is constant."""
    L = min(len(ref), len(pred))
    if L == 0:
        return None
    r, p = np.asarray(ref[:L], f32).astype(np.float64), np.asarray(pred[:L], f32).astype(np.float64)
    rc, pc = r - np.mean(r), p - np.mean(p)
    if np.allclose(rc, 0) or np.allclose(pc, 0):
        return None
    return np.correlate(pc, rc, mode="full")


def lag_frames(ref, pred) -> float:
    c = correlation(ref, pred)
    return math.nan if c is None else float(int(np.argmax(c)) - (min(len(ref), len(pred)) - 1))


def lag_margin(ref, pred) -> float:
    """How far the best correlation exceeds the runner-up, relative to the best."""
    c = np.sort(correlation(ref, pred))
    return float((c[-1] - c[-2]) / abs(c[-1]))


def overshoot_cents(ref, pred) -> float:
    L = min(len(ref), len(pred))
    if L == 0:
        return math.nan
    target, peak = float(f32(ref[L - 1])), float(np.max(np.asarray(pred[:L], f32)))
    return math.nan if target <= 0 or peak <= 0 else 1200.0 * math.log2(peak / target)


def final_error_cents(ref, pred) -> float:
    L = min(len(ref), len(pred))
    if L == 0 or not float(ref[L - 1]) > 0:
        return math.nan
    return 1200.0 * math.log2(max(float(f32(pred[L - 1])), 1e-5) / max(float(f32(ref[L - 1])), 1e-5))


def dynamic_metrics(ref, pred) -> dict:
    return dict(RMSE_cents=rms_cents(ref, pred), Lag_frames=lag_frames(ref, pred),
                Overshoot_cents=overshoot_cents(ref, pred), Final_error_cents=final_error_cents(ref, pred))


def shifted_vibrato_track(shift, frames=64, rate_hz=6.0, period_ms=12.5, base=220.0, depth_cents=60.0) -> np.ndarray:
    """A vibrato F0 track sampled every ``period_ms``, delayed by ``shift`` frames: the margin input of the lag tests."""
    t = (np.arange(frames, dtype=np.float64) - shift) * (period_ms / 1000.0)
    return (base * 2.0 ** ((depth_cents / 1200.0) * np.sin(2.0 * np.pi * rate_hz * t))).astype(f32)
