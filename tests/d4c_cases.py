"""The rows tests/test_d4c_gpu.py analyses, with their float64 and float32 restatements (tests/d4c_ref.py) computed once
per configuration and never modified, and the frames the verdict comparison leaves out.  tests/test_d4c_cpu.py checks,
with the restatements alone, that those stay under the cap the GPU test asserts."""
import numpy as np

from tests import cheaptrick_ref as ct
from tests import d4c_ref as d4

# (fs, frame period in ms, LoveTrain threshold): 1 band at 2048 points; 3 bands at 2048, with pyworld's threshold and
# with the data layer's; 5 bands at 4096; and a rate whose LoveTrain transform (2048) is half the band analysis's (4096)
CONFIGS = [(16000, 5.0, 0.85), (24000, 5.0, 0.85), (24000, 12.5, 0.0), (48000, 5.0, 0.85), (25000, 10.0, 0.85)]
MARGIN = 1000.0                                                   # x the yardstick: frames left out of the verdicts
_CASES = {}


def voice(fs, seconds, f0, seed, level=0.5, noise=1e-2):
    """A harmonic complex (1 / h partials up to 0.45 fs) over white noise."""
    n = int(seconds * fs)
    t = np.arange(n) / fs
    rng = np.random.default_rng(seed)
    f0 = np.broadcast_to(np.asarray(f0, dtype=np.float64), (n,))
    phase = 2 * np.pi * np.cumsum(f0) / fs
    x = sum(np.sin(h * phase + h) / h for h in range(1, max(2, int(0.45 * fs / f0.max()))))
    x = level * x / np.abs(x).max() + noise * rng.standard_normal(n)
    return x.astype(np.float32)


def rows(fs, fp):
    """name -> (wave float32, f0 float32): 0.25 to 0.4 s each, but for the rows that are short on purpose."""
    frames = lambda x: 1 + int(len(x) / (fs * fp / 1000.0))  # noqa: E731  the last frames sit at and past the end
    out = {}
    x = voice(fs, 0.3, 132.7, 1, noise=3e-2)
    out["vowel_noise"] = (x, np.full(frames(x), 132.7, np.float32))
    n = int(0.4 * fs)
    x = voice(fs, 0.4, np.linspace(64.0, 30.0, n), 2)
    out["glide_47_40"] = (x, np.linspace(64.0, 30.0, frames(x)).astype(np.float32))     # crosses 47 Hz, ends below 40
    x = voice(fs, 0.3, 201.3, 3)
    f0 = np.full(frames(x), 201.3, np.float32)
    L = f0.size
    f0[:2] = 0.0
    f0[L // 3:L // 3 + 4] = 0.0
    f0[-3] = np.nan
    out["unvoiced_stretches"] = (x, f0)
    out["one_frame"] = (voice(fs, 0.25, 200.0, 4), np.array([200.0], np.float32))
    out["zeros"] = (np.zeros(int(0.25 * fs), np.float32), np.full(6, 150.0, np.float32))
    x = voice(fs, 0.3, 180.0, 6, level=0.9)
    x[len(x) // 2:] *= np.float32(1e-4 / 0.9)                     # a 1e-4 passage after a full-scale one
    out["quiet_after_loud"] = (x, np.full(frames(x), 180.0, np.float32))
    # 4 ms under a 33 ms window: most indices are clamped.  Two frames: a later one's window would lie wholly past the
    # end, where the wave is a constant, the windowed one rounding noise alone and a0 a ratio of two such sums
    out["shorter_than_a_window"] = (voice(fs, 0.004, 700.0, 7), np.full(2, 90.0, np.float32))
    x = voice(fs, 0.25, 1000.0, 8)
    out["f0_1000"] = (x, np.full(frames(x), 1000.0, np.float32))
    return out


def cases(cfg):
    """name -> x, f0, and per restatement (64 / 32): ap, b (frames x {a0, coarse}), pmin."""
    if cfg not in _CASES:
        fs, fp, thr = cfg
        out = {}
        for name, (x, f0) in rows(fs, fp).items():
            c = dict(x=x, f0=f0)
            for tag, fp32 in (("64", False), ("32", True)):
                c["ap" + tag], c["b" + tag], c["pmin" + tag] = d4.d4c(x.astype(np.float64), f0, fs, fp, threshold=thr,
                                                                      fft_size=ct.default_fft_size(fs), fp32=fp32)
            for a in c.values():
                a.setflags(write=False)
            out[name] = c
        _CASES[cfg] = out
    return _CASES[cfg]


def a0_yardstick(all_cases):
    """The float32 restatement's largest deviation from the float64 one in a0 over a configuration's frames."""
    return max(float(np.abs(c["b32"][:, 0] - c["b64"][:, 0]).max(initial=0.0)) for c in all_cases.values())


def excluded_frames(all_cases, c, cfg):
    """Frames of the row ``c`` whose verdict float32 arithmetic may flip: the float64 a0 within MARGIN x the a0
    yardstick of the threshold, or the float64 smallest smoothed power within MARGIN x the float32 restatement's
    deviation in it of zero."""
    thr = cfg[2]
    voiced = c["f0"] > 0
    near_thr = voiced & (np.abs(c["b64"][:, 0] - thr) <= MARGIN * a0_yardstick(all_cases))
    dev = np.nan_to_num(np.abs(c["pmin32"] - c["pmin64"]), nan=0.0)
    near_zero = np.nan_to_num(c["pmin64"], nan=np.inf) <= MARGIN * dev
    return near_thr | near_zero
