"""The rows tests/test_world_warp_gpu.py transforms, with their float64 and float32 restatements (tests/world_warp_ref.py)
computed once per configuration and never modified.  The envelopes are CheapTrick's (tests/cheaptrick_ref.py) of the
signals of tests/d4c_cases.py, the aperiodicities D4C's float32 restatement of the same frames, both as float32: what
the kernel is handed.  tests/test_world_warp_cpu.py checks, with the restatements alone, that the float32 restatement's
own deviation is a usable yardstick on every row (finite, not zero, no element left out) and that the three restated
mistakes exceed the bound the GPU test asserts."""
import math

import numpy as np

from tests import cheaptrick_ref as ct
from tests import d4c_cases as dc
from tests import world_warp_ref as wwr

# (fs, frame period ms, fft_size, D4C threshold or None: no ap, rate, alpha, tilt dB / octave, breath dB)
# 257 / 513 / 1025 bins (tails against the 256-wide workgroup); rates below, at and above 1; alpha below and above 1;
# the time interpolation alone (alpha 1, no tilt); ap absent and given
CONFIGS = [
    (8000, 5.0, 512, None, 0.8, 1.25, 0.0, 0.0),
    (24000, 12.5, 1024, 0.0, 1.25, 0.8, -3.0, 6.0),
    (48000, 5.0, 2048, 0.85, 1.0, 1.25, 2.0, -6.0),
    (24000, 5.0, 1024, 0.85, 0.8, 1.0, 0.0, 3.0),
]
# (signal of d4c_cases.rows, first source frame, source frames): rows of 7, 3, 2 and 0 source frames and a long one
ROWS = [("vowel_noise", 0, 7), ("glide_47_40", 4, 3), ("quiet_after_loud", 10, 2), ("f0_1000", 0, 0),
        ("quiet_after_loud", 0, None)]
_CASES = {}


def config_id(cfg):
    return "fs{}-fp{}-n{}-ap{}-r{}-a{}-t{}-b{}".format(*cfg)


def positions_for(src_frames, rate):
    """Output frames up to and two past the last source frame: frame 0 and every multiple that is whole sit exactly on
    a source frame, and the last ones are clamped to it."""
    if src_frames == 0:
        return np.zeros(0)
    return wwr.source_positions(int(math.ceil((src_frames - 1) / rate)) + 2, rate, src_frames)


def cases(cfg):
    """One dict per row of ROWS: sp, ap (or None), pos, and per restatement (64 / 32) sp and ap."""
    if cfg not in _CASES:
        fs, fp, N, thr, rate, alpha, tilt, breath = cfg
        signals = dc.rows(fs, fp)
        aps = None if thr is None else dc.cases((fs, fp, thr))
        out = []
        for name, first, count in ROWS:
            x, f0 = signals[name]
            count = len(f0) - first if count is None else count
            sp = ct.cheaptrick(x.astype(np.float64), f0, fs, fp, fft_size=N, first_frame=first,
                               n_frames=count).astype(np.float32).reshape(count, N // 2 + 1)
            ap = None if aps is None else np.asarray(aps[name]["ap32"][first:first + count], dtype=np.float32)
            c = dict(name=name, sp=sp, ap=ap, pos=positions_for(count, rate))
            for tag, fp32 in (("64", False), ("32", True)):
                c["sp" + tag], c["ap" + tag] = wwr.warp(sp, ap, c["pos"], alpha, f_hi_of(cfg), tilt, breath, fs=fs,
                                                       fp32=fp32)
            for a in c.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            out.append(c)
        _CASES[cfg] = out
    return _CASES[cfg]


def f_hi_of(cfg):
    return 4800.0 if cfg[0] > 9600 else 3000.0                   # 4800 Hz is above Nyquist at 8 kHz


def deviations(rows, got_sp, got_ap):
    """(max |ln sp - ln float64|, max |ap - float64|) over a configuration's rows, no element left out."""
    e_sp = max(float(np.abs(np.log(np.asarray(g, np.float64)) - np.log(c["sp64"])).max(initial=0.0))
               for c, g in zip(rows, got_sp))
    e_ap = max((float(np.abs(np.asarray(g, np.float64) - c["ap64"]).max(initial=0.0))
                for c, g in zip(rows, got_ap) if c["ap"] is not None), default=0.0)
    return e_sp, e_ap


def yardsticks(cfg):
    rows = cases(cfg)
    return deviations(rows, [c["sp32"] for c in rows], [c["ap32"] for c in rows])
