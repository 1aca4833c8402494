"""Float64 restatement of the augmentation cascade (``csrc/augment.hip`` through ``pitchextractor_amd.augment``) and of
its coefficient designers: plain sequential loops and the RBJ cookbook's formulas, written apart from the package.
tests/test_augment_cpu.py holds the loop to ``scipy.signal.sosfilt``; tests/test_augment_gpu.py holds the kernel to it."""
import math

import numpy as np

MAX_POLE_RADIUS = 1.0 - 2.0 ** -12


def cascade(x, sos) -> np.ndarray:
    """``x`` (any float array, widened to float64) through the stages ``sos`` (S, 5) of ``{b0, b1, b2, a1, a2}`` in
    transposed direct form II from a zero state, stage after stage, in float64 throughout."""
    y = np.asarray(x, dtype=np.float64).copy()
    for b0, b1, b2, a1, a2 in np.asarray(sos, dtype=np.float64).reshape(-1, 5):
        z1 = z2 = 0.0
        for i in range(y.size):
            v = float(y[i])
            o = b0 * v + z1
            z1 = b1 * v - a1 * o + z2
            z2 = b2 * v - a2 * o
            y[i] = o
    return y


def cascade_f32(x, sos) -> np.ndarray:
    """The kernel's result: ``cascade`` rounded once to float32."""
    return cascade(x, sos).astype(np.float32)


def magnitude_db(stage, sr, f) -> float:
    """20 log10 |H(exp(2 pi i f / sr))| of one stage, in float64 from its coefficients."""
    b0, b1, b2, a1, a2 = (float(v) for v in stage)
    z = np.exp(-2j * math.pi * f / sr)
    return 20.0 * math.log10(abs((b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)))


def pole_radius(stage) -> float:
    return float(np.max(np.abs(np.roots([1.0, float(stage[3]), float(stage[4])]))))


def _parts(sr, f, Q, gain_db=0.0):
    w0 = 2.0 * math.pi * f / sr
    return math.cos(w0), math.sin(w0) / (2.0 * Q), 10.0 ** (gain_db / 40.0)


def _norm(b, a):
    return np.array([b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]], dtype=np.float64)


def lowpass(sr, f, Q):
    c, al, _ = _parts(sr, f, Q)
    return _norm([(1 - c) / 2, 1 - c, (1 - c) / 2], [1 + al, -2 * c, 1 - al])


def highpass(sr, f, Q):
    c, al, _ = _parts(sr, f, Q)
    return _norm([(1 + c) / 2, -(1 + c), (1 + c) / 2], [1 + al, -2 * c, 1 - al])


def peaking(sr, f, gain_db, Q):
    c, al, A = _parts(sr, f, Q, gain_db)
    return _norm([1 + al * A, -2 * c, 1 - al * A], [1 + al / A, -2 * c, 1 - al / A])


def lowshelf(sr, f, gain_db, Q):
    c, al, A = _parts(sr, f, Q, gain_db)
    k = 2 * math.sqrt(A) * al
    return _norm([A * ((A + 1) - (A - 1) * c + k), 2 * A * ((A - 1) - (A + 1) * c), A * ((A + 1) - (A - 1) * c - k)],
                 [(A + 1) + (A - 1) * c + k, -2 * ((A - 1) + (A + 1) * c), (A + 1) + (A - 1) * c - k])


def highshelf(sr, f, gain_db, Q):
    c, al, A = _parts(sr, f, Q, gain_db)
    k = 2 * math.sqrt(A) * al
    return _norm([A * ((A + 1) + (A - 1) * c + k), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - k)],
                 [(A + 1) - (A - 1) * c + k, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - k])
