"""Restatement of the build-defined transform codec ("ptc") and of G.711 mu-law (``pitchextractor_amd/codec.py``,
``csrc/codec.hip``) in numpy: the MDCT and IMDCT as direct sums in float64 (and in float32, the
accuracy yardstick), the quantiser in float32 and integers exactly as the kernel does it, mu-law in integers.  Nothing
here is imported from the package."""
from __future__ import annotations

import math

import numpy as np

FRAMES = (256, 512, 1024)
Q_MAX = 8388607
TABLE = 448
ZERO_BAND = 2.0 ** -100
G_MAX = 255
_C3 = np.array([2.0 ** -0.75, 2.0 ** -0.5, 2.0 ** -0.25]).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ parameters
def default_bandwidth(sr, bitrate_kbps) -> float:
    return min(float(sr) / 2.0, 4000.0 * (float(bitrate_kbps) / 16.0) ** 0.75)


def cutoff_bin(sr, M, bandwidth_hz) -> int:
    return min(M, int(math.ceil(float(bandwidth_hz) * M / (float(sr) / 2.0))))


def budget_bits(sr, M, bitrate_kbps) -> int:
    return int(math.floor(1000.0 * float(bitrate_kbps) * M / float(sr)))


def band_edges(M: int) -> np.ndarray:
    e = [0]
    while e[-1] < M:
        e.append(min(M, e[-1] + max(4, 4 * (e[-1] // 32))))
    return np.asarray(e, dtype=np.int64)


def bands_below(M: int, k_c: int) -> int:
    return int(np.sum(band_edges(M)[:-1] < k_c))


def n_frames(n: int, M: int) -> int:
    return 0 if n <= 0 else -(-n // M) + 1


def step_tables():
    i = np.arange(TABLE, dtype=np.float64)
    return (2.0 ** ((i - 224) / 4)).astype(np.float32), (2.0 ** (-(i - 224) / 4)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ transform
def window(M: int, dtype=np.float64) -> np.ndarray:
    return np.sin(np.pi * (np.arange(2 * M, dtype=np.float64) + 0.5) / (2 * M)).astype(dtype)


def basis(M: int) -> np.ndarray:
    """cos(pi / M (j + 0.5 + M / 2)(k + 0.5)), float64, shape (2M, M)."""
    j = np.arange(2 * M, dtype=np.float64)[:, None]
    k = np.arange(M, dtype=np.float64)[None, :]
    return np.cos(np.pi / M * (j + 0.5 + M / 2) * (k + 0.5))


def frames_of(x: np.ndarray, M: int) -> np.ndarray:
    """(F, 2M): frame f holds x~[(f - 1) M + j], x~ zero outside the row."""
    n = x.size
    F = n_frames(n, M)
    pad = np.zeros((F + 1) * M, dtype=x.dtype)
    pad[M:M + n] = x
    return np.stack([pad[f * M:f * M + 2 * M] for f in range(F)]) if F else np.zeros((0, 2 * M), x.dtype)


def _direct(a: np.ndarray, b: np.ndarray, dtype) -> np.ndarray:
    """a @ b; in float32 as a plain running sum in index order, every product and sum rounded to float32."""
    if dtype == np.float64:
        return a @ b
    a, b = a.astype(np.float32), b.astype(np.float32)
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for j in range(a.shape[1]):
        acc = (acc + a[:, j:j + 1] * b[j:j + 1, :]).astype(np.float32)
    return acc


def mdct(x, M: int, dtype=np.float64) -> np.ndarray:
    """(F, M) coefficients of a row, direct sums in ``dtype``."""
    x = np.asarray(x).astype(dtype)
    z = (frames_of(x, M) * window(M, dtype)[None, :]).astype(dtype)
    return _direct(z, basis(M), dtype)


def imdct(X, n: int, M: int, dtype=np.float64) -> np.ndarray:
    """The n samples of a row from its (F, M) coefficients: second half of frame t // M plus first half of the next."""
    X = np.asarray(X).astype(dtype)
    F = X.shape[0]
    if F == 0:
        return np.zeros(0, dtype)
    y = (_direct(X, basis(M).T.copy(), dtype) * dtype(2.0 / M)).astype(dtype)
    y = (y * window(M, dtype)[None, :]).astype(dtype)
    out = (y[:-1, M:] + y[1:, :M]).astype(dtype).reshape(-1)
    return out[:n]


# ------------------------------------------------------------------------------------------------------------ quantiser
def scale_index(a: np.float32) -> int:
    """floor(4 log2 a) of a float32 a >= 2^-100 from its bits."""
    m, e = np.frexp(np.float32(a))
    return 4 * (int(e) - 1) + int(np.sum(_C3 <= np.float32(m)))


def _coef_bits(q: np.ndarray) -> np.ndarray:
    a = np.abs(q.astype(np.int64)) + 1
    lg = np.zeros_like(a)
    for s in range(1, 25):
        lg += (a >> s) > 0
    return np.where(q == 0, 1, 2 * lg + 2)


def quantize_at(X, M: int, k_c: int, g: int):
    """``(q, deq, bits)`` of one frame at the global gain index g (no budget)."""
    T, R = step_tables()
    X = np.asarray(X, dtype=np.float32).copy()
    X[k_c:] = 0
    e = band_edges(M)
    q = np.zeros(M, np.int32)
    deq = np.zeros(M, np.float32)
    bits = 8
    for b in range(len(e) - 1):
        lo, hi = int(e[b]), min(int(e[b + 1]), k_c)
        if lo >= k_c:
            break
        a = np.float32(np.max(np.abs(X[lo:hi])))
        if not a >= np.float32(ZERO_BAND):
            bits += 1
            continue
        s = scale_index(a)
        i = min(g + (2 * s) // 5 + 160, TABLE - 1)            # Python's // is the floor division
        v = np.rint((X[lo:hi] * R[i]).astype(np.float32))
        qb = np.clip(v, -Q_MAX, Q_MAX).astype(np.int32)
        q[lo:hi] = qb
        deq[lo:hi] = (qb.astype(np.float32) * T[i]).astype(np.float32)
        bits += 1 if not qb.any() else 7 + int(_coef_bits(qb).sum())
    return q, deq, bits


def quantize(X, M: int, k_c: int, budget: int):
    """``(q, g, bits, deq)`` of one frame: the smallest g in [0, 255] that fits; nothing fits: g = 255, all zero."""
    lo, hi = 0, G_MAX
    while lo < hi:
        mid = (lo + hi) // 2
        if quantize_at(X, M, k_c, mid)[2] <= budget:
            hi = mid
        else:
            lo = mid + 1
    q, deq, bits = quantize_at(X, M, k_c, lo)
    if bits > budget:
        q[:], deq[:], bits = 0, 0, 8 + bands_below(M, k_c)
    return q, lo, bits, deq


def quantize_frames(X, M, k_c, budget):
    X = np.asarray(X, dtype=np.float32).reshape(-1, M)
    out = [quantize(f, M, k_c, budget) for f in X]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32),
            np.array([o[2] for o in out], np.int32), np.stack([o[3] for o in out]))


def codec(x, sr, bitrate_kbps, M=1024, bandwidth_hz=None, bypass=False, dtype=np.float64):
    """The whole chain on one row: float64 transforms around the float32 quantiser.  Returns ``(y, g, bits)``."""
    x = np.asarray(x)
    bw = default_bandwidth(sr, bitrate_kbps) if bandwidth_hz is None else bandwidth_hz
    k_c, budget = cutoff_bin(sr, M, bw), budget_bits(sr, M, bitrate_kbps)
    X = mdct(x, M, dtype)
    if bypass or X.shape[0] == 0:
        return imdct(X, x.size, M, dtype), None, None
    _, g, bits, deq = quantize_frames(X.astype(np.float32), M, k_c, budget)
    return imdct(deq.astype(dtype), x.size, M, dtype), g, bits


# --------------------------------------------------------------------------------------------------------------- mu-law
def mulaw(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    p = np.clip(np.rint((x * np.float32(32768)).astype(np.float32)), -32768, 32767).astype(np.int64)
    m = np.minimum(np.abs(p), 32635) + 132
    e = np.floor(np.log2(m.astype(np.float64))).astype(np.int64) - 7
    mant = (m >> (e + 3)) & 15
    v = (((mant << 3) + 132) << e) - 132
    return (np.sign(p) * v).astype(np.float32) / np.float32(32768)


def mulaw_table() -> np.ndarray:
    """Brute force over all 65536 p: per segment, the 16 steps by their thresholds."""
    out = np.zeros(65536, np.int64)
    for p in range(-32768, 32768):
        m = min(abs(p), 32635) + 132
        e = 0
        while (256 << e) <= m:
            e += 1
        mant = (m - (128 << e)) // (8 << e)
        v = (mant * 8 + 132) * (1 << e) - 132
        out[p + 32768] = v if p > 0 else -v
    return out


def vibrato_complex(sr=24000, seconds=1.0, f0=220.0, depth=0.03, rate=5.5, harmonics=10) -> np.ndarray:
    t = np.arange(int(sr * seconds), dtype=np.float64) / sr
    phase = 2 * np.pi * (f0 * t - f0 * depth / (2 * np.pi * rate) * (np.cos(2 * np.pi * rate * t) - 1))
    x = sum(np.sin(h * phase) / h for h in range(1, harmonics + 1))
    return (0.5 * x / np.max(np.abs(x))).astype(np.float32)
