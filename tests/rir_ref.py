"""Float64 NumPy restatement of ``csrc/rir_synth.hip``: the image-source response of a shoebox room (Allen & Berkley
1979 with a windowed-sinc fractional delay, accumulated on the 2^-44 fixed-point grid), Schroeder's decay time, and the
bisection of a uniform wall coefficient towards a decay time.  Written from the definition in DESIGN.md section 20;
the reference project has no such code.

A room is a dict ``{"dims", "source", "mic", "beta", "n_samples"}``; ``beta`` is a scalar or six values
``[x0, x1, y0, y1, z0, z1]`` (wall at coordinate 0, wall at ``L``)."""
import math

import numpy as np

HALF = 41
FIX = 2.0 ** 44


def betas(beta) -> np.ndarray:
    b = np.asarray(beta, dtype=np.float64).reshape(-1)
    return np.full(6, b[0]) if b.size == 1 else b.reshape(6)


def _axis(L, s, r, dmax):
    """Every (n, p) of one axis whose |R| can stay within dmax: R, |n - p|, |n|."""
    n = np.arange(math.floor((r - dmax) / (2 * L)) - 2, math.ceil((r + dmax) / (2 * L)) + 3)
    n = np.repeat(n, 2)
    p = np.tile([0, 1], n.size // 2)
    R = (1 - 2 * p) * s + 2.0 * n * L - r
    keep = np.abs(R) <= dmax
    return R[keep], np.abs(n - p)[keep], np.abs(n)[keep]


def taps(A, tau, N, acc, K):
    """Adds the taps of images (A, tau) into the int64 sums ``acc`` and the counts ``K``."""
    m = np.floor(tau).astype(np.int64)
    for j in range(-HALF, HALF + 1):
        k = m + j
        x = k - tau
        ok = (np.abs(x) < HALF) & (k >= 0) & (k < N)
        if not np.any(ok):
            continue
        xs = x[ok]
        v = A[ok] * np.sinc(xs) * 0.5 * (1.0 + np.cos(np.pi * xs / HALF))
        np.add.at(acc, k[ok], np.rint(FIX * v).astype(np.int64))
        np.add.at(K, k[ok], 1)


def finish(acc) -> np.ndarray:
    return (acc.astype(np.float64) * (1.0 / FIX)).astype(np.float32)


def image_source(room, fs, c=343.0, max_order=None):
    """``(h float32, K int64, acc int64)``: the response, the number of contributions to each sample and the integer
    sums."""
    L, s, r = (np.asarray(room[k], dtype=np.float64) for k in ("dims", "source", "mic"))
    b, N = betas(room["beta"]), int(room["n_samples"])
    dmax = (N + HALF) * c / fs
    acc, K = np.zeros(N, np.int64), np.zeros(N, np.int64)
    axes = [_axis(L[a], s[a], r[a], dmax) for a in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = [np.power(b[2 * a], axes[a][1].astype(np.float64)) * np.power(b[2 * a + 1], axes[a][2].astype(np.float64))
             for a in range(3)]
    o = [axes[a][1] + axes[a][2] for a in range(3)]
    Ry2, Rz2 = axes[1][0] ** 2, axes[2][0] ** 2
    yz2 = Ry2[:, None] + Rz2[None, :]
    gyz, oyz = g[1][:, None] * g[2][None, :], o[1][:, None] + o[2][None, :]
    for i, Rx in enumerate(axes[0][0]):
        d = np.sqrt(Rx * Rx + yz2)
        tau = d * fs / c
        A = g[0][i] * gyz / (4.0 * np.pi * d)
        ok = (A != 0.0) & (tau < N + HALF)
        if max_order is not None:
            ok &= (o[0][i] + oyz) <= int(max_order)
        if np.any(ok):
            taps(A[ok], tau[ok], N, acc, K)
    return finish(acc), K, acc


def image_source_brute(room, fs, c=343.0, max_order=2, reach=4):
    """The same by a triple loop over the images, scalar arithmetic: ``max_order <= reach - 1``."""
    assert max_order is not None and max_order < reach
    L, s, r = (np.asarray(room[k], dtype=np.float64).tolist() for k in ("dims", "source", "mic"))
    b, N = betas(room["beta"]).tolist(), int(room["n_samples"])
    acc = [0] * N
    rng = range(-reach, reach + 1)
    for nx in rng:
        for ny in rng:
            for nz in rng:
                for q in range(8):
                    n, p = (nx, ny, nz), (q & 1, (q >> 1) & 1, (q >> 2) & 1)
                    if sum(abs(n[a] - p[a]) + abs(n[a]) for a in range(3)) > max_order:
                        continue
                    R = [(1 - 2 * p[a]) * s[a] + 2 * n[a] * L[a] - r[a] for a in range(3)]
                    d = math.sqrt(R[0] ** 2 + R[1] ** 2 + R[2] ** 2)
                    tau = d * fs / c
                    A = 1.0
                    for a in range(3):
                        A *= (b[2 * a] ** abs(n[a] - p[a])) * (b[2 * a + 1] ** abs(n[a]))     # Python: 0.0 ** 0 == 1.0
                    A /= 4.0 * math.pi * d
                    if A == 0.0 or tau >= N + HALF:
                        continue
                    for k in range(max(0, math.floor(tau) - HALF), min(N, math.floor(tau) + HALF + 2)):
                        x = k - tau
                        if abs(x) < HALF:
                            sinc = 1.0 if x == 0.0 else math.sin(math.pi * x) / (math.pi * x)
                            acc[k] += int(np.rint(FIX * (A * sinc * 0.5 * (1.0 + math.cos(math.pi * x / HALF)))))
    return finish(np.asarray(acc, dtype=np.int64))


def schroeder(h, fs, lo_db=-5.0, hi_db=-25.0, margin=None) -> dict:
    """``{t60, slope, intercept, k_lo, k_hi, db_last, db}`` of one response.  ``margin``: asserts that the decay curve
    stays that many dB away from both thresholds at the indices that decide ``k_lo`` and ``k_hi``."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    N = h.size
    E = np.cumsum((h * h)[::-1])[::-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        db = 10.0 * np.log10(E / E[0])
    below_lo, below_hi = np.nonzero(db < lo_db)[0], np.nonzero(db < hi_db)[0]
    k_lo = int(below_lo[0]) if below_lo.size else N
    k_hi = int(below_hi[0]) if below_hi.size else N
    if margin is not None:
        for k, thr in ((k_lo, lo_db), (k_hi, hi_db)):
            for at in (k - 1, k):
                if 0 <= at < N:
                    assert abs(db[at] - thr) >= margin, (at, db[at], thr)
    out = dict(t60=float("nan"), slope=float("nan"), intercept=float("nan"), k_lo=k_lo, k_hi=k_hi,
               db_last=float(db[-1]), db=db)
    if k_hi < N and k_hi - k_lo >= 2:
        slope, intercept = np.polyfit(np.arange(k_lo, k_hi) / fs, db[k_lo:k_hi], 1)
        out.update(t60=float(-60.0 / slope), slope=float(slope), intercept=float(intercept))
    return out


def eyring_beta(dims, t60) -> float:
    Lx, Ly, Lz = (float(v) for v in dims)
    V, S = Lx * Ly * Lz, 2.0 * (Lx * Ly + Ly * Lz + Lx * Lz)
    return math.sqrt(math.exp(-0.161 * V / (S * float(t60))))


def calibrate(room, t60, fs, rtol=0.02, max_iter=20, tail=1.5, c=343.0, measure=None):
    """``(beta, measured t60, path)``: bisection of a uniform beta in [0, 0.9999] from Eyring's value, the length
    ``ceil(tail t60 fs)`` held fixed.  A response that never reaches -25 dB counts as too long, any other NaN as too
    short.  ``path``: ``(beta, measured)`` of every step.  ``measure(room) -> (t60, k_hi)``: default this module's."""
    N = int(math.ceil(tail * t60 * fs))
    if measure is None:
        def measure(rm):
            m = schroeder(image_source(rm, fs, c)[0], fs)
            return m["t60"], m["k_hi"]
    lo, hi = 0.0, 0.9999
    beta = min(max(eyring_beta(room["dims"], t60), lo), hi)
    path = []
    for _ in range(int(max_iter)):
        got, k_hi = measure(dict(room, beta=beta, n_samples=N))
        path.append((beta, got))
        if abs(got - t60) <= rtol * t60:
            return beta, got, path
        too_long = k_hi >= N if math.isnan(got) else got > t60
        if too_long:
            hi = beta
        else:
            lo = beta
        beta = 0.5 * (lo + hi)
    raise ValueError(f"calibrate: {max_iter} steps did not reach {t60} s within {rtol}")
