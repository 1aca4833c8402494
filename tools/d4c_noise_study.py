"""Where float32 costs D4C's band values: a CPU study with the restatements of tests/d4c_ref.py (no GPU).

The kernel of csrc/d4c.hip is held to 4 x the float32 restatement's deviation from the float64 one.  Its first version
measured 5.2 x at 48 kHz, on the F0 = 1000 Hz row, and 2.8 - 3.5 x elsewhere.  This tool finds the stage.  It prints, for
the rows of tests/d4c_cases.py at one rate, the largest |coarse - float64| in dB of

  plain        the float32 restatement as it is (numpy sums in float32 are pairwise; scipy's float32 transforms);
  round <s>    the float64 pipeline with ONE float32 rounding injected after stage <s>: what a stage's output costs
               when everything before and after it is exact;
  packed       the float32 restatement with the kernel's two-to-one transforms (a centroid's wave and its ramped copy,
               two bands) as one complex64 transform each;
  running      ... and the interval sums of the linear smoothing as float32 running sums, term after term, as the
               kernel's first version had them;
  double       ... and those sums accumulated in double and rounded once, as the kernel has them now.

Measured (48 kHz, F0 = 1000 Hz row; float64 of the same row as the reference): plain 2.3e-4 dB, packed 4.0e-4, running
9.7e-4 (the first kernel measured 1.19e-3 on the device), double 2.3e-4 (the kernel now: 4.3e-4).  One rounding of the
group delay's first smoothing alone costs 4.9e-5, the largest of the single roundings: its second smoothing is
subtracted from it, and at 1000 Hz each interval sum has 85 terms.

    python tools/d4c_noise_study.py [--fs 48000]
"""
import argparse
import math
import sys
from pathlib import Path

import numpy as np
import scipy.fft

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tests import cheaptrick_ref as ct  # noqa: E402
from tests import d4c_cases as dc  # noqa: E402
from tests import d4c_ref as d4  # noqa: E402

ORIG = {"centroid": d4.centroid, "coarse": d4.coarse_aperiodicity, "smooth": d4.smooth}


def _split(Z, N):
    k = np.arange(N // 2 + 1)
    zc = np.conj(Z[(N - k) % N])
    return (Z[k] + zc) * np.complex64(0.5), (Z[k] - zc) * np.complex64(-0.5j)


def packed_centroid(x, fs, f0, position, N, fp32=False):
    if not fp32:
        return ORIG["centroid"](x, fs, f0, position, N, fp32)
    ft = np.float32
    w = d4.windowed(x, fs, f0, position, 4.0, True, ft)[:N]
    ss = np.sum(w * w, dtype=ft)
    w = (w * (ft(1) / np.sqrt(ss))).astype(ft) if ss > 0 else np.zeros_like(w)
    p2 = int(w.size).bit_length()
    z = np.zeros(N, np.complex64)
    z[:w.size] = w + 1j * (w * ((np.arange(w.size) + 1).astype(ft) * ft(2.0 ** -p2))).astype(ft)
    X, Y = _split(scipy.fft.fft(z), N)
    return ((X.real * Y.real + X.imag * Y.imag) * ft(2.0 ** p2)).astype(ft)


def packed_coarse(g, fs, N, bands, L, fp32=False):
    if not fp32:
        return ORIG["coarse"](g, fs, N, bands, L, fp32)
    ft = np.float32
    win, hl, bw = d4.nuttall(L, ft), L // 2, d4.matlab_round(8.0 * N / L)
    out = np.zeros(bands)
    for b in range(0, bands, 2):
        z = np.zeros(N, np.complex64)
        ca, cb = (int(d4.INTERVAL * (b + i) * N / fs) for i in (1, 2))
        z[:L] = g[ca - hl:ca + hl + 1].astype(ft) * win
        if b + 1 < bands:
            z[:L] += 1j * (g[cb - hl:cb + hl + 1].astype(ft) * win)
        for a, sp in enumerate(_split(scipy.fft.fft(z), N)[:min(2, bands - b)]):
            S = np.cumsum(np.sort((sp.real ** 2 + sp.imag ** 2).astype(ft)), dtype=ft)
            if S[N // 2] > 0:
                out[b + a] = max(float(ft(10) * np.log10(S[N // 2 - bw - 1] / S[N // 2])), d4.COARSE_FLOOR)
    return out


def smooth_as(mode):
    """The float32 interval sum with a running float32 sum (``running``) or a double accumulator (``double``)."""
    def smooth(P, h, N):
        ft = P.dtype.type
        if ft is np.float64:
            return ORIG["smooth"](P, h, N)
        H = N // 2
        h = ft(h)
        hi = int(math.floor(h))
        hf = ft(h - ft(hi))
        lo_down, up = hf > ft(0.5), hf >= ft(0.5)
        ka, kb = -hi - (1 if lo_down else 0), hi + (1 if up else 0)
        wa = ft(1.0) - (ft(1.5) - hf if lo_down else ft(0.5) - hf)
        wb = hf - ft(0.5) if up else ft(0.5) + hf
        k = np.arange(H + 1)
        if ka == kb:
            return P[ct._mirror(k + ka, N)]
        vals = P[ct._mirror(k[:, None] + np.arange(ka + 1, kb)[None, :], N)]
        lo, hi_ = P[ct._mirror(k + ka, N)], P[ct._mirror(k + kb, N)]
        if mode == "running":
            s = (wa * lo).astype(ft)
            if vals.shape[1]:
                s = (s + np.cumsum(vals, axis=1, dtype=ft)[:, -1]).astype(ft)
            return ((s + wb * hi_).astype(ft) / (ft(2) * h)).astype(ft)
        s = float(wa) * lo.astype(np.float64) + vals.astype(np.float64).sum(1) + float(wb) * hi_.astype(np.float64)
        return (s / (2.0 * float(h))).astype(ft)
    return smooth


def single_roundings(x, fs, f0, c, frames, fp):
    """Largest |coarse - float64| with one float32 rounding after each stage of the float64 pipeline."""
    N = c["N_d"]
    r32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731

    def run(pos, inj):
        def cen(p):
            w = d4.windowed(x, fs, f0, p, 4.0, True)
            w = w / np.sqrt(np.sum(w * w))
            X, Y = np.fft.rfft(w, N), np.fft.rfft(w * (np.arange(w.size) + 1), N)
            if inj == "centroid transforms":
                X, Y = (r32(v.real) + 1j * r32(v.imag) for v in (X, Y))
            return X.real * Y.real + X.imag * Y.imag
        P = np.abs(np.fft.rfft(d4.windowed(x, fs, f0, pos, 4.0, False), N)) ** 2
        P = r32(P) if inj == "power spectrum" else P
        power = d4.smooth(ct.dc_correction(P, fs, f0, N), f0 * N / (2.0 * fs), N)
        power = r32(power) if inj == "smoothed power" else power
        ce = cen(pos - 0.25 / f0) + cen(pos + 0.25 / f0)
        ce = r32(ce) if inj == "centroid" else ce
        g = ct.dc_correction(ce, fs, f0, N) / power
        g = r32(g) if inj == "group delay" else g
        g1 = d4.smooth(g, f0 * N / (4.0 * fs), N)
        g1 = r32(g1) if inj == "its first smoothing" else g1
        g2 = d4.smooth(g1, f0 * N / (2.0 * fs), N)
        g2 = r32(g2) if inj == "its second smoothing" else g2
        return d4.coarse_aperiodicity(g1 - g2, fs, N, c["bands"], c["L"])
    stages = ("power spectrum", "smoothed power", "centroid transforms", "centroid", "group delay",
              "its first smoothing", "its second smoothing")
    return {s: max(np.abs(run(f * fp / 1000.0, s) - run(f * fp / 1000.0, None)).max() for f in frames) for s in stages}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fs", type=int, default=48000)
    a = ap.parse_args()
    cfg = next(c for c in dc.CONFIGS if c[0] == a.fs)
    fs, fp, thr = cfg
    cases = dc.cases(cfg)

    def report(tag):
        worst = {}
        for name, c in cases.items():
            _, b, _ = d4.d4c(c["x"].astype(np.float64), c["f0"], fs, fp, threshold=thr, fp32=True)
            both = ~np.isnan(b[:, 1]) & ~np.isnan(c["b64"][:, 1])
            if both.any():
                worst[name] = float(np.abs(b[both, 1:] - c["b64"][both, 1:]).max())
        print(f"{tag:8s}", " ".join(f"{k} {v:.2e}" for k, v in worst.items()))

    report("plain")
    c = cases["f0_1000"]
    for stage, v in single_roundings(c["x"].astype(np.float64), fs, 1000.0, d4.constants(fs), range(5, 45, 3), fp).items():
        print(f"round {stage}: f0_1000 {v:.2e}")
    d4.centroid, d4.coarse_aperiodicity = packed_centroid, packed_coarse
    report("packed")
    d4.smooth = smooth_as("running")
    report("running")
    d4.smooth = smooth_as("double")
    report("double")


if __name__ == "__main__":
    main()
