"""NumPy restatement of the F0 bin decoders and the pitch metrics (float64 by default).

Written from the definition, not from the kernels (same role as ``pitch_shift_ref.py`` / ``split_ref.py``):

* bins: ``cents(b) = 20 b + 1997.3794084376191``, ``f(b) = 10 * 2^(cents(b) / 1200)`` (the grid of the bin loss);
* ``argmax``: lowest index among the maxima of a frame;
* ``weighted``: ``sum_w p_c cents(c) / sum_w p_c`` over ``w = [b - 4, b + 4]`` cut at the row ends,
  ``p_c = exp(l_c - l_b)``;
* ``viterbi``: path maximising ``l_0[b_0] + sum_t (log A(b_{t-1}, b_t) + l_t[b_t])``,
  ``A(i, j) = max(band - |i - j|, 0) / sum_j' max(band - |i - j'|, 0)`` with ``band = 12``, uniform prior,
  ties (predecessor and final state) to the lowest index;
* ``confidence = softmax(frame)[bin]``;
* metrics: cents re 55 Hz, as the reference's ``Utils/dynamic_pitch_tools.py:79-104``.

Every function takes ``dtype``: float64 is the reference; float32 is used by the tests only to qualify inputs and
to size tolerances (what plain float32 arithmetic loses against float64 on the same inputs).
"""
from __future__ import annotations

import numpy as np

CENTS0 = 1997.3794084376191
BAND = 12
HALF_WIN = 4
METHODS = ("argmax", "weighted", "viterbi", "weighted_viterbi")


def bin_cents(b, dtype=np.float64):
    return (dtype(20.0) * np.asarray(b).astype(dtype) + dtype(CENTS0)).astype(dtype)


def cents_to_hz(cents, dtype=np.float64):
    return (dtype(10.0) * np.exp2(np.asarray(cents, dtype=dtype) / dtype(1200.0))).astype(dtype)


def bin_hz(b, dtype=np.float64):
    return cents_to_hz(bin_cents(b, dtype), dtype)


def argmax_bins(logits):
    """(T, C) -> (T,) lowest index of each row's maximum (np.argmax returns the first occurrence)."""
    return np.argmax(np.asarray(logits), axis=-1).astype(np.int64)


def log_transition(C, band=BAND, dtype=np.float64):
    """(C, C) log A, -inf where A = 0; each row normalised by its own sum."""
    i = np.arange(C)
    tri = np.maximum(band - np.abs(i[:, None] - i[None, :]), 0).astype(dtype)
    with np.errstate(divide="ignore"):
        return (np.log(tri) - np.log(tri.sum(axis=1, keepdims=True))).astype(dtype)


def _banded_log_transition(C, band, dtype):
    """(2 band - 1, C): row k holds log A(j + d, j) for d = k - (band - 1), -inf where j + d leaves [0, C)."""
    logA = log_transition(C, band, dtype)
    out = np.full((2 * band - 1, C), -np.inf, dtype=dtype)
    j = np.arange(C)
    for k, d in enumerate(range(-(band - 1), band)):
        ok = (j + d >= 0) & (j + d < C)
        out[k, ok] = logA[j[ok] + d, j[ok]]
    return out


def viterbi_paths(logits, band=BAND, dtype=np.float64, return_delta=False):
    """(N, T, C) -> (N, T) int64 paths of N full-length sequences; un-normalised DP in ``dtype``.  Only the
    predecessors i = j + d with |d| < band can win (all others have A = 0), taken in ascending i, so the first
    maximum is the lowest i.  ``return_delta``: also (N,) max_t max_j |delta_t[j]|."""
    x = np.asarray(logits).astype(dtype)
    N, T, C = x.shape
    w = band - 1
    logA = _banded_log_transition(C, band, dtype)             # (2w + 1, C)
    delta = x[:, 0].copy()
    peak = np.abs(delta).max(axis=1)
    back = np.zeros((N, T, C), dtype=np.int64)
    cols = np.arange(C)
    win = cols[None, :] + np.arange(2 * w + 1)[:, None]       # index into the padded delta: i + w = j + k
    for t in range(1, T):
        pad = np.full((N, C + 2 * w), -np.inf, dtype=dtype)
        pad[:, w:w + C] = delta
        cand = (pad[:, win] + logA[None]).astype(dtype)       # (N, 2w + 1, C)
        k = np.argmax(cand, axis=1)                           # first maximum = lowest i
        back[:, t] = cols[None, :] + k - w
        delta = (np.take_along_axis(cand, k[:, None, :], axis=1)[:, 0] + x[:, t]).astype(dtype)
        peak = np.maximum(peak, np.abs(delta).max(axis=1))
    path = np.zeros((N, T), dtype=np.int64)
    path[:, T - 1] = np.argmax(delta, axis=1)
    rows = np.arange(N)
    for t in range(T - 1, 0, -1):
        path[:, t - 1] = back[rows, t, path[:, t]]
    return (path, peak) if return_delta else path


def viterbi_path(logits, band=BAND, dtype=np.float64, return_delta=False):
    """(T, C) -> (T,) int64 path.  ``return_delta``: also max_t max_j |delta_t[j]| of the un-normalised run."""
    out = viterbi_paths(np.asarray(logits)[None], band, dtype, return_delta)
    return (out[0][0], float(out[1][0])) if return_delta else out[0]


def path_score(logits, path, band=BAND):
    """float64 score of a path under the Viterbi objective (-inf if it uses a forbidden transition)."""
    x = np.asarray(logits, dtype=np.float64)
    logA = log_transition(x.shape[1], band)
    path = np.asarray(path, dtype=np.int64)
    s = x[0, path[0]]
    for t in range(1, len(path)):
        s = s + logA[path[t - 1], path[t]] + x[t, path[t]]
    return float(s)


def confidence(logits, bins, dtype=np.float64):
    x = np.asarray(logits).astype(dtype)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    rows = np.arange(x.shape[0])
    return (e[rows, bins] / e.sum(axis=-1, dtype=dtype)).astype(dtype)


def weighted_cents(logits, bins, dtype=np.float64):
    x = np.asarray(logits).astype(dtype)
    T, C = x.shape
    out = np.zeros(T, dtype=dtype)
    for t in range(T):
        b = int(bins[t])
        lo, hi = max(b - HALF_WIN, 0), min(b + HALF_WIN, C - 1)
        c = np.arange(lo, hi + 1)
        p = np.exp(x[t, lo:hi + 1] - x[t, b]).astype(dtype)
        out[t] = (p * bin_cents(c, dtype)).sum(dtype=dtype) / p.sum(dtype=dtype)
    return out


def decode(logits, method="argmax", length=None, dtype=np.float64, band=BAND):
    """One sequence (T, C) -> (f0_hz (T,), confidence (T,), bins (T,)); entries at t >= length are 0."""
    assert method in METHODS
    x = np.asarray(logits)
    T = x.shape[0]
    L = T if length is None else int(length)
    xs = x[:L]
    bins = viterbi_path(xs, band, dtype) if "viterbi" in method else argmax_bins(xs.astype(dtype))
    cents = weighted_cents(xs, bins, dtype) if method.startswith("weighted") else bin_cents(bins, dtype)
    f0 = np.zeros(T, dtype=dtype)
    conf = np.zeros(T, dtype=dtype)
    out_bins = np.zeros(T, dtype=np.int64)
    f0[:L] = cents_to_hz(cents, dtype)
    conf[:L] = confidence(xs, bins, dtype)
    out_bins[:L] = bins
    return f0, conf, out_bins


def brute_force_best(logits, band=BAND):
    """Enumerate all C^T paths (tiny cases): (best float64 score, the path the tie rule selects among those with
    exactly that score).  Backtracking from the lowest final state through the lowest predecessors yields the path
    that is lowest when read from its END, so the enumeration runs over reversed paths in lexicographic order and
    keeps the first maximum.  ``path_score`` adds in the order the DP does, so equal scores are exactly equal."""
    import itertools
    x = np.asarray(logits, dtype=np.float64)
    T, C = x.shape
    best, arg = -np.inf, None
    for rev in itertools.product(range(C), repeat=T):
        s = path_score(x, rev[::-1], band)
        if s > best:
            best, arg = s, rev[::-1]
    return best, np.asarray(arg, dtype=np.int64)


# ------------------------------------------------------------------ metrics
def hz_to_cents55(f, dtype=np.float64):
    f = np.asarray(f).astype(dtype)
    out = np.zeros_like(f)
    pos = f > 0
    out[pos] = dtype(1200.0) * np.log2(f[pos] / dtype(55.0))
    return out


def pitch_metrics(pred, ref, threshold_cents=50.0, dtype=np.float64):
    """dict(rms_cents, rpa, rca, vuv_error, n_voiced, n_frames) over the first min(len) frames; the inputs are
    float32 tracks (what the device holds), the arithmetic runs in ``dtype``."""
    n = min(len(pred), len(ref))
    p = np.asarray(pred, dtype=np.float32)[:n]
    r = np.asarray(ref, dtype=np.float32)[:n]
    nan = float("nan")
    if n == 0:
        return dict(rms_cents=nan, rpa=nan, rca=nan, vuv_error=nan, n_voiced=0, n_frames=0)
    voiced = r > 0
    nv = int(voiced.sum())
    vuv = float(((p > 0) != voiced).sum() / n)
    if nv == 0:
        return dict(rms_cents=nan, rpa=nan, rca=nan, vuv_error=vuv, n_voiced=0, n_frames=n)
    pv, rv = p[voiced], r[voiced]
    d = hz_to_cents55(np.maximum(pv, np.float32(1e-5)), dtype) - hz_to_cents55(rv, dtype)
    circ = np.mod(d + dtype(600.0), dtype(1200.0)) - dtype(600.0)
    ok = pv > 0
    thr = dtype(threshold_cents)
    return dict(rms_cents=float(np.sqrt(np.mean(d.astype(dtype) ** 2))),
                rpa=float((ok & (np.abs(d) <= thr)).sum() / nv),
                rca=float((ok & (np.abs(circ) <= thr)).sum() / nv),
                vuv_error=vuv, n_voiced=nv, n_frames=n)
