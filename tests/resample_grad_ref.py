"""Float64 restatement of the resampler's backward (TEST INFRASTRUCTURE ONLY): the exact transpose of
``oracle.resample_ref.resample`` in the index form of csrc/resample.hip.

For a row at the reduced ratio ``orig -> new`` with ``width``, ``taps = 2 width + orig`` and the table ``k[p][i]`` the
forward is ``y[j new + p] = sum_i k[p][i] x[j orig - width + i]``, so for an input sample ``q`` in ``[0, n_in)``

    dx[q] = sum_{j = jlo .. jhi} sum_{p < new, j new + p < n_out} k[p][q + width - j orig] * dy[j new + p]
    jlo = max(0, ceil((q + width - taps + 1) / orig)),  jhi = floor((q + width) / orig).

Besides ``dx`` it returns, per sample, ``T_q = sum |k dy|`` and the number of terms ``K_q``: a float32 ``fmaf`` chain
over float32 taps stays within ``(K_q + 2) 2^-24 T_q`` of ``dx`` (K_q roundings of the chain, one of the tap, one of
slack for the second-order term)."""
import numpy as np

from oracle.resample_ref import sinc_resample_kernel


def resample_backward(dy, orig_freq: int, new_freq: int, n_in: int, lowpass_filter_width: int = 6,
                      rolloff: float = 0.99):
    """``(dx, T, K)`` for one row: ``dy`` the ``n_out <= ceil(new n_in / orig)`` output gradients, ``dx`` float64
    (n_in,), ``T`` float64 (n_in,), ``K`` int64 (n_in,)."""
    dy = np.asarray(dy, dtype=np.float64).reshape(-1)
    n_in, n_out = int(n_in), dy.shape[0]
    if orig_freq == new_freq:
        assert n_out <= n_in
        dx = np.zeros(n_in)
        dx[:n_out] = dy
        return dx, np.abs(dx), (np.arange(n_in) < n_out).astype(np.int64)
    k, width, orig, new = sinc_resample_kernel(orig_freq, new_freq, lowpass_filter_width, rolloff)
    taps = k.shape[1]
    assert n_out <= -(-n_in * new // orig)
    q = np.arange(n_in, dtype=np.int64)
    jhi = (q + width) // orig
    jlo = np.maximum(0, -(-(q + width - taps + 1) // orig))
    dx, T, K = np.zeros(n_in), np.zeros(n_in), np.zeros(n_in, np.int64)
    dyp = np.concatenate([dy, np.zeros(1)])                # index n_out: the masked terms
    for d in range(int((jhi - jlo).max(initial=-1)) + 1):  # the d-th period of every sample, ascending j
        j = jlo + d
        i = q + width - j * orig
        live = j <= jhi
        i = np.where(live, i, 0)
        for p in range(new):
            n = j * new + p
            on = live & (n < n_out)
            term = np.where(on, k[p, i] * dyp[np.where(on, n, n_out)], 0.0)
            dx += term
            T += np.abs(term)
            K += on
    return dx, T, K
