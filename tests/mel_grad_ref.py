"""Test helper: float64 restatement of the mel front end's backward, and the torch CPU autograd
of the oracle's own arithmetic in float64 (a second, independent derivation) and float32 (the yardstick the GPU
kernel's error is measured against).

Notation of csrc/mel.hip and oracle/mel_ref.py: N = 1024, w the periodic Hann window, xp the wave reflect-padded by
512, F[k, m] the HTK filterbank.  For source frame t: X_t = rfft(w * xp[t hop : t hop + N]), P = |X|^2, M = F^T P,
out = M or (log(eps + M) - mean) / std.  Given G = dL/dout:  dM = G or G / (std (eps + M));  dP = F dM;
u_t[j] = Re sum_{k=0}^{512} 2 dP[k] X[k] exp(+2 pi i j k / N);  d xp[t hop + j] += w[j] u_t[j];  the reflect padding
is transposed by adding every padded position's gradient to the sample it mirrors.
"""
import numpy as np

from oracle import mel_ref

N_FFT = 1024


def _filterbank(sample_rate=24000, n_mels=80, f_min=0.0, f_max=None, **_unused):
    f_max = float(sample_rate // 2) if f_max is None else float(f_max)
    return mel_ref.mel_filterbank(N_FFT // 2 + 1, float(f_min), f_max, n_mels, sample_rate)


def valid_frames(n_samples, hop, frame_start=0, out_frames=None):
    """Output positions t that show a source frame (t + frame_start < 1 + n // hop) of a row of n_samples, and those
    source frames.  A row of at most 512 samples has none."""
    n_valid = mel_ref.num_frames(n_samples, hop) if n_samples > N_FFT // 2 else 0
    frame_start = max(int(frame_start), 0)
    if out_frames is None:
        out_frames = max(n_valid - frame_start, 0)
    t = np.arange(out_frames)
    t = t[t + frame_start < n_valid]
    return t, t + frame_start


def mel_backward(x, grad_out, log=True, frame_start=0, hop_length=300, **params):
    """d L / d x (float64, shape of x) for grad_out (n_mels, out_frames) = d L / d out, where output frame t is source
    frame t + frame_start.  Values of grad_out at padded positions are never read (they may be NaN)."""
    x = np.asarray(x, dtype=np.float64)
    g = np.asarray(grad_out, dtype=np.float64)
    n, hop = x.shape[0], int(hop_length)
    t_out, t_src = valid_frames(n, hop, frame_start, g.shape[1])
    if t_src.size == 0:
        return np.zeros(n)
    fb = _filterbank(**params)                                   # (513, n_mels)
    w = mel_ref.hann_window(N_FFT)
    pos = t_src[:, None] * hop + np.arange(N_FFT)[None, :]       # padded positions of every frame
    spec = np.fft.rfft(x[mel_ref.reflect_index(pos - N_FFT // 2, n)] * w[None, :], axis=1)
    d_mel = g[:, t_out].T                                        # (frames, n_mels)
    if log:
        mel = (spec.real ** 2 + spec.imag ** 2) @ fb
        d_mel = d_mel / (mel_ref.MEL_STD * (mel_ref.LOG_EPS + mel))
    y = (d_mel @ fb.T) * spec                                    # Hermitian spectrum of u / 2 ...
    y[:, 0] = 2.0 * y[:, 0].real                                 # ... whose two real bins count once in irfft
    y[:, -1] = 2.0 * y[:, -1].real
    u = np.fft.irfft(y, n=N_FFT, axis=1) * N_FFT                 # unnormalised inverse real transform
    d_pad = np.zeros(n + N_FFT)
    np.add.at(d_pad, pos, u * w[None, :])
    d_x = np.zeros(n)
    np.add.at(d_x, mel_ref.reflect_index(np.arange(n + N_FFT) - N_FFT // 2, n), d_pad)
    return d_x


def logmel_autograd(x, dtype, log=True, hop_length=300, **params):
    """(n_mels, 1 + n // hop) mel power or normalised log-mel of the torch tensor ``x`` through ``torch.stft`` and the
    dense filterbank on the CPU in ``dtype``, with autograd: the oracle's arithmetic, differentiable."""
    import torch
    spec = torch.stft(x.to(dtype), N_FFT, int(hop_length), N_FFT, torch.hann_window(N_FFT, dtype=dtype), center=True,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    power = spec.real ** 2 + spec.imag ** 2
    mel = torch.as_tensor(_filterbank(**params), dtype=dtype).T @ power
    return (torch.log(mel_ref.LOG_EPS + mel) - mel_ref.MEL_MEAN) / mel_ref.MEL_STD if log else mel


def autograd_grad(x, grad_out, dtype, log=True, frame_start=0, **params):
    """d L / d x as a float64 array by torch CPU autograd in ``dtype`` (float64: the second derivation; float32: the
    yardstick), with the semantics of :func:`mel_backward`."""
    import torch
    xt = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    out = logmel_autograd(xt, dtype, log=log, **params)
    g = np.asarray(grad_out, dtype=np.float64)
    t_out, t_src = valid_frames(xt.shape[0], params.get("hop_length", 300), frame_start, g.shape[1])
    if t_src.size == 0:
        return np.zeros(xt.shape[0])
    gt = torch.as_tensor(g[:, t_out], dtype=dtype)
    (out[:, torch.as_tensor(t_src)] * gt).sum().backward()
    return xt.grad.double().numpy()


def yardstick32(x, grad_out, **kw):
    """The float32 CPU autograd gradient: what the reference's own arithmetic gives when differentiated."""
    import torch
    return autograd_grad(x, grad_out, torch.float32, **kw)


def rel_err(g, g64):
    """max |g - g64| relative to the row's largest |g64|."""
    g64 = np.asarray(g64, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(g, dtype=np.float64) - g64)) / np.max(np.abs(g64)))
