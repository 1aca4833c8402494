"""Float64 references of the kernels that close a training step (``csrc/heads_loss.hip``), of the plain passes at the
bottom of ``csrc/elementwise.hip`` and of the dropout stream.  numpy / torch on the CPU, no device.

Conventions: u = 2^-24 is the unit roundoff of float32.  Every reference returns, next to a value, the magnitude
``mag`` its rounding error scales with (the sum of the absolute values of the terms that were added), so a test can
hold the kernel to ``count * u * mag`` per element.  ``adamw_step_ref`` is a rounding model in the manner of
``half_ref.py`` / ``split_ref.py``: the constants the kernel receives or forms in float32 are formed in float32 here
too, everything after them is float64."""
import numpy as np
import torch

from tests import noise_ref

U = 2.0 ** -24
F32 = np.float32


def _f64(t):
    """float64 numpy array of a tensor or array (the float32 values, widened exactly)."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t).astype(np.float64)


# ------------------------------------------------------------------ AdamW
def adamw_constants(lr, beta1, beta2, eps, wd, step, grad_scale=1.0, exact_bias_correction=False):
    """The constants of one step as float64 numbers holding the kernel's float32 values.

    ``lr, beta1, beta2, eps, wd, grad_scale`` are rounded to float32 (the C ABI takes ``float``); ``decay = 1f - lr wd``,
    ``w1 = 1f - beta1`` and ``w2 = 1f - beta2`` are evaluated in float32 (``adamw_kernel``); the bias corrections are
    the doubles ``1 - beta^step`` of the unrounded betas (``ops.adamw_step``) and ``step_size = float32(lr / bc1)``,
    ``bc2_sqrt = float32(sqrt(bc2))`` (``pe_adamw_step``).  ``exact_bias_correction``: keep those two in double, which
    is ``torch.optim.AdamW`` in float64 when the hyper-parameters are float32 numbers."""
    lr32, b1, b2, eps32, wd32, gs = (F32(x) for x in (lr, beta1, beta2, eps, wd, grad_scale))
    one = F32(1.0)
    bc1 = 1.0 - float(beta1) ** int(step)
    bc2 = 1.0 - float(beta2) ** int(step)
    step_size, bc2_sqrt = float(lr32) / bc1, float(np.sqrt(bc2))
    if not exact_bias_correction:
        step_size, bc2_sqrt = float(F32(step_size)), float(F32(bc2_sqrt))
    return dict(lr=float(lr32), beta1=float(b1), beta2=float(b2), eps=float(eps32), wd=float(wd32),
                grad_scale=float(gs), decay=float(F32(one - F32(lr32 * wd32))), w1=float(F32(one - b1)),
                w2=float(F32(one - b2)), step_size=step_size, bc2_sqrt=bc2_sqrt)


def adamw_step_ref(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, *, exact_bias_correction=False,
                   w2_double=False, coupled=False):
    """One AdamW step from the given ``p, g, m, v``: returns ``(m', v', mag_m, mag_v, param)``.

    ``m' = m + w1 (g - m)``, ``v' = beta2 v + w2 g^2`` with ``g`` the gradient times ``grad_scale``;
    ``mag_m = |m| + |w1 (g - m)|``, ``mag_v = |beta2 v| + w2 g^2``.  ``param(m', v') -> (p', mag_p)`` is the parameter
    update from ANY moments it is handed (the kernel's own stored ones: teacher forcing):
    ``p' = decay p - step_size m' / (sqrt(v') / bc2_sqrt + eps)``, ``mag_p = |decay p| + |step_size m' / denom|``.
    Controls that must miss: ``w2_double`` takes ``1 - beta2`` of the unrounded double ``beta2`` (for 0.98 about
    16 u away from the float32 constant, which is exactly ``1 - float32(beta2)``); ``coupled`` is L2 regularisation
    (the decay enters the gradient, not the parameter)."""
    k = adamw_constants(lr, beta1, beta2, eps, wd, step, grad_scale, exact_bias_correction)
    p, g, m, v = (_f64(t) for t in (p, g, m, v))
    g = g * k["grad_scale"]
    w2 = 1.0 - float(beta2) if w2_double else k["w2"]
    decay = k["decay"]
    if coupled:
        g, decay = g + k["wd"] * p, 1.0
    dm = k["w1"] * (g - m)
    m1 = m + dm
    v1 = k["beta2"] * v + w2 * g * g
    mag_m, mag_v = np.abs(m) + np.abs(dm), np.abs(k["beta2"] * v) + w2 * g * g

    def param(m_new, v_new):
        m_new, v_new = _f64(m_new), _f64(v_new)
        upd = k["step_size"] * (m_new / (np.sqrt(v_new) / k["bc2_sqrt"] + k["eps"]))
        return decay * p - upd, np.abs(decay * p) + np.abs(upd)

    return m1, v1, mag_m, mag_v, param


# ------------------------------------------------------------------ heads
def head_ref(x, w, b, dy):
    """``y[r] = sum_o (x[r] . w[o] + b[o])`` and its gradients: a dict of (value, mag) pairs.

    ``dx[r] = dy[r] sum_o w[o]``; ``dw[o] = sum_r dy[r] x[r]`` and ``db[o] = sum_r dy[r]`` are the same for every
    ``o`` (the output is the plain sum of the logits) and are returned as one row / one number."""
    x, w, b, dy = (_f64(t) for t in (x, w, b, dy))
    y = (x @ w.T + b).sum(1)
    mag_y = (np.abs(x) @ np.abs(w).T).sum(1) + np.abs(b).sum()
    dx = dy[:, None] * w.sum(0)[None, :]
    mag_dx = np.abs(dy)[:, None] * np.abs(w).sum(0)[None, :]
    return dict(y=(y, mag_y), dx=(dx, mag_dx), dw=(dy @ x, np.abs(dy) @ np.abs(x)),
                db=(dy.sum(), np.abs(dy).sum()))


# ------------------------------------------------------------------ losses
def sigmoid64(z):
    z = np.asarray(z, np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bce_terms(z, y):
    """``max(z, 0) - z y + log1p(exp(-|z|))`` per element."""
    return np.maximum(z, 0.0) - z * y + np.log1p(np.exp(-np.abs(z)))


def f0_sil_loss_ref(f0_pred, f0, sil_pred, sil, lambda_f0, grad_scale=1.0, *, beta=1.0, inclusive=False):
    """``lambda SmoothL1(beta = 1, mean) + BCEWithLogits(mean)``, both gradients times ``grad_scale``.

    ``lambda_f0`` and ``grad_scale`` are rounded to float32 first (the C ABI).  Returns a dict: ``total, l1`` (already
    times lambda), ``bce``; ``abs_l1, abs_bce`` = sum |terms| / R of each loss (``abs_l1`` times |lambda|); ``d_f0,
    d_sil``; ``sigma``.  Controls: ``inclusive`` takes the quadratic branch at ``|d| <= beta`` (the same value at
    ``|d| = beta``, so it must agree); another ``beta`` must miss."""
    fp, f, z, y = (_f64(t) for t in (f0_pred, f0, sil_pred, sil))
    lam, gs, R = float(F32(lambda_f0)), float(F32(grad_scale)), fp.size
    d = fp - f
    ad = np.abs(d)
    quad = (ad <= beta) if inclusive else (ad < beta)
    t1 = np.where(quad, 0.5 * d * d / beta, ad - 0.5 * beta)
    t2 = bce_terms(z, y)
    l1, bce = lam * t1.sum() / R, t2.sum() / R
    sig = sigmoid64(z)
    return dict(total=l1 + bce, l1=l1, bce=bce, abs_l1=abs(lam) * np.abs(t1).sum() / R, abs_bce=np.abs(t2).sum() / R,
                d_f0=gs * lam / R * np.where(quad, d / beta, np.sign(d)), d_sil=gs / R * (sig - y), sigma=sig)


# ------------------------------------------------------------------ dropout stream
def dropout_words(seed, offset, n_quads, rounds=10):
    """Philox4x32 words of quads ``offset .. offset + n_quads`` (64-bit counter, wrapping), ``(n_quads, 4)`` uint32."""
    ctr = (np.arange(n_quads, dtype=np.uint64) + np.uint64(int(offset) & 0xFFFFFFFFFFFFFFFF))
    return noise_ref.philox4x32(seed, ctr, rounds=rounds)


def keep_from_words(words, p, strict=False):
    """``keep = float32(word >> 8) 2^-24 >= float32(p)``: ``(n_quads * 4,)`` uint8 in word order.  (``word >> 8`` has 24
    bits, so its float32 and the product with 2^-24 are exact.)  ``strict``: ``>`` (a control)."""
    u = (words >> np.uint32(8)).astype(np.float32) * F32(2.0 ** -24)
    keep = (u > F32(p)) if strict else (u >= F32(p))
    return keep.astype(np.uint8).reshape(-1)


def dropout_keep_ref(seed, offset, n_quads, p, *, strict=False, rounds=10):
    """The keep bytes of ``ops.dropout``: quad ``q`` draws counter ``offset + q`` under key = the two seed halves."""
    return keep_from_words(dropout_words(seed, offset, n_quads, rounds), p, strict)


def dropout_scale(p):
    """``1f / (1f - p)`` in float32, as ``pe_dropout_fwd`` forms it."""
    return F32(1.0) / (F32(1.0) - F32(p))


# ------------------------------------------------------------------ max-pool
def maxpool_ref(x, pool, last=False):
    """``MaxPool2d((1, pool))`` of a channels-last ``[..., F, C]`` array: ``(values, positions)`` over ``F // pool``
    windows (the remainder of ``F`` is ignored).  ``positions`` is the FIRST place of the maximum inside the window
    (``argmax`` over the window axis; +0.0 and -0.0 tie) and ``values`` is the element found there, bits included.
    ``last``: the last maximum instead (a control)."""
    x = np.asarray(x)
    *lead, Fq, C = x.shape
    Fo = Fq // pool
    win = x[..., :Fo * pool, :].reshape(*lead, Fo, pool, C)
    if last:
        pos = pool - 1 - np.argmax(win[..., ::-1, :], axis=-2)
    else:
        pos = np.argmax(win, axis=-2)
    val = np.take_along_axis(win, pos[..., None, :], axis=-2)[..., 0, :]
    return val, pos.astype(np.uint8)
