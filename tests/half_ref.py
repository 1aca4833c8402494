"""Float64 references for the 16-bit operand kernels (mixed precision: ``ops.matmul_bf16(True, half)``).

Every operand the kernels feed to a 16-bit MFMA is the fp32 value rounded to nearest even to the operand type;
``hr`` is that rounding, and the references multiply and sum the rounded values in float64.  ``half=None`` is the
unrounded float64 computation (the CPU self-test holds it against torch.nn.LSTM and autograd).

The LSTM references take ONE step at a time from the kernel's own stored state (teacher forcing): a free-running
float64 recurrence is useless here, because a 1e-7 difference in h flips a 16-bit rounding somewhere and from then on
the two runs disagree by a rounding step.
"""
import torch

HALF = {"bf16": torch.bfloat16, "f16": torch.float16}
# The persistent backward hands its partial dh tiles between workgroups as bf16 in BOTH half modes: store_sc1_h in
# csrc/lstm_persistent.hip packs bf16 whatever the operand type is (fp32 exponent range for the exchanged sums).
XCHG_HALF = "bf16"
TILE_K = 32            # hidden units per producer workgroup of the k-split backward (H / 32 producers)
ACC_NOISE = 2.0 ** -20  # bound on the fp32 accumulation error of a partial tile, relative to the sum of |terms|


def hr(t, half):
    """t rounded (RNE) to the 16-bit type ``half`` ("bf16" / "f16"), as float64; None: unrounded float64."""
    t = t.detach().cpu()
    return t.double() if half is None else t.to(HALF[half]).double()


def _acts(pre):
    i, f, g, o = pre.chunk(4, dim=-1)
    return torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)


def lstm_fwd_step(xg, h_prev, c_prev, whh, half):
    """One forward step (gate order i, f, g, o).  xg [B, 4H]: the input gates x W_ih^T + b_ih + b_hh as the kernel
    reads them; h_prev, c_prev [B, H] (None on the first step of the direction); whh [4H, H].
    Returns (activated gates [B, 4H], c [B, H], h [B, H]) in float64."""
    pre = xg.detach().cpu().double()
    if h_prev is not None:
        pre = pre + hr(h_prev, half) @ hr(whh, half).T
    i, f, g, o = _acts(pre)
    c = i * g if c_prev is None else f * c_prev.detach().cpu().double() + i * g
    return torch.cat([i, f, g, o], dim=-1), c, o * torch.tanh(c)


def ksplit_partials(dg_next, whh, half):
    """The backward's k-split of dgates_{t+-1} . W_hh: producer p owns k = {g H + 32 p + jj : g < 4, jj < 32} and
    hands every consumer its share of the product.  Returns (partials [P, B, H], sums of |terms| [P, B, H])."""
    B, K = dg_next.shape
    H = K // 4
    P = H // TILE_K
    a = hr(dg_next, half).view(B, 4, P, TILE_K)
    w = hr(whh, half).view(4, P, TILE_K, H)
    return torch.einsum("bgpj,gpjn->pbn", a, w), torch.einsum("bgpj,gpjn->pbn", a.abs(), w.abs())


def round_partials(parts, mags, xhalf):
    """Sum of the partials each rounded to ``xhalf`` as it is handed over.  Also returns, per element, the slack for
    rounding boundaries: one ``xhalf`` ulp of every partial that lies within fp32 accumulation noise of a rounding
    midpoint (the kernel's fp32 partial may round either way), and the number of such partials."""
    if xhalf is None:
        return parts.sum(0), torch.zeros(parts.shape[1:], dtype=torch.float64), 0
    noise = ACC_NOISE * mags
    lo, hi = hr(parts - noise, xhalf), hr(parts + noise, xhalf)
    amb = lo != hi
    slack = ((hi - lo).abs() * amb).sum(0)
    return hr(parts, xhalf).sum(0), slack, int(amb.sum())


def lstm_bwd_step(dy, dg_next, gates, c, c_prev, whh, dc_in, half, xhalf=XCHG_HALF, err_dc_in=None):
    """One backward step.  dy [B, H]: dL/dh_t from above; dg_next [B, 4H]: the pre-activation gate gradients of the
    step processed before this one (None on the first); gates [B, 4H]: the activated gates of step t; c, c_prev:
    cell states c_t, c_{t-+1} (None on the direction's first step); dc_in: dL/dc carried from the previous step
    (float64; None on the first).  err_dc_in: error bound of dc_in.
    Returns (dgates [B, 4H], dc_out, error bound of dgates, error bound of dc_out, ambiguous partials)."""
    dh = dy.detach().cpu().double()
    e_dh = torch.zeros_like(dh)
    n_amb = 0
    if dg_next is not None:
        parts, mags = ksplit_partials(dg_next, whh, half)
        s, e_dh, n_amb = round_partials(parts, mags, xhalf if half is not None else None)
        dh = dh + s
    i, f, g, o = gates.detach().cpu().double().chunk(4, dim=-1)
    tc = torch.tanh(c.detach().cpu().double())
    cp = torch.zeros_like(tc) if c_prev is None else c_prev.detach().cpu().double()
    dc = dh * o * (1 - tc * tc) + (0.0 if dc_in is None else dc_in)
    e_dc = e_dh * (o * (1 - tc * tc)).abs() + (0.0 if err_dc_in is None else err_dc_in)
    dgates = torch.cat([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], -1)
    err = torch.cat([e_dc * (g * i * (1 - i)).abs(), e_dc * (cp * f * (1 - f)).abs(), e_dc * (i * (1 - g * g)).abs(),
                     e_dh * (tc * o * (1 - o)).abs()], -1)
    return dgates, dc * f, err, e_dc * f.abs(), n_amb


def _order(T, reverse):
    """Time steps in processing order and the previous step of each (None first)."""
    ts = list(range(T - 1, -1, -1)) if reverse else list(range(T))
    return [(t, ts[k - 1] if k else None) for k, t in enumerate(ts)]


def lstm_fwd_teacher(xg, y, cbuf, whh, reverse, half):
    """Per-step forward references from the stored state: step t starts from y[:, t-+1] and cbuf[:, t-+1] (the
    kernel's own outputs).  xg [B, T, 4H] input gates (a copy taken before the call: the kernel overwrites them with
    the activated gates).  Returns (gates, c, h) [B, T, .] float64."""
    B, T, _ = xg.shape
    H = whh.shape[1]
    G = torch.empty(B, T, 4 * H, dtype=torch.float64)
    C = torch.empty(B, T, H, dtype=torch.float64)
    Y = torch.empty(B, T, H, dtype=torch.float64)
    for t, tp in _order(T, reverse):
        G[:, t], C[:, t], Y[:, t] = lstm_fwd_step(xg[:, t], None if tp is None else y[:, tp],
                                                  None if tp is None else cbuf[:, tp], whh, half)
    return G, C, Y


def lstm_bwd_teacher(dy, gates, cbuf, whh, reverse, half, dgates_src=None, xhalf=XCHG_HALF):
    """Per-step backward references.  gates [B, T, 4H]: activated gates (the forward's output, copied before the
    backward overwrites them); cbuf [B, T, H]; dgates_src: the tensor the step before's gate gradients are read from
    (the GPU's in-place output -- teacher forcing), None: the reference's own.  dc is carried in float64.
    Returns (dgates [B, T, 4H], error bound [B, T, 4H], ambiguous partials)."""
    B, T, _ = gates.shape
    H = whh.shape[1]
    D = torch.empty(B, T, 4 * H, dtype=torch.float64)
    E = torch.zeros(B, T, 4 * H, dtype=torch.float64)
    dc = edc = None
    n_amb = 0
    src = D if dgates_src is None else dgates_src
    for t, tn in _order(T, not reverse):                   # the backward walks the direction's steps in reverse
        tp = t + 1 if reverse else t - 1                   # c_{t-1} of the forward direction
        cp = cbuf[:, tp] if 0 <= tp < T else None
        D[:, t], dc, E[:, t], edc, k = lstm_bwd_step(dy[:, t], None if tn is None else src[:, tn], gates[:, t],
                                                     cbuf[:, t], cp, whh, dc, half, xhalf, edc)
        n_amb += k
    return D, E, n_amb


def shifted_y(y, reverse):
    """h_{t-1} of every step t (h_{t+1} for a reverse cell), zero where there is none: the W_hh-gradient operand."""
    ys = torch.zeros_like(y)
    if reverse:
        ys[:, :-1] = y[:, 1:]
    else:
        ys[:, 1:] = y[:, :-1]
    return ys


def whh_grad_ref(dgates, y, reverse, half):
    """dW_hh [4H, H] = sum over (b, t) of r(dgates[b, t])^T r(h_{t-+1}[b])."""
    B, T, K = dgates.shape
    H = K // 4
    a = hr(dgates, half).reshape(B * T, K)
    b = hr(shifted_y(y.detach().cpu(), reverse), half).reshape(B * T, H)
    return a.T @ b
