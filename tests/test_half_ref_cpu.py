"""Self-test of the float64 references in tests/half_ref.py (no GPU): with rounding disabled the per-step LSTM
references reproduce torch.nn.LSTM (float64) and its autograd gradients step by step, the k-split partials sum to the
unsplit product, and the rounding helpers are RNE."""
import pytest
import torch

from tests import half_ref as R


def _lstm(In, H, seed=0):
    torch.manual_seed(seed)
    return torch.nn.LSTM(In, H, num_layers=1, batch_first=True).double()


def _states(ref, x):
    """y [B, T, H] and c [B, T, H] of every step of a float64 nn.LSTM (c from the prefix runs)."""
    y, _ = ref(x)
    c = torch.stack([ref(x[:, :t + 1])[1][1][0] for t in range(x.shape[1])], dim=1)
    return y, c


@pytest.mark.parametrize("reverse", [0, 1])
def test_lstm_step_references_reproduce_nn_lstm(reverse):
    B, T, In, H = 3, 5, 8, 64
    ref = _lstm(In, H)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, T, In, generator=g, dtype=torch.float64, requires_grad=True)
    xs = x.flip(1) if reverse else x                            # a reverse cell is the forward cell on the flipped input
    y, c = _states(ref, xs)
    if reverse:
        y, c = y.flip(1), c.flip(1)
    P = dict(ref.named_parameters())
    xg = (x @ P["weight_ih_l0"].T + P["bias_ih_l0"] + P["bias_hh_l0"]).detach()
    whh = P["weight_hh_l0"].detach()

    G, C, Y = R.lstm_fwd_teacher(xg, y.detach(), c.detach(), whh, reverse, None)
    assert torch.allclose(Y, y.detach(), rtol=0, atol=1e-12) and torch.allclose(C, c.detach(), rtol=0, atol=1e-12)

    dy = torch.randn(B, T, H, generator=g, dtype=torch.float64)
    y.backward(dy)
    D, E, n_amb = R.lstm_bwd_teacher(dy, G, C, whh, reverse, None)
    assert n_amb == 0 and (E == 0).all()
    # step by step: dx_t = dgates_t W_ih, and the parameter gradients
    dx = D @ P["weight_ih_l0"].detach()
    for t in range(T):
        assert torch.allclose(dx[:, t], x.grad[:, t], rtol=0, atol=1e-12), t
    assert torch.allclose(D.sum((0, 1)), P["bias_ih_l0"].grad, rtol=0, atol=1e-11)
    assert torch.allclose(R.whh_grad_ref(D, Y, reverse, None), P["weight_hh_l0"].grad, rtol=0, atol=1e-11)


def test_ksplit_partials_sum_to_the_unsplit_product():
    g = torch.Generator().manual_seed(2)
    B, H = 5, 384
    dg = torch.randn(B, 4 * H, generator=g)
    whh = torch.randn(4 * H, H, generator=g) * 0.05
    for half in (None, "bf16", "f16"):
        parts, mags = R.ksplit_partials(dg, whh, half)
        assert parts.shape == (H // 32, B, H) and (mags >= parts.abs()).all()
        full = R.hr(dg, half) @ R.hr(whh, half)
        assert torch.allclose(parts.sum(0), full, rtol=0, atol=1e-12)
    # rounding each partial to bf16 moves the sum by at most half an ulp per partial; the slack flags are rare
    s, slack, n_amb = R.round_partials(parts, mags, "bf16")
    bound = (parts.abs() * 2.0 ** -8).sum(0)
    assert ((s - parts.sum(0)).abs() <= bound).all()
    assert n_amb < 0.02 * parts.numel() and (slack >= 0).all()


def test_rounding_is_round_to_nearest_even():
    # bf16: 1 + 2^-8 is the midpoint between 1 and 1 + 2^-7 -> even (1); 1 + 3 * 2^-8 -> 1 + 2^-6 (even)
    x = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20])
    assert R.hr(x, "bf16").tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7]
    # fp16: the same at 2^-11; the range ends at 65504 (65519 rounds down, 65520 overflows), subnormals are kept
    y = torch.tensor([1 + 2.0 ** -11, 65504.0, 65519.0, 65520.0, 2.0 ** -20, 3 * 2.0 ** -26])
    assert R.hr(y, "f16").tolist() == [1.0, 65504.0, 65504.0, float("inf"), 2.0 ** -20, 2.0 ** -24]
    assert R.hr(y, None).dtype == torch.float64


def test_bwd_step_error_bound_follows_the_slack():
    """A perturbation of dh within the slack moves every gate gradient by at most the returned bound."""
    g = torch.Generator().manual_seed(3)
    B, H = 4, 384
    gates = torch.rand(B, 4 * H, generator=g, dtype=torch.float64)
    c, cp = torch.randn(B, H, generator=g, dtype=torch.float64), torch.randn(B, H, generator=g, dtype=torch.float64)
    dy = torch.randn(B, H, generator=g, dtype=torch.float64)
    dg = torch.randn(B, 4 * H, generator=g)
    whh = torch.randn(4 * H, H, generator=g) * 0.05
    d0, dc0, err, edc, n = R.lstm_bwd_step(dy, dg, gates, c, cp, whh, None, "bf16")
    parts, mags = R.ksplit_partials(dg, whh, "bf16")
    _, slack, _ = R.round_partials(parts, mags, "bf16")
    sign = torch.where(torch.rand(B, H, generator=g) < 0.5, -1.0, 1.0).double()
    d1, dc1, _, _, _ = R.lstm_bwd_step(dy + sign * slack, dg, gates, c, cp, whh, None, "bf16")
    assert ((d1 - d0).abs() <= err * (1 + 1e-9) + 1e-15).all()
    assert ((dc1 - dc0).abs() <= edc * (1 + 1e-9) + 1e-15).all()
