"""The resampler's backward on the GPU (csrc/resample.hip: pe_resample_backward, pe_resample_ragged_backward;
ops.resample_backward / ops.resample_ragged_backward; the autograd wrappers of resample.py; inference.f0_from_wave
with ``sample_rate=`` / ``rates=``).

Parity bound, derived and not measured: per input sample ``|dx_gpu - dx_ref| <= (K_q + 2) 2^-24 T_q`` against the
float64 restatement of tests/resample_grad_ref.py, ``K_q`` the terms of the sample's fmaf chain (one rounding each),
one more for the float32 tap, one of slack for the second-order term, ``T_q = sum |k dy|``.

The reference is evaluated at the parameters the plan is built with.  ``rolloff`` crosses the C ABI as a float, so the
plan's table is the float32 rounding of the taps at rolloff ``float32(0.99)`` = 0.9900000095..., not at 0.99: near a
zero crossing of the sinc a tap moves by many of its own roundings between the two (t k'(t) / k(t) is large there), so
"one rounding for the float32 tap" only holds against taps at ``ROLLOFF`` below.  Against the oracle's default 0.99
the same float32 chain (its CPU emulation gives the device's figures to the digit) reaches 1.019 of the bound at
96 kHz -> 24 kHz (a 25-sample row, K_q = 7) and 1.044 at 96 kHz -> 16 kHz, and stays below 0.98 elsewhere; with taps
at ``ROLLOFF`` the largest figure on the MI355X is 0.510 (32 kHz -> 16 kHz).  The forward reads the same table and is
left as it is."""
import functools
import math

import numpy as np
import pytest
import torch

from pitchextractor_amd import inference, ops
from pitchextractor_amd.resample import RaggedResampler, Resampler
from tests import resample_grad_ref as ref
from tests.test_resample_ragged_gpu import RATES, _width

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
ROLLOFF = float(np.float32(Resampler(2, 1).rolloff))       # the default rolloff as pe_resample_plan_create receives it
TARGETS = (24000, 16000)


def dev(a, device):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device)


@functools.lru_cache(maxsize=None)
def resampler(rate, target):
    return Resampler(rate, target)


@functools.lru_cache(maxsize=None)
def ragged(target):
    return RaggedResampler(target)


@functools.lru_cache(maxsize=None)
def rows_of(target):
    """The batch of a target rate, made once and left unchanged: per source rate the lengths 1, width - 1, width, one
    phase period, 9001 and one drawn under 2 s, in a drawn order; per row ``dy = 0.3 N(0, 1)`` over its whole output
    and the float64 reference ``(dx, T, K)``."""
    rng = np.random.default_rng(target + 1)
    rates, lengths = [], []
    for r in RATES:
        w = _width(r, target)
        for n in (1, max(1, w - 1), w, r // math.gcd(r, target), 9001, int(rng.integers(1, 2 * r))):
            rates.append(r)
            lengths.append(n)
    perm = rng.permutation(len(rates))
    rates, lengths = [rates[k] for k in perm], [lengths[k] for k in perm]
    out_lengths = [ragged(target).out_len(r, n) for r, n in zip(rates, lengths)]
    dys = [(0.3 * rng.standard_normal(m)).astype(np.float32) for m in out_lengths]
    refs = [ref.resample_backward(dy, r, target, n, rolloff=ROLLOFF) for dy, r, n in zip(dys, rates, lengths)]
    return rates, lengths, out_lengths, dys, refs


def padded(rows, width=None, fill=0.0):
    width = max(len(r) for r in rows) if width is None else width
    out = np.full((len(rows), width), fill, np.float32)
    for k, r in enumerate(rows):
        out[k, :len(r)] = r
    return out


@functools.lru_cache(maxsize=None)
def alone(target, device):
    """``ops.resample_backward`` on every row of ``rows_of(target)`` alone, as host arrays."""
    rates, lengths, _, dys, _ = rows_of(target)
    return [ops.resample_backward(resampler(r, target), dev(dy, device)[None], n)[0].cpu().numpy()
            for r, n, dy in zip(rates, lengths, dys)]


# ------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("target", TARGETS)
def test_parity_with_the_float64_restatement(hip_device, target):
    """Worst |dx_gpu - dx_ref| / ((K_q + 2) 2^-24 T_q) per source rate, as measured on the MI355X: DESIGN section 27."""
    rates, lengths, _, _, refs = rows_of(target)
    got = alone(target, str(hip_device))
    worst = {}
    for r, (rate, n, g, (dx, T, K)) in enumerate(zip(rates, lengths, got, refs)):
        assert g.shape == (n,) and np.isfinite(g).all()
        err, bound = np.abs(g.astype(np.float64) - dx), (K + 2) * EPS * T
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
        worst[rate] = max(worst.get(rate, 0.0), ratio)
    for rate in RATES:
        print(f"{rate} -> {target}: worst error / bound = {worst[rate]:.3f}")
    assert all(w <= 1.0 for w in worst.values()), worst


# ------------------------------------------------------------------------------------------- 2. adjoint on the device
@pytest.mark.parametrize("rate,target", [(44100, 24000), (16000, 24000), (11025, 24000), (48000, 16000)])
def test_adjoint_on_the_device(hip_device, rate, target):
    """<R x, dy> and <x, R^T dy>, each summed in float64 on the host from the float32 results, agree within the sum of
    the per-sample bounds of both sides: with S_q = |x_q| T_q (the same total S = sum |k| |x| |dy| seen from either
    side), the forward is within (taps + 2) 2^-24 S (a chain of `taps` terms per output) and the backward within
    sum_q (K_q + 2) 2^-24 S_q of the exact inner product."""
    rng = np.random.default_rng(rate)
    rs, n = resampler(rate, target), 5000
    taps = 2 * _width(rate, target) + rate // math.gcd(rate, target)
    x = rng.standard_normal((2, n)).astype(np.float32)
    dy = (0.3 * rng.standard_normal((2, rs.out_len(n)))).astype(np.float32)
    y = rs(dev(x, hip_device)).cpu().numpy().astype(np.float64)
    dx = ops.resample_backward(rs, dev(dy, hip_device), n).cpu().numpy().astype(np.float64)
    for b in range(2):
        _, T, K = ref.resample_backward(dy[b], rate, target, n, rolloff=ROLLOFF)
        S = np.abs(x[b].astype(np.float64)) * T
        bound = (taps + 2) * EPS * S.sum() + ((K + 2) * EPS * S).sum()
        lhs, rhs = float(y[b] @ dy[b].astype(np.float64)), float(x[b].astype(np.float64) @ dx[b])
        print(f"{rate} -> {target} row {b}: |lhs - rhs| / bound = {abs(lhs - rhs) / bound:.4f}")
        assert abs(lhs - rhs) <= bound


# --------------------------------------------------------------------------------------------------- 3. bit identities
@pytest.mark.parametrize("target", TARGETS)
def test_bit_identities_of_the_ragged_launch(hip_device, target):
    rates, lengths, out_lengths, dys, _ = rows_of(target)
    want = alone(target, str(hip_device))
    rr, B = ragged(target), len(rates)
    g = dev(padded(dys), hip_device)
    packed = ops.resample_ragged_backward(rr, g, rates, lengths, packed=True)
    assert packed.shape == (sum(lengths),)
    assert np.array_equal(packed.cpu().numpy(), np.concatenate(want))                  # each row alone, bit for bit
    # padded equals packed; the output buffer starts as NaN and is wider than the longest row
    width = max(lengths) + 300
    out = torch.full((B, width), float("nan"), device=hip_device)
    pad = ops.resample_ragged_backward(rr, g, rates, lengths, packed=False, out=out)
    assert pad is out and np.array_equal(pad.cpu().numpy(), padded(want, width))       # exact zeros past n_in
    assert torch.equal(ops.resample_ragged_backward(rr, g, rates, lengths, packed=False),
                       pad[:, :max(lengths)])
    # two runs
    assert torch.equal(ops.resample_ragged_backward(rr, g, rates, lengths, packed=True), packed)
    # any batch order
    perm = np.random.default_rng(3).permutation(B)
    shuffled = ops.resample_ragged_backward(rr, g[dev(perm, hip_device)], [rates[k] for k in perm],
                                            [lengths[k] for k in perm], packed=False, width=width)
    assert torch.equal(shuffled, pad[dev(perm, hip_device)])
    # grad_out at a wider row stride, NaN past each row's own output: that region is never read
    wide = dev(padded(dys, g.shape[1] + 77, fill=np.nan), hip_device)
    for view in (wide, wide[:, :g.shape[1]]):
        assert view.stride(0) == g.shape[1] + 77
        assert torch.equal(ops.resample_ragged_backward(rr, view, rates, lengths, packed=True), packed)
    # a copied-rate row is a bit copy
    copies = [r for r in range(B) if rates[r] == target]
    assert len(copies) == 6
    for r in copies:
        assert np.array_equal(want[r], dys[r]) and np.array_equal(pad[r, :lengths[r]].cpu().numpy(), dys[r])
    # linearity is exact for powers of two
    assert torch.equal(ops.resample_ragged_backward(rr, 2 * g, rates, lengths, packed=True), 2 * packed)


def test_single_rate_stride_truncation_and_linearity(hip_device):
    """pe_resample_backward reads grad_out at its own row stride and never past n_out, which may stay below the full
    output length; batch rows are independent."""
    rs, n = resampler(44100, 24000), 3001
    rng = np.random.default_rng(11)
    m = rs.out_len(n)
    dy = (0.3 * rng.standard_normal((3, m))).astype(np.float32)
    base = ops.resample_backward(rs, dev(dy, hip_device), n)
    for b in range(3):
        assert torch.equal(ops.resample_backward(rs, dev(dy[b:b + 1], hip_device), n)[0], base[b])
    wide = dev(padded(dy, m + 50, fill=np.nan), hip_device)
    assert torch.equal(ops.resample_backward(rs, wide[:, :m], n), base)
    assert torch.equal(ops.resample_backward(rs, dev(2 * dy, hip_device), n), 2 * base)
    cut = m - 200                                           # the last 200 outputs carry no gradient
    zeroed = dy.copy()
    zeroed[:, cut:] = 0
    assert torch.equal(ops.resample_backward(rs, wide[:, :cut], n), ops.resample_backward(rs, dev(zeroed, hip_device), n))
    dx, T, K = ref.resample_backward(dy[0, :cut], 44100, 24000, n, rolloff=ROLLOFF)
    got = ops.resample_backward(rs, wide[:1, :cut], n)[0].cpu().numpy().astype(np.float64)
    # Right behind the cut a sample keeps only its terms at the window's clamped edge, where cos^2 leaves taps of
    # 1e-48: below float32's smallest denormal 2^-149, so they round to 0 with an absolute error, not a relative one.
    # Every rounding the bound counts is therefore within max(2^-24 |v|, 2^-150), and the floor joins the bound.
    assert (np.abs(got - dx) <= (K + 2) * (EPS * T + 2.0 ** -150)).all()


def test_shape_checks(hip_device):
    rs, rr = resampler(44100, 24000), ragged(24000)
    g = torch.zeros(2, 81, device=hip_device)
    with pytest.raises(ValueError, match="longer than the output"):
        ops.resample_backward(rs, g, 147)                  # 147 samples give 80 outputs
    with pytest.raises(ValueError, match="expected \\(B, n_out\\) rows"):
        ops.resample_backward(rs, g[0], 147)
    with pytest.raises(RuntimeError, match="float32 device grad_out"):
        ops.resample_backward(rs, g.double(), 147)
    with pytest.raises(ValueError, match="one rate and one length"):
        ops.resample_ragged_backward(rr, g, [44100], [147, 10], packed=True)
    with pytest.raises(ValueError, match="narrower than a row's output"):
        ops.resample_ragged_backward(rr, g, [44100, 16000], [147, 100], packed=True)     # 150 outputs
    with pytest.raises(ValueError, match="below the rows' extent"):
        ops.resample_ragged_backward(rr, g, [44100, 16000], [147, 10], packed=False, width=100)
    empty = ops.resample_ragged_backward(rr, g, [44100, 16000], [0, 0], packed=False, width=5)
    assert empty.shape == (2, 5) and not empty.any()


# ------------------------------------------------------------------------------------------------ 4. autograd plumbing
def test_autograd_of_the_single_rate_resampler(hip_device):
    rs, n = resampler(44100, 24000), 2000
    rng = np.random.default_rng(2)
    x = dev((0.3 * rng.standard_normal((3, n))).astype(np.float32), hip_device)
    dy = dev((0.3 * rng.standard_normal((3, rs.out_len(n)))).astype(np.float32), hip_device)
    plain = rs(x)
    assert plain.grad_fn is None and not plain.requires_grad
    w = x.clone().requires_grad_()
    y = rs(w)
    assert y.grad_fn is not None and torch.equal(y.detach(), plain)
    (grad,) = torch.autograd.grad(y, w, dy)
    assert torch.equal(grad, ops.resample_backward(rs, dy, n))
    with torch.no_grad():
        assert rs(w).grad_fn is None
    # 1-D
    w1 = x[0].clone().requires_grad_()
    y1 = rs(w1)
    assert y1.shape == plain[0].shape and torch.equal(y1.detach(), plain[0])
    (g1,) = torch.autograd.grad(y1, w1, dy[0])
    assert g1.shape == (n,) and torch.equal(g1, grad[0])
    # non-contiguous input: every other sample of a longer wave
    long = dev((0.3 * rng.standard_normal((2, 2 * n))).astype(np.float32), hip_device).requires_grad_()
    y2 = rs(long[:, ::2])
    assert torch.equal(y2.detach(), rs(long.detach()[:, ::2].contiguous()))
    (g2,) = torch.autograd.grad(y2, long, dy[:2])
    assert not g2[:, 1::2].any() and torch.equal(g2[:, ::2], ops.resample_backward(rs, dy[:2], n))
    # a summed output hands over an expanded gradient
    w3 = x.clone().requires_grad_()
    rs(w3).sum().backward()
    assert torch.equal(w3.grad, ops.resample_backward(rs, torch.ones_like(dy), n))
    # orig == new returns the wave itself: the gradient passes through
    same = resampler(24000, 24000)
    w4 = x.clone().requires_grad_()
    assert same(w4) is w4
    (g4,) = torch.autograd.grad((same(w4) * 3.0).sum(), w4)
    assert torch.equal(g4, torch.full_like(x, 3.0))
    assert torch.equal(ops.resample_backward(same, dy, dy.shape[1]), dy)


def test_autograd_of_the_ragged_resampler(hip_device):
    rr = ragged(24000)
    rates, lengths = [16000, 24000, 44100, 48000, 11025], [700, 901, 3000, 1, 2222]
    rng = np.random.default_rng(4)
    rows = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in lengths]
    out_lengths = [rr.out_len(r, n) for r, n in zip(rates, lengths)]
    dy = dev((0.3 * rng.standard_normal((5, max(out_lengths)))).astype(np.float32), hip_device)
    for layout in ("padded", "packed"):
        x = dev(padded(rows, max(lengths) + 9) if layout == "padded" else np.concatenate(rows + [np.zeros(4, np.float32)]),
                hip_device)
        plain, plain_len = rr(x, rates, lengths)
        assert plain.grad_fn is None
        w = x.clone().requires_grad_()
        y, out_len = rr(w, rates, lengths)
        assert y.grad_fn is not None and torch.equal(y.detach(), plain)
        assert out_len.grad_fn is None and not out_len.requires_grad and torch.equal(out_len, plain_len)
        (grad,) = torch.autograd.grad(y, w, dy)
        assert grad.shape == x.shape
        want = ops.resample_ragged_backward(rr, dy, rates, lengths, packed=layout == "packed", width=x.shape[-1])
        assert torch.equal(grad, want)
        if layout == "packed":
            assert not grad[sum(lengths):].any()
        with torch.no_grad():
            assert rr(w, rates, lengths)[0].grad_fn is None


# ------------------------------------------------------------------------------------------------------ 5. end to end
def _frozen_net(device, monkeypatch):
    from tests.test_input_grad_gpu import build
    monkeypatch.setattr(ops, "FP32_MATMUL", "h2")
    net = build("bilstm", device).eval().requires_grad_(False)
    assert net.is_frozen()
    return net


def test_f0_loss_reaches_audio_at_44100(hip_device, monkeypatch):
    """audio at 44.1 kHz -> resampler -> log-mel -> frozen JDCNet -> loss, and back: wave.grad is the resampler's
    backward of the gradient the same loss leaves on the 24 kHz intermediate, bit for bit."""
    from tests.test_mel_grad_gpu import transform, wave_of
    net, mel, T = _frozen_net(hip_device, monkeypatch), transform("default"), 32
    rs = resampler(44100, 24000)
    x = dev(np.stack([wave_of("noise", 8822, seed=s) for s in (0, 1)]), hip_device)
    target = torch.linspace(80.0, 300.0, 2 * T, device=hip_device)

    wave = x.clone().requires_grad_()
    cls, _ = inference.f0_from_wave(net, wave, mel_transform=mel, max_frames=T, sample_rate=44100)
    torch.nn.functional.smooth_l1_loss(cls.reshape(-1), target).backward()
    assert torch.isfinite(wave.grad).all() and wave.grad.any() and wave.grad.shape == x.shape

    mid = rs(x).requires_grad_()                                       # the 24 kHz intermediate as a leaf
    cls2, _ = inference.f0_from_wave(net, mid, mel_transform=mel, max_frames=T)
    assert torch.equal(cls2, cls.detach())
    torch.nn.functional.smooth_l1_loss(cls2.reshape(-1), target).backward()
    assert torch.equal(wave.grad, ops.resample_backward(rs, mid.grad, x.shape[1]))
    # max_frames defaults to the frames of the resampled row
    with torch.no_grad():
        assert inference.f0_from_wave(net, x, mel_transform=mel, sample_rate=44100)[0].shape[1] == \
            mel.num_frames(rs.out_len(x.shape[1]))


def test_f0_loss_reaches_a_mixed_rate_batch(hip_device, monkeypatch):
    from tests.test_mel_grad_gpu import transform, wave_of
    net, mel, T = _frozen_net(hip_device, monkeypatch), transform("default"), 32
    rr = ragged(24000)
    rates, lengths = [16000, 24000, 44100, 48000], [3300, 4801, 9000, 10000]
    x = dev(padded([wave_of("noise", n, seed=k) for k, n in enumerate(lengths)], max(lengths) + 3), hip_device)
    target = torch.linspace(80.0, 300.0, 4 * T, device=hip_device)

    wave = x.clone().requires_grad_()
    cls, _ = inference.f0_from_wave(net, wave, lengths, mel_transform=mel, max_frames=T, rates=rates)
    torch.nn.functional.smooth_l1_loss(cls.reshape(-1), target).backward()
    assert torch.isfinite(wave.grad).all() and wave.grad.shape == x.shape
    for r, n in enumerate(lengths):
        assert wave.grad[r, :n].any() and not wave.grad[r, n:].any()

    mid, out_lengths = rr(x, rates, lengths)
    mid.requires_grad_()
    cls2, _ = inference.f0_from_wave(net, mid, out_lengths, mel_transform=mel, max_frames=T)
    assert torch.equal(cls2, cls.detach())
    torch.nn.functional.smooth_l1_loss(cls2.reshape(-1), target).backward()
    assert torch.equal(wave.grad, ops.resample_ragged_backward(rr, mid.grad, rates, lengths, packed=False,
                                                               width=x.shape[1]))
