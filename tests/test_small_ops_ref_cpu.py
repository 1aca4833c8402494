"""The float64 references of tests/small_ops_ref.py against stock torch / their own defining properties (no device)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import small_ops_ref as S


def test_adamw_step_ref_is_torch_adamw_in_float64():
    """Hyper-parameters that are float32 numbers, bias corrections kept in double: torch.optim.AdamW in float64 over 5
    steps, to 1e-15.  With the kernel's float32 step_size / bc2_sqrt the parameter moves by at most 2 u of the step."""
    lr, b1, b2, eps, wd = 2.0 ** -10, 0.875, 0.96875, 2.0 ** -30, 2.0 ** -4
    g = torch.Generator().manual_seed(3)
    n = 257
    p0 = torch.randn(n, generator=g, dtype=torch.float64)
    ref_p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref_p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.numpy().copy(), np.zeros(n), np.zeros(n)
    for step in range(1, 6):
        grad = torch.randn(n, generator=g, dtype=torch.float64)
        ref_p.grad = grad.clone()
        opt.step()
        m1, v1, mag_m, mag_v, param = S.adamw_step_ref(p, grad, m, v, lr, b1, b2, eps, wd, step,
                                                       exact_bias_correction=True)
        p1, mag_p = param(m1, v1)
        st = opt.state[ref_p]
        assert np.abs(m1 - st["exp_avg"].numpy()).max() <= 1e-15
        assert np.abs(v1 - st["exp_avg_sq"].numpy()).max() <= 1e-15
        assert np.abs(p1 - ref_p.detach().numpy()).max() <= 1e-15
        assert (mag_m >= np.abs(m1) - 1e-18).all() and (mag_v >= v1 - 1e-18).all() and (mag_p >= np.abs(p1) - 1e-18).all()
        # the rounding model: float32 step_size and bc2_sqrt, one relative u each
        m2, v2, _, _, param32 = S.adamw_step_ref(p, grad, m, v, lr, b1, b2, eps, wd, step)
        assert np.array_equal(m2, m1) and np.array_equal(v2, v1)
        p2, _ = param32(m1, v1)
        assert (np.abs(p2 - p1) <= 2.001 * S.U * np.abs(p1 - (1.0 - lr * wd) * p)).all()
        p, m, v = p1, m1, v1


def test_adamw_constants_round_as_the_c_abi_does():
    k = S.adamw_constants(1e-4, 0.9, 0.98, 1e-9, 5e-4, 7, 1.0 / 8)
    f = np.float32
    assert k["w2"] == float(f(1.0) - f(0.98)) and k["w1"] == float(f(1.0) - f(0.9))
    # 1f - float32(beta2) is exact; it is the rounding of beta2 itself that puts the constant about 16 u away from
    # the double 1 - 0.98 (what eats the tolerance of a comparison with torch's fp32 AdamW)
    assert k["w2"] == 1.0 - float(f(0.98))
    assert 12 * S.U < abs(k["w2"] - (1.0 - 0.98)) / 0.02 < 20 * S.U
    assert k["decay"] == float(f(1.0) - f(f(1e-4) * f(5e-4)))
    assert k["step_size"] == float(f(float(f(1e-4)) / (1.0 - 0.9 ** 7)))
    assert k["bc2_sqrt"] == float(f(np.sqrt(1.0 - 0.98 ** 7)))
    # controls differ from the model
    x = np.linspace(-1, 1, 9)
    base = S.adamw_step_ref(x, x[::-1], 0.1 * x, x * x, 1e-3, 0.9, 0.98, 1e-9, 0.1, 3)
    for kw in (dict(w2_double=True), dict(coupled=True)):
        other = S.adamw_step_ref(x, x[::-1], 0.1 * x, x * x, 1e-3, 0.9, 0.98, 1e-9, 0.1, 3, **kw)
        assert not np.array_equal(other[4](base[0], base[1])[0], base[4](base[0], base[1])[0]) or \
            not np.array_equal(other[1], base[1])


@pytest.mark.parametrize("grad_scale", [1.0, 65536.0, 0.125])
def test_loss_ref_is_torch_smooth_l1_and_bce_in_float64(grad_scale):
    g = torch.Generator().manual_seed(1)
    R = 301
    f0 = torch.where(torch.randn(R, generator=g) > -0.5, torch.rand(R, generator=g) * 200 + 80, torch.zeros(R))
    f0p = torch.randn(R, generator=g) * 150 + 100
    edge = torch.tensor([0.0, 1.0, -1.0, 1 - 2.0 ** -24, -(1 - 2.0 ** -24), 1 + 2.0 ** -23, -(1 + 2.0 ** -23), 0.3])
    f0[:8], f0p[:8] = 0.0, edge                                     # |d| exactly 1 and its float32 neighbours
    silp = torch.randn(R, generator=g) * 3
    silp[:5] = torch.tensor([100.0, -100.0, 1e4, -1e4, 0.0])
    sil = (f0 == 0).float()
    lam = 0.5                                                       # a float32 number: nothing to round
    a = f0p.double().requires_grad_(True)
    z = silp.double().requires_grad_(True)
    l1 = torch.nn.SmoothL1Loss()(a, f0.double())
    bce = torch.nn.BCEWithLogitsLoss()(z, sil.double())
    ((lam * l1 + bce) * grad_scale).backward()
    r = S.f0_sil_loss_ref(f0p, f0, silp, sil, lam, grad_scale)
    assert abs(r["l1"] - lam * l1.item()) <= 1e-15 * abs(r["l1"])
    assert abs(r["bce"] - bce.item()) <= 1e-15 * abs(r["bce"])
    assert abs(r["total"] - (lam * l1 + bce).item()) <= 1e-15 * abs(r["total"])
    assert np.abs(r["d_f0"] - a.grad.numpy()).max() <= 1e-15 * grad_scale
    assert (np.abs(r["d_sil"] - z.grad.numpy()) <= 1e-15 * np.abs(r["d_sil"]) + 1e-300).all()
    assert r["abs_l1"] == pytest.approx(abs(r["l1"]), rel=1e-15) and r["abs_bce"] == pytest.approx(r["bce"], rel=1e-15)
    # |d| <= 1 takes the same value at |d| = 1; another beta is another loss
    r2 = S.f0_sil_loss_ref(f0p, f0, silp, sil, lam, grad_scale, inclusive=True)
    assert r2["l1"] == r["l1"] and np.array_equal(r2["d_f0"], r["d_f0"])
    r3 = S.f0_sil_loss_ref(f0p, f0, silp, sil, lam, grad_scale, beta=0.5)
    assert abs(r3["l1"] - r["l1"]) > 1e-4 * r["l1"]
    b = f0p.double().requires_grad_(True)
    l1b = torch.nn.SmoothL1Loss(beta=0.5)(b, f0.double())
    assert abs(r3["l1"] - lam * l1b.item()) <= 1e-15 * abs(r3["l1"])


def test_head_ref_is_autograd():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(37, 12, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(3, 12, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(3, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(37, generator=g, dtype=torch.float64)
    y = (x @ w.T + b).sum(-1)
    y.backward(dy)
    r = S.head_ref(x, w, b, dy)
    assert np.abs(r["y"][0] - y.detach().numpy()).max() <= 1e-14
    assert np.abs(r["dx"][0] - x.grad.numpy()).max() <= 1e-14
    for o in range(3):
        assert np.abs(r["dw"][0] - w.grad[o].numpy()).max() <= 1e-13
        assert abs(r["db"][0] - b.grad[o].item()) <= 1e-13
    for v, mag in r.values():
        assert (np.abs(v) <= mag * (1 + 1e-12)).all()


@pytest.mark.parametrize("pool", [1, 2, 3, 5, 10])
def test_maxpool_ref_positions_are_torch_indices_under_ties(pool):
    Fq, C, B, T = 23, 8, 2, 3
    g = torch.Generator().manual_seed(pool)
    x = torch.randint(-2, 3, (B, T, Fq, C), generator=g).float()     # integers in [-2, 2]: full of ties
    x[torch.rand(B, T, Fq, C, generator=g) < 0.2] *= -0.0            # some zeros become -0.0
    val, pos = S.maxpool_ref(x.numpy(), pool)
    y, idx = F.max_pool2d(x.permute(0, 3, 1, 2), (1, pool), return_indices=True)      # NCHW, flat index t * F + f
    Fo = Fq // pool
    assert val.shape == (B, T, Fo, C) and pos.dtype == np.uint8
    assert np.array_equal(val, y.permute(0, 2, 3, 1).numpy())
    f_idx = (idx % Fq).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(pos.astype(np.int64) + np.arange(Fo)[None, None, :, None] * pool, f_idx)
    if pool > 1:
        assert not np.array_equal(S.maxpool_ref(x.numpy(), pool, last=True)[1], pos)
    assert np.array_equal(S.maxpool_ref(x.numpy(), pool, last=True)[0], val)


def test_maxpool_ref_empty_when_window_exceeds_rows():
    val, pos = S.maxpool_ref(np.zeros((2, 3, 4, 8), np.float32), 5)
    assert val.shape == (2, 3, 0, 8) and pos.shape == (2, 3, 0, 8)


def test_dropout_keep_ref_keeps_everything_at_p_zero():
    for seed, off in ((123, 0), (2 ** 63 + 5, 7), (5, 2 ** 32 - 3), (5, 2 ** 40 + 1)):
        assert S.dropout_keep_ref(seed, off, 1000, 0.0).all()


@pytest.mark.parametrize("offset,n,k", [(0, 64, 1), (7, 100, 37), (2 ** 32 - 3, 10, 3), (2 ** 32 - 3, 10, 2),
                                        (2 ** 40 + 1, 33, 32), (2 ** 64 - 2, 8, 2)])
def test_dropout_keep_ref_reproduces_itself_across_an_offset_split(offset, n, k):
    """mask(offset, n) == mask(offset, k) ++ mask(offset + k, n - k), also where the 64-bit counter crosses 2^32 (its
    high word c[1] changes inside the range) and where it wraps."""
    seed, p = 2 ** 63 + 5, 0.5
    whole = S.dropout_keep_ref(seed, offset, n, p)
    parts = np.concatenate([S.dropout_keep_ref(seed, offset, k, p), S.dropout_keep_ref(seed, offset + k, n - k, p)])
    assert whole.shape == (4 * n,) and np.array_equal(whole, parts)
    assert 0.3 < whole.mean() < 0.7 or n < 16
    # the counter's high word matters: the same low words under another high word draw another mask
    assert not np.array_equal(S.dropout_keep_ref(seed, offset, n, p), S.dropout_keep_ref(seed, offset + 2 ** 32, n, p))


def test_dropout_keep_ref_is_the_known_answer_stream():
    """Counter {lo, hi, 0, 0}, key = seed halves: the Random123 known answer of tests/test_noise_cpu.py's Philox, seen
    through the keep rule."""
    from tests import noise_ref
    w = noise_ref.philox4x32(0xFFFFFFFFFFFFFFFF, [0xFFFFFFFFFFFFFFFF])
    keep = S.keep_from_words(w, 0.5)
    assert np.array_equal(keep, ((w.reshape(-1) >> 8) >= 2 ** 23).astype(np.uint8))
    assert np.array_equal(S.dropout_keep_ref(0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 1, 0.5), keep)
    assert S.dropout_scale(0.5) == 2.0 and S.dropout_scale(0.0) == 1.0
    assert not np.array_equal(S.dropout_keep_ref(5, 0, 4096, 0.5, rounds=9), S.dropout_keep_ref(5, 0, 4096, 0.5))
