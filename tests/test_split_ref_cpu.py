"""CPU self-test of the float64 split models in tests/split_ref.py (no GPU): the x3 split is exact where it should be
and its loss below is pinned, the h2 split obeys its operand error bound and the precision table in its docstring,
the h2 product model stays within the bound that follows, and the scale puts every tensor maximum in [2^13, 2^14)."""
import math

import numpy as np
import torch

from tests import split_ref as S


def _random_f32(n, seed):
    """n random float32 bit patterns (finite, both signs, every exponent)"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32)
    return torch.from_numpy(x[np.isfinite(x)].copy())


def test_x3_split_is_exact_down_to_2_pow_minus_110_and_loses_little_below():
    x = _random_f32(2_000_000, 1)
    x = torch.cat([x, torch.tensor([S.X3_EXACT_MIN, -S.X3_EXACT_MIN, 3.4028235e38, 2.0 ** -126, 1e-45, 0.0])])
    hi, mid, lo = S.split_x3(x)
    back = hi + mid + lo                                       # exact in float64: 3 x 8 bits at nearby exponents
    xd = x.double()
    exact = back == xd
    big = xd.abs() >= S.X3_EXACT_MIN
    assert exact[big].all()
    # below 2^-110 the second residual can be an fp32 subnormal; truncating it to bf16 drops bits: pin how many
    bad = ~exact
    assert bad.any() and (xd[bad].abs() < S.X3_EXACT_MIN).all()
    assert ((back - xd).abs()[bad] < 2.0 ** -133).all()                  # < 2^16 subnormal ulps of 2^-149
    assert 0.03 < bad.double().mean().item() < 0.09                      # ~6 % of random bit patterns
    # every term is a bf16 value and the terms are the truncations split3 stores
    for t in (hi, mid, lo):
        assert torch.equal(t.float().to(torch.bfloat16).double(), t)
    assert torch.equal(hi, (x.view(torch.int32) & -65536).view(torch.float32).double())


def test_fp16_rounding_matches_torch_on_float32_values():
    """rne_f16 (numpy, one rounding from float64) == torch's float32 -> float16 on fp32 values, subnormals included"""
    x = torch.cat([torch.randn(200_000) * torch.exp2(torch.randint(-30, 17, (200_000,))),
                   torch.tensor([65519.0, 65520.0, 2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -24 * 1.5])])
    assert torch.equal(S.rne_f16(x.double()), x.to(torch.float16).double())


def test_h2_scale_puts_the_maximum_of_every_exponent_in_2_13_to_2_14():
    for E in range(0, 256):
        es = S.h2_scale_exp(E << 23)
        assert 1 <= es <= 253
        if 14 <= E <= 254:                                    # unclamped: max |x| s in [2^13, 2^14) for every mantissa
            for m in (0, 1, 0x400000, 0x7FFFFF):
                v = float(np.array((E << 23) | m, dtype=np.uint32).view(np.float32))
                assert 2.0 ** 13 <= v * S.h2_scale(E << 23) < 2.0 ** 14, (E, m)
        elif E < 14:                                          # zero / subnormal / tiny words: 2^126, no overflow
            assert es == 253
            v = float(np.array((E << 23) | 0x7FFFFF, dtype=np.uint32).view(np.float32))
            assert v * S.h2_scale(E << 23) < 2.0 ** 13
        else:                                                 # Inf / NaN word
            assert es == 12
    assert S.h2_scale_exp(0) == 253 and S.h2_scale_exp(1) == 253 and S.h2_scale_exp(0x7FC00000) == 12


def test_h2_split_obeys_its_operand_bound_and_reproduces_the_precision_table():
    for top in ("below", "pow2"):
        for scale in (1.0, 2.0 ** -70, 2.0 ** 60):
            x = S.heavy((64, 900), 1, seed=3, top=top, scale=scale)
            A = x.abs().max().item()
            hi, lo, s = S.split_h2(x)
            err = ((hi + lo) / s - x.double()).abs()
            assert (err <= S.H2_REL * x.double().abs() + S.H2_ABS * A).all()
            assert (hi.abs() <= 2.0 ** 14).all() and hi.abs().max().item() >= 2.0 ** 13     # (RNE may reach 2^14)
    # full binades at or above 2^-14 A: 2^-23 relative
    g = torch.Generator().manual_seed(4)
    amax = torch.tensor([1.5], dtype=torch.float32)
    for k in (0, 8, 14):
        x = torch.cat([((torch.rand(100_000, generator=g, dtype=torch.float64) + 1) * 2.0 ** -k * 0.75).float(), amax])
        hi, lo, s = S.split_h2(x)
        rel = (((hi + lo) / s - x.double()).abs() / x.double().abs())[:-1].max().item()
        assert -23.01 < math.log2(rel) <= -23.0, (k, rel)
    # at 2^-k of the maximum (A = 1.5, A s = 1.5 2^13), k >= 16: the absolute error 2^-25 / s of an fp16 subnormal
    # term, i.e. relative 2^(k - 38.58) -- one bit per binade
    table = {16: -22.6, 20: -18.6, 24: -14.6, 28: -10.6, 32: -6.6, 38: -1.6}
    for k, want in table.items():
        x = torch.cat([(2.0 ** -k * 1.5 * (1 + torch.rand(100_000, generator=g, dtype=torch.float64) / 64)).float(),
                       amax])
        hi, lo, s = S.split_h2(x)
        rel = (((hi + lo) / s - x.double()).abs() / x.double().abs())[:-1].max().item()
        assert abs(math.log2(rel) - want) < 0.05, (k, math.log2(rel))


def test_h2_product_model_stays_within_the_bound_that_follows():
    """|model - a.b| <= sum_k (e_a|b| + |a|e_b + e_a e_b + |lo_a lo_b| / (s_a s_b)), e = 2^-23|x| + 2^-38 A"""
    a = S.heavy((70, 300), 0, seed=5)
    b = S.heavy((50, 300), 1, seed=6, top="pow2", scale=2.0 ** -20)
    val, mag = S.h2_product(S.op_nt, a, b)
    ex = a.double() @ b.double().T
    A, B = a.abs().max().item(), b.abs().max().item()
    ea = S.H2_REL * a.double().abs() + S.H2_ABS * A
    eb = S.H2_REL * b.double().abs() + S.H2_ABS * B
    _, la, sa = S.split_h2(a)
    _, lb, sb = S.split_h2(b)
    bound = ea @ b.double().abs().T + a.double().abs() @ eb.T + ea @ eb.T + (la.abs() @ lb.abs().T) / (sa * sb)
    assert ((val - ex).abs() <= bound * (1 + 1e-12)).all()
    assert (mag >= 0).all() and torch.isfinite(val).all()
    # the bound is not vacuous: rows of a at 2^-36 of its maximum lose most of their bits
    rel = ((val - ex).abs() / (a.double().abs() @ b.double().abs().T + 1e-300))
    assert rel[S.KS.index(36)::len(S.KS)].max().item() > 2.0 ** -6 and rel[0].max().item() < 2.0 ** -21


def test_conv_models_match_torch():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 5, 6, 7, generator=g, dtype=torch.float64)
    w = torch.randn(4, 5, 3, 3, generator=g, dtype=torch.float64)
    dy = torch.randn(2, 4, 6, 7, generator=g, dtype=torch.float64)
    assert torch.allclose(S.op_conv(x, w), torch.nn.functional.conv2d(x, w, padding=1), rtol=1e-12, atol=1e-12)
    assert torch.allclose(S.op_conv(dy, S.dgrad_weight(w)), torch.nn.grad.conv2d_input(x.shape, w, dy, padding=1),
                          rtol=1e-12, atol=1e-12)
    assert torch.allclose(S.op_wgrad(x, dy), torch.nn.grad.conv2d_weight(x, w.shape, dy, padding=1), rtol=1e-12,
                          atol=1e-12)


def test_heavy_operands():
    x = S.heavy((9, 20), 0, seed=8)
    assert (x == 0).any() and ((x != 0) & (x.abs() < 2.0 ** -126)).any()
    assert x.view(-1)[-1].abs() == x.abs().max() and x.abs().max().item() == 1 - 2.0 ** -24
    ratio = x.abs().amax(1)[:-1] / x.abs().max()
    for i in range(8):
        assert 2.0 ** -S.KS[i] * 0.01 < ratio[i] < 2.0 ** -S.KS[i]
    assert S.heavy((9, 20), 1, seed=8, top="pow2", scale=4.0).abs().max().item() == 4.0
