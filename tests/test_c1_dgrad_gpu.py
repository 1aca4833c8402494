"""Data gradient of the first convolution (pe_conv3x3_c1_dgrad) against torch.nn.grad.conv2d_input in float64.

The operation is linear in dy, so every element is held to a rounding bound, none is left out.  The kernel multiplies
in plain fp32 (no split-product form: the weights are 576 floats in registers, there is no matrix pipe in it) and adds
with fp32 FMAs / adds, 576 terms per output in a fixed order, so

    |dx - ref| <= 576 * 2^-24 * (|w| (*) |dy|)        per element,

the standard n * u bound of a length-576 sum, with the operands as stored: a bf16 / fp16 dy is rounded first and the
reference is computed from the rounded values (as tests/half_ref.py does), widening is exact.
"""
import numpy as np
import pytest
import torch

from pitchextractor_amd import ops

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
# (B, T, F): every pixel a corner or an edge | small | odd T, the model's F, 2 x 5 tiles with a tail | 31 = 30 + 1 rows
# and 20 = 16 + 4 columns: one row and four columns past the 30 x 16 tile, pixel count no multiple of it
SHAPES = [(2, 1, 4), (2, 5, 8), (3, 37, 80), (1, 31, 20)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def operands(B, T, F, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    dy = (torch.randn(B, T, F, 64, generator=g) * 0.7).to(dtype)
    w = torch.randn(64, 1, 3, 3, generator=g) * 0.3
    return dy, w


def reference(dy, w):
    """(dx, bound) in float64 from the stored operands: dy [B,T,F,64] of any float type, w [64,1,3,3] float32."""
    B, T, F, _ = dy.shape
    d64, w64 = dy.double().permute(0, 3, 1, 2).contiguous(), w.double()
    dx = torch.nn.grad.conv2d_input((B, 1, T, F), w64, d64, padding=1)[:, 0]
    mag = torch.nn.grad.conv2d_input((B, 1, T, F), w64.abs(), d64.abs(), padding=1)[:, 0]
    return dx.numpy(), (576 * U * mag).numpy()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("B,T,F", SHAPES)
def test_matches_conv2d_input_float64(hip_device, B, T, F, dtype):
    dy, w = operands(B, T, F, dtype, seed=B * 1000 + T)
    ref, bound = reference(dy, w)
    got = ops.conv3x3_c1_dgrad(dy.to(hip_device), w.to(hip_device))
    assert got.shape == (B, T, F) and got.dtype == torch.float32 and got.is_contiguous()
    err = np.abs(got.cpu().double().numpy() - ref)
    print(f"{(B, T, F)} {dtype}: max err / bound = {(err / bound).max():.3f}, max err = {err.max():.3e}")
    assert (err <= bound).all(), (float((err / bound).max()), int((err > bound).sum()))


def test_writes_into_a_given_output_and_is_deterministic(hip_device):
    dy, w = operands(3, 37, 80, torch.float32, seed=5)
    dyd, wd = dy.to(hip_device), w.to(hip_device)
    out = torch.full((3, 37, 80), 7.0, device=hip_device)
    assert ops.conv3x3_c1_dgrad(dyd, wd, out=out) is out
    assert torch.equal(out, ops.conv3x3_c1_dgrad(dyd, wd))
    # the same sample gives the same bits wherever it sits in a larger batch (the grid is split per sample and tile)
    big = ops.conv3x3_c1_dgrad(dyd.repeat(3, 1, 1, 1), wd)
    assert torch.equal(big[:3], out) and torch.equal(big[6:], out)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_one_pixel_spreads_the_flipped_stencil(hip_device, dtype):
    """dy non-zero in ONE pixel (t0, f0): dx[t0 + i - 1, f0 + j - 1] = sum_co w[co, i, j] * dy[co] for the nine (i, j),
    whatever falls outside the grid is dropped, everything else is exactly zero.  The pixel visits the corners, the
    edges and the interior."""
    T, F = 5, 8
    g = torch.Generator().manual_seed(9)
    w = torch.randn(64, 1, 3, 3, generator=g)
    v = torch.randn(64, generator=g).to(dtype)
    for t0 in (0, 2, T - 1):
        for f0 in (0, 3, F - 1):
            dy = torch.zeros(1, T, F, 64, dtype=dtype)
            dy[0, t0, f0] = v
            got = ops.conv3x3_c1_dgrad(dy.to(hip_device), w.to(hip_device))[0].cpu().double().numpy()
            want, bound = np.zeros((T, F)), np.zeros((T, F))
            for i in range(3):
                for j in range(3):
                    t, f = t0 + i - 1, f0 + j - 1
                    if 0 <= t < T and 0 <= f < F:
                        want[t, f] = (w[:, 0, i, j].double() * v.double()).sum().item()
                        bound[t, f] = 64 * U * (w[:, 0, i, j].double().abs() * v.double().abs()).sum().item()
            assert (np.abs(got - want) <= bound).all(), (t0, f0)
            assert ((got != 0) == (want != 0)).all(), (t0, f0)


def test_refuses_what_the_kernel_does_not_serve(hip_device):
    w = torch.zeros(64, 1, 3, 3, device=hip_device)
    with pytest.raises(Exception):
        ops.conv3x3_c1_dgrad(torch.zeros(1, 4, 6, 64, device=hip_device), w)              # F % 4 != 0
    with pytest.raises(ValueError):
        ops.conv3x3_c1_dgrad(torch.zeros(1, 4, 8, 32, device=hip_device), w)              # not 64 channels
    with pytest.raises(ValueError):
        ops.conv3x3_c1_dgrad(torch.zeros(1, 4, 8, 64), w)                                 # host tensor
