"""The nine-tap weight-gradient kernel (csrc/conv.hip conv3x3_wgrad9_x3_kernel) on border-heavy shapes: short
utterances (T = 1 .. 3, so many utterance boundaries fall inside every 32-pixel k-tile), narrow frequency axes
(F = 10 / 20: X staged as one halo; F = 40: three row windows), P not a multiple of 32 and more than one k-split.
Border taps read an all-zero LDS row instead of masking the fragment, so every wrong redirect shows up here as a
product with a neighbour from the other side of a border.

h2 / x3 are held to the float64 split models with the bounds of tests/test_split_products_gpu.py, the 16-bit
operand modes to float64 of the rounded operands, and every mode to torch.nn.grad.conv2d_weight of the fp32
operands in float64 (loosely: that is what the product approximates).  A second call must return the same bits."""
import pytest
import torch

from pitchextractor_amd import ops
from tests import half_ref as R
from tests import split_ref as S
from tests.plan_ref import wgrad_tile_and_splits
from tests.test_ops_gpu import close, nhwc, rnd
from tests.test_split_products_gpu import ACC_EXTRA, acc_tol, check, model

pytestmark = pytest.mark.gpu

# (B, T, F, Cin, Cout): P = B T F is not a multiple of 32 and above 2048 (two or more k-splits)
BORDER_SHAPES = [(41, 5, 10, 64, 64), (103, 1, 20, 64, 128), (37, 3, 20, 128, 64), (70, 3, 10, 64, 192),
                 (27, 2, 40, 64, 64)]


def _splits(P):
    """k-splits of wgrad_plan for a single 64 x 64 tile (csrc/conv.hip)"""
    return wgrad_tile_and_splits(P, 64, 64)[1]


def test_border_shapes_are_border_heavy():
    for B, T, Fq, Ci, Co in BORDER_SHAPES:
        assert (B * T * Fq) % 32 and T <= 5 and _splits(B * T * Fq) >= 2
    assert {2 * Fq + 34 <= 80 for _, _, Fq, _, _ in BORDER_SHAPES} == {True, False}    # halo and three windows


def _run_twice(x, dy, Ci, Co):
    dws = []
    for _ in range(2):
        dw = torch.full((Co, Ci, 3, 3), float("nan"), device=x.device)
        ops.conv3x3_wgrad(x, dy, dw)
        dws.append(dw)
    torch.cuda.synchronize()
    assert torch.equal(dws[0].view(torch.int32), dws[1].view(torch.int32)), "not deterministic"
    return dws[0]


@pytest.mark.parametrize("B,T,Fq,Ci,Co", BORDER_SHAPES)
@pytest.mark.parametrize("mode", ("h2", "x3"))
def test_wgrad9_borders_split(hip_device, B, T, Fq, Ci, Co, mode, monkeypatch):
    monkeypatch.setattr(ops, "FP32_MATMUL", mode)
    x = rnd(B, Ci, T, Fq, seed=B + Fq)
    dy = rnd(B, Co, T, Fq, seed=T + Co)
    dw = _run_twice(nhwc(x).to(hip_device), nhwc(dy).to(hip_device), Ci, Co)
    check(dw, model(mode, S.op_wgrad, x, dy), acc_tol(B * T * Fq, mode, ACC_EXTRA + 64))
    close(dw, torch.nn.grad.conv2d_weight(x.double(), (Co, Ci, 3, 3), dy.double(), padding=1))


@pytest.mark.parametrize("B,T,Fq,Ci,Co", BORDER_SHAPES)
@pytest.mark.parametrize("half", ("bf16", "f16"))
def test_wgrad9_borders_half(hip_device, B, T, Fq, Ci, Co, half):
    x = rnd(B, Ci, T, Fq, seed=B + Fq)
    dy = rnd(B, Co, T, Fq, seed=T + Co)
    with ops.matmul_bf16(True, half):
        dw = _run_twice(nhwc(x).to(hip_device), nhwc(dy).to(hip_device), Ci, Co)
    close(dw, torch.nn.grad.conv2d_weight(R.hr(x, half), (Co, Ci, 3, 3), R.hr(dy, half), padding=1))
