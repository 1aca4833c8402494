"""pe_lstm_whh_grad is pe_gemm_tn behind a time-shifted loader (csrc/splitk.h: one kernel, one launcher, one reduce):
dW_hh must equal, bit for bit, the TN product of dgates with a materialised copy of y shifted by one step, in every
product form.  H = 128 puts both sides on the 128 x 128 tile and so on the same plan; y is a slice of a [B, T, 2H]
buffer (ldy != H) on the LSTM side and dense on the GEMM side."""
import pytest
import torch

from pitchextractor_amd import ops
from tests.plan_ref import whh_splits
from tests.test_ops_gpu import rnd

pytestmark = pytest.mark.gpu

H = 128
SIZES = [(3, 11), (9, 301)]        # K = 33: one split, K % 32 != 0;  K = 2709: five splits of 544, the last ragged


def test_sizes_take_the_direct_and_the_slab_path():
    for multi in (False, True):
        assert whh_splits(3, 11, H, multi) == 1 and whh_splits(9, 301, H, multi) > 1
    assert all((B * T) % 32 for B, T in SIZES)


@pytest.fixture(scope="module")
def operands(hip_device):
    out = {}
    for B, T in SIZES:
        dg = rnd(B, T, 4 * H, seed=B).to(hip_device)
        ybuf = torch.tanh(rnd(B, T, 2 * H, seed=T)).to(hip_device)
        out[(B, T)] = (dg, ybuf, ops.absmax(dg))
    return out


@pytest.mark.parametrize("B,T", SIZES)
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("form", ["native", "x3", "h2", "bf16", "f16"])
def test_lstm_whh_grad_equals_gemm_tn_of_shifted_y(hip_device, operands, form, reverse, B, T, monkeypatch):
    dg, ybuf, amax_dg = operands[(B, T)]
    y = ybuf[:, :, reverse * H:(reverse + 1) * H]
    ysh = torch.zeros(B, T, H, device=hip_device)                # y_shifted[b, t] = y[b, t -+ 1], zero at the open end
    if reverse:
        ysh[:, :-1] = y[:, 1:]
    else:
        ysh[:, 1:] = y[:, :-1]
    if form in ("bf16", "f16"):
        ctx = ops.matmul_bf16(True, form)
    else:
        monkeypatch.setattr(ops, "FP32_MATMUL", form)
        ctx = ops.matmul_bf16(False)
    # h2: the same two scale words on both sides (the LSTM side's default for y is the word of 1.0, not absmax(y))
    amax = (amax_dg, ops._unit_amax(hip_device)) if form == "h2" else (None, None)
    with ctx:
        dw = ops.lstm_whh_grad(ops.Scaled(dg, amax[0]), ops.Scaled(y, amax[1]),
                               torch.full((4 * H, H), float("nan"), device=hip_device), reverse, B, T, H)
        ref = ops.gemm_tn(ops.Scaled(dg.view(B * T, 4 * H), amax[0]), ops.Scaled(ysh.view(B * T, H), amax[1]))
    assert torch.equal(dw.view(torch.int32), ref.view(torch.int32))
    assert dw.abs().max() > 0
