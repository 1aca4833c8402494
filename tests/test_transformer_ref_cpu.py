"""oracle.model_ref.transformer_head off its defaults, against stock torch.nn.TransformerEncoder in float64.

The golden vectors pin the oracle at one geometry (nhead = 8, T = 192, dim_feedforward = 1536); the GPU shape tests
lean on it at other head counts, lengths and widths, so it is held here to the module it restates: outputs and the
input gradient to 1e-10 of the tensor's largest magnitude (float64 on both sides, only summation orders differ)."""
import pytest
import torch
import torch.nn as nn

from oracle import model_ref

D = 512
PREFIX = "sequence_classifier"


def _stock_head(state, nhead, ff):
    layer = nn.TransformerEncoderLayer(D, nhead, ff, dropout=0.0, batch_first=True, activation="gelu")
    enc = nn.TransformerEncoder(layer, num_layers=2, enable_nested_tensor=False).double()
    pre = f"{PREFIX}.model."
    enc.load_state_dict({k[len(pre):]: v.double() for k, v in state.items() if k.startswith(pre)}, strict=True)
    norm = nn.LayerNorm(D, eps=1e-5).double()
    norm.load_state_dict({"weight": state[f"{PREFIX}.layer_norm.weight"].double(),
                          "bias": state[f"{PREFIX}.layer_norm.bias"].double()})
    pe = state[f"{PREFIX}.pos_encoding.pe"].double()
    enc.train()                      # dropout is 0; train mode keeps the module off its fused inference path
    return lambda x: enc(norm(x + pe[:, :x.shape[1]]))


@pytest.mark.parametrize("nhead,T,ff", [(4, 40, 256), (16, 36, 512), (8, 100, 1024)])
def test_transformer_head_oracle_matches_stock_encoder(nhead, T, ff):
    B = 2
    state = model_ref.seeded_state(17, model_type="transformer", num_layers=2, nhead=nhead, dim_feedforward=ff)
    st64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in state.items()}
    cfg = {"model_type": "transformer", "num_layers": 2, "nhead": nhead, "dim_feedforward": ff, "dropout": 0.0}
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    dy = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    outs = []
    for fn in (_stock_head(state, nhead, ff),
               lambda t: model_ref.transformer_head(t, st64, PREFIX, cfg, train=True, masks=None)):
        xi = x.clone().requires_grad_(True)
        y = fn(xi)
        y.backward(dy)
        outs.append((y.detach(), xi.grad))
    (y_ref, dx_ref), (y, dx) = outs
    assert y.shape == (B, T, D)
    assert (y - y_ref).abs().max().item() <= 1e-10 * y_ref.abs().max().item()
    assert (dx - dx_ref).abs().max().item() <= 1e-10 * dx_ref.abs().max().item()


def test_transformer_head_oracle_refuses_more_frames_than_positions():
    state = model_ref.seeded_state(17, model_type="transformer", num_layers=2, nhead=8, dim_feedforward=256,
                                   max_len=32)
    st64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in state.items()}
    cfg = {"model_type": "transformer", "num_layers": 2, "nhead": 8, "dim_feedforward": 256, "dropout": 0.0}
    x = torch.zeros(2, 40, D, dtype=torch.float64)
    with pytest.raises(RuntimeError):
        model_ref.transformer_head(x, st64, PREFIX, cfg, train=False, masks=None)
    model_ref.transformer_head(x[:, :32], st64, PREFIX, cfg, train=False, masks=None)      # T == max_len is fine
