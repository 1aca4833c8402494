"""JDCNet as a differentiable function of its input: ``x.grad`` after a backward, in train and eval mode, for both
heads, in every fp32 product mode and with bf16 activation storage; the frozen (loss-network) mode.

Reference: tests/golden/input_grad_golden.npz, the reference model's float64 input gradient of the training loss on
``golden_input(3, T=T)`` (tests/golden/make_input_grad_golden.py).  Model, inputs and loss (``ops.f0_sil_loss``) are
those of tests/test_model_gpu.py::train_pass.  Tolerances are the ones test_gradients_match_reference_float64 holds the
parameter gradients to -- 5e-3 of the tensor's largest element, 2e-3 on the norm -- because the input gradient is one
more data-gradient product down the same chain.  At most 1 % of the elements may miss the element bound: the network
has max-pools and LeakyReLU kinks, and a near-tie that rounds the other way moves a whole gradient path.  That 1 % is
a condition, not a measurement: the float32 oracle leaves out none on these inputs
(tests/test_input_grad_cpu.py), and the 8.75 % of pixels on the border of a 32 x 80 grid cannot hide under it.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import model_ref
from pitchextractor_amd import inference, ops
from pitchextractor_amd import model as pe_model
from pitchextractor_amd.model import JDCNet
from tests.golden.make_golden import SEQ_CFG, TF_CFG, golden_input, golden_targets
from tests.test_transformer_gpu import BF16_GRAD_TOL

pytestmark = pytest.mark.gpu
SEED = 3
ELEM_TOL, NORM_TOL, MAX_OUTLIERS = 5e-3, 2e-3, 0.01
BF16_ELEM_TOL = {"eval": 2 * 0.292, "train": 2 * 0.195}     # see test_input_gradient_with_bf16_activation_storage
WGRAD_CALLS = ("pe_conv3x3_wgrad", "pe_conv3x3_c1_wgrad", "pe_gemm_tn", "pe_lstm_whh_grad", "pe_colsum")


@functools.lru_cache(maxsize=None)
def head_state(head):
    if head == "tf":
        return model_ref.seeded_state(11, num_class=1, model_type="transformer")
    return model_ref.seeded_state(11, num_class=1, hidden_size=384)


def build(head, device):
    cfg = dict(TF_CFG, dropout=0.0) if head == "tf" else dict(SEQ_CFG, hidden_size=384, dropout=0.0)
    net = JDCNet(num_class=1, sequence_model_config=cfg)
    net.load_state_dict(head_state(head), strict=True)
    net.block_dropout = 0.0
    return net.to(device)


def batch(T, device):
    f0, sil = (t.to(device) for t in golden_targets(SEED, T=T))
    return golden_input(SEED, T=T).to(device), f0, sil


def step(net, x, f0, sil, want_dx=True):
    """Forward, ``f0_sil_loss`` and backward as in train_pass; returns (x.grad or None, cls, det)."""
    x = x.clone().requires_grad_(want_dx)
    cls, det = net(x)
    _, d_f0, d_sil = ops.f0_sil_loss(cls.detach().reshape(-1), f0.reshape(-1), det.detach().reshape(-1),
                                     sil.reshape(-1), 0.1)
    torch.autograd.backward([cls, det], [d_f0.view_as(cls), d_sil.view_as(det)])
    return x.grad, cls.detach(), det.detach()


def check_dx(dx, ref, what, elem_tol=ELEM_TOL, norm_tol=NORM_TOL, max_outliers=MAX_OUTLIERS):
    got = dx.detach().cpu().double().numpy()
    assert got.shape == ref.shape
    err = np.abs(got - ref) / np.abs(ref).max()
    out = float((err > elem_tol).mean())
    nerr = abs(np.linalg.norm(got) - np.linalg.norm(ref)) / np.linalg.norm(ref)
    print(f"{what}: max |dx - golden| / max|golden| = {err.max():.3e}, beyond {elem_tol:g}: {100 * out:.3f} %, "
          f"norm error {nerr:.3e}")
    assert out <= max_outliers, (what, out, float(err.max()))
    assert nerr <= norm_tol, (what, nerr)


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(golden_dir / "input_grad_golden.npz")


@pytest.fixture(scope="module", params=["h2", "x3", "native"])
def fp32_mode(request):
    prev, ops.FP32_MATMUL = ops.FP32_MATMUL, request.param
    yield request.param
    ops.FP32_MATMUL = prev


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("head", ["bilstm", "tf"])
def test_input_gradient_matches_reference_float64(G, hip_device, fp32_mode, head, mode):
    """T = 32, both heads, eval and train mode, parameters trainable.  In eval mode the parameter gradients are those
    of nn.BatchNorm2d.eval() under autograd: every norm within 2e-3 of the reference's."""
    net = build(head, hip_device).train(mode == "train")
    x, f0, sil = batch(32, hip_device)
    dx, _, _ = step(net, x, f0, sil)
    assert dx.shape == x.shape == (2, 1, 32, 80) and dx.dtype == x.dtype and dx.is_contiguous()
    check_dx(dx, G[f"{head}_T32_{mode}_dx"], f"{fp32_mode} {head} T=32 {mode}")
    assert not ops.persistent_lstm_error(hip_device)
    if mode == "eval":
        norms = dict(zip((str(n) for n in G[f"{head}_grad_names"]), G[f"{head}_T32_eval_grad_norms"]))
        bad = [(n, p.grad.double().norm().item(), norms[n]) for n, p in net.named_parameters()
               if abs(p.grad.double().norm().item() - norms[n]) > 2e-3 * norms[n] + 1e-12]
        assert not bad, bad


def test_input_gradient_at_full_length(G, hip_device, monkeypatch):
    """T = 192, BiLSTM, eval, "h2" (the float32 reference: 0 elements beyond 5e-3, norm error 6e-7)."""
    monkeypatch.setattr(ops, "FP32_MATMUL", "h2")
    net = build("bilstm", hip_device).eval()
    dx, _, _ = step(net, *batch(192, hip_device))
    check_dx(dx, G["bilstm_T192_eval_dx"], "h2 bilstm T=192 eval")


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_input_gradient_with_bf16_activation_storage(G, hip_device, mode):
    """Mixed precision with bf16 activation tensors (BiLSTM, T = 32) against the float64 golden.  The norm is held to
    BF16_GRAD_TOL (tests/test_transformer_gpu.py).  Element by element, the 2e-2 of the tensor's largest element that
    tests/test_model_gpu.py states for the gradients of the bf16 BiLSTM step does not fit: that test compares two
    bf16 runs that round alike, this one a bf16 run with float64.  Every pixel of the input gradient is a sum of
    cancelling terms that went through fourteen bf16 convolutions, and bf16 storage makes exact ties in the max-pools
    common, so whole gradient paths move while the norm hardly does.  Measured against the golden: largest element error
    0.292 of the largest element in eval mode (norm error 4.7e-3) and 0.195 in train mode; the bounds are twice that."""
    net = build("bilstm", hip_device).train(mode == "train")
    with ops.matmul_bf16(True, "bf16", act16=True):
        dx, _, _ = step(net, *batch(32, hip_device))
    assert dx.dtype == torch.float32
    check_dx(dx, G[f"bilstm_T32_{mode}_dx"], f"bf16 act16 bilstm T=32 {mode}",
             elem_tol=BF16_ELEM_TOL[mode], norm_tol=BF16_GRAD_TOL, max_outliers=0.0)


class _Reducer:
    def __init__(self):
        self.calls = []

    def reduce_range(self, *a, **k):
        self.calls.append((a, k))


@pytest.mark.parametrize("head", ["bilstm", "tf"])
def test_frozen_network_computes_the_input_gradient_and_nothing_else(hip_device, head, monkeypatch):
    x, f0, sil = batch(32, hip_device)
    ref_dx, ref_cls, ref_det = step(build(head, hip_device).eval(), x, f0, sil)

    net = build(head, hip_device).eval().requires_grad_(False)
    assert net.is_frozen()
    dp = _Reducer()
    net.attach_data_parallel(dp)
    calls, streams, orig_call, orig_side = [], [], ops._call, pe_model._side_stream
    monkeypatch.setattr(ops, "_call", lambda name, *a, **k: (calls.append(name), orig_call(name, *a, **k))[1])
    monkeypatch.setattr(pe_model, "_side_stream", lambda dev: (streams.append(dev), orig_side(dev))[1])
    dx, cls, det = step(net, x, f0, sil)
    assert torch.equal(cls, ref_cls) and torch.equal(det, ref_det)
    assert torch.equal(dx, ref_dx)                                  # bit for bit the unfrozen eval-mode gradient
    assert all(p.grad is None for p in net.parameters())
    assert net._grad_flat is None
    assert dp.calls == [] and streams == []
    assert not [c for c in calls if c in WGRAD_CALLS], sorted(set(calls))
    assert calls.count("pe_conv3x3_c1_dgrad") == 1
    assert net.backward_status.shape == (1,) and net.backward_status.is_cuda and net.backward_status.item() == 0
    # without an input that requires grad there is nothing to differentiate
    cls2, _ = net(x)
    assert not cls2.requires_grad


@pytest.mark.parametrize("train", [False, True], ids=["eval_frozen", "train"])
def test_checkpointed_forward_gives_the_same_input_gradient(hip_device, train):
    x, f0, sil = batch(32, hip_device)
    outs = []
    for ckpt in (False, True):
        net = build("bilstm", hip_device).train(train)
        if not train:
            net.requires_grad_(False)
        net.checkpoint_forward = ckpt
        outs.append(step(net, x, f0, sil)[0])
    assert torch.equal(outs[0], outs[1])


def test_training_step_is_unchanged_when_the_input_takes_no_gradient(hip_device, monkeypatch):
    """x without requires_grad: the launches are those of a training step (no input-gradient kernel), and outputs and
    parameter gradients equal, bit for bit, those of a second, untouched model whose input does take one."""
    x, f0, sil = batch(32, hip_device)
    calls, orig_call = [], ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a, **k: (calls.append(name), orig_call(name, *a, **k))[1])
    a = build("bilstm", hip_device).train()
    dx_a, cls_a, det_a = step(a, x, f0, sil, want_dx=False)
    assert dx_a is None and "pe_conv3x3_c1_dgrad" not in calls
    assert calls.count("pe_conv3x3_c1_wgrad") == 1
    plain = list(calls)
    calls.clear()
    b = build("bilstm", hip_device).train()
    dx_b, cls_b, det_b = step(b, x, f0, sil, want_dx=True)
    assert dx_b is not None and [c for c in calls if c != "pe_conv3x3_c1_dgrad"] == plain
    assert torch.equal(cls_a, cls_b) and torch.equal(det_a, det_b)
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
    assert torch.equal(a.status_slot(), b.status_slot())


def test_load_model_frozen(hip_device, tmp_path):
    torch.save({"model": head_state("bilstm")}, tmp_path / "m.pth")
    net = inference.load_model(tmp_path / "m.pth", device=hip_device, frozen=True)
    assert not net.training and net.is_frozen() and not any(p.requires_grad for p in net.parameters())
    x, f0, sil = batch(32, hip_device)
    dx, _, _ = step(net, x, f0, sil)
    assert dx is not None and dx.shape == x.shape and torch.isfinite(dx).all() and dx.abs().max() > 0
    assert all(p.grad is None for p in net.parameters())
    assert inference.load_model(tmp_path / "m.pth", device=hip_device).classifier.weight.requires_grad
