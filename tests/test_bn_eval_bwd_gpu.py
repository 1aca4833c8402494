"""Eval-mode BatchNorm backward: pe_bn_act_pool_bwd / pe_bn_act_pool_tap_bwd with eval_mode = 1.

With running statistics the layer is the per-channel affine map z = scale * x + shift, so
    dx = scale * lrelu'(z) * unpool(dy)  (+ the tap's gradient where a tap is folded),
    dgamma = sum dz * (x - running_mean) / sqrt(running_var + eps),   dbeta = sum dz,
which is what nn.BatchNorm2d.eval() + LeakyReLU + max_pool2d give under autograd in float64.  The running statistics
sit far from the batch's own, so a pass that applied the batch-statistics terms would miss by orders of magnitude.
Tolerance: the 2e-5 of the tensor's scale that tests/test_ops_gpu.py holds the train-mode pass to.  The train-mode
passes must still leave the bits of the build before the mode existed (tests/golden/bn_bwd_train_bits.json).
"""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pitchextractor_amd import ops
from tests import bn_bwd_cases as cases

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SLOPE = 0.01
TOL = 2e-5
# F, C, tap_pool, channel offset of the tap (the folded-tap shapes of tests/test_tap_fold_gpu.py), BN pool 2
TAP_GEOMETRIES = [(80, 64, 40, 0), (40, 128, 20, 64), (20, 192, 10, 192)]


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def close(got, ref, tol=TOL):
    got, ref = got.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    assert got.shape == ref.shape
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    assert err <= tol * scale, (err, scale)


def eval_bn(C, seed=0):
    """nn.BatchNorm2d in eval mode (float64) whose running statistics are far from those of x ~ N(0.5, 2^2)."""
    bn = torch.nn.BatchNorm2d(C).double()
    with torch.no_grad():
        bn.weight.copy_(rnd(C, seed=seed + 2).abs() + 0.5)
        bn.bias.copy_(rnd(C, seed=seed + 3))
        bn.running_mean.copy_(rnd(C, seed=seed + 4) * 1.5 + 2.0)
        bn.running_var.copy_(rnd(C, seed=seed + 5).abs() * 3.0 + 0.3)
    return bn.eval()


def device_state(bn, dev):
    p = [t.detach().float().to(dev) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)]
    st = ops.bn_eval_affine(*p, eps=bn.eps)
    return st, p


@pytest.mark.parametrize("C,Fq,pool", [(64, 80, 1), (128, 40, 2), (192, 20, 2), (256, 10, 4), (64, 8, 4)])
def test_eval_backward_matches_torch_float64(hip_device, C, Fq, pool):
    dev, B, T = hip_device, 2, 5
    x = (rnd(B, C, T, Fq, seed=1) * 2 + 0.5).double().requires_grad_(True)
    bn = eval_bn(C)
    z = F.leaky_relu(bn(x), SLOPE)
    y = F.max_pool2d(z, (1, pool)) if pool > 1 else z
    dy = rnd(*y.shape, seed=6).double()
    y.backward(dy)
    st, (g, b, rm, rv) = device_state(bn, dev)
    # the state is complete: the statistics the layer normalised with, not uninitialised memory
    assert st.eval
    close(st.mean, bn.running_mean, 1e-7)
    close(st.invstd, 1.0 / torch.sqrt(bn.running_var + bn.eps), 1e-6)
    xd, dyd = nhwc(x.detach().float()).to(dev), nhwc(dy.float()).to(dev)
    close(ops.bn_act_pool_fwd(xd, st, pool=pool).permute(0, 3, 1, 2), y)
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    dx = ops.bn_act_pool_bwd(xd, dyd, st, dg, db, pool=pool)
    close(dx.permute(0, 3, 1, 2), x.grad)
    close(dg, bn.weight.grad)
    close(db, bn.bias.grad)
    # input gradient only: no parameter sums, no workspace, the same dx bit for bit
    w0, w1 = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2))
    dx_sums = ops.bn_act_pool_bwd(xd, dyd, st, dg, db, pool=pool, amax_out=w0)
    dx_only = ops.bn_act_pool_bwd(xd, dyd, st, None, None, pool=pool, amax_out=w1)
    assert torch.equal(dx_only, dx) and torch.equal(dx_sums, dx) and torch.equal(w0, w1)
    assert w0.view(torch.float32).item() == dx.abs().max().item()
    # bf16 storage: the same arithmetic, rounded once on the way out
    if pool in (1, 2, 4):
        x16 = xd.to(BF)
        dy16 = dyd.to(BF)
        ref16 = ops.bn_act_pool_bwd(x16.float(), dy16.float(), st, None, None, pool=pool)
        assert torch.equal(ops.bn_act_pool_bwd(x16, dy16, st, None, None, pool=pool), ref16.to(BF))


def test_train_state_needs_its_sums(hip_device):
    """Batch statistics have mean / projection terms: an input gradient without dgamma / dbeta exists in eval mode only."""
    x = rnd(1, 3, 8, 64, seed=1).to(hip_device)
    st = ops.bn_train_stats(x, torch.ones(64, device=hip_device), torch.zeros(64, device=hip_device), None, None)
    assert not st.eval
    with pytest.raises(ValueError):
        ops.bn_act_pool_bwd(x, x.clone(), st, None, None, pool=1)


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows", [3, 5])
@pytest.mark.parametrize("Fq,C,tap_pool,coff", TAP_GEOMETRIES)
def test_eval_backward_with_a_folded_tap(hip_device, Fq, C, tap_pool, coff, rows, dt):
    """The folded-tap pass in eval mode: dx = BN-block gradient + the tap's max-pool gradient, against float64 autograd
    (fp32 storage) and bit for bit against the two separate passes (both storage types), with and without the sums."""
    dev, pool, Ft = hip_device, 2, Fq // tap_pool
    xv = (rnd(1, rows, Fq, C, seed=1) * 3).to(BF).float()               # bf16-representable: both storage types
    dyv, dwv = rnd(1, rows, Fq // pool, C, seed=4).to(BF).float(), rnd(1, rows, Ft, 640, seed=5).to(BF).float()
    bn = eval_bn(C, seed=20)
    x = xv.permute(0, 3, 1, 2).double().requires_grad_(True)            # [1, C, rows, F]
    y = F.max_pool2d(F.leaky_relu(bn(x), SLOPE), (1, pool))
    tapv = F.max_pool2d(x, (1, tap_pool))
    (y * dyv.permute(0, 3, 1, 2).double()).sum().backward(retain_graph=True)
    g_ref, b_ref = bn.weight.grad.clone(), bn.bias.grad.clone()
    (tapv * dwv[..., coff:coff + C].permute(0, 3, 1, 2).double()).sum().backward()

    st, _ = device_state(bn, dev)
    xd, dyd, dwd = xv.to(dev).to(dt), dyv.to(dev).to(dt), dwv.to(dev).to(dt)
    wide = torch.zeros(1, rows, Ft, 640, device=dev, dtype=dt)
    tap = ops.Tap(wide, tap_pool, coff, want_argmax=True)
    ops.bn_act_pool_fwd(xd, st, pool=pool, tap=tap)
    tap.grad = dwd
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    w = torch.zeros(1, dtype=torch.int32, device=dev)
    dx = ops.bn_act_pool_bwd(xd, dyd, st, dg, db, pool=pool, amax_out=w, tap=tap)
    assert dx.dtype == dt
    close(dg, g_ref)
    close(db, b_ref)
    if dt == torch.float32:
        close(dx.permute(0, 3, 1, 2), x.grad)
    # the two passes the fold replaces
    dg2, db2 = torch.empty(C, device=dev), torch.empty(C, device=dev)
    w2 = torch.zeros(1, dtype=torch.int32, device=dev)
    dx2 = ops.bn_act_pool_bwd(xd, dyd, st, dg2, db2, pool=pool, amax_out=w2)
    ops.maxpool_bwd_add(xd, dwd, dx2, tap_pool, coff=coff, amax_out=w2, argmax=tap.argmax)
    assert torch.equal(dx, dx2) and torch.equal(w, w2) and torch.equal(dg, dg2) and torch.equal(db, db2)
    w3 = torch.zeros(1, dtype=torch.int32, device=dev)
    assert torch.equal(ops.bn_act_pool_bwd(xd, dyd, st, None, None, pool=pool, amax_out=w3, tap=tap), dx)
    assert torch.equal(w3, w)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_train_mode_leaves_the_bits_it_left_before(hip_device, golden_dir, name):
    """Every output of the train-mode passes -- dx, dgamma, dbeta, the absmax word -- has the digest recorded with the
    build before the passes took a mode, also with eval-mode calls on the same stream (and workspace) in between."""
    want = json.loads((golden_dir / "bn_bwd_train_bits.json").read_text())[name]
    first = {k: cases.digest(v) for k, v in cases.run_train_case(ops, name, hip_device).items()}
    rows, Fq, C, pool, _, dt = cases.CASES[name]
    t = cases.case_inputs(name)
    bn = eval_bn(C)
    st, _ = device_state(bn, hip_device)
    dg, db = torch.empty(C, device=hip_device), torch.empty(C, device=hip_device)
    ops.bn_act_pool_bwd(t["x"].to(hip_device), t["dy"].to(hip_device), st, dg, db, pool=pool)
    ops.bn_act_pool_bwd(t["x"].to(hip_device), t["dy"].to(hip_device), st, None, None, pool=pool)
    again = {k: cases.digest(v) for k, v in cases.run_train_case(ops, name, hip_device).items()}
    assert first == want
    assert again == want
