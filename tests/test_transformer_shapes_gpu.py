"""The Transformer head's kernels away from the one geometry the other tests run them at (B = 3, H = 8, T = 192,
dh = 64): the batched products at ragged sizes and on strided head views, the row softmax from L = 1 to its limit, the
LayerNorm at D = 1024 / one row / more rows than waves, the GELU grid-stride tail, the fused attention at grids that
are no multiple of 8 workgroups, other head counts, scales, dropout rates and leading dimensions, and the whole model
at other T and nhead.  Every reference is float64 torch on the CPU; layout, mask, replay and fused-equals-separate
checks are bit exact.

Tolerances are the project's (`close` 1e-5 of the reference's largest magnitude; attention forward 1e-5, gradients
2e-5; LayerNorm gradients 2e-5; whole model as in test_transformer_gpu.py) except where the argument of an exponent or
a cancelling mean makes |x| * 2^-24 exceed them.  There the same formula was evaluated in fp32 torch on the CPU, its
error against float64 measured, and the kernel is allowed four times that (never less than the project tolerance): the
numbers stand next to each constant below."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import model_ref
from pitchextractor_amd import _lib, ops
from pitchextractor_amd.model import JDCNet
from tests.golden.make_golden import TF_CFG, golden_input, golden_targets
from tests.test_ops_gpu import close, rnd

pytestmark = pytest.mark.gpu

CANARY = -777.25


def relerr(got, ref):
    """max |got - ref| / max |ref| (what `close` bounds), for the checks that print their figure first."""
    got, ref = got.detach().cpu().double(), ref.detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


def cut(rows, cols, fill, device, data=None, r0=2, c0=4, spare_rows=3, spare_cols=8):
    """A rows x cols matrix cut out of a larger buffer filled with `fill`: rows before and after it, columns left and
    right of it.  Returns (buffer, view); the view's first element is 16-byte aligned and its ld is a multiple of 4
    when cols is."""
    buf = torch.full((r0 + rows + spare_rows, c0 + cols + spare_cols), fill, dtype=torch.float32, device=device)
    view = buf[r0:r0 + rows, c0:c0 + cols]
    if data is not None:
        view.copy_(data)
    return buf, view


def outside_untouched(buf, view_rows, view_cols, fill, r0=2, c0=4):
    b = buf.clone()
    b[r0:r0 + view_rows, c0:c0 + view_cols] = fill
    return bool((b == fill).all())


# ------------------------------------------------------------------ (a) batched products
def _views(T, H, dh):
    D = H * dh
    return (3 * D, T * 3 * D, dh), (T, H * T * T, T * T), (D, T * D, dh)          # hview, pview, oview


@pytest.mark.parametrize("B,H,T,dh", [(1, 3, 100, 32), (2, 4, 68, 128), (1, 16, 36, 32), (2, 2, 4, 64)])
def test_bgemm_model_products_at_ragged_shapes(hip_device, B, H, T, dh):
    """The products _tf_forward / _tf_backward issue on the unfused path (S = Q K^T, O = Pd V, dV = Pd^T dO,
    dPd = dO V^T, dQ = dS K, dK = dS^T Q), on the model's own head views, at sizes that are no multiple of the 64 x 64
    tile or of the 32-wide k-tile; plus alpha != 1 and accumulate."""
    dev, D = hip_device, H * dh
    hview, pview, oview = _views(T, H, dh)
    qkv = rnd(B * T, 3 * D, seed=1).to(dev)
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    heads = lambda t: t.cpu().double().reshape(B, T, H, dh).transpose(1, 2)          # (B,H,T,dh)
    merge = lambda t: t.transpose(1, 2).reshape(B * T, D)
    canary = lambda *shape: torch.full(shape, CANARY, dtype=torch.float32, device=dev)
    # forward
    S = canary(B * H * T, T)
    ops.bgemm(0, q, hview, k, hview, S, pview, H, B * H, T, T, dh)
    refS = heads(q) @ heads(k).transpose(-1, -2)
    close(S.view(B, H, T, T), refS)
    ops.bgemm(0, q, hview, k, hview, S, pview, H, B * H, T, T, dh, alpha=0.37)
    close(S.view(B, H, T, T), 0.37 * refS)
    P = torch.softmax(rnd(B * H * T, T, seed=2), dim=-1).to(dev)
    P64 = P.cpu().double().view(B, H, T, T)
    O = canary(B * T, D)
    ops.bgemm(1, P, pview, v, hview, O, oview, H, B * H, T, dh, T)
    refO = merge(P64 @ heads(v))
    close(O, refO)
    acc = rnd(B * T, D, seed=4).to(dev)
    ref_acc = acc.cpu().double() + 0.5 * refO
    ops.bgemm(1, P, pview, v, hview, acc, oview, H, B * H, T, dh, T, alpha=0.5, accumulate=True)
    close(acc, ref_acc)
    # backward: each product writes its third of dqkv and nothing else
    dO = rnd(B * T, D, seed=3).to(dev)
    dqkv = canary(B * T, 3 * D)
    dq, dk, dv = dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:]
    ops.bgemm(2, P, pview, dO, oview, dv, hview, H, B * H, T, dh, T)
    close(dv, merge(P64.transpose(-1, -2) @ heads(dO)))
    assert (dqkv[:, :2 * D] == CANARY).all()
    dv_bits = dv.clone()
    dP = canary(B * H * T, T)
    ops.bgemm(0, dO, oview, v, hview, dP, pview, H, B * H, T, T, dh)
    close(dP.view(B, H, T, T), heads(dO) @ heads(v).transpose(-1, -2))
    dS = rnd(B * H * T, T, seed=5).to(dev)
    dS64 = dS.cpu().double().view(B, H, T, T)
    ops.bgemm(1, dS, pview, k, hview, dq, hview, H, B * H, T, dh, T)
    close(dq, merge(dS64 @ heads(k)))
    assert (dk == CANARY).all() and torch.equal(dv, dv_bits)
    dq_bits = dq.clone()
    ops.bgemm(2, dS, pview, q, hview, dk, hview, H, B * H, T, dh, T)
    close(dk, merge(dS64.transpose(-1, -2) @ heads(q)))
    assert torch.equal(dq, dq_bits) and torch.equal(dv, dv_bits)


@pytest.mark.parametrize("mode,M,N,K", [(0, 36, 68, 100), (1, 68, 100, 36), (2, 100, 36, 68)])
def test_bgemm_reads_nothing_outside_its_operands(hip_device, mode, M, N, K):
    """One matrix per operand (inner = 1, batch = 1), each cut out of a NaN field with ld > cols and spare rows behind
    it, C out of a canary field: a NaN that reaches an MFMA slot that counts (a row past K of a k-major operand, the
    k-tail of a k-contiguous one: 0 * NaN) poisons the result, and a store outside C changes a canary.  (Rows past
    M / N of a k-contiguous operand and columns past the width of a k-major one only feed accumulators of rows / columns
    the store guard drops: KRowLoader's `col < cols` bit changes no stored value, with or without it.)"""
    dev = hip_device
    a_shape = (M, K) if mode != 2 else (K, M)
    b_shape = (N, K) if mode == 0 else (K, N)
    A, Bm = rnd(*a_shape, seed=1), rnd(*b_shape, seed=2)
    _, Av = cut(*a_shape, float("nan"), dev, data=A)
    _, Bv = cut(*b_shape, float("nan"), dev, data=Bm)
    Cbuf, Cv = cut(M, N, CANARY, dev)
    ops.bgemm(mode, Av, (Av.stride(0), 0, 0), Bv, (Bv.stride(0), 0, 0), Cv, (Cv.stride(0), 0, 0), 1, 1, M, N, K)
    A64, B64 = A.double(), Bm.double()
    ref = A64 @ B64.T if mode == 0 else (A64 @ B64 if mode == 1 else A64.T @ B64)
    close(Cv, ref)
    assert outside_untouched(Cbuf, M, N, CANARY)


def test_bgemm_refusals_leave_the_output_alone(hip_device):
    dev = hip_device
    A, Bm = rnd(64, 64, seed=1).to(dev), rnd(64, 64, seed=2).to(dev)
    A66 = rnd(40, 66, seed=3).to(dev)
    C = torch.full((64, 64), CANARY, dtype=torch.float32, device=dev)
    v64 = (64, 0, 0)
    with pytest.raises(_lib.HipLibraryError, match="unsupported"):      # K & 3 in mode 0
        ops.bgemm(0, A, v64, Bm, v64, C, v64, 1, 1, 32, 32, 30)
    with pytest.raises(_lib.HipLibraryError, match="unsupported"):      # lda & 3
        ops.bgemm(0, A66, (66, 0, 0), Bm, v64, C, v64, 1, 1, 32, 32, 32)
    with pytest.raises(_lib.HipLibraryError, match="unsupported"):      # more matrices than gridDim.y holds
        ops.bgemm(0, A, v64, Bm, v64, C, v64, 1, 65536, 32, 32, 32)
    torch.cuda.synchronize()
    assert (C == CANARY).all()


# ------------------------------------------------------------------ (b) row softmax
def _softmax_case(dev, s, dp, scale, tol_fwd=1e-5, tol_bwd=1e-5, tag=""):
    rows, L = s.shape
    s64 = s.double().requires_grad_(True)
    p64 = torch.softmax(s64 * scale, dim=-1)
    p64.backward(dp.double())
    guard = torch.full((rows + 2, L), CANARY, dtype=torch.float32, device=dev)      # a row before and one behind
    sd = guard[1:rows + 1]
    sd.copy_(s)
    ops.softmax_fwd_(sd, scale)
    e_f = relerr(sd, p64.detach())
    dguard = guard.clone()
    dpd = dguard[1:rows + 1]
    dpd.copy_(dp)
    ops.softmax_bwd_(sd, dpd, scale)
    e_b = relerr(dpd, s64.grad)
    if tag:
        print(f"{tag}: softmax forward error {e_f:.2e} (allowed {tol_fwd:.2e}), backward {e_b:.2e} ({tol_bwd:.2e})")
    assert e_f <= tol_fwd and e_b <= tol_bwd, (e_f, e_b)
    for gd in (guard, dguard):
        assert (gd[0] == CANARY).all() and (gd[-1] == CANARY).all()


@pytest.mark.parametrize("scale", [0.125, 1.0])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("L", [1, 4, 63, 64, 65, 100, 1000, 1024])
def test_softmax_row_lengths(hip_device, L, rows, scale):
    _softmax_case(hip_device, rnd(rows, L, seed=L) * 4, rnd(rows, L, seed=L + 1), scale)


# Scores x 30 (|x| up to 120 at scale 1): the exponent's argument carries |x| * 2^-24 = 7e-6, above 1e-5 / 4.  The fp32
# CPU restatement (exp(v - max) / sum; scale * p * (dp - sum p dp)) is off float64 by 7.3e-8 forward and 3.0e-7
# backward on this input; four times that is still below the project tolerance, which therefore holds.
SOFTMAX_X30_TOL_FWD = 1e-5
SOFTMAX_X30_TOL_BWD = 1e-5


def test_softmax_large_scores_and_flat_row(hip_device):
    _softmax_case(hip_device, rnd(5, 100, seed=21) * 30, rnd(5, 100, seed=22), 1.0, SOFTMAX_X30_TOL_FWD,
                  SOFTMAX_X30_TOL_BWD, tag="scores x 30")
    _softmax_case(hip_device, torch.full((1, 100), 3.7), rnd(1, 100, seed=23), 0.125)        # all values equal


def test_softmax_refuses_rows_past_its_limit(hip_device):
    s = torch.full((2, 1025), CANARY, dtype=torch.float32, device=hip_device)
    dp = torch.full((2, 1025), CANARY, dtype=torch.float32, device=hip_device)
    with pytest.raises(_lib.HipLibraryError, match="unsupported"):
        ops.softmax_fwd_(s, 1.0)
    with pytest.raises(_lib.HipLibraryError, match="unsupported"):
        ops.softmax_bwd_(s, dp, 1.0)
    torch.cuda.synchronize()
    assert (s == CANARY).all() and (dp == CANARY).all()


# ------------------------------------------------------------------ (c) LayerNorm
def _ln_case(dev, a, g, be, dy, b=None, pe=None, tol_y=1e-5, tol_dz=2e-5, tol_dg=2e-5, tol_db=2e-5, tag=""):
    R, D = a.shape
    a64, g64, be64 = (t.double().requires_grad_(True) for t in (a, g, be))
    z = a64
    if b is not None:
        z = z + b.double()
    if pe is not None:
        z = z + pe.double()[torch.arange(R) % pe.shape[0]]
    y64 = F.layer_norm(z, (D,), g64, be64, 1e-5)
    y64.backward(dy.double())
    f = lambda t: None if t is None else t.to(dev)
    yd, st = ops.layernorm_fwd(f(a), f(g), f(be), b2d=f(b), pe=f(pe))
    dg, db = torch.empty(D, device=dev), torch.empty(D, device=dev)
    dz = ops.layernorm_bwd(f(dy), st, f(g), dg, db)
    errs = (relerr(yd, y64.detach()), relerr(st.z, z.detach()), relerr(dz, a64.grad), relerr(dg, g64.grad),
            relerr(db, be64.grad))
    if tag:
        print(f"{tag}: y {errs[0]:.2e} (allowed {tol_y:.2e}), dz {errs[2]:.2e} ({tol_dz:.2e}), "
              f"dgamma {errs[3]:.2e} ({tol_dg:.2e}), dbeta {errs[4]:.2e} ({tol_db:.2e})")
    assert errs[0] <= tol_y and errs[1] <= 1e-5 and errs[2] <= tol_dz and errs[3] <= tol_dg and errs[4] <= tol_db, errs
    y_only, st_only = ops.layernorm_fwd(f(a), f(g), f(be), b2d=f(b), pe=f(pe), keep_z=False)
    assert st_only.z is None and torch.equal(y_only, yd)
    assert torch.equal(st_only.mean, st.mean) and torch.equal(st_only.rstd, st.rstd)


@pytest.mark.parametrize("with_b,with_pe", [(True, True), (True, False), (False, True), (False, False)])
def test_layernorm_d1024(hip_device, with_b, with_pe):
    R, D, T = 37, 1024, 10
    _ln_case(hip_device, rnd(R, D, seed=1), rnd(D, seed=4).abs() + 0.5, rnd(D, seed=5), rnd(R, D, seed=6),
             b=rnd(R, D, seed=2) if with_b else None, pe=rnd(T, D, seed=3) if with_pe else None)


@pytest.mark.parametrize("R", [1, 4100])
def test_layernorm_one_row_and_more_rows_than_waves(hip_device, R):
    """R = 1: 2047 of the backward's 2048 waves write all-zero partials; R = 4100: its row loop runs up to three
    times per wave."""
    D = 256
    _ln_case(hip_device, rnd(R, D, seed=1), rnd(D, seed=4).abs() + 0.5, rnd(D, seed=5), rnd(R, D, seed=6),
             b=rnd(R, D, seed=2), pe=rnd(7, D, seed=3))


# Rows of mean 100 and standard deviation 1 (D = 512, R = 37): the mean of 512 values near 100 is rounded at 2^-24 of
# their sum, and x - mean cancels two digits.  The fp32 CPU restatement of the kernel's formulas is off float64 by
# 3.14e-6 (y), 3.1e-7 (dz), 5.43e-6 (dgamma), 9.4e-8 (dbeta) of each tensor's largest element on this input; the kernel
# gets four times that where it exceeds the project tolerance (1e-5 forward, 2e-5 gradients).
LN_MEAN100_TOL_Y = 4 * 3.14e-6            # 1.26e-5
LN_MEAN100_TOL_DZ = 2e-5                  # 4 * 3.1e-7 is below it
LN_MEAN100_TOL_DG = 4 * 5.43e-6           # 2.17e-5
LN_MEAN100_TOL_DB = 2e-5                  # 4 * 9.4e-8 is below it


def test_layernorm_rows_far_from_zero(hip_device):
    R, D = 37, 512
    _ln_case(hip_device, 100.0 + rnd(R, D, seed=31), rnd(D, seed=32).abs() + 0.5, rnd(D, seed=33), rnd(R, D, seed=34),
             tol_y=LN_MEAN100_TOL_Y, tol_dz=LN_MEAN100_TOL_DZ, tol_dg=LN_MEAN100_TOL_DG, tol_db=LN_MEAN100_TOL_DB,
             tag="rows of mean 100")


def test_layernorm_fused_backward_d1024_equals_separate_passes(hip_device):
    dev, R, D, p = hip_device, 37, 1024, 0.1
    a, b = rnd(R, D, seed=1).to(dev), rnd(R, D, seed=2).to(dev)
    gam, bet = rnd(D, seed=3).to(dev), rnd(D, seed=4).to(dev)
    bd, m_ref = ops.dropout(b, p, seed=9, offset=1234)
    y_ref, st_ref = ops.layernorm_fwd(a, gam, bet, b2d=bd)
    y, st, m = ops.layernorm_dropout_fwd(a, b, gam, bet, p, seed=9, offset=1234)
    assert torch.equal(m, m_ref) and torch.equal(y, y_ref) and torch.equal(st.z, st_ref.z)
    assert torch.equal(st.mean, st_ref.mean) and torch.equal(st.rstd, st_ref.rstd)
    dy, dy2 = rnd(R, D, seed=6).to(dev), rnd(R, D, seed=7).to(dev)
    dg_ref, db_ref = torch.empty(D, device=dev), torch.empty(D, device=dev)
    dz_ref = ops.layernorm_bwd(dy + dy2, st_ref, gam, dg_ref, db_ref)
    dzd_ref, _ = ops.dropout(dz_ref, p, mask_in=m_ref)
    dg, db = torch.empty(D, device=dev), torch.empty(D, device=dev)
    dz, dzd = ops.layernorm_bwd(dy, st, gam, dg, db, dy_add=dy2, drop_mask=m, p=p)
    assert torch.equal(dz, dz_ref) and torch.equal(dzd, dzd_ref) and torch.equal(dg, dg_ref) and torch.equal(db, db_ref)
    dg2, db2 = torch.empty(D, device=dev), torch.empty(D, device=dev)
    assert torch.equal(ops.layernorm_bwd(dy, st, gam, dg2, db2, dy_add=dy2), dz_ref)
    assert torch.equal(dg2, dg_ref) and torch.equal(db2, db_ref)


def test_layernorm_refuses_other_widths(hip_device):
    dev, R, D = hip_device, 8, 100
    a, gam, bet = rnd(R, D, seed=1).to(dev), rnd(D, seed=2).to(dev), rnd(D, seed=3).to(dev)
    with pytest.raises(_lib.HipLibraryError, match="unsupported"):
        ops.layernorm_fwd(a, gam, bet)
    st = ops.LnState(a, torch.zeros(R, device=dev), torch.ones(R, device=dev))
    dz = torch.full((R, D), CANARY, dtype=torch.float32, device=dev)
    dg, db = torch.full((D,), CANARY, device=dev), torch.full((D,), CANARY, device=dev)
    with pytest.raises(_lib.HipLibraryError, match="unsupported"):
        ops.layernorm_bwd(a, st, gam, dg, db, dz=dz)
    torch.cuda.synchronize()
    assert (dz == CANARY).all() and (dg == CANARY).all() and (db == CANARY).all()


# ------------------------------------------------------------------ (d) GELU
N_BIG = 4 * (16384 * 256 + 1000)          # 1000 float4s more than one sweep of the largest grid


def _gelu64(x, dy):
    x, dy = x.double(), dy.double()
    cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    return x * cdf, dy * (cdf + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))


@pytest.fixture(scope="module")
def gelu_big():
    x, dy = rnd(N_BIG, seed=1) * 3, rnd(N_BIG, seed=2)
    return (x, dy) + _gelu64(x, dy)


def test_gelu_past_one_grid_sweep(hip_device, gelu_big):
    x, dy, y64, dx64 = gelu_big
    xd, dyd = x.to(hip_device), dy.to(hip_device)
    tail = slice(N_BIG - 4 * 1000 - 64, N_BIG)                 # what the second iteration of the loop writes, and a bit
    for got, ref in ((ops.gelu_fwd(xd, out=torch.full_like(xd, float("nan"))), y64),
                     (ops.gelu_bwd(xd, dyd, out=torch.full_like(xd, float("nan"))), dx64)):
        close(got, ref)
        close(got[tail], ref[tail])


def test_gelu_across_its_range(hip_device):
    x = torch.linspace(-10.0, 10.0, 4096)
    dy = rnd(4096, seed=3)
    y64, dx64 = _gelu64(x, dy)
    xd = x.to(hip_device)
    close(ops.gelu_fwd(xd), y64)
    close(ops.gelu_bwd(xd, dy.to(hip_device)), dx64)


def test_gelu_refuses_sizes_that_are_no_float4(hip_device):
    dev = hip_device
    x, dy = rnd(1002, seed=1).to(dev), rnd(1002, seed=2).to(dev)
    out = torch.full((1002,), CANARY, dtype=torch.float32, device=dev)
    with pytest.raises(_lib.HipLibraryError, match="unsupported"):
        ops.gelu_fwd(x, out=out)
    with pytest.raises(_lib.HipLibraryError, match="unsupported"):
        ops.gelu_bwd(x, dy, out=out)
    torch.cuda.synchronize()
    assert (out == CANARY).all()


def test_gelu_dropout_past_one_grid_sweep_equals_separate_passes(hip_device, gelu_big):
    p = 0.1
    h = gelu_big[0].to(hip_device).view(-1, 32)
    da = gelu_big[1].to(hip_device).view(-1, 32)
    act_ref, m_ref = ops.dropout(ops.gelu_fwd(h), p, seed=9, offset=77)
    act, m = ops.gelu_dropout_fwd(h, p, seed=9, offset=77)
    assert torch.equal(m, m_ref) and torch.equal(act, act_ref)
    assert 0.09 < 1.0 - m.float().mean().item() < 0.11
    dh_ref = ops.gelu_bwd(h, ops.dropout(da, p, mask_in=m_ref)[0])
    assert torch.equal(ops.gelu_dropout_bwd(h, da, m, p), dh_ref)


# ------------------------------------------------------------------ (e) fused attention (T = 192, dh = 64)
AT, ADH = 192, 64
GRIDS = [(1, 1), (1, 3), (5, 4), (2, 12)]          # 3, 9, 60, 72 workgroups: the first three are no multiple of 8


def _attn_ref(qkv, d_o, B, H, scale, p, mask):
    """float64 softmax(Q K^T * scale) -> dropout with the kernel's exported keep mask -> V, and its autograd gradient."""
    D = H * ADH
    ref_in = qkv.cpu().double().requires_grad_(True)
    q, k, v = (ref_in[:, i * D:(i + 1) * D].view(B, AT, H, ADH).transpose(1, 2) for i in range(3))
    s = (q @ k.transpose(-1, -2)) * scale
    P = torch.softmax(s, dim=-1)
    if p > 0:
        P = P * mask.cpu().view(B, H, AT, AT).double() / (1 - p)
    ref_o = (P @ v).transpose(1, 2).reshape(B * AT, D)
    ref_o.backward(d_o.cpu().double())
    return ref_o.detach(), torch.logsumexp(s, dim=-1).detach(), ref_in.grad, s.detach()


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("scale", [0.125, 0.2])
@pytest.mark.parametrize("B,H", GRIDS)
def test_fused_attention_grids_scales_rates(hip_device, B, H, scale, p):
    dev, D = hip_device, H * ADH
    assert ops.attn_supported(AT, ADH)
    qkv = (rnd(B * AT, 3 * D, seed=1) * 1.5).to(dev)
    d_o = rnd(B * AT, D, seed=2).to(dev)
    o, lse, mask = ops.attn_fwd(qkv, B, AT, H, scale, p, seed=11, offset=1000)
    if p > 0:
        _, m2 = ops.dropout(torch.ones(B * H * AT, AT, device=dev), p, seed=11, offset=1000)
        assert torch.equal(m2, mask)                               # the unfused dropout's Philox stream
    else:
        assert mask is None
    ref_o, ref_lse, ref_g, _ = _attn_ref(qkv, d_o, B, H, scale, p, mask)
    close(o, ref_o, 1e-5)
    close(lse.view(B, H, AT), ref_lse, 1e-5)
    dqkv = ops.attn_bwd(qkv, o, d_o, lse, mask, B, AT, H, scale, p)
    for i in range(3):
        close(dqkv[:, i * D:(i + 1) * D], ref_g[:, i * D:(i + 1) * D], 2e-5)
    if p > 0:                                                      # replay of the exported bytes
        o2, lse2, m3 = ops.attn_fwd(qkv, B, AT, H, scale, p, mask_in=mask.clone())
        assert torch.equal(o, o2) and torch.equal(lse, lse2) and torch.equal(m3, mask)
        assert torch.equal(ops.attn_bwd(qkv, o2, d_o, lse2, m3, B, AT, H, scale, p), dqkv)


# qkv x 4 (scaled scores up to 169): a score is rounded at |s| * 2^-24 = 1e-5 before it is exponentiated.  The fp32 CPU
# restatement (fp32 matmuls, softmax, autograd) is off float64 by 6.13e-6 (o), 3.2e-7 (lse), 8.46e-6 (dq), 7.20e-6 (dk),
# 1.96e-6 (dv) of each tensor's largest element on this input; the kernel gets four times that where it exceeds the
# project tolerance (1e-5 forward, 2e-5 gradients).
ATTN_X4_TOL_O = 4 * 6.13e-6               # 2.45e-5
ATTN_X4_TOL_LSE = 1e-5                    # 4 * 3.2e-7 is below it
ATTN_X4_TOL_DQ = 4 * 8.46e-6              # 3.38e-5
ATTN_X4_TOL_DK = 4 * 7.20e-6              # 2.88e-5
ATTN_X4_TOL_DV = 2e-5                     # 4 * 1.96e-6 is below it


def test_fused_attention_large_scores(hip_device):
    dev, B, H = hip_device, 1, 3
    D = H * ADH
    qkv = (rnd(B * AT, 3 * D, seed=1) * 1.5 * 4).to(dev)
    d_o = rnd(B * AT, D, seed=2).to(dev)
    o, lse, _ = ops.attn_fwd(qkv, B, AT, H, 0.125, 0.0)
    dqkv = ops.attn_bwd(qkv, o, d_o, lse, None, B, AT, H, 0.125, 0.0)
    ref_o, ref_lse, ref_g, s = _attn_ref(qkv, d_o, B, H, 0.125, 0.0, None)
    assert s.abs().max().item() > 100.0
    errs = [relerr(o, ref_o), relerr(lse.view(B, H, AT), ref_lse)] + \
           [relerr(dqkv[:, i * D:(i + 1) * D], ref_g[:, i * D:(i + 1) * D]) for i in range(3)]
    tols = [ATTN_X4_TOL_O, ATTN_X4_TOL_LSE, ATTN_X4_TOL_DQ, ATTN_X4_TOL_DK, ATTN_X4_TOL_DV]
    print("qkv x 4: " + ", ".join(f"{n} {e:.2e} (allowed {t:.2e})" for n, e, t in zip(("o", "lse", "dq", "dk", "dv"),
                                                                                      errs, tols)))
    assert all(e <= t for e, t in zip(errs, tols)), (errs, tols)


def test_fused_attention_strided_rows(hip_device):
    """ld_qkv = 3 D + 4 and ld_o = D + 8 through the C entry points, called as ops.attn_fwd / ops.attn_bwd call them:
    inputs cut from NaN fields, outputs from canary fields; same bits as the dense call, gaps untouched.  60 workgroups,
    so a block order that skips a (batch, head, part) leaves canaries where its output belongs."""
    dev, B, H, scale, p = hip_device, 5, 4, 0.125, 0.1
    D, R = H * ADH, B * AT
    qkv = (rnd(R, 3 * D, seed=1) * 1.5).to(dev)
    d_o = rnd(R, D, seed=2).to(dev)
    o, lse, mask = ops.attn_fwd(qkv, B, AT, H, scale, p, seed=11, offset=1000)
    dqkv = ops.attn_bwd(qkv, o, d_o, lse, mask, B, AT, H, scale, p)
    kw = dict(r0=2, c0=0, spare_rows=3)
    _, qkv_v = cut(R, 3 * D, float("nan"), dev, data=qkv, spare_cols=4, **kw)
    _, do_v = cut(R, D, float("nan"), dev, data=d_o, spare_cols=8, **kw)
    o_buf, o_v = cut(R, D, CANARY, dev, spare_cols=8, **kw)
    dq_buf, dq_v = cut(R, 3 * D, CANARY, dev, spare_cols=4, **kw)
    ld_qkv, ld_o = qkv_v.stride(0), o_v.stride(0)
    assert (ld_qkv, ld_o) == (3 * D + 4, D + 8)
    lse2 = torch.empty_like(lse)
    mask2 = torch.empty_like(mask)
    prod = ops.products_for("attn")
    ops._call("pe_attn_fwd", qkv_v.data_ptr(), ld_qkv, o_v.data_ptr(), ld_o, lse2.data_ptr(), 0, mask2.data_ptr(),
              B, AT, H, ADH, scale, p, 11, 1000, ops._s(), products=prod)
    assert torch.equal(o_v, o) and torch.equal(lse2, lse) and torch.equal(mask2, mask)
    assert outside_untouched(o_buf, R, D, CANARY, r0=2, c0=0)
    ops._call("pe_attn_bwd", qkv_v.data_ptr(), ld_qkv, o_v.data_ptr(), do_v.data_ptr(), ld_o, lse2.data_ptr(),
              mask2.data_ptr(), dq_v.data_ptr(), B, AT, H, ADH, scale, p, ops._s(), products=prod)
    assert torch.equal(dq_v, dqkv)
    assert outside_untouched(dq_buf, R, 3 * D, CANARY, r0=2, c0=0)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,H", [(1, 3), (5, 4)])
def test_fused_attention_bf16_operands_other_grids(hip_device, B, H, p):
    """test_fused_attention_bf16_operands (its rounding model and its tolerances) at 9 and 60 workgroups."""
    dev, D, T, dh = hip_device, H * ADH, AT, ADH
    qkv = (rnd(B * T, 3 * D, seed=1) * 1.5).to(dev)
    d_o = rnd(B * T, D, seed=2)
    o32, lse32, mask32 = ops.attn_fwd(qkv, B, T, H, 0.125, p, seed=11, offset=1000)
    with ops.matmul_bf16(True, "bf16"):
        o, lse, mask = ops.attn_fwd(qkv, B, T, H, 0.125, p, seed=11, offset=1000)
        dqkv = ops.attn_bwd(qkv, o, d_o.to(dev), lse, mask, B, T, H, 0.125, p)
    if p > 0:
        assert torch.equal(mask, mask32)
    r16 = lambda t: t.to(torch.bfloat16).double()
    x = qkv.cpu()
    q, k, v = (r16(x[:, i * D:(i + 1) * D]).view(B, T, H, dh).transpose(1, 2) for i in range(3))
    s = (q @ k.transpose(-1, -2)) * 0.125
    P = torch.softmax(s, dim=-1)
    if p > 0:
        P = P * mask.cpu().view(B, H, T, T).double() / (1 - p)
    ref_o = (r16(P.float()) @ v).transpose(1, 2).reshape(B * T, D)
    assert (o.cpu().double() - ref_o).abs().max().item() <= 1e-3 * ref_o.abs().max().item()
    assert (lse.cpu().double().view(B, H, T) - torch.logsumexp(s, dim=-1)).abs().max().item() <= 1e-5 * s.abs().max().item()
    assert (o - o32).abs().max().item() <= 2e-2 * o32.abs().max().item()
    _, _, ref_g, _ = _attn_ref(qkv, d_o, B, H, 0.125, p, mask)          # exact gradient of the exact forward
    for i in range(3):
        ref = ref_g[:, i * D:(i + 1) * D]
        err = (dqkv[:, i * D:(i + 1) * D].cpu().double() - ref).abs().max().item()
        assert err <= 2e-2 * ref.abs().max().item(), ("qkv"[i], err, ref.abs().max().item())


@pytest.mark.parametrize("B,H", GRIDS)
def test_fused_attention_agrees_with_the_unfused_chain(hip_device, B, H):
    """The same qkv through pe_bgemm + pe_softmax + pe_dropout as the model's unfused path chains them, forward and
    backward: same masks, results within 2e-5 (the in-model comparison's bound)."""
    dev, D, T, dh, scale, p = hip_device, H * ADH, AT, ADH, 0.125, 0.1
    hview, pview, oview = _views(T, H, dh)
    qkv = (rnd(B * T, 3 * D, seed=1) * 1.5).to(dev)
    d_o = rnd(B * T, D, seed=2).to(dev)
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    o, lse, mask = ops.attn_fwd(qkv, B, T, H, scale, p, seed=11, offset=1000)
    dqkv = ops.attn_bwd(qkv, o, d_o, lse, mask, B, T, H, scale, p)
    P = torch.empty(B * H * T, T, device=dev)
    ops.bgemm(0, q, hview, k, hview, P, pview, H, B * H, T, T, dh)
    ops.softmax_fwd_(P, scale)
    Pd, m2 = ops.dropout(P, p, seed=11, offset=1000)
    assert torch.equal(m2, mask)
    o2 = torch.empty(B * T, D, device=dev)
    ops.bgemm(1, Pd, pview, v, hview, o2, oview, H, B * H, T, dh, T)
    close(o, o2.cpu(), 2e-5)
    dqkv2 = torch.empty_like(qkv)
    dq, dk, dv = dqkv2[:, :D], dqkv2[:, D:2 * D], dqkv2[:, 2 * D:]
    ops.bgemm(2, Pd, pview, d_o, oview, dv, hview, H, B * H, T, dh, T)
    dP = torch.empty_like(P)
    ops.bgemm(0, d_o, oview, v, hview, dP, pview, H, B * H, T, T, dh)
    dP, _ = ops.dropout(dP, p, mask_in=m2)
    ops.softmax_bwd_(P, dP, scale)
    ops.bgemm(1, dP, pview, k, hview, dq, hview, H, B * H, T, dh, T)
    ops.bgemm(2, dP, pview, q, hview, dk, hview, H, B * H, T, dh, T)
    for i in range(3):
        close(dqkv[:, i * D:(i + 1) * D], dqkv2[:, i * D:(i + 1) * D].cpu(), 2e-5)


@pytest.mark.parametrize("T,dh", [(191, 64), (192, 32), (64, 64)])
def test_fused_attention_refuses_other_geometries(hip_device, T, dh):
    dev, B, H = hip_device, 1, 2
    D = H * dh
    assert not ops.attn_supported(T, dh)
    qkv = rnd(B * T, 3 * D, seed=1).to(dev)
    o = torch.full((B * T, D), CANARY, dtype=torch.float32, device=dev)
    dqkv = torch.full((B * T, 3 * D), CANARY, dtype=torch.float32, device=dev)
    lse = torch.full((B * H * T,), CANARY, dtype=torch.float32, device=dev)
    prod = ops.products_for("attn")
    with pytest.raises(_lib.HipLibraryError, match="unsupported"):
        ops._call("pe_attn_fwd", qkv.data_ptr(), 3 * D, o.data_ptr(), D, lse.data_ptr(), 0, 0, B, T, H, dh, 0.125, 0.0,
                  0, 0, ops._s(), products=prod)
    with pytest.raises(_lib.HipLibraryError, match="unsupported"):
        ops._call("pe_attn_bwd", qkv.data_ptr(), 3 * D, o.data_ptr(), o.data_ptr(), D, lse.data_ptr(), 0,
                  dqkv.data_ptr(), B, T, H, dh, 0.125, 0.0, ops._s(), products=prod)
    torch.cuda.synchronize()
    assert (o == CANARY).all() and (lse == CANARY).all() and (dqkv == CANARY).all()


# ------------------------------------------------------------------ (f) whole model against the float64 oracle
def _cfg(nhead, dropout=0.0, max_len=256):
    return dict(TF_CFG, num_layers=2, nhead=nhead, dim_feedforward=512, max_len=max_len, dropout=dropout)


def _state(nhead, max_len=256):
    return model_ref.seeded_state(11, model_type="transformer", num_layers=2, nhead=nhead, dim_feedforward=512,
                                  max_len=max_len)


def _net(state, cfg, device):
    net = JDCNet(num_class=1, sequence_model_config=dict(cfg))
    net.load_state_dict(state, strict=True)
    return net.to(device)


def _f64(state):
    return {k: (v.double() if v.dtype.is_floating_point else v) for k, v in state.items()}


def _rel(got, ref):
    got = np.asarray(got.detach().cpu().double()); ref = np.asarray(ref.detach().cpu().double())
    return np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30)


def _hip_step(net, x, f0, sil, device):
    cls, det = net(x.to(device))
    out3, d_f0, d_sil = ops.f0_sil_loss(cls.detach().reshape(-1), f0.to(device).reshape(-1), det.detach().reshape(-1),
                                        sil.to(device).reshape(-1), 0.1)
    torch.autograd.backward([cls, det], [d_f0.view_as(cls), d_sil.view_as(det)])
    return cls, det, out3


MODEL_CASES = [(40, 8), (100, 4), (36, 16), (192, 16), (192, 4)]


@pytest.mark.parametrize("T,nhead", MODEL_CASES)
def test_transformer_train_step_matches_live_oracle(hip_device, T, nhead):
    torch.set_num_threads(16)
    state, cfg = _state(nhead), _cfg(nhead)
    x = golden_input(7, B=2, T=T)
    f0, sil = golden_targets(7, B=2, T=T)
    # float64 CPU oracle: forward + backward of the reference-equivalent step (train mode, dropout off)
    st64 = {k: (v.double().requires_grad_(not k.endswith(("running_mean", "running_var")))
                if v.dtype.is_floating_point else v) for k, v in state.items()}
    rcls, rdet = model_ref.jdcnet_forward(st64, x.double(), cfg, train=True)
    rloss, _, _ = model_ref.jdc_loss(rcls, rdet, f0.double(), sil.double(), 0.1)
    rloss.backward()
    net = _net(state, cfg, hip_device).train()
    net.block_dropout = 0.0
    cls, det, out3 = _hip_step(net, x, f0, sil, hip_device)
    assert cls.shape == (2, T, 1)
    assert _rel(cls, rcls) <= 1e-4 and _rel(det, rdet) <= 1e-4, (_rel(cls, rcls), _rel(det, rdet))
    np.testing.assert_allclose(out3[0].item(), rloss.item(), rtol=1e-5)
    bad = []
    for n, prm in net.named_parameters():
        ref = st64[n].grad
        got = prm.grad.detach().cpu().double()
        rn, gn = ref.norm().item(), got.norm().item()
        if abs(gn - rn) > 2e-3 * rn + 1e-9:
            bad.append((n, "norm", gn, rn))
        idx = torch.linspace(0, ref.numel() - 1, min(32, ref.numel())).long()
        err = (got.flatten()[idx] - ref.flatten()[idx]).abs().max().item()
        if err > 5e-3 * ref.abs().max().item() + 1e-9:
            bad.append((n, "elements", err, ref.abs().max().item()))
    assert not bad, bad


@pytest.mark.parametrize("T,nhead", MODEL_CASES)
def test_transformer_eval_matches_live_oracle(hip_device, T, nhead):
    torch.set_num_threads(16)
    state, cfg = _state(nhead), _cfg(nhead)
    x = golden_input(8, B=2, T=T)
    with torch.no_grad():
        rcls, rdet = model_ref.jdcnet_forward(_f64(state), x.double(), cfg, train=False)
        cls, det = _net(state, cfg, hip_device).eval()(x.to(hip_device))
    assert _rel(cls, rcls) <= 1e-4 and _rel(det, rdet) <= 1e-4, (_rel(cls, rcls), _rel(det, rdet))


def test_transformer_dropout_masks_replayed_in_oracle_t68(hip_device):
    torch.set_num_threads(16)
    state, cfg = _state(8), _cfg(8, dropout=0.1)
    net = _net(state, cfg, hip_device).train()
    net.keep_last_context = True
    net.dropout_cfg.seed = 5
    x = golden_input(6, B=2, T=68)
    cls, det = net(x.to(hip_device))
    s = net.last_context
    masks = [s.mask_pool.cpu(), s.mask_det.cpu()]
    for tf in (s.tf_c, s.tf_d):
        for c in tf.layers:
            assert not c.fused
            masks += [c.mask_p.cpu(), c.mask1.cpu(), c.mask_f.cpu(), c.mask2.cpu()]
    with torch.no_grad():
        rc, rd = model_ref.jdcnet_forward(_f64(state), x.double(), cfg, train=True, masks=iter(masks))
    assert _rel(cls, rc) <= 1e-4 and _rel(det, rd) <= 1e-4, (_rel(cls, rc), _rel(det, rd))


def test_fused_and_unfused_attention_agree_in_the_model_at_120_workgroups(hip_device, monkeypatch):
    """B = 5, nhead = 8: the fused grid is 120 workgroups, a multiple of 8 other than the 48 the B = 2 tests run; live
    dropout, same Philox offsets on both paths."""
    state, cfg = _state(8), _cfg(8, dropout=0.1)
    x = golden_input(6, B=5)
    f0, sil = golden_targets(6, B=5)
    outs = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "FUSED_ATTENTION", fused)
        net = _net(state, cfg, hip_device).train()
        net.keep_last_context = True
        net.dropout_cfg.seed = 5
        cls, det, _ = _hip_step(net, x, f0, sil, hip_device)
        assert all(c.fused == fused for c in net.last_context.tf_c.layers)
        outs[fused] = (cls.detach(), det.detach(), net.flat_gradients().clone(), net.dropout_cfg.offset)
    assert outs[True][3] == outs[False][3]
    assert _rel(outs[True][0], outs[False][0]) <= 2e-5 and _rel(outs[True][1], outs[False][1]) <= 2e-5
    ga, gb = outs[True][2].double(), outs[False][2].double()
    assert ((ga - gb).norm() / gb.norm()).item() <= 1e-4


# ------------------------------------------------------------------ what the head refuses before its first launch
def test_transformer_refuses_more_frames_than_positions(hip_device):
    """T > max_len: the positional table's slice is shorter than T, and the LayerNorm kernel's `row % period` would
    wrap the positions (and drift them across batch elements); the reference fails to broadcast on the same input."""
    state, cfg = _state(8, max_len=32), _cfg(8, max_len=32)
    net = _net(state, cfg, hip_device).eval()
    with torch.no_grad():
        with pytest.raises(ValueError, match=r"T = 40 .*max_len = 32"):
            net(golden_input(6, B=2, T=40).to(hip_device))
        cls, _ = net(golden_input(6, B=2, T=32).to(hip_device))          # T == max_len is served
    assert cls.shape == (2, 32, 1)


def test_transformer_refuses_frame_counts_that_are_no_multiple_of_four(hip_device):
    net = _net(_state(8), _cfg(8), hip_device).eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match=r"T = 50 "):
        net(golden_input(6, B=2, T=50).to(hip_device))
