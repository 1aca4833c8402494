"""The fp32 product kernels in their two split modes -- "h2" (two scaled fp16 terms, the default for every conv / GEMM /
weight-gradient product) and "x3" (three truncated bf16 terms) -- against float64 models of exactly the terms they
keep (tests/split_ref.py), on heavy-tailed operands whose rows, K-slices or channels sit 0 .. 40 binades below the
tensor maximum, at the shapes that reach every tile and kernel (the shape lists of tests/test_half_operands_gpu.py).

Tolerance.  Every kept product is exact in fp32 (11 x 11 or 8 x 8 significand bits) and the unscale 1 / (s_a s_b) is a
power of two, so what separates a kernel from its model is the fp32 accumulation alone.  Each rounding of a partial
sum S adds an error of at most u |S| <= u sum|terms| (u = 2^-24), zero-mean.  We count, per output element, r roundings:
five per 16-product MFMA block and kept term pair (a binary tree over the block plus the add into the accumulator, the
most any summation order of the block can take), so r = 5 nt ceil(K / 16), plus ACC_EXTRA for the split-K reduction,
bias, residual and the final store.  By Hoeffding's inequality the sum of r such errors exceeds 8 sqrt(r) u sum|terms|
with probability below 2 exp(-32) per element, so

    |got - model|  <=  8 sqrt(r) u sum|terms|  +  8 * 2^-149            (acc_tol; the second term: fp32 subnormal outputs)

per element, where sum|terms| is that element's own sum of |kept terms| (bias and residual included), never the tensor's
maximum.  That is 2^-16.4 of sum|terms| at K = 576 in h2 and 2^-13.4 at K = 20000 in x3.

fp16-subnormal factors.  The f16 MFMA (v_mfma_f32_32x32x16_f16) does not sum products that have an fp16-subnormal
factor exactly.  test_f16_mfma_subnormal_factor_probe shows where: fed identical fp16 operands, the h2 entry point
(scale 1, lo = 0) and the one-term f16 entry point return bit-identical results, so the split, the conversions and
the v_fma_mix lo term are not involved; a single such product is exact; a 16-product block is not (up to ~2^-12.4 of
its largest product).  This fits an adder that aligns the block's products to the largest exponent FIELD and keeps
24 bits below it: a subnormal's field reads as 2^-14 although its leading bit lies up to 10 places lower, so the
product of a subnormal t and u is held on a grid of at most 2^(-14 + e_u + 2 - 24) <= 2^-36 |u| (scaled units).  The
tests add that grid per such product (split_ref.h2_subnormal_allowance: MFMA_SUB_GRID = 2^-36 times |u|, summed
linearly since truncation need not average out); the probe asserts the bound and that it is not vacuous.  The bit-exact
rounding of the block is not modelled.  The allowance is far below the precision the split itself gives such
elements (an element 2^-32 below its tensor's maximum keeps ~6.6 bits) and below a flushed or misscaled term.

The plain products of every kernel (the fragment-fed conv kernels for the forward and data gradient, every GEMM shape
that holds all nine levels of the operand generator) also show that wrong models miss the GPU result on the same
data: float64 of the unsplit operands, the h2 model with fp16 subnormal terms flushed and the h2 model with the scale
one binade off (h2), the one-term bf16 model (x3).  The bias / residual variants, the implicit-GEMM conv path and the
BatchNorm partials are held to the model without controls.
"""
import math

import numpy as np
import pytest
import torch

from pitchextractor_amd import _lib, ops
from tests import split_ref as S
from tests.half_ref import shifted_y
from tests.test_half_operands_gpu import CONV_SHAPES, NT_SHAPES, TN_SHAPES, halo_kernel
from tests.test_ops_gpu import nchw, nhwc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ACC_EXTRA = 16
TINY = 8 * 2.0 ** -149
NTERMS = {"h2": 3, "x3": 6}
MODES = ("h2", "x3")


def acc_tol(K, mode, extra=ACC_EXTRA):
    r = 5 * NTERMS[mode] * math.ceil(K / 16) + extra
    return 8 * math.sqrt(r) * U


def _excess(got, model, tol, budget=None):
    """max over elements of |got - value| / (tol sum|terms| + the subnormal-factor allowance + TINY); inf
    where finiteness differs.  ``budget``: take sum|terms| from this model instead (a wrong model is held to the bound
    of the right one)."""
    val = model[0]
    budget = model if budget is None else budget
    mag = budget[1]
    sub = budget[2] if len(budget) > 2 else 0.0
    got = got.detach().cpu().double()
    assert got.shape == val.shape, (got.shape, val.shape)
    fin = torch.isfinite(val)
    if not torch.equal(torch.isfinite(got), fin):
        return float("inf")
    if not fin.any():
        return 0.0
    bound = tol * mag + sub + TINY
    return ((got - val).abs()[fin] / bound[fin]).max().item()


def fits(got, model, tol, budget=None):
    return _excess(got, model, tol, budget) <= 1.0


def check(got, model, tol, wrong=()):
    """got fits the model per element; every wrong model (name -> model) misses it somewhere"""
    e = _excess(got, model, tol)
    assert e <= 1.0, f"error {e:.3g} x the tolerance"
    for name, m in wrong:
        assert not fits(got, m, tol, model), \
            f"the wrong model '{name}' also fits (excess {_excess(got, m, tol, model):.3g})"


def h2m(op, a, b, **kw):
    """the h2 model with the MFMA's allowance for its fp16-subnormal-factor products"""
    return S.h2_product(op, a, b, **kw) + (S.h2_subnormal_allowance(op, a, b, kw.get("amax_a"), kw.get("amax_b")),)


def model(mode, op, a, b, **kw):
    return h2m(op, a, b, **kw) if mode == "h2" else S.x3_product(op, a, b)


def wrong_models(mode, op, a, b):
    if mode == "h2":
        return [("exact float64", S.exact_product(op, a, b)), ("flushed subnormals", S.h2_product(op, a, b, flush=True)),
                ("scale one binade off", S.h2_product(op, a, b, es_delta=-1))]
    return [("one-term bf16", S.bf16_product(op, a, b))]


def plus(m, *extra):
    """model m plus extra float64 addends (bias, residual), with their magnitudes"""
    val, mag = m[:2]
    for e in extra:
        e = e.detach().cpu().double()
        val, mag = val + e, mag + e.abs()
    return (val, mag) + tuple(m[2:])


# ------------------------------------------------------------------ GEMM NT
@pytest.mark.parametrize("M,N,K", NT_SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_gemm_nt_split(hip_device, M, N, K, mode, monkeypatch):
    """rows of A and K-slices of B at 2^-k of their maxima (A's just below a power of two, B's exactly one); plain,
    with both biases, and accumulating into a residual"""
    monkeypatch.setattr(ops, "FP32_MATMUL", mode)
    dev = hip_device
    A = S.heavy((M, K), 0, seed=M + K)
    B = S.heavy((N, K), 1, seed=N + 2 * K, top="pow2", scale=2.0 ** -9)
    b0, b1 = torch.randn(N) * 1e-3, torch.randn(N) * 1e-3
    m = model(mode, S.op_nt, A, B)
    tol = acc_tol(K, mode)
    Ad, Bd = A.to(dev), B.to(dev)
    check(ops.gemm_nt(Ad, Bd), m, tol, wrong_models(mode, S.op_nt, A, B))
    check(ops.gemm_nt(Ad, Bd, bias0=b0.to(dev), bias1=b1.to(dev)), plus(m, b0, b1), tol)
    out = torch.randn(M, N) * 1e-3
    od = out.to(dev)
    check(ops.gemm_nt(Ad, Bd, out=od, accumulate=True), plus(m, out), tol)


@pytest.mark.parametrize("mode", MODES)
def test_gemm_nt_split_strided_rows(hip_device, mode, monkeypatch):
    monkeypatch.setattr(ops, "FP32_MATMUL", mode)
    big = S.heavy((300, 7, 96), 0, seed=6).to(hip_device)     # rows taken at a fixed time step: ld = 7*96
    A = big[:, 3, 32:96]
    for N in (50, 256):
        B = S.heavy((N, 64), 1, seed=N)
        out = torch.zeros(300, N + 30, device=hip_device)
        ops.gemm_nt(A, B.to(hip_device), out=out[:, 10:10 + N])
        Ac = A.cpu()
        check(out[:, 10:10 + N], model(mode, S.op_nt, Ac, B), acc_tol(64, mode), wrong_models(mode, S.op_nt, Ac, B))
        assert (out[:, :10] == 0).all() and (out[:, 10 + N:] == 0).all()


# ------------------------------------------------------------------ GEMM TN
@pytest.mark.parametrize("K,M,N", TN_SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_gemm_tn_split(hip_device, K, M, N, mode, monkeypatch):
    """columns of A (output rows) and K-slices of B at 2^-k; one-split and split-K shapes"""
    monkeypatch.setattr(ops, "FP32_MATMUL", mode)
    dev = hip_device
    A = S.heavy((K, M), 1, seed=K + M, scale=2.0 ** 40)
    B = S.heavy((K, N), 0, seed=K + N, top="pow2", scale=2.0 ** -30)
    m = model(mode, S.op_tn, A, B)
    tol = acc_tol(K, mode, extra=ACC_EXTRA + 64)                 # + the split-K slab reduction
    # (the controls need rows at every level of KS: M >= 9)
    check(ops.gemm_tn(A.to(dev), B.to(dev)), m, tol, wrong_models(mode, S.op_tn, A, B) if M >= len(S.KS) else ())
    out = torch.randn(M, N) * 1e-12
    check(ops.gemm_tn(A.to(dev), B.to(dev), out=out.to(dev), accumulate=True), plus(m, out), tol)


# ------------------------------------------------------------------ conv 3x3
@pytest.mark.parametrize("B,T,Fq,Ci,Co", CONV_SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_conv3x3_split(hip_device, B, T, Fq, Ci, Co, mode, monkeypatch):
    """forward on the fragment-fed kernel (where conv_halo_passes takes one) and on the implicit GEMM, the residual
    accumulate and the BatchNorm partials of the fragment-fed epilogue; the data gradient through the packed dgrad
    weight; the weight gradient.  The forward weight's output channels sit at 2^-k (scaled output channels) and x's
    channels; the data gradient uses a second weight with scaled input channels (its output channels).  The weight gradient gets its own operands with scaled x channels
    (its output rows).  Cin % 64 != 0 takes the per-tap weight-gradient kernels, which run the native fp32 MFMA in every
    mode: pinned against float64 of the unsplit operands, and the split model must miss them."""
    monkeypatch.setattr(ops, "FP32_MATMUL", mode)
    dev = hip_device
    x = S.heavy((B, Ci, T, Fq), 1, seed=1)
    w = S.heavy((Co, Ci, 3, 3), 0, seed=2, top="pow2", scale=2.0 ** -4)      # forward: output channels scaled
    w2 = S.heavy((Co, Ci, 3, 3), 1, seed=6, scale=2.0 ** 20)                  # data gradient: its output channels
    dy = S.heavy((B, Co, T, Fq), 1, seed=3, scale=2.0 ** 10)
    K = 9 * Ci
    m_y = model(mode, S.op_conv, x, w)
    m_dx = model(mode, S.op_conv, dy, S.dgrad_weight(w2))
    xd, dyd, wd_ = nhwc(x).to(dev), nhwc(dy).to(dev), w.to(dev)
    kinds = []
    for frag in (True, False):
        monkeypatch.setattr(ops, "CONV_WFRAG", frag)
        wf, _ = ops.conv3x3_repack(wd_, True, False)
        _, wdg = ops.conv3x3_repack(w2.to(dev), False, True)
        assert (wf.frag is not None) == frag
        y, parts = ops.conv3x3_fwd(xd, wf, bn_stats=True)
        kinds.append(halo_kernel(Fq, Co) if frag else None)
        assert (parts is not None) == (kinds[-1] is not None)
        check(nchw(y), m_y, acc_tol(K, mode), wrong_models(mode, S.op_conv, x, w) if frag else ())
        if parts is not None:          # BatchNorm partials: column sums / sums of squares of the stored outputs
            y64 = y.double().view(-1, Co)
            got = parts.sum(0).cpu()
            for j, ref in enumerate((y64.sum(0), (y64 * y64).sum(0))):
                mag = (y64.abs().sum(0) if j == 0 else (y64 * y64).sum(0)).cpu()
                assert ((got[j] - ref.cpu()).abs() <= 2.0 ** -16 * mag + 1e-300).all(), j
        acc = torch.randn(B, T, Fq, Co) * 1e-3
        ya = ops.conv3x3_fwd(xd, wf, out=acc.to(dev), accumulate=True)
        check(nchw(ya), plus(m_y, nchw(acc)), acc_tol(K, mode))
        dx = ops.conv3x3_fwd(dyd, wdg)
        check(nchw(dx), m_dx, acc_tol(9 * Co, mode),
              wrong_models(mode, S.op_conv, dy, S.dgrad_weight(w2)) if frag else ())
    # weight gradient: scaled input channels (output rows), dy rows (time) scaled
    x2 = S.heavy((B, Ci, T, Fq), 1, seed=4, top="pow2")
    dy2 = S.heavy((B, Co, T, Fq), 2, seed=5, scale=2.0 ** -50)
    dw = torch.empty(Co, Ci, 3, 3, device=dev)
    ops.conv3x3_wgrad(nhwc(x2).to(dev), nhwc(dy2).to(dev), dw)
    P = B * T * Fq
    if Ci % 64 == 0 and Co % 64 == 0:
        check(dw, model(mode, S.op_wgrad, x2, dy2), acc_tol(P, mode, ACC_EXTRA + 64),
              wrong_models(mode, S.op_wgrad, x2, dy2))
    else:                                   # per-tap kernels: fp32 products (one rounding each), every mode
        ex = S.exact_product(S.op_wgrad, x2, dy2)
        tol = acc_tol(P, "h2", ACC_EXTRA + 64 + 5 * P) + U
        check(dw, ex, tol, [("split model", model(mode, S.op_wgrad, x2, dy2))] if mode == "h2" else ())


def test_conv_split_shapes_reach_every_kernel():
    kinds = {halo_kernel(Fq, Co) for _, _, Fq, _, Co in CONV_SHAPES} | {halo_kernel(Fq, Ci) for _, _, Fq, Ci, _ in
                                                                          CONV_SHAPES}
    assert kinds == {"10-pass", "7-pass/128", "7-pass/192", None}
    assert any(Ci % 64 for _, _, _, Ci, _ in CONV_SHAPES) and any(Ci % 64 == 0 for _, _, _, Ci, _ in CONV_SHAPES)


# ------------------------------------------------------------------ LSTM dW_hh
@pytest.mark.parametrize("H", [64, 384])
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_lstm_whh_grad_split(hip_device, H, reverse, mode, monkeypatch):
    """dW_hh = sum over (b, t) of dgates[b, t]^T h_{t-+1}[b], h a strided slice of a [B, T, 2H] buffer; in h2 mode the
    h operand is scaled by the constant word of 1.0 (_unit_amax), which the model uses too"""
    monkeypatch.setattr(ops, "FP32_MATMUL", mode)
    dev = hip_device
    for B, T in ((37, 9), (130, 40)):
        dg = S.heavy((B, T, 4 * H), 2, seed=H + B)
        ybuf = S.heavy((B, T, 2 * H), 2, seed=H + T, top="below")          # |y| < 1
        ysl = ybuf[:, :, reverse * H:(reverse + 1) * H]
        dw = torch.empty(4 * H, H, device=dev)
        ops.lstm_whh_grad(dg.to(dev), ybuf.to(dev)[:, :, reverse * H:(reverse + 1) * H], dw, reverse, B, T, H)

        def op(a, b):
            return a.reshape(-1, 4 * H).T @ shifted_y(b, reverse).reshape(-1, H)
        kw = {"amax_b": S.f32_bits(1.0)} if mode == "h2" else {}
        check(dw, model(mode, op, dg, ysl, **kw), acc_tol(B * T, mode, ACC_EXTRA + 64),
              wrong_models(mode, op, dg, ysl) if mode == "x3" else
              [("exact float64", S.exact_product(op, dg, ysl)),
               ("own absmax of h", S.h2_product(op, dg, ysl)),          # ysl's maximum is below 1: another scale
               ("flushed subnormals", S.h2_product(op, dg, ysl, amax_b=S.f32_bits(1.0), flush=True)),
               ("scale one binade off", S.h2_product(op, dg, ysl, amax_b=S.f32_bits(1.0), es_delta=-1))])
        assert S.absmax_bits(ysl) >> 23 != 127


# ------------------------------------------------------------------ packed weight fragments
def _frag_ref(t, N, K, terms):
    """[N, K] term -> [K/16][ceil(N/32)][lane][8] in the fragment order (tail rows zero)"""
    nb = (N + 31) // 32
    pad = torch.zeros(nb * 32, K, dtype=t.dtype)
    pad[:N] = t
    return pad.view(nb, 32, K // 16, 2, 8).permute(2, 0, 3, 1, 4).reshape(K // 16, nb, 64, 8)


def test_wfrag_pack_h2_and_x3_products_are_the_split_in_fragment_layout(hip_device):
    """pe_wfrag_pack under PE_PROD_H2 (two fp16 terms of the weight scaled by its absmax word) and PE_PROD_X3 (three
    truncated bf16 terms): every fragment word bit-equal to the split, fp16 / fp32 subnormals included"""
    N, K = 70, 96
    w = S.heavy((N, K), 0, seed=9)
    w[1, :3] = torch.tensor([2.0 ** -130, -(2.0 ** -120), 1 + 2.0 ** -11])
    amax = ops.absmax(w.to(hip_device))
    assert amax.item() == S.absmax_bits(w)
    raw = ops.wfrag_pack(ops.Scaled(w.to(hip_device), amax), _lib.PE_PROD_H2).cpu()
    frag = raw.view(torch.int16).view(K // 16, (N + 31) // 32, 2, 64, 8)
    hi, lo, _ = S.split_h2(w)
    for i, t in enumerate((hi, lo)):
        assert torch.equal(frag[:, :, i], _frag_ref(t.to(torch.float16), N, K, 2).view(torch.int16)), i
    assert ((hi.abs() < 2.0 ** -14) & (hi != 0)).any() and ((lo.abs() < 2.0 ** -14) & (lo != 0)).any()
    raw = ops.wfrag_pack(w.to(hip_device), _lib.PE_PROD_X3).cpu()
    frag = raw.view(torch.int16).view(K // 16, (N + 31) // 32, 3, 64, 8)
    for i, t in enumerate(S.split_x3(w)):
        ref = _frag_ref(t.float(), N, K, 3).view(torch.int32) >> 16
        assert torch.equal(frag[:, :, i].to(torch.int32) & 0xFFFF, ref & 0xFFFF), i


# ------------------------------------------------------------------ absmax-word edges (h2)
def _word(v):
    return torch.tensor([S.f32_bits(v)], dtype=torch.int32)


def test_h2_amax_word_edges(hip_device, monkeypatch):
    """gemm_nt fed absmax words that are not its operand's own, each against the model built from THE WORD GIVEN:
    16x too large (precision lost exactly as modelled), one binade low (no overflow), two binades low with maxima just
    under the next power of two (Inf exactly at the outputs that read them), zero and subnormal words on a tiny
    tensor (both clamp to 2^126)."""
    monkeypatch.setattr(ops, "FP32_MATMUL", "h2")
    dev = hip_device
    M, N, K = 130, 72, 96
    A = S.heavy((M, K), 0, seed=11)
    B = S.heavy((N, K), 1, seed=12, top="pow2")
    Bd = B.to(dev)
    tol = acc_tol(K, "h2")
    amax = A.abs().max().item()
    cases = [16 * amax, amax / 2]
    for v in cases:
        got = ops.gemm_nt(ops.Scaled(A.to(dev), _word(v).to(dev)), Bd)
        m = h2m(S.op_nt, A, B, amax_a=S.f32_bits(v))
        check(got, m, tol, [("own word", S.h2_product(S.op_nt, A, B))])
        assert torch.isfinite(got).all()
    # two binades low: x s reaches [2^15, 2^16); maxima just under a power of two round to Inf (>= 65520)
    A2 = A.clone()
    rows = [5, 77]
    for r in rows:
        A2[r, 3] = -(1 - 2.0 ** -24)
    got = ops.gemm_nt(ops.Scaled(A2.to(dev), _word(amax / 4).to(dev)), Bd).cpu()
    m = h2m(S.op_nt, A2, B, amax_a=S.f32_bits(amax / 4))
    check(got, m, tol)
    bad = ~torch.isfinite(got)
    assert torch.equal(bad.any(1).nonzero().view(-1), torch.tensor(rows + [M - 1])) and bad[rows].all()
    # tiny tensor (max < 2^-113): its own word, a zero word and a subnormal word all give the scale 2^126
    At = S.heavy((M, K), 0, seed=13, scale=2.0 ** -118)
    ref = h2m(S.op_nt, At, B)
    for bits in (0, 1, S.absmax_bits(At)):
        got = ops.gemm_nt(ops.Scaled(At.to(dev), torch.tensor([bits], dtype=torch.int32, device=dev)), Bd)
        check(got, h2m(S.op_nt, At, B, amax_a=bits), tol)
        check(got, ref, tol)
        assert (got != 0).any()


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_h2_nonfinite_operand(hip_device, bad, monkeypatch):
    """An Inf or NaN operand element makes its absmax word Inf / NaN (biased exponent 255): the scale becomes 2^-115,
    the outputs that read the element are non-finite, and every other element of that operand tensor scales below
    fp16's range, so the outputs that do not read it come out exactly 0 (bias only).  Pinned, for both operands."""
    monkeypatch.setattr(ops, "FP32_MATMUL", "h2")
    dev = hip_device
    A = S.heavy((100, 64), 0, seed=14)
    B = S.heavy((72, 64), 1, seed=15)
    A[37, 11] = bad
    bias = torch.randn(72)
    got = ops.gemm_nt(A.to(dev), B.to(dev), bias0=bias.to(dev)).cpu()
    check(got, plus(h2m(S.op_nt, A, B), bias), acc_tol(64, "h2"))
    nonfin = ~torch.isfinite(got)
    assert nonfin[37].all() and not nonfin[torch.arange(100) != 37].any()
    assert torch.equal(got[torch.arange(100) != 37], bias.expand(99, 72))
    Bt = B.clone()
    Bt[5, 60] = bad                                                      # the other operand: column 5 only
    A = S.heavy((64, 100), 1, seed=17)
    got = ops.gemm_tn(A.to(dev), Bt.T.contiguous().to(dev)).cpu()
    assert (~torch.isfinite(got[:, 5])).all() and torch.equal(got[:, torch.arange(72) != 5], torch.zeros(100, 71))


# ------------------------------------------------------------------ absmax_segments
def test_absmax_segments_direct(hip_device):
    """pe_absmax_segments: the exact absmax word of every segment of one flat buffer -- lengths 0, 1, 3 and large,
    unaligned offsets, maxima in a segment's first and last element, larger neighbours right before and after a
    segment (which must not bleed in), negative maxima, NaN"""
    g = torch.Generator().manual_seed(16)
    flat = torch.randn(300_000, generator=g)
    segs = [(0, 0), (5, 1), (7, 3), (13, 250_001), (250_017, 29), (250_050, 4097), (255_001, 0), (260_003, 12),
            (270_001, 1000)]
    flat[12] = 1e6                                   # right after (7, 3) ... (7..9), and 10..12 neighbours
    flat[10] = 5e5
    flat[6] = -7e5                                   # right before (7, 3) and after (5, 1)
    flat[8] = -3.5                                   # negative maximum inside (7, 3)
    flat[250_001 + 13] = 9e6                         # right after the large segment
    flat[13 + 250_000] = -4e3                        # its last element: its maximum, negative
    flat[250_017 + 28] = 2e3                         # last element of (250_017, 29)
    flat[250_017] = -2e3                             # first element: same magnitude
    flat[250_050 + 4096] = -8e3
    flat[250_049] = 1e7                              # just before (250_050, 4097)
    flat[260_003 + 5] = float("nan")
    flat[270_001 + 999] = float("inf")
    flat[270_000] = float("nan")                     # just before the last segment
    off = torch.tensor([o for o, _ in segs], dtype=torch.int64)
    ln = torch.tensor([n for _, n in segs], dtype=torch.int64)
    got = ops.absmax_segments(flat.to(hip_device), off.to(hip_device), ln.to(hip_device)).cpu()
    ref = [S.absmax_bits(flat[o:o + n]) for o, n in segs]
    assert got.tolist() == ref
    assert ref[0] == 0 and ref[2] == S.f32_bits(3.5) and ref[3] == S.f32_bits(4e3) and ref[5] == S.f32_bits(8e3)
    assert ref[7] >> 23 == 0xFF and ref[7] & 0x7FFFFF and ref[8] == S.f32_bits(float("inf"))


# ------------------------------------------------------------------ the f16 MFMA and fp16-subnormal factors
def test_f16_mfma_subnormal_factor_probe(hip_device, monkeypatch):
    """fp16-exact operands fed to the h2 entry point with scale-1 words (hi = the operand, lo = 0) and to the one-term
    f16 entry point: bit-identical results, so the deviation on subnormal factors is the MFMA's, not the split's.  A
    single subnormal product is exact; 16-product blocks deviate by more than fp32 accumulation allows but stay within
    the derived grid 2^-36 |u| per subnormal-factor product (module docstring)."""
    dev = hip_device
    g = torch.Generator().manual_seed(1)
    M, N, K = 64, 64, 32
    A = torch.zeros(M, K, dtype=torch.float64)
    n = torch.randint(-3, 4, (M, K), generator=g).double()
    A[:32] = n[:32] * 2.0 ** -24                                   # multiples of the smallest fp16 subnormal
    A[32:48] = n[32:48] * 2.0 ** -20                               # larger subnormals
    A[48:] = torch.randn(16, K, generator=g).half().double()       # normal fp16
    B = (torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-12, 9, (N, K), generator=g).float())).half().double()
    word = torch.tensor([S.f32_bits(8192.0)], dtype=torch.int32, device=dev)      # es = 127: scale 1
    sub = S.f16_subnormal(A).double()
    single = torch.zeros(M, 16, dtype=torch.float64)
    single[:, 5] = A[:, 5]
    for k in (0, 16, K):                       # 0: one nonzero product per output in a 16-product block
        Ak = single if k == 0 else A[:, :k]
        k = k or 16
        a, b = Ak.float().to(dev), B[:, :k].float().to(dev)
        monkeypatch.setattr(ops, "FP32_MATMUL", "h2")
        h2 = ops.gemm_nt(ops.Scaled(a, word), ops.Scaled(b, word)).cpu().double()
        with ops.matmul_bf16(True, "f16"):
            f16 = ops.gemm_nt(a, b).cpu().double()
        assert torch.equal(h2, f16), k
        ex = Ak @ B[:, :k].T
        mag = Ak.abs() @ B[:, :k].abs().T
        err = (h2 - ex).abs()
        if Ak is single:
            assert torch.equal(h2, ex)
            continue
        allowance = S.MFMA_SUB_GRID * (sub[:, :k] @ B[:, :k].abs().T)
        assert (err <= acc_tol(k, "h2") * mag + allowance).all(), k
        assert (err[48:] <= acc_tol(k, "h2") * mag[48:]).all()        # normal factors: fp32 accumulation only
        assert (err[:48] > 2.0 ** -18 * mag[:48]).any()                 # ... subnormal factors: more, measurably
        assert (err[:48] > 0.25 * allowance[:48]).any()                 # the allowance is not vacuous


@pytest.mark.parametrize("op_name", ["conv3x3_fwd", "conv3x3_wgrad", "lstm_whh_grad"])
def test_h2_words_computed_inside_the_op_belong_to_their_operand(hip_device, op_name, monkeypatch):
    """Called without words, each op computes both absmax words itself; operands whose maxima lie 60 binades apart
    show whether each word reaches the operand it belongs to (a word freed and reused before the launch gave x the
    scale of dy: Inf / NaN everywhere)"""
    monkeypatch.setattr(ops, "FP32_MATMUL", "h2")
    dev = hip_device
    B, T, Fq, Ci, Co = 2, 12, 10, 64, 64
    g = torch.Generator().manual_seed(21)
    if op_name == "conv3x3_fwd":
        x, w = torch.randn(B, Ci, T, Fq, generator=g) * 2.0 ** -60, torch.randn(Co, Ci, 3, 3, generator=g)
        for frag in (True, False):
            monkeypatch.setattr(ops, "CONV_WFRAG", frag)
            wf, _ = ops.conv3x3_repack(w.to(dev), True, False)
            y, _ = ops.conv3x3_fwd(nhwc(x).to(dev), wf, bn_stats=True)
            check(nchw(y), h2m(S.op_conv, x, w), acc_tol(9 * Ci, "h2"))
    elif op_name == "conv3x3_wgrad":
        for sx, sd in ((1.0, 2.0 ** -60), (2.0 ** -60, 1.0)):
            x, dy = torch.randn(B, Ci, T, Fq, generator=g) * sx, torch.randn(B, Co, T, Fq, generator=g) * sd
            dw = torch.empty(Co, Ci, 3, 3, device=dev)
            ops.conv3x3_wgrad(nhwc(x).to(dev), nhwc(dy).to(dev), dw)
            check(dw, h2m(S.op_wgrad, x, dy), acc_tol(B * T * Fq, "h2", ACC_EXTRA + 64))
    else:
        H, Bn, T2 = 64, 9, 7
        dg = torch.randn(Bn, T2, 4 * H, generator=g) * 2.0 ** -60
        y = torch.tanh(torch.randn(Bn, T2, H, generator=g))
        dw = torch.empty(4 * H, H, device=dev)
        ops.lstm_whh_grad(dg.to(dev), y.to(dev), dw, 0, Bn, T2, H)

        def op(a, b):
            return a.reshape(-1, 4 * H).T @ shifted_y(b, 0).reshape(-1, H)
        check(dw, h2m(op, dg, y, amax_b=S.f32_bits(1.0)), acc_tol(Bn * T2, "h2", ACC_EXTRA + 64))


# ------------------------------------------------------------------ x3 persistent LSTM (H = 384), teacher forcing
@pytest.mark.parametrize("B,reverse", [(1, (0,)), (65, (1,)), (130, (0, 1))])
def test_persistent_lstm_x3_step_by_step(hip_device, B, reverse, monkeypatch, T=6):
    """pe_lstm_fwd_persistent / pe_lstm_bwd_persistent (x3) one float64 step at a time from the kernel's own stored
    state (tests/half_ref.py, half=None: the x3 split rebuilds every operand and the kept products miss at most
    2^-23 of sum|w h|; the backward exchanges its partial sums as fp32).

    Forward, per element: the pre-activation is off by at most d = 2^-20 (|xg| + |h_prev| |W_hh|^T) (accumulation and
    the dropped x3 products); sigmoid' <= 1/4 and tanh' <= 1, so a gate is off by <= d + 2^-21 (fp32 transcendentals),
    c by <= 3 max_gate(d) |.| + 2^-21 (1 + |c|) and h by <= 4 max_gate(d) + 2^-20.  Backward: per element within 1e-5
    of the step's largest gate gradient (as the 16-bit test).  Control: the one-term bf16 model misses both (from
    T = 2 on: a single step has no recurrent product).  ``T``: another sequence length
    (test_persistent_lstm_x3_one_cell_edges)."""
    from tests import half_ref as R
    monkeypatch.setattr(ops, "FP32_MATMUL", "x3")
    dev, H = hip_device, 384
    n = len(reverse)
    g = torch.Generator().manual_seed(B + n)
    whh = [(torch.rand(4 * H, H, generator=g) * 2 - 1) * H ** -0.5 for _ in range(n)]
    xg = [torch.randn(B, T, 4 * H, generator=g) for _ in range(n)]
    dyb = torch.randn(B, T, 2 * H, generator=g)
    ybuf = torch.zeros(B, T, 2 * H, device=dev)
    cols = [slice(r * H, (r + 1) * H) for r in reverse] if n == 1 else [slice(0, H), slice(H, 2 * H)]
    ysl = [ybuf[:, :, c] for c in cols]
    dsl = [dyb.to(dev)[:, :, c] for c in cols]
    gates = [x.to(dev) for x in xg]
    cbuf = [torch.empty(B, T, H, device=dev) for _ in range(n)]
    wd = [w.to(dev) for w in whh]
    ops.clear_persistent_lstm_error(dev)
    assert ops._persistent_ok(n, B, H, dev, "fwd") and ops._persistent_ok(n, B, H, dev, "bwd")
    ops.lstm_fwd(wd, gates, ysl, cbuf, list(reverse), B, T, H)
    acts = [t.cpu() for t in gates]
    assert ops.lstm_bwd([ops.transpose2d(w) for w in wd], gates, cbuf, dsl, [torch.empty(B, H, device=dev)] * n,
                        list(reverse), B, T, H) in (True, False)
    torch.cuda.synchronize()
    assert not ops.persistent_lstm_error(dev)
    for i in range(n):
        y, c, dgt = ysl[i].cpu(), cbuf[i].cpu(), gates[i].cpu()

        def fwd_ok(half):
            G, C, Y = R.lstm_fwd_teacher(xg[i], y, c, whh[i], reverse[i], half)
            mag = xg[i].double().abs()
            for t, tp in R._order(T, reverse[i]):
                if tp is not None:
                    mag[:, t] += y[:, tp].double().abs() @ whh[i].double().abs().T
            d = 2.0 ** -20 * mag
            dmax = d.view(B, T, 4, H).amax(2)
            return ((acts[i].double() - G).abs() <= d + 2.0 ** -21).all() and \
                ((c.double() - C).abs() <= 3 * dmax + 2.0 ** -21 * (1 + C.abs())).all() and \
                ((y.double() - Y).abs() <= 4 * dmax + 2.0 ** -20).all()
        assert fwd_ok(None), i
        assert T == 1 or not fwd_ok("bf16"), i
        dy = dsl[i].cpu()

        def bwd_err(half, xhalf):
            D, E, _ = R.lstm_bwd_teacher(dy, acts[i], c, whh[i], reverse[i], half, dgates_src=dgt, xhalf=xhalf)
            return (dgt.double() - D).abs(), 1e-5 * D.abs().max().item() + E
        err, tol = bwd_err(None, None)
        assert (err <= tol).all(), (err.max().item(), tol.max().item())
        err_w, _ = bwd_err("bf16", "bf16")
        assert T == 1 or not (err_w <= tol).all()


@pytest.mark.parametrize("B,T", [(65, 1), (65, 2), (32, 3), (33, 3), (64, 3)])
@pytest.mark.parametrize("reverse", [0, 1])
def test_persistent_lstm_x3_one_cell_edges(hip_device, B, T, reverse, monkeypatch):
    """test_persistent_lstm_x3_step_by_step (its models and its bounds) on one cell at the edges of the recurrence:
    T = 1 is the peeled step 0 alone and T = 2 adds the trailing cell update with no step between them; B = 32, 33
    and 64 leave the second half of the 64-sample batch tile empty, with one row and full."""
    test_persistent_lstm_x3_step_by_step(hip_device, B, (reverse,), monkeypatch, T=T)


# ------------------------------------------------------------------ amax words in a training step
EXACT_WORD_OPS = ("gemm_nt", "gemm_tn", "conv3x3_fwd", "conv3x3_repack", "conv3x3_wgrad", "lstm_whh_grad")
BOUND_FACTOR = 2.0 ** 6       # a constant-bound word may overstate its operand by at most 6 binades (6 bits lost)


@pytest.mark.parametrize("nc,H", [(1, 384), (360, 64)])
def test_h2_amax_words_in_a_training_step(hip_device, nc, H, monkeypatch):
    """One JDCNet train forward and backward in h2 mode: every absmax word a product receives from model code, with its
    operand as an ops.Scaled, is checked against that operand, after a device synchronize.  Words from absmax, absmax_segments
    and the producer epilogues (BN / pool passes, maxpool_bwd_add, the persistent backward's dgates_amax) must equal
    max|operand| exactly; the constant words of Scaled.bounded(1 / (1 - p)) and _unit_amax must bound it, within
    BOUND_FACTOR.  The number of checks per op is asserted, so a refactor cannot skip them silently."""
    from oracle import model_ref
    from tests.test_model_gpu import build
    monkeypatch.setattr(ops, "FP32_MATMUL", "h2")
    dev = hip_device
    state = model_ref.seeded_state(5, num_class=nc, hidden_size=H)
    net = build(state, nc, H, dev, dropout=0.2).train()
    counts = {k: [0, 0] for k in EXACT_WORD_OPS}                 # [exact, bound]
    factors = []

    def bound_words():
        return {t.data_ptr() for t in list(ops._BOUND_AMAX.values()) + list(ops._UNIT_AMAX.values())}

    def chk(name, word, operand):
        if word is None:
            return
        torch.cuda.synchronize()
        w = int(word.view(-1)[0].item()) & 0xFFFFFFFF
        m = S.absmax_bits(operand)
        if word.data_ptr() in bound_words():
            wv = float(np.array(w, dtype=np.uint32).view(np.float32))
            mv = float(np.array(m, dtype=np.uint32).view(np.float32))
            assert mv <= wv <= BOUND_FACTOR * max(mv, 2.0 ** -126), (name, wv, mv)
            factors.append(wv / max(mv, 2.0 ** -126))
            counts[name][1] += 1
        else:
            assert w == m, (name, hex(w), hex(m))
            counts[name][0] += 1

    orig = {k: getattr(ops, k) for k in EXACT_WORD_OPS}

    def chk_op(name, operand, default=None):         # an operand as the product gets it: plain or ops.Scaled
        t, word = ops._tw(operand)
        chk(name, default if word is None else word, t)

    def gemm_nt(A, B, *a, **k):
        chk_op("gemm_nt", A); chk_op("gemm_nt", B)
        return orig["gemm_nt"](A, B, *a, **k)

    def gemm_tn(A, B, *a, **k):
        chk_op("gemm_tn", A); chk_op("gemm_tn", B)
        return orig["gemm_tn"](A, B, *a, **k)

    def conv3x3_fwd(x, w_packed, *a, **k):
        chk_op("conv3x3_fwd", x)
        if isinstance(w_packed, ops.PackedWeight):
            chk("conv3x3_fwd", w_packed.amax, w_packed.fp32)
        return orig["conv3x3_fwd"](x, w_packed, *a, **k)

    def conv3x3_repack(w, *a, **k):
        chk_op("conv3x3_repack", w)
        return orig["conv3x3_repack"](w, *a, **k)

    def conv3x3_wgrad(x, dy, dw):
        chk_op("conv3x3_wgrad", x); chk_op("conv3x3_wgrad", dy)
        return orig["conv3x3_wgrad"](x, dy, dw)

    def lstm_whh_grad(dgates, y_slice, dwhh, reverse, B, T, H_):
        chk_op("lstm_whh_grad", dgates)
        chk_op("lstm_whh_grad", y_slice, default=ops._unit_amax(ops._tw(dgates)[0].device))
        return orig["lstm_whh_grad"](dgates, y_slice, dwhh, reverse, B, T, H_)

    for k, f in (("gemm_nt", gemm_nt), ("gemm_tn", gemm_tn), ("conv3x3_fwd", conv3x3_fwd),
                 ("conv3x3_repack", conv3x3_repack), ("conv3x3_wgrad", conv3x3_wgrad),
                 ("lstm_whh_grad", lstm_whh_grad)):
        monkeypatch.setattr(ops, k, f)
    g = torch.Generator().manual_seed(nc)
    x = torch.randn(2, 1, 64, 80, generator=g).to(dev)
    cls, det = net(x)
    torch.autograd.backward([cls, det], [torch.randn(cls.shape, generator=g).to(dev),
                                         torch.randn(det.shape, generator=g).to(dev)])
    torch.cuda.synchronize()
    print(counts, "bound factors", min(factors, default=0), max(factors, default=0))
    # (exact, bound) words checked per op in one step of this model (7 conv layers, 4 BiLSTM layers): the conv
    # counts are 7 repacks, 7 forward + 7 data-gradient convolutions and 7 weight gradients with two words each
    assert counts == {"gemm_nt": [66, 12], "gemm_tn": [26, 12], "conv3x3_fwd": [28, 0], "conv3x3_repack": [7, 0],
                      "conv3x3_wgrad": [14, 0], "lstm_whh_grad": [16, 16]}, counts
