"""Float64 models of the two fp32 product splits (csrc/gemm_engine.h), restated here from their description and kept
independent of the kernels.

"h2" (the default fp32 mode): every operand tensor is scaled by s = 2^(es - 127), es = clamp(267 - E, 1, 253), E = the
biased exponent of the tensor's absmax word, and split into two fp16 terms hi = RNE_f16(x s), lo = RNE_f16(x s - hi)
(fp16 subnormals kept).  A product keeps hi_a hi_b + hi_a lo_b + lo_a hi_b and drops lo_a lo_b; the result is divided
by s_a s_b.  For a tensor of absmax A the operand error is

    |(hi + lo) / s - x|  <=  2^-23 |x| + 2^-38 A                                              (H2_REL, H2_ABS)

the first term while lo is a normal fp16, the second once lo (from |x| < 2^-16 A) or hi (|x| < 2^-27 A) is subnormal.
Relative precision therefore falls by one bit per binade below 2^-16 A.

"x3" (the LSTM recurrences, the strict option): hi = trunc_bf16(x), mid = trunc_bf16(x - hi), lo = trunc_bf16(x - hi -
mid) with both residuals formed in fp32, as split3 packs them.  hi + mid + lo == x bit for bit for |x| >= 2^-110;
below, the second residual is an fp32 subnormal and its truncation drops bits.  A product keeps the six products of
mfma_split (all but mid.lo, lo.mid, lo.lo).

Every product model returns (value, sum of |kept terms|) per output element in float64; the GPU tests hold the kernels
to the value relative to that element's own sum of |terms|.
"""
import numpy as np
import torch
import torch.nn.functional as F

H2_REL = 2.0 ** -23          # operand error of the h2 split while lo is a normal fp16, relative to |x|
H2_ABS = 2.0 ** -38          # ... once lo or hi is an fp16 subnormal, relative to the tensor's absmax
H2_PAIRS = ((1, 0), (0, 1), (0, 0))                              # mfma_split2: lo.hi, hi.lo, hi.hi
X3_PAIRS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))      # mfma_split: the six products it keeps
X3_EXACT_MIN = 2.0 ** -110   # smallest |x| the x3 split rebuilds bit-exactly (CPU self-test)
KS = (0, 12, 16, 20, 24, 28, 32, 36, 40)                          # binades below the tensor maximum of the generator


# ------------------------------------------------------------------ scalars and conversions
def f32_bits(v):
    """IEEE bits of the float32 value v (int)."""
    return int(np.array(v, dtype=np.float32).view(np.uint32))


def absmax_bits(t):
    """The absmax word of a float32 tensor as pe_absmax computes it: the largest |x| bit pattern (NaN above Inf)."""
    b = t.detach().cpu().float().contiguous().numpy().view(np.uint32) & np.uint32(0x7FFFFFFF)
    return int(b.max()) if b.size else 0


def h2_scale_exp(amax_bits):
    """Biased exponent of the h2 scale for a tensor whose absmax word is ``amax_bits``: 267 - E, clamped to [1, 253]
    (a zero or subnormal word gives 2^126, an Inf / NaN word 2^-115)."""
    es = 267 - ((int(amax_bits) >> 23) & 0xFF)
    return min(max(es, 1), 253)


def h2_scale(amax_bits, es_delta=0):
    return 2.0 ** (h2_scale_exp(amax_bits) + es_delta - 127)


def rne_f16(x):
    """float64 tensor -> nearest-even fp16 (subnormals kept, overflow to Inf), back as float64.  numpy converts
    float64 -> float16 in one rounding (torch goes through float32 first)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return torch.from_numpy(x.detach().cpu().double().numpy().astype(np.float16).astype(np.float64))


def trunc_bf16_f32(x):
    """float32 numpy array -> its top 16 bits (bf16 by truncation), as float32."""
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


# ------------------------------------------------------------------ splits
def split_h2(x, amax_bits=None, flush=False, es_delta=0):
    """(hi, lo, s): the two scaled fp16 terms of the float32 tensor x as float64, and the scale.  ``flush`` and
    ``es_delta`` build WRONG models (fp16 subnormal terms flushed to zero; the scale ``es_delta`` binades off) that the
    GPU tests must be able to tell apart from the kernels."""
    x = x.detach().cpu().float()
    s = h2_scale(absmax_bits(x) if amax_bits is None else amax_bits, es_delta)
    with np.errstate(invalid="ignore", over="ignore"):
        t = x.double() * s                   # exact: x s is x with another exponent (float64 has the range)
        hi = rne_f16(t)
        lo = rne_f16(t - hi)                 # t - hi exact in float64; RNE once (the kernel's mixed FMA)
    if flush:
        hi = torch.where(hi.abs() < 2.0 ** -14, torch.zeros_like(hi), hi)
        lo = torch.where(lo.abs() < 2.0 ** -14, torch.zeros_like(lo), lo)
    return hi, lo, s


def split_x3(x):
    """(hi, mid, lo) float64: the truncated bf16 terms of the float32 tensor x, residuals formed in float32 as split3
    forms them."""
    v = x.detach().cpu().float().contiguous().numpy()
    hi = trunc_bf16_f32(v)
    r1 = (v - hi).astype(np.float32)
    mid = trunc_bf16_f32(r1)
    r2 = (r1 - mid).astype(np.float32)
    lo = trunc_bf16_f32(r2)
    return tuple(torch.from_numpy(t.astype(np.float64)) for t in (hi, mid, lo))


def split_bf16(x):
    """one RNE bf16 term (the mixed-precision operand): the wrong model the x3 checks must miss"""
    return (x.detach().cpu().float().to(torch.bfloat16).double(),)


# ------------------------------------------------------------------ products
def terms_product(op, ta, tb, pairs, unscale=1.0):
    """(sum over the kept pairs of op(ta[i], tb[j]), the same sum of op(|ta[i]|, |tb[j]|)), times ``unscale``.
    ``op`` is bilinear (a matmul or a convolution) and runs in float64."""
    val = mag = 0.0
    with np.errstate(invalid="ignore"):
        for i, j in pairs:
            val = val + op(ta[i], tb[j])
            mag = mag + op(ta[i].abs(), tb[j].abs())
    return val * unscale, mag * unscale


def f16_subnormal(t):
    return (t != 0) & (t.abs() < 2.0 ** -14)


MFMA_SUB_GRID = 2.0 ** -36   # per-product error of an f16 MFMA product with an fp16-subnormal factor, times |other|


def h2_subnormal_allowance(op, a, b, amax_a=None, amax_b=None):
    """Per output element, the bound on what the f16 MFMA loses on the kept h2 products that have an fp16-subnormal
    factor (tests/test_split_products_gpu.py, "fp16-subnormal factors"): MFMA_SUB_GRID |other factor| per such
    product, in scaled units, divided by s_a s_b."""
    ha, la, sa = split_h2(a, amax_a)
    hb, lb, sb = split_h2(b, amax_b)
    ta, tb = (ha, la), (hb, lb)
    out = 0.0
    with np.errstate(invalid="ignore"):
        for i, j in H2_PAIRS:
            p, q = ta[i], tb[j]
            out = out + op(f16_subnormal(p).double(), q.abs()) + op(p.abs(), f16_subnormal(q).double())
    return MFMA_SUB_GRID * out / (sa * sb)


def h2_product(op, a, b, amax_a=None, amax_b=None, flush=False, es_delta=0):
    """The h2 model of op(a, b): (value, sum of |terms|).  ``amax_*``: the absmax words the kernel is given (default:
    the operands' own)."""
    ha, la, sa = split_h2(a, amax_a, flush, es_delta)
    hb, lb, sb = split_h2(b, amax_b, flush, es_delta)
    return terms_product(op, (ha, la), (hb, lb), H2_PAIRS, 1.0 / (sa * sb))


def x3_product(op, a, b):
    return terms_product(op, split_x3(a), split_x3(b), X3_PAIRS)


def exact_product(op, a, b):
    """float64 of the unsplit operands"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return op(a, b), op(a.abs(), b.abs())


def bf16_product(op, a, b):
    return terms_product(op, split_bf16(a), split_bf16(b), ((0, 0),))


# bilinear ops of the kernels, float64, on the layouts the tests keep on the CPU
def op_nt(a, b):          # gemm_nt: A [M, K], B [N, K]
    return a @ b.T


def op_tn(a, b):          # gemm_tn: A [K, M], B [K, N]
    return a.T @ b


def im2col(x):
    """x [B, C, T, F] -> [B, C*9, T*F]: the 3x3 taps (zero padding 1) of every pixel, k = c*9 + kh*3 + kw"""
    return F.unfold(x, 3, padding=1)


def op_conv(x, w):
    """3x3 convolution, padding 1, by im2col: x [B, C, T, F], w [N, C, 3, 3] -> [B, N, T, F]"""
    B, _, T, Fq = x.shape
    return (w.reshape(w.shape[0], -1) @ im2col(x)).view(B, w.shape[0], T, Fq)


def dgrad_weight(w):
    """the weight whose forward convolution is the data gradient: w'[c, n, kh, kw] = w[n, c, 2 - kh, 2 - kw]"""
    return w.flip(2, 3).transpose(0, 1)


def op_wgrad(x, dy):
    """weight gradient: dw [N, C, 3, 3] = sum over pixels of dy[p, n] im2col(x)[p, c, tap]; x [B, C, T, F],
    dy [B, N, T, F]"""
    cols = im2col(x)                                                      # [B, C*9, P]
    d = dy.reshape(dy.shape[0], dy.shape[1], -1)                          # [B, N, P]
    return torch.einsum("bnp,bkp->nk", d, cols).view(dy.shape[1], x.shape[1], 3, 3)


# ------------------------------------------------------------------ operands
def heavy(shape, dim, seed, top="below", scale=1.0):
    """float32 operand whose slices along ``dim`` sit at 2^-k of the tensor maximum, k cycling through KS, with exact
    zeros and fp32 subnormals sprinkled in and the tensor's maximum magnitude in its LAST element: ``top`` "below" puts
    it just under the next power of two (scale * (1 - 2^-24)), "pow2" exactly at a power of two (scale); ``scale``
    should be a power of two.  Ordinary elements stay below 0.9 scale."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(*shape, generator=g, dtype=torch.float64) / 8).clamp(-0.9, 0.9)
    k = torch.tensor([KS[i % len(KS)] for i in range(shape[dim])], dtype=torch.float64)
    view = [1] * len(shape)
    view[dim] = shape[dim]
    x = (x * torch.exp2(-k).view(view) * scale).float()
    flat = x.view(-1)
    n = flat.numel()
    flat[7::97] = 0.0
    sub = flat[11::89]
    flat[11::89] = torch.randn(sub.numel(), generator=g).float() * (2.0 ** -135)        # fp32 subnormals
    flat[-1] = -(scale * (1 - 2.0 ** -24)) if top == "below" else scale
    assert n > 1 and absmax_bits(x) == f32_bits(abs(float(flat[-1])))
    return x
