"""Tensor-level wrappers over the C ABI (include/pitchextractor_hip.h).

Every function checks operand shapes/devices on the host before a kernel is launched (an
out-of-bounds launch can reset the GPU), passes raw device pointers plus the current HIP
stream, and never falls back to a torch op.  Activations are channels-last:
``[B, T, F, C]`` float32 contiguous.
"""
from __future__ import annotations

import ctypes as C

import os

import torch

from . import _lib

_WS: dict = {}


def _chk(cond, msg):
    if not cond:
        raise ValueError(msg)


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    _chk(t.is_cuda, f"{name}: expected a HIP device tensor (no CPU fallback)")
    _chk(t.dtype == torch.float32, f"{name}: expected float32")
    return t


def _dense(t: torch.Tensor, name: str) -> torch.Tensor:
    _f32c(t, name)
    _chk(t.is_contiguous(), f"{name}: expected a contiguous tensor")
    return t


# Mixed precision with bf16 ACTIVATION STORAGE (reference trainer.py:226-235 / README.md:36: autocast keeps conv and
# linear outputs in 16 bits): when True (Trainer's mixed-precision scope with the bf16 dtype turns it on) the first
# convolution writes a bf16 tensor and every pass of the conv stack follows the dtype of its inputs -- `act16 = 1`
# in the C ABI.  The temporal heads, the losses and all parameters stay fp32.
ACT_BF16 = False


def act_dtype():
    return torch.bfloat16 if (ACT_BF16 and MATMUL_BF16 and HALF_DTYPE == "bf16") else torch.float32


def _actc(t: torch.Tensor, name: str) -> torch.Tensor:
    """An activation tensor of the conv stack: float32, or bfloat16 under ``ACT_BF16``."""
    _chk(t.is_cuda, f"{name}: expected a HIP device tensor (no CPU fallback)")
    _chk(t.dtype in (torch.float32, torch.bfloat16), f"{name}: expected float32 or bfloat16")
    return t


def _actd(t: torch.Tensor, name: str) -> torch.Tensor:
    _actc(t, name)
    _chk(t.is_contiguous(), f"{name}: expected a contiguous tensor")
    return t


def _act16(*tensors) -> bool:
    """True if the given activation tensors are bfloat16, False if float32; mixing is an error."""
    kinds = {t.dtype for t in tensors if t is not None}
    _chk(len(kinds) == 1, "activation tensors of one call must share a dtype")
    return kinds.pop() == torch.bfloat16


def _rows2d(t: torch.Tensor, name: str, act=False):
    """(rows, cols, ld) of a 2-D row-major view whose rows may be strided (``act``: bf16 activations allowed)."""
    (_actc if act else _f32c)(t, name)
    _chk(t.dim() == 2 and t.stride(1) == 1, f"{name}: expected 2-D with unit column stride")
    ld = t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))
    return t.shape[0], t.shape[1], ld


def workspace(nbytes: int, device) -> torch.Tensor:
    """Grow-only scratch buffer (bytes) per device AND current stream.  Consumers on one stream run in order, so
    a single buffer serves all ops launched there; work on a side stream gets its own."""
    key = (torch.device(device), _lib.stream_ptr())
    buf = _WS.get(key)
    nbytes = max(int(nbytes), 1 << 20)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=key[0])
        _WS[key] = buf
    return buf


class KernelTimer:
    """Optional HIP-event timing of every C-ABI call (bench.py): events are recorded on the stream
    the kernels are launched on and read back after the timed region, so nothing synchronises.
    The key names the entry point and the product form it ran: the entry point, the form's suffix ("_x3", "_h2",
    "_bf16", "_f16"; none for native fp32) and "_a16" for bf16 activation tensors, e.g. ``pe_conv3x3_fwd_wf_h2`` or
    ``pe_gemm_tn_bf16_a16`` (bench.py reads the form and its peak from these keys)."""

    def __init__(self, only=None):
        self.records = {}
        self.only = None if only is None else frozenset(only)     # time just these entry points (None = all)

    def add(self, name, start, end, work):
        self.records.setdefault(name, []).append((start, end, work))

    def summary(self):
        out = {}
        for name, recs in self.records.items():
            ms = [a.elapsed_time(b) for a, b, _ in recs]
            out[name] = dict(calls=len(recs), total_ms=float(sum(ms)), avg_ms=float(sum(ms) / len(ms)),
                             work=float(sum(w for _, _, w in recs)))
        return out


TIMER: KernelTimer | None = None


TIMER_TAG = ""            # appended as "#tag" to the timer key of the calls made inside `timer_tag(tag)`


class timer_tag:
    """Label the timed C-ABI calls of a region (bench.py separates the data-gradient launches of the conv kernel,
    which share the GPU with side-stream weight-gradient kernels, from its forward launches, which run alone)."""

    def __init__(self, tag):
        self.tag, self.prev = tag, ""

    def __enter__(self):
        global TIMER_TAG
        self.prev, TIMER_TAG = TIMER_TAG, self.tag

    def __exit__(self, *exc):
        global TIMER_TAG
        TIMER_TAG = self.prev


# timer-key suffix of each pe_products value (KernelTimer)
_FORM_SUFFIX = {_lib.PE_PROD_NATIVE: "", _lib.PE_PROD_X3: "_x3", _lib.PE_PROD_H2: "_h2", _lib.PE_PROD_BF16: "_bf16",
                _lib.PE_PROD_F16: "_f16"}


def _call(name, *args, products=None, act16=None, work=0.0, key=None):
    """Launch entry point ``name``.  ``products`` and then ``act16`` go in front of ``args`` for the entry points that
    take them; ``key`` (default: see KernelTimer) is what the launch is timed and reported under."""
    if act16 is not None:
        args = (int(act16),) + args
    if products is not None:
        args = (products,) + args
    if key is None:
        key = name + ("" if products is None else _FORM_SUFFIX[products]) + ("_a16" if act16 else "")
    lib = _lib.load()
    if TIMER is None or (TIMER.only is not None and key not in TIMER.only):
        _lib.check(getattr(lib, name)(*args), key)
        return
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    _lib.check(getattr(lib, name)(*args), key)
    b.record()
    TIMER.add(key + ("#" + TIMER_TAG if TIMER_TAG else ""), a, b, work)


def _s():
    return _lib.stream_ptr()


# Opt-in mixed precision (reference trainer.py:103 autocast; config training.mixed_precision): when True the
# conv / linear products and their weight gradients round their operands to bf16 on the way into LDS and
# accumulate in fp32; the persistent LSTM recurrences round W_hh and h to bf16 as well (cell state fp32);
# attention and everything in HBM stay fp32.  False is the parity mode.
MATMUL_BF16 = False
# 16-bit operand type of that mode: "bf16" (default: fp32 exponent range, no loss scaling needed) or "f16" (the
# reference's literal autocast dtype; Trainer(amp_dtype="fp16") drives it together with a GradScaler)
HALF_DTYPE = "bf16"
# How fp32 products run (always, for the weight-gradient products; when MATMUL_BF16 is off for the rest):
#   "x3"     every fp32 operand is split exactly into three bf16 terms and six cross products are
#            accumulated in fp32 on the bf16 MFMA pipe (16x the fp32 MFMA rate on gfx950); measured
#            error against fp64 is the same as the native path's (tests/test_ops_gpu.py).  The strict option.
#   "h2"     every fp32 operand becomes TWO fp16 terms of the tensor scaled by a power of two (absmax below) and
#            three cross products are accumulated in fp32: half the matrix work of "x3".  Default.  Operand error
#            |x^ - x| <= 2^-23 |x| + 2^-38 max|x| over x's tensor: 2^-23 relative within 2^-16 of the maximum,
#            one bit less per binade below (csrc/gemm_engine.h, tests/split_ref.py).
#   "native" v_mfma_f32_32x32x2_f32.
FP32_MATMUL = os.environ.get("PE_FP32_MATMUL", "h2")
_FP32_MODES = ("native", "x3", "h2")


_UNIT_AMAX: dict = {}


def _unit_amax(device):
    """absmax word of a tensor known to lie in [-1, 1] (LSTM outputs): the bits of 1.0f, no pass over the data."""
    key = torch.device(device)
    if key not in _UNIT_AMAX:
        _UNIT_AMAX[key] = torch.full((1,), 0x3F800000, dtype=torch.int32, device=key)
    return _UNIT_AMAX[key]


def absmax_segments(flat, seg_off, seg_len, out=None):
    """out[s] = absmax word of flat[seg_off[s] : seg_off[s] + seg_len[s]] (int64 device tensors), one launch."""
    _dense(flat, "flat")
    n = seg_off.numel()
    _chk(seg_off.is_cuda and seg_len.is_cuda and seg_off.dtype == seg_len.dtype == torch.int64 and seg_len.numel() == n,
         "absmax_segments: int64 device offset / length arrays")
    if out is None:
        out = torch.empty((n,), dtype=torch.int32, device=flat.device)
    _chk(out.is_cuda and out.dtype == torch.int32 and out.numel() == n, "absmax_segments: out")
    _call("pe_absmax_segments", flat.data_ptr(), seg_off.data_ptr(), seg_len.data_ptr(), n, out.data_ptr(), _s())
    return out


def h2_active() -> bool:
    """True when fp32 products run as two scaled fp16 terms, i.e. when GEMM / conv operands need an absmax word."""
    return (not MATMUL_BF16) and FP32_MATMUL == "h2"


_AMAX_POOL: dict = {}


def amax_word():
    """A zeroed int32 device word for a producing pass to max-merge its output's absmax into ("h2" mode; None
    otherwise).  Words are cut from a 256-word block zeroed by one fill; a block lives as long as any of its words."""
    if not h2_active():
        return None
    key = (torch.cuda.current_device(), _lib.stream_ptr())
    blk = _AMAX_POOL.get(key)
    if blk is None or blk[1] >= blk[0].numel():
        blk = [torch.zeros(256, dtype=torch.int32, device="cuda"), 0]
        _AMAX_POOL[key] = blk
    blk[1] += 1
    return blk[0][blk[1] - 1:blk[1]]


_BOUND_AMAX: dict = {}


def absmax(t, out=None):
    """uint32 device word = IEEE bits of max |t| (t: float32, 1-D / 2-D row-strided / dense N-D): the scale source of
    an "h2" operand."""
    _f32c(t, "absmax operand")
    if t.dim() == 2 and t.stride(1) == 1:
        rows, cols, ld = _rows2d(t, "absmax operand")
    else:
        _chk(t.is_contiguous(), "absmax: expected a dense tensor or a row-strided matrix")
        cols = t.shape[-1] if t.dim() > 1 else t.numel()
        rows, ld = t.numel() // max(cols, 1), cols
    if out is None:
        out = torch.empty((1,), dtype=torch.int32, device=t.device)
    _chk(out.is_cuda and out.dtype == torch.int32 and out.numel() == 1, "absmax: out is an int32 device word")
    _call("pe_absmax", t.data_ptr(), rows, cols, ld, out.data_ptr(), _s())
    return out


class Scaled:
    """A tensor with its "h2" scale word: ``t``, and ``amax`` = the 1-element int32 device tensor with the IEEE bits of
    max |t| (or of a bound on it), None for "not known".  Every product takes a plain tensor or a ``Scaled`` for an
    operand and returns a plain tensor.  A plain tensor and a ``Scaled`` without a word are alike: an "h2" product then
    takes the maximum in a pass of its own; the other forms read no word.  The pairing speaks of the buffer's contents
    when it was made (a pass that overwrites ``t`` hands back a new one) and holds the reference that keeps the word's
    memory from becoming the next ``absmax()``'s output before the product that reads it is launched.  Reshaping views
    keep the word; an index or slice gives a plain tensor, whose maximum nobody knows.  Made by ``measured``, ``bounded``
    or a producing pass (``bn_act_pool_fwd`` / ``_bwd``, ``lstm_bwd``) asked with ``amax_out=True``: the pass takes a
    zeroed word of ``amax_word()`` and returns the pairing.  (A caller that passes its own zeroed word as ``amax_out``
    holds the word already and gets the plain output.)"""

    __slots__ = ("t", "amax")

    def __init__(self, t, amax=None):
        self.t, self.amax = t, amax

    @classmethod
    def measured(cls, t):
        """``t`` (plain, or a ``Scaled``: a word it has is kept) with the word of a stand-alone ``absmax`` pass in "h2"
        mode, without one otherwise."""
        t, amax = _tw(t)
        return cls(t, absmax(t) if (amax is None and h2_active()) else amax)

    @classmethod
    def bounded(cls, t, bound: float):
        """``t`` known to satisfy |t| <= bound, with the constant word of the bound ("h2" mode; no pass over the data)."""
        if not h2_active():
            return cls(t)
        key = (t.device, float(bound))
        if key not in _BOUND_AMAX:
            import struct
            bits = struct.unpack("<i", struct.pack("<f", float(bound)))[0]
            _BOUND_AMAX[key] = torch.full((1,), bits, dtype=torch.int32, device=key[0])
        return cls(t, _BOUND_AMAX[key])

    @property
    def shape(self):
        return self.t.shape

    def view(self, *shape):
        return Scaled(self.t.view(*shape), self.amax)

    def __getitem__(self, index):
        return self.t[index]


def _tw(x):
    """(tensor, scale word or None) of an operand: a plain tensor or a ``Scaled``."""
    return (x.t, x.amax) if isinstance(x, Scaled) else (x, None)


# which persistent LSTM recurrences use the three-term split when FP32_MATMUL == "x3" (tools/bench_lstm.py)
LSTM_X3 = {"fwd": os.environ.get("PE_LSTM_X3_FWD", "1") == "1", "bwd": os.environ.get("PE_LSTM_X3_BWD", "1") == "1"}


def products_for(op="gemm"):
    """The pe_products value (``_lib.PE_PROD_*``) the module state selects for one kind of product.
    "gemm": GEMMs, convolutions and weight gradients -- the 16-bit type under mixed precision (what autocast runs,
      its backward included), else FP32_MATMUL.
    "lstm_fwd" / "lstm_bwd": the persistent recurrences -- the 16-bit type under mixed precision (as autocast runs
      nn.LSTM); x3 under x3 and h2 ("h2" products need a tensor-wide scale before the first element is produced, and
      the recurrences make their operands step by step); PE_PROD_NATIVE = the one-launch-per-step kernels, which also
      serve native fp32, LSTM_X3 off and USE_PERSISTENT_LSTM off.
    "attn": the fused attention -- bf16 under bf16 mixed precision, as autocast runs it; exact fp32 MFMAs otherwise
      (the fp16 mode included)."""
    if op == "attn":
        return _lib.PE_PROD_BF16 if (MATMUL_BF16 and HALF_DTYPE == "bf16") else _lib.PE_PROD_NATIVE
    if op != "gemm" and not USE_PERSISTENT_LSTM:
        return _lib.PE_PROD_NATIVE
    if MATMUL_BF16:
        return _lib.PE_PROD_BF16 if HALF_DTYPE == "bf16" else _lib.PE_PROD_F16
    _chk(FP32_MATMUL in _FP32_MODES, "ops.FP32_MATMUL must be 'native', 'x3' or 'h2'")
    if op == "gemm":
        return {"native": _lib.PE_PROD_NATIVE, "x3": _lib.PE_PROD_X3, "h2": _lib.PE_PROD_H2}[FP32_MATMUL]
    x3 = FP32_MATMUL != "native" and LSTM_X3[op[len("lstm_"):]]
    return _lib.PE_PROD_X3 if x3 else _lib.PE_PROD_NATIVE


class matmul_bf16:
    """``with ops.matmul_bf16(True): ...`` -- the autocast-like scope Trainer.run opens for a mixed-precision step.
    ``act16=True`` (bf16 only) additionally stores the conv stack's activations and their gradients as bf16 tensors
    (``ACT_BF16``)."""

    def __init__(self, enabled=True, dtype="bf16", act16=False):
        _chk(dtype in ("bf16", "f16"), "matmul_bf16: dtype must be 'bf16' or 'f16'")
        self.enabled, self.dtype = bool(enabled), dtype
        self.act16 = bool(act16) and self.enabled and dtype == "bf16"

    def __enter__(self):
        global MATMUL_BF16, HALF_DTYPE, ACT_BF16
        self._prev = (MATMUL_BF16, HALF_DTYPE, ACT_BF16)
        MATMUL_BF16, HALF_DTYPE, ACT_BF16 = self.enabled, self.dtype, self.act16
        return self

    def __exit__(self, *exc):
        global MATMUL_BF16, HALF_DTYPE, ACT_BF16
        MATMUL_BF16, HALF_DTYPE, ACT_BF16 = self._prev
        return False


# ------------------------------------------------------------------ GEMM
def gemm_nt(A, B, bias0=None, bias1=None, out=None, accumulate=False):
    """out[M,N] = A[M,K] @ B[N,K]^T + bias0 + bias1 (+ out).  A, B: plain tensors or ``Scaled`` (the operands' absmax
    words when the caller already has them: "h2" mode; computed here otherwise)."""
    (A, amax_a), (B, amax_b) = _tw(A), _tw(B)
    M, K, lda = _rows2d(A, "A", act=True)
    N, K2, ldb = _rows2d(B, "B")
    _chk(K == K2, "gemm_nt: K mismatch")
    if out is None:
        _chk(not accumulate, "accumulate needs out")
        out = torch.empty((M, N), dtype=A.dtype, device=A.device)
    Mo, No, ldc = _rows2d(out, "out", act=True)
    _chk((Mo, No) == (M, N), "gemm_nt: out shape")
    for b in (bias0, bias1):
        if b is not None:
            _chk(_dense(b, "bias").numel() == N, "bias size")
    p, a16 = products_for(), _act16(A, out)
    _chk(not a16 or p == _lib.PE_PROD_BF16, "bfloat16 activations need the bf16 mixed-precision mode")
    if p == _lib.PE_PROD_H2:
        amax_a = absmax(A) if amax_a is None else amax_a
        amax_b = absmax(B) if amax_b is None else amax_b
    _call("pe_gemm_nt", A.data_ptr(), lda, B.data_ptr(), ldb, out.data_ptr(), ldc, M, N, K, _lib.ptr(bias0),
          _lib.ptr(bias1), int(bool(accumulate)), _lib.ptr(amax_a), _lib.ptr(amax_b), _s(), products=p, act16=a16,
          work=2.0 * M * N * K)
    return out


def gemm_tn(A, B, out=None, accumulate=False):
    """out[M,N] = A[K,M]^T @ B[K,N] (+ out); deterministic split-K.  A, B: plain tensors or ``Scaled``."""
    (A, amax_a), (B, amax_b) = _tw(A), _tw(B)
    K, M, lda = _rows2d(A, "A", act=True)
    K2, N, ldb = _rows2d(B, "B", act=True)
    _chk(K == K2, "gemm_tn: K mismatch")
    if out is None:
        _chk(not accumulate, "accumulate needs out")
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    Mo, No, ldc = _rows2d(out, "out")
    _chk((Mo, No) == (M, N), "gemm_tn: out shape")
    p, a16 = products_for(), _act16(A, B)
    _chk(not a16 or p == _lib.PE_PROD_BF16, "bfloat16 activations need the bf16 mixed-precision mode")
    ws = workspace(_lib.load().pe_gemm_tn_workspace_bytes(M, N, K), A.device)
    if p == _lib.PE_PROD_H2:
        amax_a = absmax(A) if amax_a is None else amax_a
        amax_b = absmax(B) if amax_b is None else amax_b
    _call("pe_gemm_tn", A.data_ptr(), lda, B.data_ptr(), ldb, out.data_ptr(), ldc, M, N, K, int(bool(accumulate)),
          ws.data_ptr(), ws.numel(), _lib.ptr(amax_a), _lib.ptr(amax_b), _s(), products=p, act16=a16,
          work=2.0 * M * N * K)
    return out


def transpose2d(x, out=None):
    """x^T; of a ``Scaled`` a ``Scaled`` with the same word (the same values)."""
    if isinstance(x, Scaled):
        return Scaled(transpose2d(x.t, out), x.amax)
    x = _dense(x, "x")
    _chk(x.dim() == 2, "transpose2d: 2-D")
    if out is None:
        out = torch.empty((x.shape[1], x.shape[0]), dtype=torch.float32, device=x.device)
    _chk(_dense(out, "out").numel() == x.numel(), "transpose2d: out size")
    _call("pe_transpose2d", x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], _s())
    return out


# ------------------------------------------------------------------ conv
# x3 / h2 / bf16 / f16 modes: 3x3 weights are packed once per step into MFMA B-fragment order (the form's 16-bit
# terms) and the halo kernel loads them straight from L2 into registers (csrc/conv.hip).
CONV_WFRAG = os.environ.get("PE_CONV_WFRAG", "1") == "1"


class PackedWeight:
    """One packed 3x3 weight: ``fp32`` [N, 9*C] (native MFMA path, fallback shapes) and, in the x3 / h2 / bf16 / f16
    modes, ``frag`` = the same matrix as 16-bit MFMA fragments packed for the pe_products value ``products`` (h2:
    scaled by ``amax``, the weight's absmax word).  Built from the matrix as a plain tensor or a ``Scaled``, whose word
    it keeps."""

    def __init__(self, w, frag=None, products=None):
        (self.fp32, self.amax), self.frag, self.products = _tw(w), frag, products

    @property
    def shape(self):
        return self.fp32.shape


def wfrag_pack(w2d, products):
    """[N, K] float32 (K % 16 == 0) -> fragment-ordered 16-bit terms of the form ``products`` (uint8 buffer); h2 needs
    the weight's absmax word (a ``Scaled`` with one)."""
    w2d, amax = _tw(w2d)
    N, K, ld = _rows2d(w2d, "w")
    nbytes = _lib.load().pe_wfrag_bytes(products, N, K)
    _chk(nbytes > 0, "wfrag_pack: K must be a multiple of 16 and the form x3, h2, bf16 or f16")
    _chk(products != _lib.PE_PROD_H2 or amax is not None, "wfrag_pack: two-term fragments need amax")
    out = torch.empty((nbytes,), dtype=torch.uint8, device=w2d.device)
    # timer key: x3 and bf16 fragments are reported together under the bare name
    _call("pe_wfrag_pack", products, w2d.data_ptr(), ld, N, K, _lib.ptr(amax), out.data_ptr(), _s(),
          key="pe_wfrag_pack" + {_lib.PE_PROD_H2: "_h2", _lib.PE_PROD_F16: "_f16"}.get(products, ""))
    return out


def conv3x3_repack(w, want_fwd=True, want_dgrad=True):
    """OIHW (Cout,Cin,3,3), plain or ``Scaled`` -> (w_fwd [Cout, 9*Cin], w_dgrad [Cin, 9*Cout]) as ``PackedWeight``s
    with the weight's absmax word ("h2" mode: the one handed over, else computed here)."""
    w, amax = _tw(w)
    w = _dense(w, "w")
    _chk(w.dim() == 4 and w.shape[2:] == (3, 3), "conv3x3_repack: OIHW 3x3")
    co, ci = w.shape[0], w.shape[1]
    wf = torch.empty((co, 9 * ci), dtype=torch.float32, device=w.device) if want_fwd else None
    wd = torch.empty((ci, 9 * co), dtype=torch.float32, device=w.device) if want_dgrad else None
    _call("pe_conv3x3_repack", w.data_ptr(), _lib.ptr(wf), _lib.ptr(wd), co, ci, _s())
    p = products_for()
    if p != _lib.PE_PROD_H2:
        amax = None
    elif amax is None:
        amax = absmax(w.view(co, ci * 9))                               # forward and data-gradient forms share it
    out = []
    for t in (wf, wd):
        if t is None:
            out.append(None)
        elif CONV_WFRAG and p != _lib.PE_PROD_NATIVE and t.shape[1] % 16 == 0:
            out.append(PackedWeight(Scaled(t, amax), wfrag_pack(Scaled(t, amax), p), p))
        else:
            out.append(PackedWeight(Scaled(t, amax)))
    return out[0], out[1]


def conv3x3_fwd(x, w_packed, out=None, accumulate=False, bn_stats=None):
    """x [B,T,F,C] (plain or ``Scaled``), w_packed [N, 9*C] (tensor or PackedWeight) -> y [B,T,F,N] (+= when accumulate).
    ``bn_stats`` True / False (not None) returns (y, partials): with True the fragment-fed kernel leaves the BatchNorm
    column sums of its final outputs behind ([tiles, 2, N] float64, for ``bn_train_stats(..., partials=)``);
    partials is None when not asked for or when another kernel ran."""
    x, amax = _tw(x)
    x = _actd(x, "x")
    pw = w_packed if isinstance(w_packed, PackedWeight) else PackedWeight(w_packed)
    w32 = _dense(pw.fp32, "w_packed")
    _chk(x.dim() == 4 and w32.dim() == 2, "conv3x3_fwd: ranks")
    B, T, F, Cc = x.shape
    N = w32.shape[0]
    _chk(w32.shape[1] == 9 * Cc, "conv3x3_fwd: weight K")
    if out is None:
        _chk(not accumulate, "accumulate needs out")
        out = torch.empty((B, T, F, N), dtype=x.dtype, device=x.device)
    _chk(_actd(out, "out").shape == (B, T, F, N), "conv3x3_fwd: out shape")
    p, a16 = products_for(), _act16(x, out)
    _chk(not a16 or p == _lib.PE_PROD_BF16, "bfloat16 activations need the bf16 mixed-precision mode")
    amax_w = None
    if p == _lib.PE_PROD_H2:
        amax_w = pw.amax if pw.amax is not None else absmax(w32)
        amax = absmax(x) if amax is None else amax
    h2 = (_lib.ptr(amax), _lib.ptr(amax_w))
    work = 2.0 * B * T * F * N * 9 * Cc
    if pw.frag is not None and pw.products == p and CONV_WFRAG and _lib.load().pe_conv3x3_wf_supported(F, Cc, N):
        parts = None
        if bn_stats:
            parts = torch.empty((_lib.load().pe_conv3x3_wf_stat_parts(B, T, F), 2, N), dtype=torch.float64,
                                device=x.device)
        _call("pe_conv3x3_fwd_wf", x.data_ptr(), pw.frag.data_ptr(), out.data_ptr(), B, T, F, Cc, N,
              int(bool(accumulate)), _lib.ptr(parts), *h2, _s(), products=p, act16=a16, work=work)
        return (out, parts) if bn_stats is not None else out
    _call("pe_conv3x3_fwd", x.data_ptr(), w32.data_ptr(), out.data_ptr(), B, T, F, Cc, N, int(bool(accumulate)), *h2,
          _s(), products=p, act16=a16, work=work)
    return (out, None) if bn_stats is not None else out


def conv3x3_wgrad(x, dy, dw):
    """dw (OIHW view, contiguous) = grad of conv3x3 wrt weights.  x, dy: plain tensors or ``Scaled``."""
    (x, amax_x), (dy, amax_dy) = _tw(x), _tw(dy)
    x = _actd(x, "x")
    dy = _actd(dy, "dy")
    dw = _dense(dw, "dw")
    B, T, F, Ci = x.shape
    Co = dy.shape[3]
    _chk(dy.shape[:3] == (B, T, F), "conv3x3_wgrad: dy shape")
    _chk(dw.shape == (Co, Ci, 3, 3), "conv3x3_wgrad: dw shape")
    p, a16 = products_for(), _act16(x, dy)
    _chk(not a16 or p == _lib.PE_PROD_BF16, "bfloat16 activations need the bf16 mixed-precision mode")
    ws = workspace(_lib.load().pe_conv3x3_wgrad_workspace_bytes(B, T, F, Ci, Co), x.device)
    if p == _lib.PE_PROD_H2:
        # (both words stay referenced until the launch: see ``Scaled``)
        amax_x = absmax(x) if amax_x is None else amax_x
        amax_dy = absmax(dy) if amax_dy is None else amax_dy
    _call("pe_conv3x3_wgrad", x.data_ptr(), dy.data_ptr(), dw.data_ptr(), B, T, F, Ci, Co, ws.data_ptr(), ws.numel(),
          _lib.ptr(amax_x), _lib.ptr(amax_dy), _s(), products=p, act16=a16, work=2.0 * B * T * F * Co * 9 * Ci)
    return dw


def _btf_view(x):
    """(B,T,F) float32 view with arbitrary strides (the mel batch after transpose(-1,-2))."""
    _f32c(x, "x")
    _chk(x.dim() == 3, "expected (B,T,F)")
    return x.shape, x.stride()


def conv3x3_c1_fwd(x_btf, w, out=None, bn_stats=None):
    """First convolution.  bn_stats is None: returns out.  Otherwise returns (out, partials): with bn_stats true the
    kernel also leaves the BatchNorm batch statistics of its output as [parts][2][64] float64 partial sums (else None),
    as conv3x3_fwd does."""
    (B, T, F), (sb, st, sf) = _btf_view(x_btf)
    w = _dense(w, "w")
    _chk(w.shape == (64, 1, 3, 3), "first conv is 1 -> 64")
    if out is None:
        out = torch.empty((B, T, F, 64), dtype=act_dtype(), device=x_btf.device)
    _chk(_actd(out, "out").shape == (B, T, F, 64), "conv3x3_c1_fwd: out shape")
    parts = None
    if bn_stats:
        parts = torch.empty((_lib.load().pe_conv3x3_c1_stat_parts(B, T, F), 2, 64), dtype=torch.float64,
                            device=x_btf.device)
    _call("pe_conv3x3_c1_fwd", x_btf.data_ptr(), sb, st, sf, w.data_ptr(), out.data_ptr(), B, T, F, _lib.ptr(parts), _s(),
          act16=_act16(out))
    return out if bn_stats is None else (out, parts)


def conv3x3_c1_wgrad(x_btf, dy, dw):
    (B, T, F), (sb, st, sf) = _btf_view(x_btf)
    dy = _actd(dy, "dy")
    dw = _dense(dw, "dw")
    _chk(dy.shape == (B, T, F, 64) and dw.shape == (64, 1, 3, 3), "conv3x3_c1_wgrad: shapes")
    lib = _lib.load()
    ws = workspace(lib.pe_conv3x3_wgrad_workspace_bytes(B, T, F, 1, 64), dy.device)
    _call("pe_conv3x3_c1_wgrad", x_btf.data_ptr(), sb, st, sf, dy.data_ptr(), dw.data_ptr(), B, T, F, ws.data_ptr(),
          ws.numel(), _s(), act16=_act16(dy))
    return dw


def conv3x3_c1_dgrad(dy, w, out=None):
    """Data gradient of the first convolution: dy [B,T,F,64] (float32, bfloat16 or float16) -> dx [B,T,F] float32."""
    _chk(dy.is_cuda and dy.is_contiguous() and dy.dim() == 4 and dy.shape[3] == 64 and dy.dtype in _DGRAD_ACT,
         "conv3x3_c1_dgrad: dy must be a dense [B,T,F,64] float32 / bfloat16 / float16 device tensor")
    w = _dense(w, "w")
    _chk(w.shape == (64, 1, 3, 3) and w.device == dy.device, "first conv is 1 -> 64")
    B, T, F = dy.shape[:3]
    if out is None:
        out = torch.empty((B, T, F), dtype=torch.float32, device=dy.device)
    _chk(_dense(out, "out").shape == (B, T, F) and out.device == dy.device, "conv3x3_c1_dgrad: out shape")
    a16 = _DGRAD_ACT[dy.dtype]
    _call("pe_conv3x3_c1_dgrad", a16, dy.data_ptr(), w.data_ptr(), out.data_ptr(), B, T, F, _s(),
          work=2.0 * B * T * F * 576, key="pe_conv3x3_c1_dgrad" + ("_a16" if a16 else ""))
    return out


_DGRAD_ACT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}      # the entry point's act16 values


# ------------------------------------------------------------------ BN / pooling / dropout
class BnState:
    """Per-call BN tensors: mean, invstd, scale, shift (all [C]).  ``eval``: they are the running statistics and their
    affine map (bn_eval_affine), so the backward pass has no batch-statistics terms."""

    def __init__(self, C_, device, eval=False):
        buf = torch.empty((4, C_), dtype=torch.float32, device=device)
        self.mean, self.invstd, self.scale, self.shift = buf[0], buf[1], buf[2], buf[3]
        self.eval = bool(eval)


def bn_train_stats(x, gamma, beta, running_mean, running_var, eps=1e-5, momentum=0.1, partials=None):
    """Train-mode BatchNorm statistics of x [.., C].  ``partials`` ([parts, 2, C] float64 column sums / sums of
    squares left behind by the kernel that produced x) skips the pass over x."""
    x = _actd(x, "x")
    Cc = x.shape[-1]
    for t, n in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None:
            _chk(_dense(t, n).numel() == Cc, f"{n}: size")
    st = BnState(Cc, x.device)
    lib = _lib.load()
    if partials is not None:
        _chk(partials.is_cuda and partials.dtype == torch.float64 and partials.is_contiguous() and partials.dim() == 3
             and partials.shape[1:] == (2, Cc), "bn_train_stats: partials [parts, 2, C] float64")
        ws = workspace(lib.pe_bn_workspace_bytes(Cc), x.device)
        _call("pe_bn_finalize_stats", partials.data_ptr(), partials.shape[0], x.numel() // Cc, Cc, gamma.data_ptr(),
              beta.data_ptr(), eps, momentum, _lib.ptr(running_mean), _lib.ptr(running_var), st.mean.data_ptr(),
              st.invstd.data_ptr(), st.scale.data_ptr(), st.shift.data_ptr(), ws.data_ptr(), ws.numel(), _s())
        return st
    ws = workspace(lib.pe_bn_workspace_bytes(Cc), x.device)
    _call("pe_bn_train_stats", x.data_ptr(), x.numel() // Cc, Cc, gamma.data_ptr(), beta.data_ptr(), eps, momentum,
          _lib.ptr(running_mean), _lib.ptr(running_var), st.mean.data_ptr(), st.invstd.data_ptr(),
          st.scale.data_ptr(), st.shift.data_ptr(), ws.data_ptr(), ws.numel(), _s(), act16=_act16(x))
    return st


def bn_eval_affine(gamma, beta, running_mean, running_var, eps=1e-5):
    Cc = gamma.numel()
    st = BnState(Cc, gamma.device, eval=True)
    for t in (gamma, beta, running_mean, running_var):
        _chk(_dense(t, "bn tensor").numel() == Cc, "bn tensor size")
    _call("pe_bn_eval_affine", gamma.data_ptr(), beta.data_ptr(), running_mean.data_ptr(), running_var.data_ptr(),
          eps, Cc, st.scale.data_ptr(), st.shift.data_ptr(), st.mean.data_ptr(), st.invstd.data_ptr(), _s())
    return st


def _slice_target(out, B, T, Fo, Cc, coff):
    """out is a dense [B,T,Fo,Ctot] tensor; we write channels [coff, coff+C)."""
    _actd(out, "out")
    _chk(out.dim() == 4 and out.shape[:3] == (B, T, Fo), "output pixel grid mismatch")
    ld = out.shape[3]
    _chk(0 <= coff and coff + Cc <= ld, "channel slice out of range")
    return ld


class Tap:
    """A detector tap of the tensor a BN pass reads: MaxPool2d((1, pool)) of the raw input into channels
    [coff, coff + C) of ``out`` ([B, T, F // pool, Ctot]).  ``bn_act_pool_fwd(tap=...)`` writes the slice and, with
    ``want_argmax``, leaves the positions of the maxima in ``argmax``; ``bn_act_pool_bwd(tap=...)`` reads ``grad`` (the
    gradient of ``out``, same layout) and ``argmax`` and adds the tap's gradient to the dx it writes."""

    def __init__(self, out, pool, coff, want_argmax=False):
        self.out, self.pool, self.coff, self.want_argmax = out, int(pool), int(coff), bool(want_argmax)
        self.argmax = None
        self.grad = None


def _tap_folded(x, pool, tap: Tap, with_arg) -> bool:
    """True if the library's fused pass serves this tap; otherwise the BN pass and the tap pass run one after the other."""
    B, T, F, Cc = x.shape
    return bool(_lib.load().pe_bn_act_pool_tap_supported(B * T, F, Cc, pool, tap.pool, int(with_arg)))


def bn_act_pool_fwd(x, st: BnState, pool=1, slope=0.01, out=None, coff=0, amax_out=None, tap: Tap | None = None):
    """``amax_out``: a zeroed word, where the pass leaves the absmax of its output, or True (see ``Scaled``).
    ``tap``: also max-pool the raw x into ``tap.out`` (see ``Tap``), in the same pass where the library serves it."""
    x = _actd(x, "x")
    paired, amax_out = amax_out is True, (amax_word() if amax_out is True else amax_out)
    B, T, F, Cc = x.shape
    Fo = F // pool
    if out is None:
        out = torch.empty((B, T, Fo, Cc), dtype=x.dtype, device=x.device)
    ld = _slice_target(out, B, T, Fo, Cc, coff)
    if tap is not None and _tap_folded(x, pool, tap, tap.want_argmax):
        Ft = F // tap.pool
        tld = _slice_target(tap.out, B, T, Ft, Cc, tap.coff)
        tap.argmax = torch.empty((B, T, Ft, Cc), dtype=torch.uint8, device=x.device) if tap.want_argmax else None
        _call("pe_bn_act_pool_tap_fwd", x.data_ptr(), st.scale.data_ptr(), st.shift.data_ptr(), slope, out.data_ptr(),
              B * T, F, Cc, pool, ld, coff, _lib.ptr(amax_out), tap.out.data_ptr(), tld, tap.coff, tap.pool,
              _lib.ptr(tap.argmax), _s(), act16=_act16(x, out, tap.out))
        return Scaled(out, amax_out) if paired else out
    _call("pe_bn_act_pool_fwd", x.data_ptr(), st.scale.data_ptr(), st.shift.data_ptr(), slope, out.data_ptr(),
          B * T, F, Cc, pool, ld, coff, _lib.ptr(amax_out), _s(), act16=_act16(x, out))
    if tap is not None:
        if tap.want_argmax:
            _, tap.argmax = maxpool_fwd(x, tap.pool, out=tap.out, coff=tap.coff, want_argmax=True)
        else:
            maxpool_fwd(x, tap.pool, out=tap.out, coff=tap.coff)
    return Scaled(out, amax_out) if paired else out


def bn_act_pool_bwd(x, dy, st: BnState, dgamma, dbeta, pool=1, slope=0.01, coff=0, dx=None, amax_out=None,
                    tap: Tap | None = None):
    """``amax_out``: as in ``bn_act_pool_fwd``, for dx.  ``tap`` (with ``grad`` and ``argmax`` set): dx also takes the
    gradient of the tap, and ``amax_out`` what ``maxpool_bwd_add`` would have merged into it.  The mode follows
    ``st.eval``; with an eval-mode state ``dgamma`` and ``dbeta`` may both be None (input gradient only: no per-channel
    reduction, no workspace).  ``pool`` is 1, 2 or 4: the widths the backward kernels are built for."""
    x = _actd(x, "x")
    _chk(pool in (1, 2, 4), "bn_act_pool_bwd: pool is 1, 2 or 4")
    paired, amax_out = amax_out is True, (amax_word() if amax_out is True else amax_out)
    B, T, F, Cc = x.shape
    ld = _slice_target(dy, B, T, F // pool, Cc, coff)
    if dx is None:
        dx = torch.empty_like(x)
    _chk(_actd(dx, "dx").shape == x.shape, "dx shape")
    ev = int(st.eval)
    if dgamma is None and dbeta is None:
        _chk(st.eval, "bn_act_pool_bwd: only an eval-mode BatchNorm has an input gradient without dgamma / dbeta")
        ws_ptr, ws_len = None, 0
    else:
        _chk(_dense(dgamma, "dgamma").numel() == Cc and _dense(dbeta, "dbeta").numel() == Cc, "dgamma/dbeta size")
        ws = workspace(_lib.load().pe_bn_workspace_bytes(Cc) + 8 * Cc, x.device)
        ws_ptr, ws_len = ws.data_ptr(), ws.numel()
    if tap is not None and tap.argmax is not None and _tap_folded(x, pool, tap, True):
        Ft = F // tap.pool
        _chk(tap.argmax.is_cuda and tap.argmax.dtype == torch.uint8 and tap.argmax.is_contiguous()
             and tap.argmax.shape == (B, T, Ft, Cc), "bn_act_pool_bwd: tap argmax shape")
        tld = _slice_target(tap.grad, B, T, Ft, Cc, tap.coff)
        _call("pe_bn_act_pool_tap_bwd", x.data_ptr(), dy.data_ptr(), st.scale.data_ptr(), st.shift.data_ptr(),
              st.mean.data_ptr(), st.invstd.data_ptr(), slope, dx.data_ptr(), _lib.ptr(dgamma), _lib.ptr(dbeta),
              B * T, F, Cc, pool, ld, coff, ev, ws_ptr, ws_len, _lib.ptr(amax_out), tap.grad.data_ptr(), tld,
              tap.coff, tap.pool, tap.argmax.data_ptr(), _s(), act16=_act16(x, dy, dx, tap.grad))
        return Scaled(dx, amax_out) if paired else dx
    _call("pe_bn_act_pool_bwd", x.data_ptr(), dy.data_ptr(), st.scale.data_ptr(), st.shift.data_ptr(),
          st.mean.data_ptr(), st.invstd.data_ptr(), slope, dx.data_ptr(), _lib.ptr(dgamma), _lib.ptr(dbeta),
          B * T, F, Cc, pool, ld, coff, ev, ws_ptr, ws_len, _lib.ptr(amax_out), _s(), act16=_act16(x, dy, dx))
    if tap is not None:
        maxpool_bwd_add(x, tap.grad, dx, tap.pool, coff=tap.coff, amax_out=amax_out, argmax=tap.argmax)
    return Scaled(dx, amax_out) if paired else dx


def maxpool_fwd(x, pool, out=None, coff=0, want_argmax=False):
    """MaxPool2d((1, pool)) into a channel slice.  ``want_argmax``: also return the uint8 window positions of the
    maxima ([B, T, F // pool, C]) for ``maxpool_bwd_add(argmax=...)``: returns (out, argmax)."""
    x = _actd(x, "x")
    B, T, F, Cc = x.shape
    Fo = F // pool
    if out is None:
        out = torch.empty((B, T, Fo, Cc), dtype=x.dtype, device=x.device)
    ld = _slice_target(out, B, T, Fo, Cc, coff)
    arg = torch.empty((B, T, Fo, Cc), dtype=torch.uint8, device=x.device) if want_argmax else None
    if Fo == 0:                                 # F < pool: no window, nothing to write (and no pointer to pass)
        _act16(x, out)
        return (out, arg) if want_argmax else out
    _call("pe_maxpool_fwd", x.data_ptr(), out.data_ptr(), B * T, F, Cc, pool, ld, coff, _lib.ptr(arg), _s(),
          act16=_act16(x, out))
    return (out, arg) if want_argmax else out


def maxpool_bwd_add(x, dy, dx, pool, coff=0, amax_out=None, argmax=None):
    """dx[first maximum of each window] += dy; the values written are max-merged into the word of a ``Scaled`` dx,
    which comes back as a new pairing (or into the caller's own ``amax_out`` for a plain dx).  With ``argmax`` (from
    ``maxpool_fwd``) x is only used for its shape."""
    B, T, F, Cc = x.shape
    paired = isinstance(dx, Scaled)
    if paired:
        _chk(amax_out is None, "maxpool_bwd_add: a Scaled dx brings its word")
        dx, amax_out = dx.t, dx.amax
    if argmax is None:
        x = _actd(x, "x")
    else:
        _chk(argmax.is_cuda and argmax.dtype == torch.uint8 and argmax.is_contiguous()
             and argmax.shape == (B, T, F // pool, Cc), "maxpool_bwd_add: argmax shape")
    ld = _slice_target(dy, B, T, F // pool, Cc, coff)
    _chk(_actd(dx, "dx").shape == x.shape, "dx shape")
    if F // pool == 0:                          # F < pool: no window, dx stays as it is
        _act16(dy, dx, x if argmax is None else None)
        return Scaled(dx, amax_out) if paired else dx
    _call("pe_maxpool_bwd_add", x.data_ptr() if argmax is None else 0, _lib.ptr(argmax), dy.data_ptr(), dx.data_ptr(),
          B * T, F, Cc, pool, ld, coff, _lib.ptr(amax_out), _s(), act16=_act16(dy, dx, x if argmax is None else None))
    return Scaled(dx, amax_out) if paired else dx


def dropout(x2d, p, out2d=None, mask_in=None, want_mask=True, seed=0, offset=0):
    """Row-strided 2-D dropout.  Returns (out, mask uint8 [rows, cols] or None)."""
    rows, cols, ldx = _rows2d(x2d, "x", act=True)
    if out2d is None:
        out2d = torch.empty((rows, cols), dtype=x2d.dtype, device=x2d.device)
    r2, c2, ldy = _rows2d(out2d, "out", act=True)
    _chk((r2, c2) == (rows, cols), "dropout: out shape")
    mask_out = None
    if mask_in is not None:
        _chk(mask_in.is_cuda and mask_in.dtype == torch.uint8 and mask_in.is_contiguous()
             and mask_in.numel() == rows * cols, "dropout: mask_in")
    elif want_mask:
        mask_out = torch.empty((rows, cols), dtype=torch.uint8, device=x2d.device)
    _call("pe_dropout_fwd", x2d.data_ptr(), ldx, out2d.data_ptr(), ldy, _lib.ptr(mask_in), _lib.ptr(mask_out), rows, cols,
          float(p), int(seed), int(offset), _s(), act16=_act16(x2d, out2d))
    return out2d, (mask_in if mask_in is not None else mask_out)


def nhwc_to_seq(x, Cc, coff=0, out=None):
    """x dense [B,T,2,Ctot] (channels [coff,coff+C)) -> seq [B,T,2C] with feature c*2+w."""
    x = _actd(x, "x")
    B, T, two, ld = x.shape
    _chk(two == 2 and coff + Cc <= ld, "nhwc_to_seq: shape")
    if out is None:
        out = torch.empty((B, T, 2 * Cc), dtype=torch.float32, device=x.device)
    _chk(_dense(out, "out").shape == (B, T, 2 * Cc), "nhwc_to_seq: out shape")       # the temporal heads read fp32
    _call("pe_nhwc_to_seq", x.data_ptr(), ld, coff, out.data_ptr(), B * T, Cc, _s(), act16=_act16(x))
    return out


def seq_to_nhwc(seq, out, Cc, coff=0, accumulate=False):
    seq = _dense(seq, "seq")
    out = _actd(out, "out")
    B, T, two, ld = out.shape
    _chk(two == 2 and coff + Cc <= ld and seq.shape == (B, T, 2 * Cc), "seq_to_nhwc: shape")
    _call("pe_seq_to_nhwc", seq.data_ptr(), out.data_ptr(), ld, coff, B * T, Cc, int(bool(accumulate)), _s(),
          act16=_act16(out))
    return out


def copy2d(src2d, dst2d, accumulate=False):
    r, c, lds = _rows2d(src2d, "src", act=True)
    r2, c2, ldd = _rows2d(dst2d, "dst", act=True)
    _chk((r, c) == (r2, c2), "copy2d: shape")
    _call("pe_copy2d", src2d.data_ptr(), lds, dst2d.data_ptr(), ldd, r, c, int(bool(accumulate)), _s(),
          act16=_act16(src2d, dst2d))
    return dst2d


# ------------------------------------------------------------------ LSTM
def _ptr_array(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def _int_array(vals):
    arr = (C.c_int * len(vals))()
    for i, v in enumerate(vals):
        arr[i] = int(v)
    return arr


_SYNC: dict = {}
USE_PERSISTENT_LSTM = True


def _lstm_sync(ncells, B, device):
    """Zero-initialised barrier words for the persistent LSTM kernels (word 0 = sticky error flag)."""
    lib = _lib.load()
    need = lib.pe_lstm_persistent_sync_bytes(4, max(B, 256)) // 4
    key = torch.device(device)
    buf = _SYNC.get(key)
    if buf is None or buf.numel() < need:
        buf = torch.zeros(need, dtype=torch.int32, device=key)
        _SYNC[key] = buf
    return buf


def persistent_lstm_error(device) -> bool:
    """True if a persistent-LSTM group barrier ever timed out on this device (results invalid)."""
    buf = _SYNC.get(torch.device(device))
    return bool(buf is not None and int(buf[0].item()) != 0)


def persistent_lstm_error_word(device):
    """The sticky barrier-timeout word as a 1-element device tensor (None before any persistent launch): a
    data-parallel trainer max-reduces it across ranks and reads it once (distributed.GradientAllReduce.any_rank_word)."""
    buf = _SYNC.get(torch.device(device))
    return None if buf is None else buf[0:1]


def clear_persistent_lstm_error(device) -> None:
    """Reset the sticky barrier-timeout word (the persistent kernels skip their waits while it is set)."""
    buf = _SYNC.get(torch.device(device))
    if buf is not None:
        buf[0:1].zero_()


def _persistent_ok(ncells, B, H, device, which="fwd"):
    """The persistent recurrence kernels serve this configuration: a persistent product form selected (x3 / bf16 /
    f16, see ``products_for``) and the shape / device admitted by the library."""
    if products_for("lstm_" + which) == _lib.PE_PROD_NATIVE:
        return False
    with torch.cuda.device(device):
        return bool(_lib.load().pe_lstm_persistent_supported(ncells, B, H))


def lstm_fwd(whh, gates, y_slices, cbuf, reverse, B, T, H):
    """Advance len(whh) cells through all T steps.  y_slices[i] is a view [B,T,H] into a dense
    [B,T,ldy] output (ldy = 2H for bidirectional)."""
    n = len(whh)
    _chk(1 <= n <= 4 and len(gates) == len(y_slices) == len(cbuf) == len(reverse) == n, "lstm_fwd: cell lists")
    ldy = None
    for i in range(n):
        _chk(_dense(whh[i], "whh").shape == (4 * H, H), "whh shape")
        _chk(_dense(gates[i], "gates").shape == (B, T, 4 * H), "gates shape")
        _chk(_dense(cbuf[i], "cbuf").shape == (B, T, H), "cbuf shape")
        ys = _f32c(y_slices[i], "y")
        _chk(ys.shape == (B, T, H) and ys.stride(2) == 1 and ys.stride(0) == T * ys.stride(1), "y slice layout")
        _chk(ldy in (None, ys.stride(1)), "all y slices share ldy")
        ldy = ys.stride(1)
    dev = gates[0].device
    if _persistent_ok(n, B, H, dev, "fwd"):
        sync = _lstm_sync(n, B, dev)
        _call("pe_lstm_fwd_persistent", n, _ptr_array(whh), _ptr_array(gates), _ptr_array(y_slices), _ptr_array(cbuf),
              _int_array(reverse), ldy, B, T, H, sync.data_ptr(), _s(), products=products_for("lstm_fwd"),
              work=2.0 * n * B * (T - 1) * 4 * H * H)
        return
    _call("pe_lstm_fwd", n, _ptr_array(whh), _ptr_array(gates), _ptr_array(y_slices), _ptr_array(cbuf),
          _int_array(reverse), ldy, B, T, H, _s(), work=2.0 * n * B * (T - 1) * 4 * H * H)


def lstm_bwd(whh_t, gates, cbuf, dy_slices, dcarry, reverse, B, T, H, dbias_rows=None, amax_out=None):
    """Backward recurrences of len(whh_t) cells; gates become d(pre-activation gates) in place.  dbias_rows: optional
    list of [lstm_bwd_dbias_rows(...)][4H] buffers, one per cell, that receive the per-batch-tile column sums of the
    gate gradients (only pass it when that query is non-zero); returns True if they were written.  amax_out: optional
    list of zeroed words, one per cell, filled with the gate gradients' absmax under the same condition (else
    untouched); or True (see ``Scaled``): then returns (bias rows written, the gate gradients as ``Scaled``: with the
    words the kernel filled, else without one)."""
    n = len(whh_t)
    _chk(1 <= n <= 4 and len(gates) == len(dy_slices) == len(cbuf) == len(reverse) == len(dcarry) == n,
         "lstm_bwd: cell lists")
    ld = None
    for i in range(n):
        _chk(_dense(whh_t[i], "whh_t").shape == (H, 4 * H), "whh_t shape")
        _chk(_dense(gates[i], "gates").shape == (B, T, 4 * H), "gates shape")
        _chk(_dense(cbuf[i], "cbuf").shape == (B, T, H), "cbuf shape")
        _chk(_dense(dcarry[i], "dcarry").shape == (B, H), "dcarry shape")
        d = _f32c(dy_slices[i], "dy")
        _chk(d.shape == (B, T, H) and d.stride(2) == 1 and d.stride(0) == T * d.stride(1), "dy slice layout")
        _chk(ld in (None, d.stride(1)), "all dy slices share ld")
        ld = d.stride(1)
    dev = gates[0].device
    if _persistent_ok(n, B, H, dev, "bwd"):
        sync = _lstm_sync(n, B, dev)
        rows = lstm_bwd_dbias_rows(n, B, T, H, ld, dev) if dbias_rows is not None else 0
        if rows:
            _chk(len(dbias_rows) == n and all(_dense(d, "dbias_rows").shape == (rows, 4 * H) for d in dbias_rows),
                 "lstm_bwd: dbias_rows shape")
        words = [None] * n
        if rows and amax_out is not None:
            words = [amax_word() for _ in gates] if amax_out is True else list(amax_out)
        _call("pe_lstm_bwd_persistent", n, _ptr_array(whh_t), _ptr_array(gates), _ptr_array(cbuf),
              _ptr_array(dy_slices), _int_array(reverse), ld, B, T, H, _ptr_array(dbias_rows) if rows else None,
              _ptr_array(words) if words[0] is not None else None,
              sync.data_ptr(), _s(), products=products_for("lstm_bwd"), work=2.0 * n * B * (T - 1) * 4 * H * H)
        return (bool(rows), [Scaled(g, w) for g, w in zip(gates, words)]) if amax_out is True else bool(rows)
    _call("pe_lstm_bwd", n, _ptr_array(whh_t), _ptr_array(gates), _ptr_array(cbuf), _ptr_array(dy_slices),
          _ptr_array(dcarry), _int_array(reverse), ld, B, T, H, _s(), work=2.0 * n * B * (T - 1) * 4 * H * H)
    return (False, [Scaled(g) for g in gates]) if amax_out is True else False


def lstm_bwd_dbias_rows(n, B, T, H, ld, device) -> int:
    """Rows of the per-cell [rows][4H] bias-gradient partials lstm_bwd can emit for this configuration (0: it cannot;
    sum the gate gradients with colsum instead)."""
    if not _persistent_ok(n, B, H, device, "bwd"):
        return 0
    return int(_lib.load().pe_lstm_bwd_persistent_dbias_rows(n, B, T, H, ld))


def lstm_whh_grad(dgates, y_slice, dwhh, reverse, B, T, H):
    """dgates, y_slice: plain tensors or ``Scaled``."""
    (dgates, amax_dg), (y_slice, amax_y) = _tw(dgates), _tw(y_slice)
    _chk(_dense(dgates, "dgates").shape == (B, T, 4 * H), "dgates shape")
    ys = _f32c(y_slice, "y")
    _chk(ys.shape == (B, T, H) and ys.stride(2) == 1 and ys.stride(0) == T * ys.stride(1), "y slice layout")
    _chk(_dense(dwhh, "dwhh").shape == (4 * H, H), "dwhh shape")
    lib = _lib.load()
    ws = workspace(lib.pe_lstm_whh_grad_workspace_bytes(B, T, H), dgates.device)
    p = products_for()
    if p == _lib.PE_PROD_H2:
        if amax_y is None:                 # |h| < 1 by construction (o * tanh(c)): a constant bound is a valid amax
            amax_y = _unit_amax(dgates.device)
        amax_dg = absmax(dgates) if amax_dg is None else amax_dg
    _call("pe_lstm_whh_grad", dgates.data_ptr(), ys.data_ptr(), ys.stride(1), dwhh.data_ptr(), B, T, H,
          int(bool(reverse)), ws.data_ptr(), ws.numel(), _lib.ptr(amax_dg), _lib.ptr(amax_y), _s(), products=p,
          work=2.0 * B * T * 4 * H * H)
    return dwhh


def colsum(x2d, out0, out1=None):
    rows, cols, ld = _rows2d(x2d, "x")
    _chk(_dense(out0, "out0").numel() == cols, "colsum: out size")
    if out1 is not None:
        _chk(_dense(out1, "out1").numel() == cols, "colsum: out1 size")
    lib = _lib.load()
    ws = workspace(lib.pe_colsum_workspace_bytes(cols), x2d.device)
    _call("pe_colsum", x2d.data_ptr(), rows, cols, ld, out0.data_ptr(), _lib.ptr(out1), ws.data_ptr(), ws.numel(),
          _s())
    return out0


# ------------------------------------------------------------------ heads / loss / optimiser
def head_fwd(x2d, w, bias, out=None):
    R, D, ldx = _rows2d(x2d, "x")
    w = _dense(w, "w")
    bias = _dense(bias, "bias")
    n_out = w.shape[0]
    _chk(w.shape == (n_out, D) and bias.numel() == n_out, "head_fwd: weight shape")
    if out is None:
        out = torch.empty((R,), dtype=torch.float32, device=x2d.device)
    _chk(_dense(out, "out").numel() == R, "head_fwd: out size")
    _call("pe_head_fwd", x2d.data_ptr(), ldx, w.data_ptr(), bias.data_ptr(), n_out, out.data_ptr(), R, D, _s())
    return out


def head_bwd(x2d, w, dy, dw, db, dx=None):
    R, D, ldx = _rows2d(x2d, "x")
    n_out = w.shape[0]
    _chk(_dense(dy, "dy").numel() == R, "head_bwd: dy size")
    if dw is not None or db is not None:       # (both None: data gradient only)
        _chk(_dense(dw, "dw").shape == (n_out, D) and _dense(db, "db").numel() == n_out, "head_bwd: grads shape")
    if dx is None:
        dx = torch.empty((R, D), dtype=torch.float32, device=x2d.device)
    R2, D2, lddx = _rows2d(dx, "dx")
    _chk((R2, D2) == (R, D), "head_bwd: dx shape")
    lib = _lib.load()
    ws = workspace(lib.pe_head_bwd_workspace_bytes(D), x2d.device)
    _call("pe_head_bwd", x2d.data_ptr(), ldx, w.data_ptr(), dy.data_ptr(), n_out, dx.data_ptr(), lddx,
          _lib.ptr(dw), _lib.ptr(db), R, D, ws.data_ptr(), ws.numel(), _s())
    return dx


def f0_sil_loss(f0_pred, f0, sil_pred, sil, lambda_f0, grad_scale=1.0, want_grads=True):
    R = f0.numel()
    for t, n in ((f0_pred, "f0_pred"), (f0, "f0"), (sil_pred, "sil_pred"), (sil, "sil")):
        _chk(_dense(t, n).numel() == R, f"{n}: size")
    out3 = torch.empty((3,), dtype=torch.float32, device=f0.device)
    d_f0 = torch.empty((R,), dtype=torch.float32, device=f0.device) if want_grads else None
    d_sil = torch.empty((R,), dtype=torch.float32, device=f0.device) if want_grads else None
    _call("pe_f0_sil_loss", f0_pred.data_ptr(), f0.data_ptr(), sil_pred.data_ptr(), sil.data_ptr(),
          float(lambda_f0), R, float(grad_scale), out3.data_ptr(), _lib.ptr(d_f0), _lib.ptr(d_sil), _s())
    return out3, d_f0, d_sil


def f0_bins_ce_loss(logits, f0, sil_pred, sil, lambda_f0, grad_scale=1.0, want_grads=True):
    """360-bin (CREPE-style) F0 classification loss + silence BCE (build-defined).
    logits (R, C), f0 / sil_pred / sil (R,).  Returns (out4 = [total, lambda*CE, BCE, n_voiced], d_logits, d_sil)."""
    logits = _dense(logits, "logits")
    _chk(logits.dim() == 2, "logits: expected (R, C)")
    R, C = logits.shape
    for t, n in ((f0, "f0"), (sil_pred, "sil_pred"), (sil, "sil")):
        _chk(_dense(t, n).numel() == R, f"{n}: size")
    lib = _lib.load()
    out4 = torch.empty((4,), dtype=torch.float32, device=f0.device)
    d_logits = torch.empty((R, C), dtype=torch.float32, device=f0.device) if want_grads else None
    d_sil = torch.empty((R,), dtype=torch.float32, device=f0.device) if want_grads else None
    nbytes = lib.pe_f0_bins_ce_workspace_bytes(R)
    ws = workspace(nbytes, f0.device)
    _call("pe_f0_bins_ce_loss", logits.data_ptr(), C, C, f0.data_ptr(), sil_pred.data_ptr(), sil.data_ptr(),
          float(lambda_f0), R, float(grad_scale), out4.data_ptr(), _lib.ptr(d_logits), C, _lib.ptr(d_sil),
          ws.data_ptr(), ws.numel(), _s())
    return out4, d_logits, d_sil


F0_DECODERS = ("argmax", "weighted", "viterbi", "weighted_viterbi")


def decode_f0_bins(logits, lengths=None, method="argmax"):
    """Read a pitch out of F0 classifier logits (the inverse of ``f0_bins_ce_loss``; build-defined).
    logits (N, T, C) or (T, C) float32 with unit bin stride; ``lengths`` optional (N,) int32 device tensor with
    1 <= lengths[n] <= T (frames beyond it give 0).  ``method``: "argmax" (lowest index on ties), "weighted"
    (softmax-weighted cents over the +-4 bins around the arg max), "viterbi" (triangular 12-bin transition band,
    each sequence on its own), "weighted_viterbi" (the same local average around the Viterbi bin).
    Returns (f0_hz, confidence = softmax(frame)[bin], bins): (N, T) float32 / float32 / int32 device tensors."""
    _chk(method in F0_DECODERS, f"decode_f0_bins: method must be one of {F0_DECODERS}, got {method!r}")
    _f32c(logits, "logits")
    squeeze = logits.dim() == 2
    if squeeze:
        logits = logits.unsqueeze(0)
    _chk(logits.dim() == 3, "logits: expected (N, T, C) or (T, C)")
    N, T, C = logits.shape
    _chk(N > 0 and T > 0 and 2 <= C <= 1024, "logits: need N, T >= 1 and 2 <= C <= 1024")
    _chk(logits.stride(2) == 1, "logits: expected unit stride over the bins")
    ld_t = logits.stride(1) if T > 1 else max(C, logits.stride(1))
    ld_n = logits.stride(0) if N > 1 else max((T - 1) * ld_t + C, logits.stride(0))
    _chk(ld_t >= C and ld_n >= (T - 1) * ld_t + C, "logits: frames or sequences overlap in memory")
    if lengths is not None:
        _chk(lengths.is_cuda and lengths.dtype == torch.int32 and lengths.is_contiguous() and lengths.numel() == N,
             "lengths: expected a contiguous int32 device tensor of N entries")
    dev = logits.device
    bins = torch.empty((N, T), dtype=torch.int32, device=dev)
    f0 = torch.empty((N, T), dtype=torch.float32, device=dev)
    conf = torch.empty((N, T), dtype=torch.float32, device=dev)
    path = None
    if method in ("viterbi", "weighted_viterbi"):
        nbytes = _lib.load().pe_f0_viterbi_workspace_bytes(N, T, C)
        ws = workspace(nbytes, dev) if nbytes else None
        _call("pe_f0_viterbi", logits.data_ptr(), ld_t, ld_n, C, _lib.ptr(lengths), N, T, bins.data_ptr(),
              _lib.ptr(ws), ws.numel() if ws is not None else 0, _s())
        path = bins
    frame_method = _lib.PE_F0_WEIGHTED if method.startswith("weighted") else _lib.PE_F0_ARGMAX
    _call("pe_f0_decode_frames", logits.data_ptr(), ld_t, ld_n, C, _lib.ptr(lengths), _lib.ptr(path), N, T,
          frame_method, 0 if path is not None else bins.data_ptr(), f0.data_ptr(), conf.data_ptr(), _s())
    return (f0[0], conf[0], bins[0]) if squeeze else (f0, conf, bins)


def _host_table(t, fields_fn: str, name: str):
    """(rows, host array) of an int64 host table of ``fields_fn()`` columns."""
    import numpy as np
    _chk(isinstance(t, np.ndarray) and t.dtype == np.int64 and t.ndim == 2 and t.flags.c_contiguous
         and t.shape[1] == getattr(_lib.load(), fields_fn)(), f"{name}: expected a C-contiguous int64 host table")
    return int(t.shape[0]), t


def _device_table(t, host, name: str):
    _chk(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()
         and tuple(t.shape) == host.shape, f"{name}: expected the device copy of the host table")
    return t


def mel_forward_chunks(mel, wave, chunks, chunks_d, chunk_size, out=None, log=True):
    """Mel of chunk table entries in the model's input layout (``pe_mel_forward_chunks``): ``mel`` a
    ``MelSpectrogram``, ``wave`` float32 device audio (1-D packed or 2-D padded rows), ``chunks`` the (n, 3) int64 host
    table {sample offset of the row from ``wave``'s first element, samples of the row, first frame} and ``chunks_d``
    its device copy.  Returns ``out`` (n, 1, chunk_size, n_mels), frames past a row's end 0: the normalised log-mel
    with the kernel's own logarithm (what ``log_mel_ragged`` writes), or with ``log=False`` the mel power (what the
    transform itself returns)."""
    from .mel import LOG_EPS, MEL_MEAN, MEL_STD
    _f32c(wave, "wave")
    _chk(wave.dim() in (1, 2) and (wave.numel() == 0 or wave.stride(-1) == 1),
         "wave: expected 1-D or 2-D rows of unit stride")
    n, chunks = _host_table(chunks, "pe_mel_chunk_fields", "chunks")
    _device_table(chunks_d, chunks, "chunks_d")
    chunk_size = int(chunk_size)
    _chk(chunk_size >= 1, "chunk_size must be positive")
    if wave.dim() == 1 or wave.shape[0] == 0:
        elems = wave.numel()
    else:
        elems = (wave.shape[0] - 1) * wave.stride(0) + wave.shape[1]
    if out is None:
        out = torch.empty((n, 1, chunk_size, mel.n_mels), dtype=torch.float32, device=wave.device)
    _chk(_dense(out, "out").shape == (n, 1, chunk_size, mel.n_mels), "mel_forward_chunks: out shape")
    if n == 0:
        return out
    with torch.cuda.device(wave.device):
        _call("pe_mel_forward_chunks", mel._get_plan(wave.device), wave.data_ptr(), elems, chunks_d.data_ptr(),
              chunks.ctypes.data, n, chunk_size, out.data_ptr(), out.stride(0), out.stride(3), out.stride(2),
              int(bool(log)), LOG_EPS, MEL_MEAN, MEL_STD, 0.0, _s(), work=float(n * chunk_size * 4 * (mel.hop_length + mel.n_mels)))
    return out


def mel_backward(mel, wave, grad_out, *, lengths=None, frame_start=None, log=True, frames_last=True):
    """Gradient of the mel front end with respect to the waveform (``pe_mel_backward`` / ``pe_mel_backward_ragged``):
    ``mel`` a ``MelSpectrogram``, ``wave`` the (B, N) float32 device audio the forward saw, ``grad_out`` d loss / d out
    of ``mel(wave)`` (``log=False``: (B, n_mels, T)) or of ``log_mel_batch`` / ``log_mel_ragged`` (``log=True``:
    (B, 1, n_mels, T)); with ``frames_last=False`` the last two axes are (T, n_mels), the model's input layout.  It is
    read at its own strides, so a transposed view costs no copy.  ``lengths`` / ``frame_start``: the int32 device
    tensors of ``log_mel_ragged``.  Positions the forward padded are never read.  Returns (B, N) float32, every element
    written by the kernels; the spectrum is recomputed from ``wave``, nothing of the forward is needed."""
    from .mel import LOG_EPS, MEL_MEAN, MEL_STD
    _f32c(wave, "wave")
    _f32c(grad_out, "grad_out")
    _chk(wave.dim() == 2 and (wave.shape[1] <= 1 or wave.stride(1) == 1), "wave: expected (B, N) rows of unit stride")
    B, N = wave.shape
    g = grad_out
    if g.dim() == 4:
        _chk(g.shape[1] == 1, "grad_out: expected (B, 1, n_mels, T) or (B, 1, T, n_mels)")
        g = g[:, 0]
    _chk(g.dim() == 3 and g.shape[0] == B and g.shape[1 if frames_last else 2] == mel.n_mels
         and g.device == wave.device, "grad_out: expected one (n_mels, T) or (T, n_mels) map per wave row")
    T = g.shape[2 if frames_last else 1]
    g_sm, g_st = (g.stride(1), g.stride(2)) if frames_last else (g.stride(2), g.stride(1))
    ragged = lengths is not None
    _chk(ragged or frame_start is None, "frame_start needs lengths")
    for t, nme in ((lengths, "lengths"), (frame_start, "frame_start")):
        _chk(t is None or (t.is_cuda and t.dtype == torch.int32 and t.numel() == B and t.is_contiguous()),
             f"{nme}: expected a contiguous int32 device tensor of size B")
    _chk(ragged or N > mel.n_fft // 2, "wave: reflect padding needs more than n_fft / 2 samples")
    grad_wave = torch.empty((B, N), dtype=torch.float32, device=wave.device)
    if B == 0 or N == 0 or T == 0:
        return grad_wave.zero_()
    ld = wave.stride(0) if B > 1 else max(N, wave.stride(0))
    plan = mel._get_plan(wave.device)
    need = _lib.load().pe_mel_backward_workspace_bytes(plan, B, N, T)
    ws = workspace(need, wave.device)
    frames = B * T if ragged else B * min(mel.num_frames(N), T)
    # algorithmic bytes per valid frame: hop samples read, hop written, n_mels floats of grad_out read
    work = float(frames * 4 * (2 * mel.hop_length + mel.n_mels))
    tail = (g.data_ptr(), g.stride(0), g_sm, g_st, T, int(bool(log)), LOG_EPS, MEL_MEAN, MEL_STD, grad_wave.data_ptr(),
            grad_wave.stride(0), ws.data_ptr(), ws.numel(), _s())
    with torch.cuda.device(wave.device):
        if ragged:
            _call("pe_mel_backward_ragged", plan, wave.data_ptr(), B, N, ld, lengths.data_ptr(), _lib.ptr(frame_start),
                  *tail, work=work)
        else:
            _call("pe_mel_backward", plan, wave.data_ptr(), B, N, ld, *tail, work=work)
    return grad_wave


def _grad_rows(grad_out, who: str) -> torch.Tensor:
    """``grad_out`` as (B, W) float32 device rows of unit element stride that do not overlap (what autograd hands over
    may be an expanded scalar); a host tensor is refused."""
    if not isinstance(grad_out, torch.Tensor) or not grad_out.is_cuda or grad_out.dtype != torch.float32:
        raise RuntimeError(f"{who} (HIP) needs a float32 device grad_out; no CPU fallback exists")
    _chk(grad_out.dim() == 2, f"{who}: grad_out: expected (B, n_out) rows")
    B, W = grad_out.shape
    if (W > 1 and grad_out.stride(1) != 1) or (B > 1 and grad_out.stride(0) < W):
        grad_out = grad_out.contiguous()
    return grad_out


def resample_backward(resampler, grad_out, n_in):
    """Gradient of ``Resampler`` with respect to its input (``pe_resample_backward``): ``grad_out`` (B, n_out) float32
    device rows, d loss / d y of ``resampler(x)`` for x of (B, n_in), read at its own row stride; ``n_out`` may stay
    below ``resampler.out_len(n_in)`` (the missing outputs carry no gradient).  Returns (B, n_in) float32, every
    element written by the kernel: the exact transpose of the forward over the same float32 taps, each sample one
    ``fmaf`` chain in ascending output index.  Nothing of the forward is needed; the operator is linear."""
    g = _grad_rows(grad_out, "resample_backward")
    n_in = int(n_in)
    B, n_out = g.shape
    _chk(n_in >= 0 and n_out <= resampler.out_len(n_in), "resample_backward: grad_out is longer than the output of "
         "n_in samples")
    if resampler.orig_freq == resampler.new_freq:
        return g
    dx = torch.empty((B, n_in), dtype=torch.float32, device=g.device)
    if B == 0 or n_in == 0:
        return dx
    ld = g.stride(0) if B > 1 else max(n_out, g.stride(0))
    with torch.cuda.device(g.device):
        # algorithmic bytes: grad_out read once, the gradient written once
        _call("pe_resample_backward", resampler._get_plan(g.device), g.data_ptr(), B, n_out, ld, dx.data_ptr(),
              dx.stride(0), n_in, _s(), work=float(4 * B * (n_out + n_in)))
    return dx


def resample_ragged_backward(resampler, grad_out, rates, lengths, *, packed: bool, width: int | None = None,
                             out=None):
    """Gradient of ``RaggedResampler`` with respect to its input in ONE launch (``pe_resample_ragged_backward``):
    ``grad_out`` (B, W) float32 device rows, d loss / d y of ``resampler(x, rates, lengths)``; row r is read up to its
    own output length and never past it.  ``rates``, ``lengths``: the host sequences of the forward.  Returns the
    gradient in the layout the forward read: ``packed=True`` a flat tensor of the rows back to back (``width``: its
    size, default ``sum(lengths)``; the slack is zero), ``packed=False`` (B, ``width``) padded rows (default
    ``max(lengths)``), zero past each row's length; ``out``: a contiguous tensor of that layout to write instead (its
    last dimension is the width; every element of it is written).  Row r equals ``resample_backward`` on that row alone bit for bit;
    a row at the target rate is a copy."""
    g = _grad_rows(grad_out, "resample_ragged_backward")
    rates, lengths = [int(r) for r in rates], [int(n) for n in lengths]
    B = g.shape[0]
    _chk(len(rates) == B and len(lengths) == B, "resample_ragged_backward: one rate and one length per grad_out row")
    _chk(all(n >= 0 for n in lengths), "resample_ragged_backward: a row length is negative")
    _chk(all(resampler.out_len(r, n) <= g.shape[1] for r, n in zip(rates, lengths)),
         "resample_ragged_backward: grad_out is narrower than a row's output")
    total = sum(lengths) if packed else max(lengths, default=0)
    if out is not None:
        _chk(_dense(out, "out").device == g.device and (out.dim() == 1 if packed else out.dim() == 2 and
                                                        out.shape[0] == B),
             "resample_ragged_backward: out: expected a flat tensor for packed rows, (B, width) for padded rows")
        width = out.shape[-1]
    width = total if width is None else int(width)
    _chk(width >= total, "resample_ragged_backward: width is below the rows' extent")
    if packed:
        dx = torch.empty((width,), dtype=torch.float32, device=g.device) if out is None else out
        if width > total:
            dx[total:].zero_()
        offsets, acc = [], 0
        for n in lengths:
            offsets.append(acc)
            acc += n
    else:
        dx = torch.empty((B, width), dtype=torch.float32, device=g.device) if out is None else out
        offsets = [r * width for r in range(B)]
    if total == 0:                                          # no row has a sample: nothing to launch
        return dx.zero_()
    distinct = tuple(sorted(set(rates)))
    index = {r: k for k, r in enumerate(distinct)}
    host32 = torch.tensor(lengths + [index[r] for r in rates], dtype=torch.int32).pin_memory()
    host64 = torch.tensor(offsets, dtype=torch.int64).pin_memory()
    dev32 = host32.to(g.device, non_blocking=True)
    dev64 = host64.to(g.device, non_blocking=True)
    ld = g.stride(0) if B > 1 else max(g.shape[1], g.stride(0))
    with torch.cuda.device(g.device):
        _call("pe_resample_ragged_backward", resampler._get_plan(distinct, g.device), g.data_ptr(), ld,
              dev64.data_ptr(), dev32.data_ptr(), dev32[B:].data_ptr(), host32[:B].data_ptr(), host32[B:].data_ptr(), B,
              dx.data_ptr(), 0 if packed else width, _s(),
              work=float(4 * (sum(lengths) + sum(resampler.out_len(r, n) for r, n in zip(rates, lengths)))))
    return dx


def stitch_chunks(x, runs, runs_d, out, det=None, det_out=None):
    """Chunk outputs to stitched rows by a run table (``pe_stitch_chunks``, ``inference.chunk_plan``): ``x``
    (n_chunks, chunk_size, C) or (n_chunks, chunk_size) float32 with unit stride over C and evenly spaced frames,
    ``out`` (n_dst, C) or (n_dst,) with unit stride over C, ``runs`` the (n_runs, 8) int64 host table and ``runs_d``
    its device copy; ``det`` (n_chunks, chunk_size) and ``det_out`` (n_dst,), both dense, go together.  Every element
    of ``out`` is written: a copy, a blend, or 0 where no run lands.  One launch."""
    _f32c(x, "x")
    _f32c(out, "out")
    _chk(x.dim() in (2, 3) and out.dim() == x.dim() - 1,
         "stitch_chunks: x (n, T, C) with out (n_dst, C), or (n, T) with (n_dst,)")
    if x.dim() == 2:
        x, out = x.unsqueeze(-1), out.unsqueeze(-1)
    n_chunks, T, C = x.shape
    n_dst = out.shape[0]
    _chk(out.shape[1] == C, "stitch_chunks: x and out differ in columns")
    _chk(1 <= C <= 1024, "stitch_chunks: need 1 <= C <= 1024")
    _chk(C == 1 or (x.stride(2) == 1 and out.stride(1) == 1), "stitch_chunks: expected unit stride over the columns")
    ld_x = x.stride(1) if T > 1 else max(C, x.stride(1))
    ld_out = out.stride(0) if n_dst > 1 else max(C, out.stride(0))
    _chk(ld_x >= C and ld_out >= C and (n_chunks <= 1 or x.stride(0) == T * ld_x),
         "stitch_chunks: frames overlap in memory or chunks are not evenly spaced")
    n_runs, runs = _host_table(runs, "pe_stitch_run_fields", "runs")
    _device_table(runs_d, runs, "runs_d")
    _chk((det is None) == (det_out is None), "stitch_chunks: det and det_out go together")
    if det is not None:
        _chk(_dense(det, "det").shape == (n_chunks, T), "det: expected (n_chunks, chunk_size)")
        _chk(_dense(det_out, "det_out").shape == (n_dst,), "det_out: expected (n_dst,)")
    if n_dst == 0:
        return out
    with torch.cuda.device(x.device):
        _call("pe_stitch_chunks", x.data_ptr(), ld_x, _lib.ptr(det), runs_d.data_ptr(), runs.ctypes.data, n_runs,
              n_chunks, T, C, out.data_ptr(), ld_out, _lib.ptr(det_out), n_dst, _s(),
              work=float(2 * 4 * n_dst * (C + (det is not None))))
    return out


def pitch_metrics(f0_pred, f0_ref, threshold_cents=50.0):
    """float64 device tensor [rms_cents, rpa, rca, vuv_error, n_voiced, n_frames] of a predicted F0 track against a
    reference, both (n,) float32 device tensors of one length (see ``inference.pitch_metrics``)."""
    n = _dense(f0_pred, "f0_pred").numel()
    _chk(n > 0 and _dense(f0_ref, "f0_ref").numel() == n, "pitch_metrics: need two tracks of one non-zero length")
    _chk(threshold_cents >= 0, "pitch_metrics: threshold_cents must not be negative")
    out = torch.empty((6,), dtype=torch.float64, device=f0_pred.device)
    _call("pe_pitch_metrics", f0_pred.data_ptr(), f0_ref.data_ptr(), n, float(threshold_cents), out.data_ptr(), _s())
    return out


def nonfinite_flag(x, flag=None):
    """int32 device scalar: 1 if any element of the flat float32 tensor ``x`` is inf / nan (GradScaler's test)."""
    x = _dense(x, "x")
    if flag is None:
        flag = torch.empty((1,), dtype=torch.int32, device=x.device)
    _chk(flag.is_cuda and flag.dtype == torch.int32 and flag.numel() == 1, "flag: int32 device scalar")
    if x.numel() == 0:                          # nothing to test (and no pointer to pass): the word is cleared
        return flag.zero_()
    _call("pe_nonfinite_flag", x.data_ptr(), x.numel(), flag.data_ptr(), _s())
    return flag


def adamw_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0,
               skip_flag=None):
    """``skip_flag``: optional 1-element float32 device tensor; non-zero at execution time = update nothing."""
    n = param.numel()
    for t, nme in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(_dense(t, nme).numel() == n, f"{nme}: size")
    _chk(int(step) >= 1, "adamw_step: steps count from 1 (step 0 has no bias correction: the step size is infinite)")
    bc1 = 1.0 - float(beta1) ** int(step)
    bc2 = 1.0 - float(beta2) ** int(step)
    _call("pe_adamw_step", param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), n,
          float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), bc1, bc2, float(grad_scale),
          _lib.ptr(skip_flag), _s())


# ------------------------------------------------------------------ transformer pieces
def bgemm(mode, A, a_view, B, b_view, C, c_view, inner, batch, M, N, K, alpha=1.0, accumulate=False):
    """Batched 64x64-tiled GEMM.  ``*_view`` = (ld, outer_stride, inner_stride) in elements; matrix b
    of an operand starts at element (b // inner) * outer + (b % inner) * inner_stride of its tensor
    (tensors may be views: the data pointer carries any extra offset)."""
    for t, n in ((A, "A"), (B, "B"), (C, "C")):
        _f32c(t, n)

    def _extent(view, rows, cols):
        ld, so, si = view
        return ((batch - 1) // inner) * so + ((batch - 1) % inner if batch > 0 else 0) * si + (rows - 1) * ld + cols

    a_rows, a_cols = (M, K) if mode != 2 else (K, M)
    b_rows, b_cols = (N, K) if mode == 0 else (K, N)
    for t, view, r, c, n in ((A, a_view, a_rows, a_cols, "A"), (B, b_view, b_rows, b_cols, "B"),
                             (C, c_view, M, N, "C")):
        avail = t.untyped_storage().nbytes() // 4 - t.storage_offset()
        _chk(_extent(view, r, c) <= avail, f"bgemm: operand {n} exceeds its storage")
    _call("pe_bgemm", int(mode), A.data_ptr(), *map(int, a_view), B.data_ptr(), *map(int, b_view), C.data_ptr(),
          *map(int, c_view), int(inner), int(batch), int(M), int(N), int(K), float(alpha), int(bool(accumulate)),
          _s(), work=2.0 * batch * M * N * K)
    return C


FUSED_ATTENTION = os.environ.get("PE_FUSED_ATTENTION", "1") == "1"


def attn_supported(T, dh):
    return bool(FUSED_ATTENTION and _lib.load().pe_attn_supported(int(T), int(dh)))


def attn_fwd(qkv, B, T, H, scale, p=0.0, mask_in=None, seed=0, offset=0):
    """Fused softmax(Q K^T * scale) -> dropout(p) -> . V for packed projections qkv [B*T, 3*H*dh].
    Returns (o [B*T, H*dh], lse [B*H*T], keep mask uint8 [B*H*T, T] or None)."""
    qkv = _dense(qkv, "qkv")
    R, D3 = qkv.shape
    D = D3 // 3
    dh = D // H
    _chk(R == B * T and D3 == 3 * H * dh, "attn_fwd: qkv shape")
    o = torch.empty((R, D), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((B * H * T,), dtype=torch.float32, device=qkv.device)
    mask_out = None
    if p > 0.0:
        if mask_in is not None:
            _chk(mask_in.is_cuda and mask_in.dtype == torch.uint8 and mask_in.is_contiguous()
                 and mask_in.numel() == B * H * T * T, "attn_fwd: mask_in")
        else:
            mask_out = torch.empty((B * H * T, T), dtype=torch.uint8, device=qkv.device)
    _call("pe_attn_fwd", qkv.data_ptr(), D3, o.data_ptr(), D, lse.data_ptr(), _lib.ptr(mask_in if p > 0.0 else None),
          _lib.ptr(mask_out), B, T, H, dh, float(scale), float(p), int(seed), int(offset), _s(),
          products=products_for("attn"), work=4.0 * B * H * T * T * dh)
    return o, lse, (mask_in if (p > 0.0 and mask_in is not None) else mask_out)


def attn_bwd(qkv, o, d_o, lse, mask, B, T, H, scale, p=0.0):
    """Gradient of attn_fwd wrt the packed projections: dqkv [B*T, 3*H*dh]."""
    qkv, o, d_o, lse = _dense(qkv, "qkv"), _dense(o, "o"), _dense(d_o, "d_o"), _dense(lse, "lse")
    R, D3 = qkv.shape
    D = D3 // 3
    dh = D // H
    _chk(o.shape == (R, D) and d_o.shape == (R, D) and lse.numel() == B * H * T, "attn_bwd: shapes")
    if p > 0.0:
        _chk(mask is not None and mask.is_cuda and mask.dtype == torch.uint8 and mask.numel() == B * H * T * T,
             "attn_bwd: mask")
    dqkv = torch.empty_like(qkv)
    _call("pe_attn_bwd", qkv.data_ptr(), D3, o.data_ptr(), d_o.data_ptr(), D, lse.data_ptr(),
          _lib.ptr(mask if p > 0.0 else None), dqkv.data_ptr(), B, T, H, dh, float(scale), float(p), _s(),
          products=products_for("attn"), work=10.0 * B * H * T * T * dh)
    return dqkv


def softmax_fwd_(s2d, scale):
    rows, L, ld = _rows2d(s2d, "scores")
    _chk(ld == L, "softmax: dense rows")
    _call("pe_softmax_fwd", s2d.data_ptr(), rows, L, float(scale), _s())
    return s2d


def softmax_bwd_(p2d, dp2d, scale):
    rows, L, ld = _rows2d(p2d, "p")
    r2, L2, ld2 = _rows2d(dp2d, "dp")
    _chk((rows, L, ld) == (r2, L2, ld2) and ld == L, "softmax_bwd: shapes")
    _call("pe_softmax_bwd", p2d.data_ptr(), dp2d.data_ptr(), rows, L, float(scale), _s())
    return dp2d


class LnState:
    def __init__(self, z, mean, rstd):
        self.z, self.mean, self.rstd = z, mean, rstd


def layernorm_fwd(a2d, gamma, beta, b2d=None, pe=None, eps=1e-5, keep_z=True):
    """y = LN(a + b + pe[row % period]); returns (y, LnState).  ``pe`` is [period, D] contiguous."""
    a2d = _dense(a2d, "a")
    R, D = a2d.shape
    if b2d is not None:
        _chk(_dense(b2d, "b").shape == (R, D), "layernorm: b shape")
    period = 0
    if pe is not None:
        _chk(_dense(pe, "pe").dim() == 2 and pe.shape[1] == D, "layernorm: pe shape")
        period = pe.shape[0]
    _chk(_dense(gamma, "gamma").numel() == D and _dense(beta, "beta").numel() == D, "layernorm: affine size")
    need_z = keep_z and (b2d is not None or pe is not None)
    z = torch.empty_like(a2d) if need_z else None
    y = torch.empty_like(a2d)
    mean = torch.empty((R,), dtype=torch.float32, device=a2d.device)
    rstd = torch.empty((R,), dtype=torch.float32, device=a2d.device)
    _call("pe_layernorm_fwd", a2d.data_ptr(), _lib.ptr(b2d), _lib.ptr(pe), period, gamma.data_ptr(), beta.data_ptr(),
          float(eps), _lib.ptr(z), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), R, D, _s())
    return y, LnState(z if need_z else (a2d if keep_z else None), mean, rstd)


def layernorm_bwd(dy2d, st: LnState, gamma, dgamma, dbeta, dz=None, dy_add=None, drop_mask=None, p=0.0):
    """dz = dLN(dy [+ dy_add]).  With ``drop_mask`` (uint8 [R, D], rate ``p``) returns (dz, dropout_bwd(dz)) from the
    same pass."""
    dy2d = _dense(dy2d, "dy")
    R, D = dy2d.shape
    _chk(_dense(st.z, "z").shape == (R, D), "layernorm_bwd: z shape")
    if dz is None:
        dz = torch.empty_like(dy2d)
    _chk(_dense(dz, "dz").shape == (R, D), "layernorm_bwd: dz shape")
    if dgamma is not None or dbeta is not None:    # (both None: data gradient only, the sums are not reduced)
        _chk(_dense(dgamma, "dgamma").numel() == D and _dense(dbeta, "dbeta").numel() == D, "layernorm_bwd: grads")
    lib = _lib.load()
    ws = workspace(lib.pe_layernorm_bwd_workspace_bytes(D), dy2d.device)
    if dy_add is None and drop_mask is None:
        _call("pe_layernorm_bwd", dy2d.data_ptr(), st.z.data_ptr(), st.mean.data_ptr(), st.rstd.data_ptr(),
              gamma.data_ptr(), dz.data_ptr(), _lib.ptr(dgamma), _lib.ptr(dbeta), R, D, ws.data_ptr(), ws.numel(),
              _s())
        return dz
    if dy_add is not None:
        _chk(_dense(dy_add, "dy_add").shape == (R, D), "layernorm_bwd: dy_add shape")
    dz_drop = None
    if drop_mask is not None:
        _chk(drop_mask.is_cuda and drop_mask.dtype == torch.uint8 and drop_mask.is_contiguous()
             and drop_mask.numel() == R * D, "layernorm_bwd: drop_mask")
        dz_drop = torch.empty_like(dy2d)
    _call("pe_layernorm_bwd_fused", dy2d.data_ptr(), _lib.ptr(dy_add), st.z.data_ptr(), st.mean.data_ptr(),
          st.rstd.data_ptr(), gamma.data_ptr(), dz.data_ptr(), _lib.ptr(drop_mask), float(p), _lib.ptr(dz_drop),
          _lib.ptr(dgamma), _lib.ptr(dbeta), R, D, ws.data_ptr(), ws.numel(), _s())
    return dz if drop_mask is None else (dz, dz_drop)


def layernorm_dropout_fwd(a2d, b2d, gamma, beta, p, mask_in=None, seed=0, offset=0, eps=1e-5):
    """y = LN(a + dropout(b)); returns (y, LnState, mask uint8 [R, D]).  Same masks and values as ``dropout`` followed
    by ``layernorm_fwd(a, b2d=...)``."""
    a2d, b2d = _dense(a2d, "a"), _dense(b2d, "b")
    R, D = a2d.shape
    _chk(b2d.shape == (R, D), "layernorm_dropout: b shape")
    _chk(_dense(gamma, "gamma").numel() == D and _dense(beta, "beta").numel() == D, "layernorm_dropout: affine size")
    mask_out = None
    if mask_in is not None:
        _chk(mask_in.is_cuda and mask_in.dtype == torch.uint8 and mask_in.is_contiguous()
             and mask_in.numel() == R * D, "layernorm_dropout: mask_in")
    else:
        mask_out = torch.empty((R, D), dtype=torch.uint8, device=a2d.device)
    z = torch.empty_like(a2d)
    y = torch.empty_like(a2d)
    mean = torch.empty((R,), dtype=torch.float32, device=a2d.device)
    rstd = torch.empty((R,), dtype=torch.float32, device=a2d.device)
    _call("pe_layernorm_dropout_fwd", a2d.data_ptr(), b2d.data_ptr(), None, 0, gamma.data_ptr(), beta.data_ptr(),
          float(eps), z.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), R, D, _lib.ptr(mask_in),
          _lib.ptr(mask_out), float(p), int(seed), int(offset), _s())
    return y, LnState(z, mean, rstd), (mask_in if mask_in is not None else mask_out)


def gelu_dropout_fwd(x, p, mask_in=None, seed=0, offset=0):
    """dropout(gelu(x)) in one pass; returns (out, mask uint8 of x's shape)."""
    x = _dense(x, "x")
    out = torch.empty_like(x)
    mask_out = None
    if mask_in is not None:
        _chk(mask_in.is_cuda and mask_in.dtype == torch.uint8 and mask_in.is_contiguous()
             and mask_in.numel() == x.numel(), "gelu_dropout: mask_in")
    else:
        mask_out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _call("pe_gelu_dropout_fwd", x.data_ptr(), out.data_ptr(), x.numel(), _lib.ptr(mask_in), _lib.ptr(mask_out),
          float(p), int(seed), int(offset), _s())
    return out, (mask_in if mask_in is not None else mask_out)


def gelu_dropout_bwd(x, dy, mask, p, out=None):
    x, dy = _dense(x, "x"), _dense(dy, "dy")
    _chk(x.numel() == dy.numel() == mask.numel() and mask.dtype == torch.uint8 and mask.is_contiguous(),
         "gelu_dropout_bwd: sizes")
    if out is None:
        out = torch.empty_like(x)
    _call("pe_gelu_dropout_bwd", x.data_ptr(), dy.data_ptr(), mask.data_ptr(), float(p), out.data_ptr(), x.numel(),
          _s())
    return out


def gelu_fwd(x, out=None):
    x = _dense(x, "x")
    if out is None:
        out = torch.empty_like(x)
    _chk(_dense(out, "out").numel() == x.numel(), "gelu: out size")
    _call("pe_gelu_fwd", x.data_ptr(), out.data_ptr(), x.numel(), _s())
    return out


def gelu_bwd(x, dy, out=None):
    x, dy = _dense(x, "x"), _dense(dy, "dy")
    _chk(x.numel() == dy.numel(), "gelu_bwd: sizes")
    if out is None:
        out = torch.empty_like(x)
    _call("pe_gelu_bwd", x.data_ptr(), dy.data_ptr(), out.data_ptr(), x.numel(), _s())
    return out
