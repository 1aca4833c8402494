"""Codec stress conditions of the reference's Utils/codec_and_bandwidth_torture.ipynb on the device
(``csrc/codec.hip``): a build-defined MDCT transform codec ("ptc") and G.711 mu-law at 8 kHz.  There is no CPU path.
``tests/codec_ref.py`` is the restatement that pins both; DESIGN.md section 28 is the specification.

The transform codec is what opus, mp3 and aac have in common and what hurts a pitch tracker: a block transform (MDCT,
sine window, 50 % overlap), a bandwidth that shrinks with the bitrate, band-wise scale factors with signal-dependent
steps and a rate loop that coarsens the quantiser until the frame fits its bit budget.  It writes no bitstream: a
frame's bits are those of a cost model (CBR per frame, no reservoir), so its kbps are NOT comparable kbps for kbps with
those of opus, mp3 or aac.

Every call takes a ragged batch the way the stress conditions do (``ragged.device_plan``): one 1-D wave, rows packed
back to back with ``lengths``, or a padded 2-D batch.  The result has the input's shape (dense; zero outside the rows);
a row of it is bit-identical alone, packed at any offset, padded or in any batch order, and the launch count does not
depend on the rows."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, ops, stress
from .ragged import (check_device_tensor, device_plan, fft_roots, host_ptrs, i64, plan_arrays, row_layout, workspace)

FRAMES = (256, 512, 1024)
STEP_TABLE = 448
G711_RATE = 8000
G711_KBPS = 64.0


# ------------------------------------------------------------------------------------------------------------ host side
def default_bandwidth(sr, bitrate_kbps) -> float:
    """``min(sr / 2, 4000 (bitrate_kbps / 16) ** 0.75)`` Hz, in float64."""
    return min(float(sr) / 2.0, 4000.0 * (float(bitrate_kbps) / 16.0) ** 0.75)


def band_edges(frame: int) -> np.ndarray:
    """The bin edges of the scale-factor bands of a frame size (``pe_codec_bands``): 29 bands at 256, 41 at 1024."""
    if frame not in FRAMES:
        raise ValueError(f"codec: frame {frame!r} is not one of {FRAMES}")
    edges = np.zeros(64, np.int32)
    nb = _lib.load().pe_codec_bands(int(frame), edges.ctypes.data, edges.size)
    if nb < 0:
        _lib.check(nb, "pe_codec_bands")
    return edges[:nb + 1].astype(np.int64)


def plan_rows(lengths, offsets, out_offsets, frame: int = 1024) -> dict:
    """``pe_codec_plan`` (host only): the row plan of a frame size and its constants."""
    if frame not in FRAMES:
        raise ValueError(f"codec: frame {frame!r} is not one of {FRAMES}")
    mismatch = "codec plan: one offset and one output offset per row"
    R, n, xo, meta = plan_arrays("pe_codec_plan_fields", lengths, offsets, mismatch)
    yo = i64(out_offsets)
    if yo.size != R:
        raise ValueError(mismatch)
    consts, totals = np.zeros(4, np.int64), np.zeros(2, np.int64)
    _lib.check(_lib.load().pe_codec_plan(R, int(frame), *host_ptrs(n, xo, yo, consts, meta, totals)), "pe_codec_plan")
    frames = meta[:R, 3].copy()
    return dict(rows=R, lengths=n, meta=meta, frame=int(consts[0]), table_floats=int(consts[1]), bands=int(consts[2]),
                frames=frames, frame_offsets=meta[:R, 4].copy(), n_samples=int(totals[0]), n_frames=int(totals[1]))


def host_tables(frame: int) -> np.ndarray:
    """The float32 table of a frame size M, every entry rounded from float64: the roots of the M / 2-point transform,
    the DCT-IV twiddles exp(-i pi (8 n + 1) / 8M), the window, and the step tables T and R."""
    M = int(frame)
    n = np.arange(M // 2, dtype=np.float64)
    a = np.pi * (8 * n + 1) / (8 * M)
    i = np.arange(STEP_TABLE, dtype=np.float64)
    return np.concatenate([fft_roots(M // 2).reshape(-1), np.stack([np.cos(a), -np.sin(a)], axis=1).reshape(-1),
                           np.sin(np.pi * (np.arange(2 * M, dtype=np.float64) + 0.5) / (2 * M)),
                           2.0 ** ((i - 224) / 4), 2.0 ** (-(i - 224) / 4)]).astype(np.float32)


def _tables(frame, device):
    return _lib.device_table(("codec", int(frame)), device, lambda: host_tables(frame))


def _batch(x, lengths, frame, what):
    """The plan of ``x`` in one of the three layouts with its device copy, and the zeroed dense output."""
    def plan(lengths, offsets):
        width = int(x.shape[1]) if x.dim() == 2 else 0
        out = [r * width for r in range(len(lengths))] if x.dim() == 2 else offsets
        return plan_rows(lengths, offsets, out, frame)
    pl = device_plan(x, lengths, plan, what)
    return pl, torch.zeros(tuple(x.shape), dtype=torch.float32, device=x.device)


def _positive(who, name, v) -> None:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or \
            not math.isfinite(float(v)) or not float(v) > 0:
        raise ValueError(f"{who}: {name} must be a positive finite number, got {v!r}")


def _check_parameters(who, bitrate_kbps, frame, bandwidth_hz) -> None:
    """What can be said of a codec's parameters without the sample rate."""
    if isinstance(frame, bool) or frame not in FRAMES:
        raise ValueError(f"{who}: frame {frame!r} is not one of {FRAMES}")
    _positive(who, "bitrate_kbps", bitrate_kbps)
    if bandwidth_hz is not None:
        _positive(who, "bandwidth_hz", bandwidth_hz)


# ------------------------------------------------------------------------------------------------------ transform codec
class TransformCodec:
    """The transform codec at one setting: ``TransformCodec(sr, bitrate_kbps, frame=1024, bandwidth_hz=None)``.
    ``bandwidth_hz`` defaults to ``default_bandwidth``.  ``ValueError`` for anything else than a positive finite rate,
    bitrate and bandwidth, a frame in ``FRAMES``, and a budget ``floor(1000 bitrate_kbps frame / sr)`` of at least 8
    bits plus one per band below the cutoff.  Attributes: ``cutoff_bin`` (K_c), ``budget`` (bits per frame),
    ``edges`` (band edges), ``bands`` (those below the cutoff)."""

    def __init__(self, sr, bitrate_kbps, frame: int = 1024, bandwidth_hz=None):
        _check_parameters("TransformCodec", bitrate_kbps, frame, bandwidth_hz)
        _positive("TransformCodec", "sr", sr)
        self.sr, self.bitrate_kbps, self.frame = float(sr), float(bitrate_kbps), int(frame)
        bw = default_bandwidth(sr, bitrate_kbps) if bandwidth_hz is None else bandwidth_hz
        self.bandwidth_hz = float(bw)
        M = self.frame
        self.cutoff_bin = min(M, int(math.ceil(self.bandwidth_hz * M / (self.sr / 2.0))))
        self.budget = int(math.floor(1000.0 * self.bitrate_kbps * M / self.sr))
        self.edges = band_edges(M)
        self.bands = int(np.sum(self.edges[:-1] < self.cutoff_bin))
        if self.budget < 8 + self.bands:
            raise ValueError(f"TransformCodec: {self.bitrate_kbps:g} kbps at {self.sr:g} Hz gives a frame of {M} "
                             f"{self.budget} bits, fewer than the {8 + self.bands} of an empty frame")
        if self.budget > 2 ** 31 - 1:
            raise ValueError("TransformCodec: the frame budget exceeds 2^31 - 1 bits")

    def __repr__(self):
        return (f"TransformCodec(sr={self.sr:g}, bitrate_kbps={self.bitrate_kbps:g}, frame={self.frame}, "
                f"bandwidth_hz={self.bandwidth_hz:g})")

    def plan(self, lengths, offsets=None, out_offsets=None) -> dict:
        """The host row plan (``plan_rows``) of rows of ``lengths`` (packed when ``offsets`` is None)."""
        R, n, xo, _ = plan_arrays("pe_codec_plan_fields", lengths, offsets, "codec plan: one offset per row")
        return plan_rows(n, xo, xo if out_offsets is None else out_offsets, self.frame)

    def mdct(self, x: torch.Tensor, lengths=None):
        """``(coefs (frames, M) float32, plan)``: the rows' frames in plan order (``plan["frame_offsets"]``)."""
        pl, _ = _batch(x, lengths, self.frame, "TransformCodec.mdct")
        coefs = torch.zeros((pl["n_frames"], self.frame), dtype=torch.float32, device=x.device)
        if pl["rows"] and pl["n_samples"]:
            t = _tables(self.frame, x.device)
            with torch.cuda.device(x.device):
                ops._call("pe_codec_mdct", x.data_ptr(), pl["meta_d"].data_ptr(), pl["meta"].ctypes.data, pl["rows"],
                          self.frame, t.data_ptr(), t.numel(), coefs.data_ptr(), _lib.stream_ptr())
        return coefs, pl

    def quantize(self, coefs: torch.Tensor, budget=None, cutoff_bin=None):
        """``(q int32 (frames, M), g int32 (frames,), bits int32 (frames,), dequantised (frames, M))`` of coefficient
        frames at this codec's budget and cutoff (or the given ones)."""
        check_device_tensor(coefs, "TransformCodec.quantize")
        if coefs.dim() != 2 or coefs.shape[1] != self.frame:
            raise ValueError(f"TransformCodec.quantize: coefficients of shape (frames, {self.frame}) are expected")
        budget = self.budget if budget is None else int(budget)
        k_c = self.cutoff_bin if cutoff_bin is None else int(cutoff_bin)
        if not 1 <= k_c <= self.frame or budget < 8 + int(np.sum(self.edges[:-1] < k_c)) or budget > 2 ** 31 - 1:
            raise ValueError("TransformCodec.quantize: the cutoff lies outside 1 .. frame or the budget below that of "
                             "an empty frame")
        F, dev = int(coefs.shape[0]), coefs.device
        q = torch.zeros((F, self.frame), dtype=torch.int32, device=dev)
        g = torch.zeros((F,), dtype=torch.int32, device=dev)
        bits = torch.zeros((F,), dtype=torch.int32, device=dev)
        deq = torch.zeros((F, self.frame), dtype=torch.float32, device=dev)
        if F:
            t = _tables(self.frame, dev)
            with torch.cuda.device(dev):
                ops._call("pe_codec_quantize", coefs.data_ptr(), F, self.frame, k_c, budget, t.data_ptr(), t.numel(),
                          q.data_ptr(), g.data_ptr(), bits.data_ptr(), deq.data_ptr(), _lib.stream_ptr())
        return q, g, bits, deq

    def imdct(self, coefs: torch.Tensor, like: torch.Tensor, lengths=None) -> torch.Tensor:
        """The rows of a batch laid out as ``like`` (with ``lengths``) from their coefficient frames in plan order."""
        check_device_tensor(coefs, "TransformCodec.imdct")
        pl, y = _batch(like, lengths, self.frame, "TransformCodec.imdct")
        if coefs.dim() != 2 or tuple(coefs.shape) != (pl["n_frames"], self.frame):
            raise ValueError(f"TransformCodec.imdct: coefficients of shape ({pl['n_frames']}, {self.frame}) are "
                             "expected")
        if pl["rows"] and pl["n_samples"]:
            t = _tables(self.frame, like.device)
            ws_bytes = _lib.load().pe_codec_workspace_bytes(self.frame, pl["n_frames"])
            ws = workspace(ws_bytes, like.device)
            with torch.cuda.device(like.device):
                ops._call("pe_codec_imdct", coefs.data_ptr(), pl["meta_d"].data_ptr(), pl["meta"].ctypes.data,
                          pl["rows"], self.frame, t.data_ptr(), t.numel(), y.data_ptr(), ws.data_ptr(), ws_bytes,
                          _lib.stream_ptr())
        return y

    def __call__(self, x: torch.Tensor, lengths=None, return_stats: bool = False):
        """``x`` through the codec (``pe_codec_apply``: the three stages fused, two launches).  ``return_stats``: also
        ``{"g", "bits"}`` (int32 per frame, plan order) and ``{"frame_offsets", "frames"}`` (per row, host)."""
        pl, y = _batch(x, lengths, self.frame, "TransformCodec")
        g = bits = None
        if return_stats:
            g = torch.zeros((pl["n_frames"],), dtype=torch.int32, device=x.device)
            bits = torch.zeros((pl["n_frames"],), dtype=torch.int32, device=x.device)
        if pl["rows"] and pl["n_samples"]:
            t = _tables(self.frame, x.device)
            ws_bytes = _lib.load().pe_codec_workspace_bytes(self.frame, pl["n_frames"])
            ws = workspace(ws_bytes, x.device)
            with torch.cuda.device(x.device):
                ops._call("pe_codec_apply", x.data_ptr(), pl["meta_d"].data_ptr(), pl["meta"].ctypes.data, pl["rows"],
                          self.frame, self.cutoff_bin, self.budget, t.data_ptr(), t.numel(), y.data_ptr(), _lib.ptr(g),
                          _lib.ptr(bits), ws.data_ptr(), ws_bytes, _lib.stream_ptr())
        if return_stats:
            return y, dict(g=g, bits=bits, frame_offsets=pl["frame_offsets"], frames=pl["frames"])
        return y


def apply_transform_codec(x: torch.Tensor, sr, bitrate_kbps, lengths=None, frame: int = 1024, bandwidth_hz=None,
                          return_stats: bool = False):
    """``TransformCodec(sr, bitrate_kbps, frame, bandwidth_hz)(x, lengths, return_stats)``."""
    return TransformCodec(sr, bitrate_kbps, frame, bandwidth_hz)(x, lengths, return_stats)


# --------------------------------------------------------------------------------------------------------------- mu-law
def apply_mulaw(x: torch.Tensor, lengths=None) -> torch.Tensor:
    """G.711 mu-law encoded and decoded, elementwise on ``p = clamp(rint(32768 x), -32768, 32767)``.  One launch."""
    pl, y = _batch(x, lengths, 1024, "apply_mulaw")
    if pl["rows"] and pl["n_samples"]:
        with torch.cuda.device(x.device):
            ops._call("pe_codec_mulaw", x.data_ptr(), pl["meta_d"].data_ptr(), pl["meta"].ctypes.data, pl["rows"],
                      pl["frame"], y.data_ptr(), _lib.stream_ptr())
    return y


def apply_g711u(x: torch.Tensor, sr: int, lengths=None):
    """A telephone line: ``RaggedResampler`` to 8 kHz, ``apply_mulaw``, and back to ``sr``.  Returns ``(y (B, width)
    padded, lengths)``; the lengths change as in ``stress.apply_resample_condition``."""
    if isinstance(sr, bool) or not isinstance(sr, (int, np.integer)) or int(sr) <= 0:
        raise ValueError(f"apply_g711u: sr must be a positive integer, got {sr!r}")
    down, down_lengths = stress.resample_rows(x, int(sr), G711_RATE, lengths, "apply_g711u")
    return stress.resample_rows(apply_mulaw(down, down_lengths), G711_RATE, int(sr), down_lengths, "apply_g711u")


# ------------------------------------------------------------------------------------------------------------ condition
class CodecCondition(stress.Condition):
    """A codec condition of a sweep: ``CodecCondition(label, codec="transform", bitrate_kbps=..., frame=1024,
    bandwidth_hz=None)`` or ``CodecCondition(label, codec="g711u")``.  ``kind == "codec"``; it carries its own
    ``apply(x, sr, lengths) -> (y, lengths)``, which ``stress.apply_condition`` calls.  The parameters are checked
    here (``ValueError``), the ones that depend on the sample rate (the frame budget) when it is applied."""
    kind = "codec"
    CODECS = ("transform", "g711u")

    def __init__(self, label: str, codec: str = "transform", **params):
        if codec not in self.CODECS:
            raise ValueError(f"CodecCondition: codec {codec!r} is not one of {self.CODECS}")
        allowed = {"transform": ("bitrate_kbps", "frame", "bandwidth_hz"), "g711u": ()}[codec]
        unknown = sorted(set(params) - set(allowed))
        if unknown:
            raise ValueError(f"CodecCondition: a {codec} condition takes {allowed}, got {unknown}")
        if codec == "transform":
            if "bitrate_kbps" not in params:
                raise ValueError("CodecCondition: a transform condition needs bitrate_kbps")
            _check_parameters("CodecCondition", params["bitrate_kbps"], params.get("frame", 1024),
                              params.get("bandwidth_hz"))
        self.codec, self.label, self.params = codec, str(label), dict(params)
        self.bitrate_kbps = float(params["bitrate_kbps"]) if codec == "transform" else G711_KBPS

    def __repr__(self):
        return f"CodecCondition({self.label!r}, codec={self.codec!r}, **{self.params!r})"

    def apply(self, x: torch.Tensor, sr: int, lengths=None):
        if self.codec == "g711u":
            return apply_g711u(x, sr, lengths)
        row_lengths, _ = row_layout(x, lengths, whole_by_default=True)
        p = self.params
        return apply_transform_codec(x, sr, p["bitrate_kbps"], lengths, p.get("frame", 1024),
                                     p.get("bandwidth_hz")), row_lengths
