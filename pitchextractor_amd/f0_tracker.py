"""F0 labels on the device: Boersma's autocorrelation method (Praat's "Sound: To Pitch (ac)"), the algorithm behind
the reference's ``praat`` / ``parselmouth`` backend (f0_backends.py:437-593), as a fixed number of HIP launches (five) per ragged batch
(``csrc/f0_track.hip``).  There is no CPU path.  Written from the published algorithm; parity with Praat's own
binary is unpinned (DESIGN.md "F0 tracking"), the float64 restatement in ``tests/f0_track_ref.py`` is the oracle.

Only ``method: ac`` / ``autocorrelation``, ``unit: Hertz`` and ``very_accurate: false`` are built; anything else is
refused with ``NotImplementedError`` when the tracker (or a dataset that names it) is constructed.

``WorldDioTracker`` (below) is the reference's ``pyworld`` backend with ``algorithm: dio``: WORLD's DIO + StoneMask
(``csrc/f0_dio.hip``), pinned by ``tests/dio_ref.py`` in the same way.

Both stand on ``_RaggedTracker``, and that on ``ragged`` (the host layer of every ragged audio entry point);
``NATIVE_BACKENDS`` alone says which entries of a backend chain run on the device.
"""
from __future__ import annotations

import logging
import re
from collections import namedtuple

import numpy as np
import torch

from . import _lib, ops
from .ragged import device_plan, fft_roots, host_ptrs, plan_arrays, real_split_roots, workspace

logger = logging.getLogger(__name__)

NATIVE_TYPES = ("praat", "parselmouth")            # native whatever the config says; see NATIVE_BACKENDS
DEFAULT_CONFIG = dict(min_pitch=40.0, max_pitch=1100.0, silence_threshold=0.03, voicing_threshold=0.45,
                      octave_cost=0.01, octave_jump_cost=1.0, voiced_unvoiced_cost=0.3, very_accurate=False)
_CONFIG_ORDER = ("min_pitch", "max_pitch", "silence_threshold", "voicing_threshold", "octave_cost",
                 "octave_jump_cost", "voiced_unvoiced_cost")
_IGNORED_KEYS = {"name", "type", "backend", "enabled", "cache_key_suffix"}
N_CAND = 15


def _flag(value) -> bool:
    if isinstance(value, str):
        return value.strip().lower() in {"1", "true", "yes", "on"}
    return bool(value)


def check_config(config: dict | None, require_method: bool = False) -> dict:
    """Validated copy of a ``praat`` backend config with the reference's defaults filled in (f0_backends.py:448-456).
    What this build does not implement is refused.  ``require_method``: a dataset's backend entry must name its
    method, as the shipped config.yml does (without one the reference calls Praat's plain ``to_pitch``, which takes
    none of the costs); the tracker class itself defaults to the one method it has."""
    cfg = dict(config or {})
    method = cfg.pop("method", None)
    if method is None and not require_method:
        method = "ac"
    key = None if method is None else re.sub(r"[^a-z0-9]+", "", str(method).strip().lower())
    if key not in ("ac", "autocorrelation"):
        raise NotImplementedError(f"praat F0 backend: method {method!r} is not built on the HIP path; only 'ac' / "
                                  "'autocorrelation' is (no 'cc', and a dataset entry must name its method)")
    unit = cfg.pop("unit", "Hertz")
    if str(unit).lower() not in ("hertz", "hz"):
        raise NotImplementedError(f"praat F0 backend: unit {unit!r} is not built; only 'Hertz' is")
    out = dict(DEFAULT_CONFIG)
    for k, v in cfg.items():
        if k in out:
            out[k] = v
        elif k not in _IGNORED_KEYS:                  # the reference's PraatBackend reads no other key either
            logger.warning("praat F0 backend: option %r is not read (the reference ignores it too)", k)
    if _flag(out.pop("very_accurate")):
        raise NotImplementedError("praat F0 backend: very_accurate (Gaussian window, 6 periods) is not built")
    return {k: float(out[k]) for k in _CONFIG_ORDER}


class _RaggedTracker:
    """What the trackers share: device audio at ``sr`` goes through a host-side row plan (a row's fields 0 .. 3: offset,
    length, frames, frame prefix offset) and comes back as one contour per row.  A subclass has ``plan()``."""

    def __init__(self, sr: int, hop_length: int):
        self.sr, self.hop_length = int(sr), int(hop_length)

    def _device_plan(self, waves, lengths):
        """The plan of ``waves`` in one of ``track``'s three layouts, with its device copy as ``meta_d``."""
        return device_plan(waves, lengths, self.plan, type(self).__name__)

    def frame_count(self, n_samples: int) -> int:
        return int(self.plan([int(n_samples)])["frames"][0])

    def _contours(self, f0, plan):
        f0_h = f0.cpu().numpy()
        return [f0_h[int(o):int(o) + int(n)].copy() for o, n in zip(plan["frame_offsets"], plan["frames"])]

    def _row_stats(self, waves, meta_d, R, stats, stream, work):
        """``pe_row_stats``: stats[r] = {mean, max |x - mean|} of the R rows of a device plan, at the plan's own stride."""
        ws_bytes = _lib.load().pe_row_stats_workspace_bytes(R)
        ws = workspace(ws_bytes, waves.device)
        ops._call("pe_row_stats", waves.data_ptr(), meta_d.data_ptr(), int(meta_d.shape[1]), R, stats.data_ptr(),
                  ws.data_ptr(), ws_bytes, stream, work=float(work))


class PraatACTracker(_RaggedTracker):
    """``PraatACTracker(sr, hop_length, method="ac", **config)``: time step ``hop_length / sr`` (f0_backends.py:497).

    ``track`` runs a ragged batch in a fixed number of launches; a row's contour is bit-identical whether it is
    tracked alone or inside any batch."""
    cache_key = "praat"

    def __init__(self, sr: int, hop_length: int, **config):
        super().__init__(sr, hop_length)
        self.config = check_config(config)
        self._cfg = np.array([self.config[k] for k in _CONFIG_ORDER], dtype=np.float64)
        # the constants of the configuration (host only): also validates (sr, hop, config) against the kernels' range
        plan = self.plan([0])
        (self.nsamp_window, self.nsamp_period, self.n_fft, self.max_lag, self.half_window, self.half_period,
         self.n_table, self.lds_frames) = (int(v) for v in plan["consts"])
        self.ceiling, self.time_step = (float(v) for v in plan["dconsts"])

    # ---- host side ----------------------------------------------------------------------------------------------
    def plan(self, lengths, offsets=None) -> dict:
        """``pe_f0_track_plan``: per-row frame counts / offsets / first frame centres for rows of ``lengths``."""
        R, lengths, offsets, meta = plan_arrays("pe_f0_track_plan_fields", lengths, offsets,
                                                 "f0 tracker: one offset per row")
        t1 = np.zeros(max(R, 1), np.float64)
        consts, dconsts, totals = np.zeros(8, np.int64), np.zeros(2, np.float64), np.zeros(2, np.int64)
        _lib.check(_lib.load().pe_f0_track_plan(R, *host_ptrs(lengths, offsets), self.sr, self.hop_length,
                                                *host_ptrs(self._cfg, consts, dconsts, meta, t1, totals)),
                   "pe_f0_track_plan")
        return dict(n_rows=R, lengths=lengths, offsets=offsets, meta=meta, t1=t1, consts=consts, dconsts=dconsts,
                    frames=meta[:R, 2].copy(), frame_offsets=meta[:R, 3].copy(), n_frames=int(totals[0]),
                    workspace_bytes=int(totals[1]))

    def frame_times(self, n_samples: int) -> np.ndarray:
        pl = self.plan([int(n_samples)])
        return pl["t1"][0] + np.arange(int(pl["frames"][0]), dtype=np.float64) * self.time_step

    def host_tables(self) -> np.ndarray:
        """float32 tables of the frame kernel, built in float64: FFT roots, real-split roots, window, window_r."""
        C, nw, hw = self.n_fft // 2, self.nsamp_window, self.half_window
        window = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1, nw + 1, dtype=np.float64) / (nw + 1))
        spec = np.fft.rfft(window, self.n_fft)
        ac = np.fft.irfft(spec.real ** 2 + spec.imag ** 2, self.n_fft)
        window_r = ac[:hw + 1] / ac[0]
        out = np.concatenate([fft_roots(C).reshape(-1), real_split_roots(C).reshape(-1), window,
                              window_r]).astype(np.float32)
        assert out.size == self.n_table
        return out

    # ---- device side --------------------------------------------------------------------------------------------
    def track(self, waves: torch.Tensor, lengths=None, *, return_candidates: bool = False):
        """``waves``: float32 device audio at ``sr``: one 1-D wave, rows packed back to back in a 1-D tensor
        (``lengths`` required) or a padded 2-D batch (``lengths`` per row, default the width).  Returns one float32
        contour per row (Hz, 0 = unvoiced; empty when the row is shorter than one window), or with
        ``return_candidates`` a dict with the candidate tables as well."""
        pl = self._device_plan(waves, lengths)
        R, G = pl["n_rows"], pl["n_frames"]
        dev = waves.device
        cand_f = torch.zeros((G, N_CAND), dtype=torch.float32, device=dev)
        cand_s = torch.zeros((G, N_CAND), dtype=torch.float32, device=dev)
        cand_n = torch.zeros((G,), dtype=torch.int32, device=dev)
        f0 = torch.zeros((G,), dtype=torch.float32, device=dev)
        if R and G:
            meta_h, meta, t1 = pl["meta"], pl["meta_d"], torch.from_numpy(pl["t1"]).to(dev)
            stats = torch.empty((R, 2), dtype=torch.float32, device=dev)
            tables = _lib.device_table(("f0_track", self.n_fft, self.nsamp_window), dev, self.host_tables)
            ws_bytes = pl["workspace_bytes"]
            ws = workspace(ws_bytes, dev) if ws_bytes else None
            cfg = self._cfg.ctypes.data
            flop = 2 * 2.5 * self.n_fft * np.log2(self.n_fft)
            with torch.cuda.device(dev):
                s = _lib.stream_ptr()
                self._row_stats(waves, meta, R, stats, s, int(pl["lengths"].sum()) * 8)
                ops._call("pe_f0_track_frames", waves.data_ptr(), meta.data_ptr(), meta_h.ctypes.data, t1.data_ptr(),
                          stats.data_ptr(), tables.data_ptr(), int(tables.numel()), R, self.sr, self.hop_length, cfg,
                          cand_f.data_ptr(), cand_s.data_ptr(), cand_n.data_ptr(), s, work=float(G * flop))
                ops._call("pe_f0_track_path", cand_f.data_ptr(), cand_s.data_ptr(), cand_n.data_ptr(),
                          meta.data_ptr(), meta_h.ctypes.data, R, self.sr, self.hop_length, cfg, f0.data_ptr(),
                          _lib.ptr(ws), ws_bytes, s, work=float(G * (2 * N_CAND * 4 + 8)))
        contours = self._contours(f0, pl)
        if not return_candidates:
            return contours
        return dict(f0=contours, cand_f=cand_f.cpu().numpy(), cand_s=cand_s.cpu().numpy(),
                    cand_n=cand_n.cpu().numpy(), frames=pl["frames"], frame_offsets=pl["frame_offsets"])


# --------------------------------------------------------------------------- WORLD DIO + StoneMask (pyworld backend)
DIO_DEFAULTS = dict(f0_floor=71.0, f0_ceil=800.0, channels_in_octave=2.0, allowed_range=0.1)
_DIO_ORDER = ("f0_floor", "f0_ceil", "channels_in_octave", "allowed_range")
_DIO_NUTTALL = (0.355768, 0.487396, 0.144232, 0.012604)
_DIO_KINDS = 4


def dio_fallback_ok(fallback) -> bool:
    """A ``dio`` run whose fallback is ``dio`` reruns the same computation: a no-op."""
    return fallback is None or str(fallback).strip().lower() in ("", "none", "dio")


def check_dio_config(config: dict | None, sr: int, hop: int, require_algorithm: bool = False) -> dict:
    """Validated copy of a ``pyworld`` backend config (f0_backends.py's PyWorldBackend keys plus the DIO options for
    direct users).  ``require_algorithm``: a dataset entry without ``algorithm`` means ``harvest`` in the reference,
    which is not built; the tracker class itself defaults to the one algorithm it has."""
    cfg = dict(config or {})
    algorithm = cfg.pop("algorithm", None if require_algorithm else "dio")
    if str(algorithm).strip().lower() != "dio":
        raise NotImplementedError(f"pyworld F0 backend: algorithm {algorithm!r} is not built on the HIP path; only "
                                  "'dio' is (the reference's default without the key is 'harvest')")
    fallback = cfg.pop("fallback", None)
    if not dio_fallback_ok(fallback):
        raise NotImplementedError(f"pyworld F0 backend: fallback {fallback!r} is not built; only none / 'dio' is")
    speed = cfg.pop("speed", 1)
    if int(speed) != 1:
        raise NotImplementedError("pyworld F0 backend: speed (decimation) other than 1 is not built")
    period = cfg.pop("frame_period_ms", None)
    if period is not None and abs(float(period) - hop * 1000.0 / sr) > 1e-9 * max(1.0, abs(float(period))):
        raise NotImplementedError(f"pyworld F0 backend: frame_period_ms {period!r} is not hop * 1000 / sr = "
                                  f"{hop * 1000.0 / sr!r}; labels on another grid are not built")
    out = dict(DIO_DEFAULTS, stonemask=_flag(cfg.pop("stonemask", True)),
               min_voiced_frames=int(cfg.pop("min_voiced_frames", 5)))
    for k, v in cfg.items():
        if k in DIO_DEFAULTS:
            out[k] = float(v)
        elif k not in _IGNORED_KEYS:
            logger.warning("pyworld F0 backend: option %r is not read (the reference ignores it too)", k)
    return out


class WorldDioTracker(_RaggedTracker):
    """``WorldDioTracker(sr, hop_length, **config)``: ``pyworld.dio`` + ``pyworld.stonemask`` with pyworld's defaults
    at ``frame_period = hop_length * 1000 / sr`` as HIP launches over a ragged batch (``csrc/f0_dio.hip``).  A row's
    contour is bit-identical whether it is tracked alone or inside any batch.  There is no CPU path."""

    cache_key = "pyworld"

    def __init__(self, sr: int, hop_length: int, **config):
        super().__init__(sr, hop_length)
        if self.sr <= 0 or self.hop_length <= 0:
            raise ValueError("WorldDioTracker: sr and hop_length must be positive")
        self.config = check_dio_config(config, self.sr, self.hop_length)
        self.stonemask = self.config["stonemask"]
        self.min_voiced_frames = self.config["min_voiced_frames"]
        self._cfg = np.array([self.config[k] for k in _DIO_ORDER], dtype=np.float64)
        plan = self.plan([0])
        (self.bands, self.n_fft, self.taps, self.block_step, self.lead, self.voice_range_minimum, self.n_table,
         self.event_chunk, self.cut, self.n_roots) = (int(v) for v in plan["consts"])
        self.half_average_length = [int(v) for v in plan["half"][:self.bands]]
        self.frame_period = float(plan["dconsts"][0])
        self.boundary = [float(v) for v in plan["dconsts"][1:1 + self.bands]]

    # ---- host side ----------------------------------------------------------------------------------------------
    def plan(self, lengths, offsets=None) -> dict:
        """``pe_f0_dio_plan``: the constants and the per-row layout for rows of ``lengths``."""
        R, lengths, offsets, meta = plan_arrays("pe_f0_dio_plan_fields", lengths, offsets,
                                                 "f0 tracker: one offset per row")
        consts, half = np.zeros(10, np.int64), np.zeros(16, np.int64)
        dconsts, totals = np.zeros(17, np.float64), np.zeros(6, np.int64)
        _lib.check(_lib.load().pe_f0_dio_plan(R, *host_ptrs(lengths, offsets), self.sr, self.hop_length,
                                              *host_ptrs(self._cfg, consts, half, dconsts, meta, totals)),
                   "pe_f0_dio_plan")
        return dict(n_rows=R, lengths=lengths, offsets=offsets, meta=meta, consts=consts, half=half, dconsts=dconsts,
                    frames=meta[:R, 2].copy(), frame_offsets=meta[:R, 3].copy(), sample_offsets=meta[:R, 4].copy(),
                    event_offsets=meta[:R, 7].copy(), n_frames=int(totals[0]), n_samples=int(totals[1]),
                    n_blocks=int(totals[2]), n_event_slots=int(totals[3]), n_chunks=int(totals[4]),
                    workspace_bytes=int(totals[5]))

    def frame_times(self, n_samples: int) -> np.ndarray:
        return np.arange(self.frame_count(n_samples), dtype=np.float64) * self.frame_period / 1000.0

    def host_tables(self) -> np.ndarray:
        """float32 tables of the band kernel, built in float64: FFT roots, real-split roots, and per band the
        spectrum (divided by C) of low-cut filter * Nuttall low-pass, delayed to the longest band's delay."""
        N, C = self.n_fft, self.n_fft // 2
        n_cut = 2 * self.cut + 1
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1, n_cut + 1, dtype=np.float64) / (n_cut + 1))
        low_cut = -w / np.sum(w)
        low_cut[self.cut] += 1.0
        parts = [fft_roots(C).reshape(-1), real_split_roots(C).reshape(-1)]
        a = _DIO_NUTTALL
        for h in self.half_average_length:
            t = np.arange(4 * h, dtype=np.float64) / (4 * h - 1.0)
            nut = a[0] - a[1] * np.cos(2 * np.pi * t) + a[2] * np.cos(4 * np.pi * t) - a[3] * np.cos(6 * np.pi * t)
            g = np.zeros(N)
            shift = 2 * (self.half_average_length[0] - h)
            taps = np.convolve(low_cut, nut)
            g[shift:shift + taps.size] = taps
            G = np.fft.rfft(g) / C
            parts.append(np.stack([G.real, G.imag], axis=1).reshape(-1))
        out = np.concatenate(parts).astype(np.float32)
        assert out.size == self.n_table
        return out

    def host_roots(self) -> np.ndarray:
        out = np.concatenate([fft_roots(1 << lg).reshape(-1) for lg in range(7, 13)]).astype(np.float32)
        assert out.size == self.n_roots
        return out

    # ---- device side: one method per stage ----------------------------------------------------------------------
    def _args(self, pl):
        return (pl["n_rows"], self.sr, self.hop_length, self._cfg.ctypes.data)

    def stage_bands(self, waves, pl):
        """(bands, samples of the batch) float32 band signals, rows back to back."""
        dev, R = waves.device, pl["n_rows"]
        sig = torch.zeros((self.bands, max(pl["n_samples"], 1)), dtype=torch.float32, device=dev)
        stats = torch.zeros((max(R, 1), 2), dtype=torch.float32, device=dev)
        tables = _lib.device_table(("f0_dio", self.sr, tuple(self.half_average_length)), dev, self.host_tables)
        s = _lib.stream_ptr()
        if R and pl["n_samples"]:
            self._row_stats(waves, pl["meta_d"], R, stats, s, pl["n_samples"] * 8)
        if pl["n_samples"]:
            ops._call("pe_f0_dio_bands", waves.data_ptr(), pl["meta_d"].data_ptr(), pl["meta"].ctypes.data,
                      stats.data_ptr(), tables.data_ptr(), int(tables.numel()), *self._args(pl), sig.data_ptr(), s,
                      work=float(pl["n_blocks"] * (1 + self.bands) * 2.5 * self.n_fft * np.log2(self.n_fft)))
        return sig[:, :pl["n_samples"]] if pl["n_samples"] else sig[:, :0]

    def stage_events(self, sig, pl):
        """(e_idx, e_frac, e_count (rows, bands, 4)) from band signals (a view of at least the batch's samples)."""
        dev, R = sig.device, pl["n_rows"]
        slots = max(pl["n_event_slots"] * self.bands * _DIO_KINDS, 1)
        e_idx = torch.zeros((slots,), dtype=torch.int32, device=dev)
        e_frac = torch.zeros((slots,), dtype=torch.float32, device=dev)
        e_count = torch.zeros((max(R, 1), self.bands, _DIO_KINDS), dtype=torch.int32, device=dev)
        if R:
            sig = sig.contiguous()
            ws = workspace(max(pl["workspace_bytes"], 4), dev)
            ops._call("pe_f0_dio_events", sig.data_ptr(), pl["meta_d"].data_ptr(), pl["meta"].ctypes.data,
                      *self._args(pl), e_idx.data_ptr(), e_frac.data_ptr(), e_count.data_ptr(), ws.data_ptr(),
                      pl["workspace_bytes"], _lib.stream_ptr(), work=float(2 * self.bands * pl["n_samples"] * 4))
        return e_idx, e_frac, e_count[:R]

    def stage_candidates(self, e_idx, e_frac, e_count, pl):
        """(cand (bands, frames), score, best (frames,), best_band)."""
        dev, G = e_idx.device, pl["n_frames"]
        cand = torch.zeros((self.bands, G), dtype=torch.float32, device=dev)
        score = torch.zeros((self.bands, G), dtype=torch.float32, device=dev)
        best = torch.zeros((G,), dtype=torch.float32, device=dev)
        band = torch.zeros((G,), dtype=torch.int32, device=dev)
        if pl["n_rows"] and G:
            ops._call("pe_f0_dio_candidates", e_idx.data_ptr(), e_frac.data_ptr(), e_count.contiguous().data_ptr(),
                      pl["meta_d"].data_ptr(), pl["meta"].ctypes.data, *self._args(pl), cand.data_ptr(),
                      score.data_ptr(), best.data_ptr(), band.data_ptr(), _lib.stream_ptr(),
                      work=float(G * self.bands * 64))
        return cand, score, best, band

    def stage_fix(self, best, cand, pl):
        """(4, frames): the contour after FixF0Contour's steps 1 .. 4."""
        G = pl["n_frames"]
        steps = torch.zeros((4, G), dtype=torch.float32, device=best.device)
        if pl["n_rows"] and G:
            ops._call("pe_f0_dio_fix", best.contiguous().data_ptr(), cand.contiguous().data_ptr(),
                      pl["meta_d"].data_ptr(), pl["meta"].ctypes.data, *self._args(pl), steps.data_ptr(),
                      _lib.stream_ptr(), work=float(G * self.bands * 8))
        return steps

    def stage_stonemask(self, waves, f0, pl):
        G = pl["n_frames"]
        out = torch.zeros((G,), dtype=torch.float32, device=waves.device)
        if pl["n_rows"] and G and pl["n_samples"]:
            roots = _lib.device_table(("f0_stonemask_roots",), waves.device, self.host_roots)
            ops._call("pe_f0_stonemask", waves.data_ptr(), pl["meta_d"].data_ptr(), pl["meta"].ctypes.data,
                      f0.contiguous().data_ptr(), roots.data_ptr(), int(roots.numel()), pl["n_rows"], self.sr,
                      self.hop_length, float(self.config["f0_floor"]), out.data_ptr(), _lib.stream_ptr(),
                      work=float(G * 5 * 1024 * 10))
        return out

    def track(self, waves: torch.Tensor, lengths=None, *, return_stages: bool = False):
        """``waves``: float32 device audio at ``sr``, in one of ``PraatACTracker.track``'s three layouts.  Returns one
        float32 contour per row (Hz, 0 = unvoiced; ``(int)(1000 n / sr / frame_period) + 1`` frames), or with
        ``return_stages`` a dict with every stage's output as well (host arrays)."""
        pl = self._device_plan(waves, lengths)
        with torch.cuda.device(waves.device):
            sig = self.stage_bands(waves, pl)
            e_idx, e_frac, e_count = self.stage_events(sig, pl)
            cand, score, best, band = self.stage_candidates(e_idx, e_frac, e_count, pl)
            steps = self.stage_fix(best, cand, pl)
            f0 = self.stage_stonemask(waves, steps[3], pl) if self.stonemask else steps[3]
        contours = self._contours(f0, pl)
        if not return_stages:
            return contours
        return dict(f0=contours, plan=pl, bands=sig.cpu().numpy(), e_idx=e_idx.cpu().numpy(),
                    e_frac=e_frac.cpu().numpy(), e_count=e_count.cpu().numpy(), cand=cand.cpu().numpy(),
                    score=score.cpu().numpy(), best=best.cpu().numpy(), best_band=band.cpu().numpy(),
                    steps=steps.cpu().numpy(), frames=pl["frames"], frame_offsets=pl["frame_offsets"])

    def row_events(self, e_idx, e_frac, e_count, pl, row):
        """Host view of one row's events: [band][kind] -> (idx, frac)."""
        n = int(pl["lengths"][row])
        cap = n // 2 + 1
        base = int(pl["event_offsets"][row]) * self.bands * _DIO_KINDS
        out = []
        for b in range(self.bands):
            kinds = []
            for k in range(_DIO_KINDS):
                at, c = base + (b * _DIO_KINDS + k) * cap, int(e_count[row, b, k])
                kinds.append((np.asarray(e_idx[at:at + c], np.int64), np.asarray(e_frac[at:at + c])))
            out.append(kinds)
        return out


# --------------------------------------------------------------------------- the backends this build runs on the device
# key: what ``inference.track_f0(backend=...)`` takes; types: the chain-entry ``type`` values served; accepts(config): is
# such an entry this backend's (else it is outside this build); check(config, sr, hop): a dataset entry's validated config
NativeBackend = namedtuple("NativeBackend", "key tracker types accepts check")


def _asks_for_dio(config: dict) -> bool:
    """A ``pyworld`` entry runs on the device iff it asks for DIO alone: ``algorithm: dio`` (a missing key means
    harvest in the reference) and a fallback that reruns dio or is none."""
    return str(config.get("algorithm", "harvest")).strip().lower() == "dio" and dio_fallback_ok(config.get("fallback"))


NATIVE_BACKENDS = (
    NativeBackend("praat", PraatACTracker, NATIVE_TYPES, lambda config: True,
                  lambda config, sr, hop: check_config(config, require_method=True)),
    NativeBackend("dio", WorldDioTracker, ("pyworld",), _asks_for_dio,
                  lambda config, sr, hop: check_dio_config(config, sr, hop, require_algorithm=True)),
)


def native_backend(btype: str, config):
    """The row of ``NATIVE_BACKENDS`` that runs a backend-chain entry of type ``btype`` with ``config``, or None."""
    config = config if isinstance(config, dict) else {}
    return next((row for row in NATIVE_BACKENDS if btype in row.types and row.accepts(config)), None)
