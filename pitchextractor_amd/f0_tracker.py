"""F0 labels on the device: Boersma's autocorrelation method (Praat's "Sound: To Pitch (ac)"), the algorithm behind
the reference's ``praat`` / ``parselmouth`` backend (f0_backends.py:437-593), as a fixed number of HIP launches (five) per ragged batch
(``csrc/f0_track.hip``).  There is no CPU path.  Written from the published algorithm; parity with Praat's own
binary is unpinned (DESIGN.md "F0 tracking"), the float64 restatement in ``tests/f0_track_ref.py`` is the oracle.

Only ``method: ac`` / ``autocorrelation``, ``unit: Hertz`` and ``very_accurate: false`` are built; anything else is
refused with ``NotImplementedError`` when the tracker (or a dataset that names it) is constructed.
"""
from __future__ import annotations

import logging
import re

import numpy as np
import torch

from . import _lib, ops
from .ragged import packed_offsets, row_layout

logger = logging.getLogger(__name__)

NATIVE_TYPES = ("praat", "parselmouth")
DEFAULT_CONFIG = dict(min_pitch=40.0, max_pitch=1100.0, silence_threshold=0.03, voicing_threshold=0.45,
                      octave_cost=0.01, octave_jump_cost=1.0, voiced_unvoiced_cost=0.3, very_accurate=False)
_CONFIG_ORDER = ("min_pitch", "max_pitch", "silence_threshold", "voicing_threshold", "octave_cost",
                 "octave_jump_cost", "voiced_unvoiced_cost")
_IGNORED_KEYS = {"name", "type", "backend", "enabled", "cache_key_suffix"}
N_CAND = 15


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
    va = out.pop("very_accurate")
    if isinstance(va, str):
        va = va.strip().lower() in {"1", "true", "yes", "on"}
    if va:
        raise NotImplementedError("praat F0 backend: very_accurate (Gaussian window, 6 periods) is not built")
    return {k: float(out[k]) for k in _CONFIG_ORDER}


class PraatACTracker:
    """``PraatACTracker(sr, hop_length, method="ac", **config)``: time step ``hop_length / sr`` (f0_backends.py:497).

    ``track`` runs a ragged batch in a fixed number of launches; a row's contour is bit-identical whether it is
    tracked alone or inside any batch."""

    def __init__(self, sr: int, hop_length: int, **config):
        self.sr, self.hop_length = int(sr), int(hop_length)
        self.config = check_config(config)
        self._cfg = np.array([self.config[k] for k in _CONFIG_ORDER], dtype=np.float64)
        # the constants of the configuration (host only): also validates (sr, hop, config) against the kernels' range
        plan = self.plan([0])
        (self.nsamp_window, self.nsamp_period, self.n_fft, self.max_lag, self.half_window, self.half_period,
         self.n_table, self.lds_frames) = (int(v) for v in plan["consts"])
        self.ceiling, self.time_step = (float(v) for v in plan["dconsts"])

    @property
    def cache_key(self) -> str:
        return "praat"

    # ---- host side ----------------------------------------------------------------------------------------------
    def plan(self, lengths, offsets=None) -> dict:
        """``pe_f0_track_plan``: per-row frame counts / offsets / first frame centres for rows of ``lengths``."""
        lengths = np.ascontiguousarray(lengths, dtype=np.int64).reshape(-1)
        R = lengths.size
        if offsets is None:
            offsets = packed_offsets(lengths)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if offsets.size != R:
            raise ValueError("f0 tracker: one offset per row")
        lib = _lib.load()
        K = lib.pe_f0_track_plan_fields()
        meta = np.zeros((max(R, 1), K), np.int64)
        t1 = np.zeros(max(R, 1), np.float64)
        consts, dconsts, totals = np.zeros(8, np.int64), np.zeros(2, np.float64), np.zeros(2, np.int64)
        p = lambda a: a.ctypes.data  # noqa: E731
        _lib.check(lib.pe_f0_track_plan(R, p(lengths), p(offsets), self.sr, self.hop_length, p(self._cfg), p(consts),
                                        p(dconsts), p(meta), p(t1), p(totals)), "pe_f0_track_plan")
        return dict(n_rows=R, lengths=lengths, offsets=offsets, meta=meta, t1=t1, consts=consts, dconsts=dconsts,
                    frames=meta[:R, 2].copy(), frame_offsets=meta[:R, 3].copy(), n_frames=int(totals[0]),
                    workspace_bytes=int(totals[1]))

    def frame_count(self, n_samples: int) -> int:
        return int(self.plan([int(n_samples)])["frames"][0])

    def frame_times(self, n_samples: int) -> np.ndarray:
        pl = self.plan([int(n_samples)])
        return pl["t1"][0] + np.arange(int(pl["frames"][0]), dtype=np.float64) * self.time_step

    def host_tables(self) -> np.ndarray:
        """float32 tables of the frame kernel, built in float64: FFT roots, real-split roots, window, window_r."""
        C, nw, hw = self.n_fft // 2, self.nsamp_window, self.half_window
        m = np.arange(C, dtype=np.float64)
        k = np.arange(C + 1, dtype=np.float64)
        tw = np.stack([np.cos(2 * np.pi * m / C), -np.sin(2 * np.pi * m / C)], axis=1)
        tr = np.stack([np.cos(np.pi * k / C), -np.sin(np.pi * k / C)], axis=1)
        window = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1, nw + 1, dtype=np.float64) / (nw + 1))
        spec = np.fft.rfft(window, self.n_fft)
        ac = np.fft.irfft(spec.real ** 2 + spec.imag ** 2, self.n_fft)
        window_r = ac[:hw + 1] / ac[0]
        out = np.concatenate([tw.reshape(-1), tr.reshape(-1), window, window_r]).astype(np.float32)
        assert out.size == self.n_table
        return out

    # ---- device side --------------------------------------------------------------------------------------------
    def track(self, waves: torch.Tensor, lengths=None, *, return_candidates: bool = False):
        """``waves``: float32 device audio at ``sr``: one 1-D wave, rows packed back to back in a 1-D tensor
        (``lengths`` required) or a padded 2-D batch (``lengths`` per row, default the width).  Returns one float32
        contour per row (Hz, 0 = unvoiced; empty when the row is shorter than one window), or with
        ``return_candidates`` a dict with the candidate tables as well."""
        if not isinstance(waves, torch.Tensor) or not waves.is_cuda or waves.dtype != torch.float32 or \
                waves.dim() not in (1, 2) or waves.stride(-1) != 1:
            raise RuntimeError("PraatACTracker (HIP) needs contiguous-row float32 device audio; no CPU fallback exists")
        lengths, offsets = row_layout(waves, lengths, whole_by_default=True)
        pl = self.plan(lengths, offsets)
        R, G = pl["n_rows"], pl["n_frames"]
        dev = waves.device
        cand_f = torch.zeros((G, N_CAND), dtype=torch.float32, device=dev)
        cand_s = torch.zeros((G, N_CAND), dtype=torch.float32, device=dev)
        cand_n = torch.zeros((G,), dtype=torch.int32, device=dev)
        f0 = torch.zeros((G,), dtype=torch.float32, device=dev)
        if R and G:
            meta_h, t1_h = pl["meta"], pl["t1"]
            meta = torch.from_numpy(meta_h).to(dev)
            t1 = torch.from_numpy(t1_h).to(dev)
            stats = torch.empty((R, 2), dtype=torch.float32, device=dev)
            tables = _lib.device_table(("f0_track", self.n_fft, self.nsamp_window), dev, self.host_tables)
            ws_bytes = pl["workspace_bytes"]
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev) if ws_bytes else None
            cfg = self._cfg.ctypes.data
            flop = 2 * 2.5 * self.n_fft * np.log2(self.n_fft)
            with torch.cuda.device(dev):
                s = _lib.stream_ptr()
                sws_bytes = _lib.load().pe_f0_track_stats_workspace_bytes(R)
                sws = torch.empty((sws_bytes,), dtype=torch.uint8, device=dev)
                ops._call("pe_f0_track_stats", waves.data_ptr(), meta.data_ptr(), R, stats.data_ptr(), sws.data_ptr(),
                          sws_bytes, s, work=float(sum(lengths) * 8))
                ops._call("pe_f0_track_frames", waves.data_ptr(), meta.data_ptr(), meta_h.ctypes.data, t1.data_ptr(),
                          stats.data_ptr(), tables.data_ptr(), int(tables.numel()), R, self.sr, self.hop_length, cfg,
                          cand_f.data_ptr(), cand_s.data_ptr(), cand_n.data_ptr(), s, work=float(G * flop))
                ops._call("pe_f0_track_path", cand_f.data_ptr(), cand_s.data_ptr(), cand_n.data_ptr(),
                          meta.data_ptr(), meta_h.ctypes.data, R, self.sr, self.hop_length, cfg, f0.data_ptr(),
                          _lib.ptr(ws), ws_bytes, s, work=float(G * (2 * N_CAND * 4 + 8)))
        frames, foff = pl["frames"], pl["frame_offsets"]
        f0_h = f0.cpu().numpy()
        contours = [f0_h[int(o):int(o) + int(n)].copy() for o, n in zip(foff, frames)]
        if not return_candidates:
            return contours
        return dict(f0=contours, cand_f=cand_f.cpu().numpy(), cand_s=cand_s.cpu().numpy(),
                    cand_n=cand_n.cpu().numpy(), frames=frames, frame_offsets=foff)
