"""Robustness stress conditions of the reference's evaluation notebooks on the device (``csrc/stress.hip``): room
impulse responses and microphone colouration (Utils/room_and_microphone_stress.ipynb), sample clipping and AGC pumping
(Utils/amplitude_pathologies.ipynb), the down/up resample (Utils/codec_and_bandwidth_torture.ipynb) and additive noise
at an SNR (``noise.py``).  There is no CPU path.  ``tests/stress_ref.py`` (the noise: ``tests/noise_ref.py``) is the
float64 restatement that pins every one of them.

Every condition takes a ragged batch the way the F0 trackers do (``ragged.device_plan``): a 1-D wave of rows packed back
to back with ``lengths``, or a padded 2-D batch.  The result has the input's shape (dense; zero outside the rows) and a
row of it is bit-identical whether the row is processed alone, packed or padded.  The launch count of a condition does
not depend on the rows.  ``inference.stress_sweep`` runs a model over a list of ``Condition``.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, ops
from .ragged import (PackedRecordings, check_waves, device_plan, fft_roots, host_ptrs, i64, pack_tracks, per_row,
                     plan_arrays, real_split_roots, row_layout, workspace)
from .resample import RaggedResampler

MAX_STAGES = 8
# Utils/room_and_microphone_stress.ipynb, CONFIG["microphone_eq"]
MICROPHONE_PROFILES = {
    "smartphone": ({"freq": 180.0, "gain_db": -6.0, "Q": 0.8}, {"freq": 3500.0, "gain_db": 5.0, "Q": 1.2},
                   {"freq": 9000.0, "gain_db": 3.0, "Q": 1.0}),
    "headset": ({"freq": 120.0, "gain_db": -2.0, "Q": 0.7}, {"freq": 2400.0, "gain_db": 3.0, "Q": 1.4},
                {"freq": 6000.0, "gain_db": 2.5, "Q": 1.1}),
    "studio_ldc": ({"freq": 80.0, "gain_db": 2.0, "Q": 0.9}, {"freq": 4500.0, "gain_db": -1.5, "Q": 1.3},
                   {"freq": 12000.0, "gain_db": 1.5, "Q": 0.9}),
}
CONDITION_KINDS = ("rir", "microphone", "clipping", "agc", "resample", "additive_noise")
POLE_RADIUS_LIMIT = 1.0 - 1e-9


class Condition:
    """One stress condition of a sweep: ``Condition(kind, label, **params)``, ``kind`` one of ``CONDITION_KINDS``.
    params -- rir: ``rirs`` (a ``RirSet``), ``rir_index`` (an int, or one per item); microphone: ``curve`` (a name in
    ``MICROPHONE_PROFILES`` or a list of stages); clipping: ``percent``; agc: ``level_db`` [, ``target_rms``];
    resample: ``target_rate``; additive_noise: ``snr_db`` [, ``source`` (a colour of ``noise.colour_sections`` or a
    ``noise.NoiseSet``; default white), ``seed``, ``bed_index``, ``bed_start``, ``warmup``, ``peak_normalize``].  An
    additive_noise condition is checked here: ``ValueError`` for a missing or non-finite ``snr_db`` or an unknown
    ``source``."""

    def __init__(self, kind: str, label: str, **params):
        if kind not in CONDITION_KINDS:
            raise ValueError(f"Condition: kind {kind!r} is not one of {CONDITION_KINDS}")
        if kind == "additive_noise":
            _check_noise_condition(params)
        self.kind, self.label, self.params = kind, str(label), dict(params)

    def __repr__(self):
        return f"Condition({self.kind!r}, {self.label!r}, **{self.params!r})"


# ------------------------------------------------------------------------------------------------------------ host side
def _check_noise_condition(params: dict) -> None:
    from . import noise
    if "snr_db" not in params:
        raise ValueError("Condition: an additive_noise condition needs snr_db")
    if not np.all(np.isfinite(np.asarray(params["snr_db"], dtype=np.float64))):
        raise ValueError(f"Condition: snr_db must be finite, got {params['snr_db']!r}")
    source = params.get("source", "white")
    if not isinstance(source, noise.NoiseSet):
        noise.colour_sections(source, 24000)               # ValueError for what is not a colour


def prepare_rir(audio) -> np.ndarray:
    """The notebook's load-time normalisation of an impulse response, ``audio / (max|audio| + 1e-6)`` in float32."""
    a = np.asarray(audio, dtype=np.float32).reshape(-1)
    if a.size == 0:
        raise ValueError("prepare_rir: an impulse response needs at least one sample")
    return (a / (np.max(np.abs(a)) + np.float32(1e-6))).astype(np.float32)


def peaking_biquad(sr: float, freq: float, gain_db: float, Q: float):
    """``(b, a)`` of a peaking equaliser, float64 triples normalised to ``a[0] == 1``: what
    ``torchaudio.functional.equalizer_biquad`` computes (the RBJ cookbook's peaking EQ)."""
    w0 = 2.0 * math.pi * float(freq) / float(sr)
    A = math.exp(float(gain_db) / 40.0 * math.log(10.0))
    alpha = math.sin(w0) / 2.0 / float(Q)
    a0 = 1.0 + alpha / A
    b = np.array([(1.0 + alpha * A) / a0, -2.0 * math.cos(w0) / a0, (1.0 - alpha * A) / a0], dtype=np.float64)
    a = np.array([1.0, -2.0 * math.cos(w0) / a0, (1.0 - alpha / A) / a0], dtype=np.float64)
    return b, a


def pole_radius(a) -> float:
    """Largest pole modulus of ``1 + a[1] z^-1 + a[2] z^-2``."""
    return float(np.max(np.abs(np.roots([1.0, float(a[1]), float(a[2])]))))


def cascade_coefficients(sr: float, curve) -> np.ndarray:
    """``(stages, 5)`` float64 rows ``{b0, b1, b2, a1, a2}`` of a microphone curve (a name in ``MICROPHONE_PROFILES`` or
    a sequence of ``{"freq", "gain_db", "Q"}``, the notebook's defaults 1000 Hz / 0 dB / 0.707 for a missing key).
    A stage whose ``b`` and ``a`` are equal is the identity (``{1, 0, 0, 0, 0}``; the stage's clamp stays): 12 kHz at
    24 kHz is one, where ``sin(pi)`` rounds ``alpha`` away.  Any other stage with a pole radius >= 1 - 1e-9 raises
    ``ValueError``."""
    if isinstance(curve, str):
        if curve not in MICROPHONE_PROFILES:
            raise ValueError(f"microphone profile {curve!r} is not one of {sorted(MICROPHONE_PROFILES)}")
        curve = MICROPHONE_PROFILES[curve]
    curve = list(curve)
    if not 1 <= len(curve) <= MAX_STAGES:
        raise ValueError(f"a microphone curve has 1 .. {MAX_STAGES} stages, got {len(curve)}")
    rows = []
    for stage in curve:
        freq, gain, q = float(stage.get("freq", 1000.0)), float(stage.get("gain_db", 0.0)), float(stage.get("Q", 0.707))
        if not (freq > 0.0 and q > 0.0 and math.isfinite(gain) and math.isfinite(freq) and math.isfinite(q)):
            raise ValueError(f"microphone stage {stage!r}: freq and Q must be positive and finite")
        b, a = peaking_biquad(sr, freq, gain, q)
        if np.array_equal(b, a):
            rows.append([1.0, 0.0, 0.0, 0.0, 0.0])
            continue
        radius = pole_radius(a)
        if not radius < POLE_RADIUS_LIMIT:
            raise ValueError(f"microphone stage {stage!r} at {sr} Hz: pole radius {radius!r} is not below 1 - 1e-9")
        rows.append([b[0], b[1], b[2], a[1], a[2]])
    return np.array(rows, dtype=np.float64)


def agc_parameters(level_db: float, sr: int, target_rms: float) -> dict:
    """The notebook's host-side numbers of ``apply_agc_pumping``: attack 0.01 s, release, depth and smoothing length by
    ``np.interp`` over the level, both coefficients ``exp(-1 / (tau sr))`` as float64."""
    level_db = float(level_db)
    attack = 0.01
    release = float(np.interp(level_db, [0.0, 10.0], [0.05, 0.4]))
    depth_db = float(np.interp(level_db, [0.0, 10.0], [3.0, 18.0]))
    return dict(attack_coeff=float(np.exp(-1.0 / (attack * sr))), release_coeff=float(np.exp(-1.0 / (release * sr))),
                max_gain=float(10 ** (depth_db / 20.0)), target_rms=float(target_rms),
                smoothing=int(sr * np.interp(level_db, [0.0, 10.0], [0.01, 0.12])))


def plan_rows(lengths, offsets, out_offsets) -> dict:
    """``pe_stress_plan`` (host only): the row plan and its constants."""
    mismatch = "stress plan: one offset and one output offset per row"
    R, n, xo, meta = plan_arrays("pe_stress_plan_fields", lengths, offsets, mismatch)
    yo = i64(out_offsets)
    if yo.size != R:
        raise ValueError(mismatch)
    consts, totals = np.zeros(4, np.int64), np.zeros(2, np.int64)
    _lib.check(_lib.load().pe_stress_plan(R, *host_ptrs(n, xo, yo, consts, meta, totals)), "pe_stress_plan")
    return dict(rows=R, lengths=n, meta=meta, block_step=int(consts[0]), table_floats=int(consts[1]),
                piece=int(consts[2]), clip_chunk=int(consts[3]), n_samples=int(totals[0]), n_blocks=int(totals[1]))


def host_tables() -> np.ndarray:
    """Roots of the packed 2048-point transform and of its split into the 4096-point real one, float32."""
    C = plan_rows([], [], [])["block_step"]
    return np.concatenate([fft_roots(C).reshape(-1), real_split_roots(C).reshape(-1)]).astype(np.float32)


def _tables(device):
    return _lib.device_table("stress_fft", device, host_tables)


def _batch(x, lengths, what):
    """The plan of ``x`` in one of the three layouts, its device copy, and the zeroed dense output of ``x``'s shape."""
    def plan(lengths, offsets):                 # a padded row goes to its own row of the output, a packed one in place
        width = int(x.shape[1]) if x.dim() == 2 else 0
        return plan_rows(lengths, offsets, [r * width for r in range(len(lengths))] if x.dim() == 2 else offsets)
    pl = device_plan(x, lengths, plan, what)
    return pl, torch.zeros(tuple(x.shape), dtype=torch.float32, device=x.device)


# ------------------------------------------------------------------------------------------------------------ conditions
_RIR_SPECTRA = {}


class RirSet(PackedRecordings):
    """K impulse responses (1-D float arrays of any length >= 1, taken as they are: see ``prepare_rir``) as one ragged
    batch (``rirs``, ``lengths``, ``offsets``, ``packed``, ``key``, ``plan``).  Their partition spectra are made on the
    device once per set and device and kept."""

    def __init__(self, rirs):
        super().__init__(rirs, "RirSet: at least one impulse response, each of at least one sample")
        self.rirs = self._items
        self.plan = plan_rows(self.lengths, self.offsets, self.offsets)

    def device_spectra(self, device):
        """``(plan on the device, partition spectra)`` of the set."""
        k = (self.key, str(device))
        if k not in _RIR_SPECTRA:
            audio = _lib.device_table(("stress_rir", self.key), device, lambda: self.packed)
            meta_d = torch.from_numpy(self.plan["meta"]).to(device)
            C = self.plan["block_step"]
            spectra = torch.empty((self.plan["n_blocks"], C, 2), dtype=torch.float32, device=device)
            tables = _tables(device)
            with torch.cuda.device(device):
                ops._call("pe_stress_spectra", audio.data_ptr(), meta_d.data_ptr(), self.plan["meta"].ctypes.data,
                          len(self), 1, tables.data_ptr(), tables.numel(), spectra.data_ptr(), _lib.stream_ptr())
            _RIR_SPECTRA[k] = (meta_d, spectra)
        return _RIR_SPECTRA[k]


def apply_rir(x: torch.Tensor, rirs: RirSet, rir_index=0, lengths=None) -> torch.Tensor:
    """Row r convolved with ``rirs[rir_index[r]]`` (one int serves every row), causal and cut to the row's length, then
    divided by ``max|y| + 1e-6`` if ``max|y| > 0.99``: the notebook's ``apply_rir``.  Three launches."""
    pl, y = _batch(x, lengths, "apply_rir")
    R = pl["rows"]
    index = per_row(rir_index, R, "apply_rir: one rir_index per row").tolist()
    if any(k < 0 or k >= len(rirs) for k in index):
        raise ValueError("apply_rir: a rir_index lies outside the set")
    if R == 0 or pl["n_samples"] == 0:
        return y
    lib = _lib.load()
    rir_meta_d, spectra = rirs.device_spectra(x.device)
    host_index = np.asarray(index, dtype=np.int32)
    index_d = torch.from_numpy(host_index).to(x.device)
    tables = _tables(x.device)
    ws_bytes = lib.pe_stress_rir_workspace_bytes(pl["n_blocks"])
    ws = workspace(ws_bytes, x.device)
    with torch.cuda.device(x.device):
        ops._call("pe_stress_rir", x.data_ptr(), pl["meta_d"].data_ptr(), pl["meta"].ctypes.data, R, spectra.data_ptr(),
                  rir_meta_d.data_ptr(), rirs.plan["meta"].ctypes.data, len(rirs), index_d.data_ptr(),
                  host_index.ctypes.data, tables.data_ptr(), tables.numel(), y.data_ptr(), ws.data_ptr(), ws_bytes,
                  _lib.stream_ptr())
    return y


def apply_microphone_eq(x: torch.Tensor, sr: float, curve, lengths=None) -> torch.Tensor:
    """The cascade of peaking biquads of ``curve`` (``cascade_coefficients``), each stage clamped to [-1, 1] as
    ``torchaudio``'s ``lfilter`` clamps: the notebook's ``apply_microphone_eq``.  State and sums in double, each stage
    stored as float32.  One launch."""
    coeffs = cascade_coefficients(sr, curve)
    pl, y = _batch(x, lengths, "apply_microphone_eq")
    if pl["rows"] == 0 or pl["n_samples"] == 0:
        return y
    with torch.cuda.device(x.device):
        ops._call("pe_stress_biquad", x.data_ptr(), pl["meta_d"].data_ptr(), pl["meta"].ctypes.data, pl["rows"],
                  coeffs.ctypes.data, int(coeffs.shape[0]), y.data_ptr(), _lib.stream_ptr())
    return y


def _clip(x, lengths, q, copy, what, return_threshold=False):
    pl, y = _batch(x, lengths, what)
    thr = torch.full((max(pl["rows"], 1),), float("nan"), dtype=torch.float32, device=x.device)
    if pl["rows"] and pl["n_samples"]:
        with torch.cuda.device(x.device):
            ops._call("pe_stress_clip", x.data_ptr(), pl["meta_d"].data_ptr(), pl["meta"].ctypes.data, pl["rows"],
                      float(q), int(copy), y.data_ptr(), thr.data_ptr(), _lib.stream_ptr())
    return (y, thr[:pl["rows"]]) if return_threshold else y


def copy_rows(x: torch.Tensor, lengths=None) -> torch.Tensor:
    """The rows of ``x`` in a dense tensor of its shape (what a condition at level 0 returns)."""
    return _clip(x, lengths, 0.0, True, "copy_rows")


def apply_sample_clipping(x: torch.Tensor, percent: float, lengths=None, return_threshold: bool = False):
    """``clip(x, -thr, thr)`` per row, ``thr = np.quantile(|x|, max(0, 1 - percent / 100))`` exactly as numpy 2 computes
    it for a float32 row; a copy for ``percent <= 0`` or ``thr <= 0``: the notebook's ``apply_sample_clipping``.  One
    launch.  ``return_threshold``: also the thresholds (NaN for a copy)."""
    percent = float(percent)
    if not math.isfinite(percent):
        raise ValueError("apply_sample_clipping: percent must be finite")
    q = max(0.0, 1.0 - percent / 100.0)
    return _clip(x, lengths, q, percent <= 0, "apply_sample_clipping", return_threshold)


def apply_sample_clipping_rows(x: torch.Tensor, percents, lengths=None, return_threshold: bool = False):
    """``apply_sample_clipping`` with one ``percent`` per row in one launch (``pe_stress_clip_rows``, the same kernel):
    row r is bit for bit ``apply_sample_clipping(row, percents[r])``, a copy for ``percents[r] <= 0``."""
    pl, y = _batch(x, lengths, "apply_sample_clipping_rows")
    R = pl["rows"]
    percent = per_row(percents, R, "apply_sample_clipping_rows: one percent per row", np.float64)
    if not np.all(np.isfinite(percent)):
        raise ValueError("apply_sample_clipping_rows: percent must be finite")
    q = np.maximum(0.0, 1.0 - percent / 100.0)
    copy = (percent <= 0).astype(np.int32)
    thr = torch.full((max(R, 1),), float("nan"), dtype=torch.float32, device=x.device)
    if R and pl["n_samples"]:
        q_d, copy_d = torch.from_numpy(q).to(x.device), torch.from_numpy(copy).to(x.device)
        with torch.cuda.device(x.device):
            ops._call("pe_stress_clip_rows", x.data_ptr(), pl["meta_d"].data_ptr(), pl["meta"].ctypes.data, R,
                      q_d.data_ptr(), q.ctypes.data, copy_d.data_ptr(), copy.ctypes.data, y.data_ptr(), thr.data_ptr(),
                      _lib.stream_ptr())
    return (y, thr[:R]) if return_threshold else y


def apply_agc_pumping(x: torch.Tensor, level_db: float, sr: int, target_rms: float = 0.15, lengths=None) -> torch.Tensor:
    """The notebook's ``apply_agc_pumping``: envelope follower, gain towards ``target_rms`` within +- depth, moving
    average of the gains, product, clip.  A copy for ``level_db <= 0``.  ``ValueError`` for a row shorter than the
    smoothing length (the reference's ``np.convolve`` returns the longer length there and its product fails).  Two
    launches."""
    if float(level_db) <= 0:
        return copy_rows(x, lengths)
    prm = agc_parameters(level_db, sr, target_rms)
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
        check_waves(x, "apply_agc_pumping")
    row_lengths, _ = row_layout(x, lengths, whole_by_default=True)
    if prm["smoothing"] > 1 and any(n < prm["smoothing"] for n in row_lengths):
        raise ValueError(f"apply_agc_pumping: a row is shorter than the smoothing length {prm['smoothing']}")
    pl, y = _batch(x, lengths, "apply_agc_pumping")
    if pl["rows"] == 0 or pl["n_samples"] == 0:
        return y
    lib = _lib.load()
    params = np.array([prm["attack_coeff"], prm["release_coeff"], prm["target_rms"], prm["max_gain"]], np.float64)
    ws_bytes = lib.pe_stress_agc_workspace_bytes(pl["n_samples"])
    ws = workspace(ws_bytes, x.device)
    with torch.cuda.device(x.device):
        ops._call("pe_stress_agc", x.data_ptr(), pl["meta_d"].data_ptr(), pl["meta"].ctypes.data, pl["rows"],
                  params.ctypes.data, prm["smoothing"], y.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr())
    return y


_RESAMPLERS = {}


def resample_rows(x: torch.Tensor, sr: int, target_rate: int, lengths=None, who: str = "resample_rows"):
    """``(y (B, width) padded, lengths)``: the rows of ``x`` at ``sr`` through ``RaggedResampler`` to ``target_rate``;
    a copy when the two are equal."""
    check_waves(x, who)
    row_lengths, _ = row_layout(x, lengths, whole_by_default=True)
    B = len(row_lengths)
    if target_rate == sr:
        y = copy_rows(x, lengths)
        if y.dim() == 1:                                          # packed rows -> padded rows
            width = max(row_lengths, default=0)
            pad = torch.zeros((B, width), dtype=torch.float32, device=x.device)
            o = 0
            for r, n in enumerate(row_lengths):
                pad[r, :n] = y[o:o + n]
                o += n
            y = pad
        return y, row_lengths
    if target_rate not in _RESAMPLERS:
        _RESAMPLERS[target_rate] = RaggedResampler(target_rate)
    if x.dim() == 1 and lengths is None:
        lengths = row_lengths
    y, _ = _RESAMPLERS[target_rate](x, [sr] * B, lengths)
    return y, [_RESAMPLERS[target_rate].out_len(sr, n) for n in row_lengths]


def apply_resample_condition(x: torch.Tensor, sr: int, target_rate: int, lengths=None):
    """``RaggedResampler`` to ``target_rate`` and back to ``sr``: the notebook's ``apply_resample_condition``.  Returns
    ``(y (B, width) padded, lengths)``: the round trip changes a row's length as the reference's does.
    ``target_rate == sr`` is a copy."""
    sr, target_rate = int(sr), int(target_rate)
    down, down_lengths = resample_rows(x, sr, target_rate, lengths, "apply_resample_condition")
    if target_rate == sr:
        return down, down_lengths
    return resample_rows(down, target_rate, sr, down_lengths, "apply_resample_condition")


def apply_additive_noise(x: torch.Tensor, sr, snr_db, source="white", seed=0, bed_index=0, bed_start=0,
                         warmup: int = 4096, lengths=None, peak_normalize: bool = True, return_stats: bool = False):
    """Noise added to every row at ``snr_db`` (a number, or one per row) over the whole row (``noise.mix_at_snr``): the
    condition the reference's Utils/noise_robustness_evaluation.ipynb is meant to apply.  ``source``: a colour name
    (``noise.NOISE_COLOURS``) or a custom colour, drawn on the device with row r seeded ``seed + r`` (or ``seed[r]``)
    after ``warmup`` settling samples; or a ``noise.NoiseSet``, row r looping recording ``bed_index`` from its sample
    ``bed_start`` (numbers, or one per row).  ``peak_normalize``: the notebooks' ``max|y| > 0.99`` rule.
    ``return_stats``: also the ``(rows, 4)`` float64 ``noise.STAT_KEYS``.  Six to eight launches: the noise (one for
    white or a bed, three for a colour) and the mix's five (one fewer without the peak rule)."""
    from . import noise
    check_waves(x, "apply_additive_noise")
    x = x.contiguous()
    row_lengths, offsets = row_layout(x, lengths, whole_by_default=True)
    flat = torch.zeros((max(x.numel(), 1),), dtype=torch.float32, device=x.device)
    if isinstance(source, noise.NoiseSet):
        noise.bed(source, row_lengths, bed_index, bed_start, offsets=offsets, out=flat)
    elif source == "white":
        noise.white(row_lengths, seed, offsets=offsets, out=flat)
    else:
        noise.coloured(row_lengths, source, sr, seeds=seed, warmup=warmup, offsets=offsets, out=flat)
    return noise.mix_at_snr(x, flat[:x.numel()].view(x.shape), snr_db, lengths, peak_normalize, return_stats)


def apply_condition(cond: Condition, x: torch.Tensor, sr: int, lengths=None):
    """``(y, lengths)`` of one ``Condition`` on a ragged batch.  A condition that brings its own ``apply(x, sr,
    lengths)`` (``codec.CodecCondition``) is asked."""
    if hasattr(cond, "apply"):
        return cond.apply(x, sr, lengths)
    row_lengths, _ = row_layout(x, lengths, whole_by_default=True)
    p = cond.params
    if cond.kind == "rir":
        return apply_rir(x, p["rirs"], p.get("rir_index", 0), lengths), row_lengths
    if cond.kind == "microphone":
        return apply_microphone_eq(x, sr, p["curve"], lengths), row_lengths
    if cond.kind == "clipping":
        return apply_sample_clipping(x, p["percent"], lengths), row_lengths
    if cond.kind == "agc":
        return apply_agc_pumping(x, p["level_db"], sr, p.get("target_rms", 0.15), lengths), row_lengths
    if cond.kind == "additive_noise":
        return apply_additive_noise(x, sr, p["snr_db"], p.get("source", "white"), p.get("seed", 0),
                                    p.get("bed_index", 0), p.get("bed_start", 0), p.get("warmup", 4096), lengths,
                                    p.get("peak_normalize", True)), row_lengths
    return apply_resample_condition(x, sr, p["target_rate"], lengths)


# ------------------------------------------------------------------------------------------------------------ metrics
METRIC_KEYS = ("RPA", "RCA", "VUV", "OctaveError", "VUV_flips", "n_voiced", "n_frames")


def melody_metrics_rows(preds, refs, baselines=None, voicing_threshold_hz: float = 10.0, device="cuda"):
    """The notebooks' ``compute_metrics`` for R rows in one launch (``pe_melody_metrics``): ``preds[r]`` against
    ``refs[r]`` over their first ``min(len)`` frames, and ``VUV_flips`` against ``baselines[r]`` (``None``: NaN) over the
    first ``min(len)`` frames of the two.  Tracks are arrays or tensors of Hz.  Returns one dict per row."""
    R = len(preds)
    if len(refs) != R or (baselines is not None and len(baselines) != R):
        raise ValueError("melody_metrics: one reference (and one baseline) per prediction")
    if R == 0:
        return []
    (pred, po, pn), (ref, ro, rn) = pack_tracks(preds, device), pack_tracks(refs, device)
    base, bo, bn = (None, [0] * R, [0] * R) if baselines is None else pack_tracks(baselines, device)
    tracks = np.zeros((R, _lib.load().pe_melody_metrics_fields()), np.int64)
    for r in range(R):
        tracks[r] = (po[r], min(pn[r], rn[r]), ro[r], bo[r], 0 if base is None else min(pn[r], bn[r]))
    dev = pred.device
    out = torch.empty((R, 7), dtype=torch.float64, device=dev)
    tracks_d = torch.from_numpy(tracks).to(dev)
    with torch.cuda.device(dev):
        ops._call("pe_melody_metrics", pred.data_ptr(), ref.data_ptr(), _lib.ptr(base),
                  tracks_d.data_ptr(), tracks.ctypes.data, R, float(voicing_threshold_hz),
                  out.data_ptr(), _lib.stream_ptr())
    rows = out.cpu().tolist()
    return [dict(RPA=v[0], RCA=v[1], VUV=v[2], OctaveError=v[3], VUV_flips=v[4], n_voiced=int(v[5]), n_frames=int(v[6]))
            for v in rows]
