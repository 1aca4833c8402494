"""The synthetic training items of the data layer: one object per kind, in one ordered registry (``KINDS``).

A kind supplies
  ``name``     as it appears in ``MelDataset._synthetic_generators``;
  ``Request``  what a worker hands the device for one item (the item tuple's last element); has ``out_len``;
  ``Batch``    its rows collated; has ``rows`` and ``out_len`` (int64 tensors);
  ``generate(ds, ...)``                       one item, its draws in the documented order, or None;
  ``collate(batch, rows, row_rates, mixed)``  the ``Batch`` of rows ``rows`` of the item list ``batch``;
  ``run(loader, waves, lengths, dev_batch, host_batch, src_sr)``  the device stage: writes each row's window to
      ``waves[row, :out_len]`` (``waves`` is wide enough and contiguous) and returns ``(waves, lengths)``.
``Request`` and ``Batch`` are top-level ``NamedTuple``s: pickle carries them across worker processes and ``pin_memory``
rebuilds them field by field.  The registry's order is that of the batches in the collated tuple and of the device
stages; ``meldataset`` reads it at call time.  What the kinds share lives there (``MelDataset._base_file_attempt``,
``_labels_and_window``; ``DeviceMelLoader._run_stage``) or below, once."""
from __future__ import annotations

import functools
import logging
import random
from typing import NamedTuple

import numpy as np
import torch

from . import world
from .mel import MAX_MEL_LENGTH
from .pitch_shift import pitch_shift_ragged
from .world import (CHEAPTRICK_Q1, VoiceTransform, check_fft_size, cheaptrick_fft_size, label_curve, noise_seed,
                    output_length, resynthesize_ragged, source_positions, time_warp_curve, warped_frames,
                    warped_length, world_synthesize_ragged)

logger = logging.getLogger(__name__)


class PitchShiftRequest(NamedTuple):
    """One pitch-shifted item.  ``n``: samples of the base file at the model rate; the device writes shifted samples
    [out_start, out_start + out_len) to the batch row, whose mel frame ``frame_start`` is then the item's first kept
    frame (``crop`` of the whole file)."""
    path: str
    n_steps: float
    gain: float
    n: int
    crop: int
    out_start: int
    out_len: int
    frame_start: int
    noise: np.ndarray | None                   # float32 (out_len,) slice of the reference's full-length draw


class PitchShiftBatch(NamedTuple):
    """Collated synthetic rows: their base files packed back to back (no padding), plus per-row parameters."""
    rows: torch.Tensor                         # int64 (K,) batch rows
    src: torch.Tensor                          # float32 flat source audio at the files' own rate
    src_len: torch.Tensor                      # int64 (K,)
    n: torch.Tensor                            # int64 (K,) lengths at the model rate
    n_steps: torch.Tensor                      # float32 (K,)
    gains: torch.Tensor                        # float32 (K,)
    out_start: torch.Tensor                    # int64 (K,)
    out_len: torch.Tensor                      # int64 (K,)
    noise: torch.Tensor | None                 # float32 flat, the windows back to back
    src_sr: torch.Tensor | None = None         # int32 (K,) the base files' rates when the batch mixes rates


class WorldRequest(NamedTuple):
    """One WORLD-vocoder item: the drawn curve's pulse table instead of audio.  ``n``: samples of the whole utterance;
    the device writes synthesized samples [out_start, out_start + out_len) to the batch row, as for a pitch shift."""
    template: int
    gain: float
    n: int
    crop: int
    out_start: int
    out_len: int
    frame_start: int
    curve: np.ndarray                          # float64 (frames,) the drawn F0 curve
    index: np.ndarray                          # the pulse table (world.time_base); with ``time_base: device`` all
    shift: np.ndarray                          # three are empty and the device stage computes the batch's tables
    vuv: np.ndarray
    seed: int                                  # of the aperiodic noise, drawn on the device
    noise: np.ndarray | None                   # float32 (out_len,) slice of the reference's full-length draw


class WorldBatch(NamedTuple):
    """Collated WORLD-vocoder rows.  Only what the kernels read travels to the device as tensors; the curves and
    their pulse tables feed the host-side plan and stay numpy arrays."""
    rows: torch.Tensor                         # int64 (K,) batch rows
    gains: torch.Tensor                        # float32 (K,)
    out_len: torch.Tensor                      # int64 (K,)
    noise: torch.Tensor | None                 # float32 flat, the windows back to back
    templates: np.ndarray                      # int64 (K,)
    out_start: np.ndarray                      # int64 (K,)
    curves: tuple                              # K float64 curves
    tables: tuple                              # K (index, shift, vuv)
    seeds: tuple                               # K ints


class ResynthesisRequest(NamedTuple):
    """One analysis / resynthesis item (its first element is the base file's audio, as for a pitch-shifted one).  The
    device estimates the file's CheapTrick envelope under ``base_curve`` and synthesizes samples [out_start, out_start +
    out_len) of it on ``curve``, which is the item's labels.  ``n``: samples of the base file at the model rate.  With a
    ``transform`` (the ``world.VoiceTransform`` drawn for the item) ``curve``, the window and the noise are on the
    output time axis, whose frame g reads the source frame ``positions[g]``."""
    path: str
    gain: float
    n: int
    crop: int
    out_start: int
    out_len: int
    frame_start: int
    base_curve: np.ndarray                     # float64 (frames,) the file's F0 labels, one per hop
    curve: np.ndarray                          # float64 (frames,) the new curve = the labels (world.label_curve)
    index: np.ndarray                          # the new curve's pulse table (world.time_base; empty, as shift and
                                               # vuv, with ``time_base: device``)
    shift: np.ndarray
    vuv: np.ndarray
    seed: int                                  # of the aperiodic noise, drawn on the device
    noise: np.ndarray | None                   # float32 (out_len,) slice of the full-length additive draw
    transform: tuple | None = None             # (formant, rate, tilt, breath, f_hi), or None: the file's own voice
    positions: np.ndarray | None = None        # float64 (frames of curve,) source frame of each output frame


class ResynthesisBatch(NamedTuple):
    """Collated resynthesis rows: their base files packed back to back (no padding) and their F0 labels likewise; the
    new curves and their pulse tables feed the host-side plan and stay numpy arrays."""
    rows: torch.Tensor                         # int64 (K,) batch rows
    src: torch.Tensor                          # float32 flat source audio at the files' own rate
    src_len: torch.Tensor                      # int64 (K,)
    n: torch.Tensor                            # int64 (K,) lengths at the model rate
    base: torch.Tensor                         # float32 flat, the base curves back to back
    gains: torch.Tensor                        # float32 (K,)
    out_len: torch.Tensor                      # int64 (K,)
    noise: torch.Tensor | None                 # float32 flat, the windows back to back
    src_sr: torch.Tensor                       # int32 (K,) the base files' rates
    out_start: np.ndarray                      # int64 (K,)
    curves: tuple                              # K float64 curves
    tables: tuple                              # K (index, shift, vuv)
    seeds: tuple                               # K ints
    transforms: tuple | None = None            # K transforms (None: that row has none), or None: no row has one
    positions: tuple | None = None             # K position arrays (None where the row has no transform)
    base_len: tuple | None = None              # K lengths of the base curves (they differ from the curves' at a rate)


def synthetic_window(n: int, crop: int, hop: int, n_fft: int, max_frames: int = MAX_MEL_LENGTH):
    """(out_start, out_len, frame_start): the shifted samples that mel frames crop .. crop + max_frames - 1 of an
    n-sample wave read (centre padding n_fft // 2), laid out so that the batch row's frame ``frame_start`` is frame
    ``crop`` of the whole wave and the row's reflect padding happens only where the whole wave's does."""
    frames = 1 + n // hop
    if frames <= max_frames:
        return 0, n, 0
    margin = -(-(n_fft // 2) // hop)
    start, first = (hop * (crop - margin), margin) if crop >= margin else (0, crop)
    return start, min(n - start, hop * (first + max_frames - 1) + n_fft // 2), first


# --------------------------------------------------------------------------- what the kinds share
_i64 = functools.partial(torch.tensor, dtype=torch.int64)
_f32 = functools.partial(torch.tensor, dtype=torch.float32)


def _window_noise(reqs):
    """The rows' additive-noise windows back to back, or None when the kind's block draws none."""
    noise = [r.noise for r in reqs]
    return None if noise[0] is None else torch.from_numpy(np.concatenate(noise).astype(np.float32))


def _noise_window(noise, start, count):
    return None if noise is None else np.ascontiguousarray(noise[start:start + count], dtype=np.float32)


def _gain_range(value):
    """A block's ``gain_db_range``: None, or its values as floats (one number: both ends)."""
    if isinstance(value, (int, float)):
        return float(value), float(value)
    return None if value is None else tuple(float(v) for v in value)


def _draw_gain(gain_db_range):
    if gain_db_range is None:
        return 1.0
    low, high = sorted(gain_db_range)
    return 10.0 ** (random.uniform(low, high) / 20.0)


def _draw_noise(noise_db, n):
    return None if noise_db is None else np.random.normal(scale=10.0 ** (noise_db / 20.0), size=(n,)).astype(np.float32)


def _base_files_at_model_rate(loader, src, rates, src_len):
    """Packed base files as they are when each is at the model rate, else ragged-resampled: (K, width), one per row."""
    sr = loader.mel.sample_rate
    if any(r and r != sr for r in rates):
        src, _ = loader._ragged(src, [r or sr for r in rates], src_len)
    return src


# --------------------------------------------------------------------------- the kinds
class PitchShift:
    """``synthetic_data.pitch_shift``: meldataset.py:423-517 with the signal work left to the device: the same draws
    in the same order, the labels built on the host, the shift itself requested through a ``PitchShiftRequest``."""
    name, Request, Batch = "pitch_shift", PitchShiftRequest, PitchShiftBatch

    def generate(self, ds, force=False):
        cfg = ds.synthetic_pitch_shift_config or {}
        semitone_choices = cfg.get("semitones") or [-4, -2, -1, 1, 2, 4]
        max_attempts = max(1, int(cfg.get("max_attempts", 5)))
        min_voiced_fraction = float(cfg.get("min_voiced_fraction", 0.05))
        gain_db_range = _gain_range(cfg.get("gain_db_range", [-6.0, 3.0]))
        noise_db = None if cfg.get("noise_db") is None else float(cfg["noise_db"])
        keep_original_when_zero = bool(cfg.get("keep_zero_pitch", True))
        for attempt in range(max_attempts):
            paths = [p for p in ds.data_list if p not in ds._invalid_paths]
            if not paths:
                if force and attempt == max_attempts - 1:
                    raise RuntimeError("No valid audio files available for pitch shifting")
                return None
            base = ds._base_file_attempt(paths, min_voiced_fraction)
            if base is None:
                continue
            base_path, wave, wave_sr, n, base_f0 = base
            semitone = random.choice(semitone_choices)
            if semitone == 0 and not force:
                continue
            shifted_f0 = base_f0.astype(np.float32) * float(2 ** (semitone / 12.0))
            if keep_original_when_zero:
                shifted_f0[base_f0 == 0] = 0.0
            gain = _draw_gain(gain_db_range)
            noise = _draw_noise(noise_db, n)
            f0, sil, crop, start, count, first = ds._labels_and_window(shifted_f0, n)
            f0 = np.where(np.isnan(f0), np.float32(ds.zero_value), f0).astype(np.float32)
            req = PitchShiftRequest(base_path, float(semitone), float(gain), int(n), crop, start, count, first,
                                    _noise_window(noise, start, count))
            return torch.from_numpy(wave), torch.from_numpy(f0), torch.from_numpy(sil), first, int(wave_sr), req
        return None

    def collate(self, batch, rows, row_rates, mixed):
        reqs = [batch[i][-1] for i in rows]
        return PitchShiftBatch(_i64(rows), torch.cat([batch[i][0].reshape(-1) for i in rows]),
                               _i64([int(batch[i][0].shape[0]) for i in rows]), _i64([r.n for r in reqs]),
                               _f32([r.n_steps for r in reqs]), _f32([r.gain for r in reqs]),
                               _i64([r.out_start for r in reqs]), _i64([r.out_len for r in reqs]), _window_noise(reqs),
                               torch.tensor([row_rates[i] for i in rows], dtype=torch.int32) if mixed else None)

    def run(self, loader, waves, lengths, pack, host, src_sr):
        """Resample the rows' packed base files (if needed), shift them and write each row's window."""
        n = host.n.numpy()
        offsets = np.concatenate([[0], np.cumsum(n)[:-1]])
        rates = host.src_sr.tolist() if host.src_sr is not None else [src_sr] * len(n)
        src = _base_files_at_model_rate(loader, pack.src, rates, host.src_len.tolist())
        if src.dim() == 2:
            offsets = np.arange(len(n), dtype=np.int64) * src.stride(0)
            src = src.reshape(-1)
        cfg = getattr(loader.dataset, "synthetic_pitch_shift_config", None) or {}
        pitch_shift_ragged(src, offsets, n, host.n_steps.numpy(), pack.gains, waves, host.rows.numpy(),
                           host.out_start.numpy(), host.out_len.numpy(), sr=loader.mel.sample_rate,
                           res_type=cfg.get("resample_type", "kaiser_best"), noise=pack.noise)
        return waves, lengths


class WorldVocoder:
    """``synthetic_data.world_vocoder``: Utils/synthetic.py:194-220 + _build_training_example (meldataset.py:629-677)
    with the synthesis left to the device: the generator's draws in its order, then the crop draw; labels built here.
    With ``time_base: device`` in the block the request's pulse table is empty and ``run`` asks for the device's."""
    name, Request, Batch = "world_vocoder", WorldRequest, WorldBatch

    def generate(self, ds):
        draw = ds._world_generator.draw()
        n = output_length(draw.curve.shape[0], ds.sr, ds._world_generator.frame_period)
        f0, sil, crop, start, count, first = ds._labels_and_window(draw.curve.astype(np.float32), n)
        f0 = np.where(np.isnan(f0), np.float32(ds.zero_value), f0).astype(np.float32)
        req = WorldRequest(int(draw.template), float(draw.gain), n, crop, start, count, first, draw.curve,
                           draw.table.index, draw.table.shift, draw.table.vuv, noise_seed(draw.curve),
                           _noise_window(draw.noise, start, count))
        return torch.zeros(0, dtype=torch.float32), torch.from_numpy(f0), torch.from_numpy(sil), first, int(ds.sr), req

    def collate(self, batch, rows, row_rates, mixed):
        reqs = [batch[i][-1] for i in rows]
        return WorldBatch(_i64(rows), _f32([r.gain for r in reqs]), _i64([r.out_len for r in reqs]),
                          _window_noise(reqs), np.array([r.template for r in reqs], dtype=np.int64),
                          np.array([r.out_start for r in reqs], dtype=np.int64), tuple(r.curve for r in reqs),
                          tuple((r.index, r.shift, r.vuv) for r in reqs), tuple(r.seed for r in reqs))

    def run(self, loader, waves, lengths, pack, host, src_sr):
        """Synthesize each row's window from its pulse table and vowel template."""
        gen = loader.dataset._world_generator
        world_synthesize_ragged(pack.curves, gen.device_templates(loader.device).reshape(-1),
                                pack.templates * (gen.fft_size // 2 + 1), np.zeros(len(pack.curves), np.int64),
                                pack.gains, waves, host.rows.numpy(), pack.out_start, host.out_len.numpy(),
                                fs=gen.sample_rate, frame_period=gen.frame_period, fft_size=gen.fft_size,
                                tables="device" if gen.time_base == "device" else pack.tables, seeds=pack.seeds,
                                out_noise=pack.noise)
        return waves, lengths


class WorldResynthesis:
    """``synthetic_data.world_resynthesis`` (not a key of the reference): a listed file resynthesized on a new F0 curve
    (``world.resynthesize_ragged`` over its CheapTrick envelope), which is then its exact label.  Draws per attempt, in
    this order, after ``PitchShift``: the file (``random.choice``); the semitone (``random.choice``; 0 is allowed: the
    file's own pitch); the gain (``random.uniform``, unless ``gain_db_range`` is null); the vibrato (``random.random``
    against its probability and, when it applies with a positive depth, ``random.uniform`` for its rate); the additive
    noise (``np.random.normal`` of the file's length, unless ``noise_db`` is null); the crop (``np.random.randint``, for
    a file longer than 192 frames).  With a ``transform`` block whose ``probability`` is positive, between the vibrato
    and the noise: ``random.random`` against the probability and, when the transform applies, one ``random.uniform``
    per range that is not a single value, in the order formant, rate, tilt, breath; the noise and the crop are then
    drawn for the output length ``round(n / rate)``.  An unreadable, unlabelled or too sparsely voiced file ends the attempt after the
    file draw; ``generate`` returns None when every attempt failed.  ``time_base: host`` (the default) computes the new
    curve's pulse table in the worker, ``time_base: device`` ships an empty one and has the device stage compute the
    batch's tables (``world.time_base_device``); the time base consumes no draw, so every draw, label and crop is the
    same in both."""
    name, Request, Batch = "world_resynthesis", ResynthesisRequest, ResynthesisBatch
    KEYS = ("enabled", "backend", "semitones", "gain_db_range", "noise_db", "min_voiced_fraction", "max_attempts",
            "modulation", "aperiodicity", "d4c_threshold", "q1", "transform", "time_base")
    MODULATION_KEYS = ("vibrato_probability", "vibrato_semitones", "vibrato_rate_range")
    TRANSFORM_KEYS = ("probability", "formant_ratio_range", "rate_range", "tilt_db_per_octave_range", "breath_db_range",
                      "f_hi")
    # a range's key, its identity, and the values it may take
    TRANSFORM_RANGES = (("formant_ratio_range", 1.0, (0.5, 2.0)), ("rate_range", 1.0, (0.5, 2.0)),
                        ("tilt_db_per_octave_range", 0.0, (-12.0, 12.0)), ("breath_db_range", 0.0, (-40.0, 40.0)))

    def _check_transform(self, ds, block):
        """The ``transform`` block as {probability, ranges (four sorted pairs), f_hi}, or None when it is absent or its
        probability is 0: then no draw is added."""
        if block is None:
            return None
        for k in block:
            if k not in self.TRANSFORM_KEYS:
                logger.warning("world_resynthesis.transform: option %r is not read", k)
        probability = float(block.get("probability", 0.5))
        if not 0.0 <= probability <= 1.0:
            raise ValueError("world_resynthesis: transform.probability must lie in [0, 1]")
        ranges = []
        for key, identity, (low, high) in self.TRANSFORM_RANGES:
            value = block.get(key, identity)
            pair = (float(value),) * 2 if isinstance(value, (int, float)) else tuple(sorted(float(v) for v in value))
            if len(pair) != 2 or not all(np.isfinite(pair)) or pair[0] < low or pair[1] > high:
                raise ValueError(f"world_resynthesis: transform.{key} must be two values within [{low}, {high}]")
            ranges.append(pair)
        f_hi = float(block.get("f_hi", VoiceTransform().f_hi))
        if not 0.0 < f_hi < ds.sr / 2.0:
            raise ValueError("world_resynthesis: transform.f_hi must lie between 0 and half the sample rate")
        return None if probability == 0.0 else {"probability": probability, "ranges": tuple(ranges), "f_hi": f_hi}

    def check_config(self, ds, cfg):
        """The ``world_resynthesis`` block with its defaults filled in; a key it does not read gets a warning, a value
        it cannot use a ``ValueError``."""
        mod = dict(cfg.get("modulation", {}) or {})
        transform = self._check_transform(ds, cfg.get("transform"))
        for where, block, keys in (("", cfg, self.KEYS), (".modulation", mod, self.MODULATION_KEYS)):
            for k in block:
                if k not in keys:
                    logger.warning("world_resynthesis%s: option %r is not read", where, k)
        gain = _gain_range(cfg.get("gain_db_range", [-6.0, 3.0]))
        if gain is not None and len(gain) != 2:
            raise ValueError("world_resynthesis: gain_db_range must provide two values")
        aperiodicity = cfg.get("aperiodicity", 0.0)
        if isinstance(aperiodicity, str):
            if aperiodicity != "d4c":
                raise ValueError(f"world_resynthesis: aperiodicity {aperiodicity!r} is neither a number nor 'd4c'")
            if not 15800 < ds.sr <= 48000:
                raise ValueError("world_resynthesis: aperiodicity 'd4c' needs a sample rate above 15.8 kHz (its "
                                 "voicing test reads up to 7.9 kHz) and of 48 kHz at the most")
        else:
            aperiodicity = float(aperiodicity)
            if not 0.0 <= aperiodicity < 1.0:
                raise ValueError("world_resynthesis: aperiodicity must lie in [0, 1)")
        # 0, not pyworld's 0.85: a frame the label calls voiced keeps a periodic part
        d4c_threshold = float(cfg.get("d4c_threshold", 0.0))
        if not 0.0 <= d4c_threshold < 1.0:
            raise ValueError("world_resynthesis: d4c_threshold must lie in [0, 1)")
        rate = tuple(float(v) for v in mod.get("vibrato_rate_range", (4.0, 7.0)))
        if len(rate) != 2:
            raise ValueError("world_resynthesis: vibrato_rate_range must provide two values")
        hop = int(ds.mel_params["hop_length"])
        noise_db = cfg.get("noise_db", None)
        return {"semitones": list(cfg.get("semitones") or [-4, -2, -1, 1, 2, 4]), "gain_db_range": gain,
                "noise_db": None if noise_db is None else float(noise_db),
                "min_voiced_fraction": float(cfg.get("min_voiced_fraction", 0.05)),
                "max_attempts": max(1, int(cfg.get("max_attempts", 5))),
                "vibrato_probability": float(mod.get("vibrato_probability", 0.6)),
                "vibrato_semitones": float(mod.get("vibrato_semitones", 0.35)), "vibrato_rate_range": rate,
                "aperiodicity": aperiodicity, "d4c_threshold": d4c_threshold, "q1": float(cfg.get("q1", CHEAPTRICK_Q1)),
                "fft_size": check_fft_size(cheaptrick_fft_size(ds.sr)), "frame_period": 1000.0 * hop / ds.sr,
                "transform": transform, "time_base": world.check_time_base_mode(cfg.get("time_base", "host"))}

    @staticmethod
    def _draw_transform(tcfg):
        """The item's ``VoiceTransform``, or None when the block is off or the draw says the file keeps its voice."""
        if tcfg is None or not random.random() < tcfg["probability"]:
            return None
        return VoiceTransform(*(low if low == high else random.uniform(low, high) for low, high in tcfg["ranges"]),
                              tcfg["f_hi"])

    def generate(self, ds):
        cfg = ds.synthetic_resynthesis_config
        fft_size, frame_period = cfg["fft_size"], cfg["frame_period"]
        for _ in range(cfg["max_attempts"]):
            paths = [p for p in ds.data_list if p not in ds._invalid_paths]
            if not paths:
                return None
            base = ds._base_file_attempt(paths, cfg["min_voiced_fraction"])
            if base is None:
                continue
            base_path, wave, wave_sr, n, base_f0 = base
            mel_len = 1 + n // int(ds.mel_params["hop_length"])
            if mel_len < 2:
                continue
            # one analysis frame per mel frame: frame f of both sits on sample f * hop
            base = ds.align_length(np.asarray(base_f0, dtype=np.float32), mel_len).astype(np.float64)
            base = np.where(np.isfinite(base) & (base > 0), base, 0.0)
            semitone = random.choice(cfg["semitones"])
            gain = _draw_gain(cfg["gain_db_range"])
            vibrato, depth = None, 0.0
            if random.random() < cfg["vibrato_probability"]:
                depth = max(cfg["vibrato_semitones"], 0.0)
                if depth > 0:
                    vibrato = random.uniform(*cfg["vibrato_rate_range"])
            transform = self._draw_transform(cfg.get("transform"))
            positions, frames, n_out = None, mel_len, n
            if transform is not None:                            # the output time axis: frame g sits on sample g * hop
                hop = int(ds.mel_params["hop_length"])
                n_out = warped_length(n, transform.rate)
                frames = warped_frames(n, hop, transform.rate)
                if frames < 2:
                    continue
                positions = source_positions(frames, transform.rate, mel_len)
            new = (base if positions is None else time_warp_curve(base, positions)) * float(2 ** (semitone / 12.0))
            if vibrato is not None:
                t = np.arange(frames, dtype=np.float64) * (frame_period / 1000.0)
                new = new * 2.0 ** (np.sin(2.0 * np.pi * vibrato * t) * (depth / 12.0))
            curve = label_curve(new, ds.sr, fft_size)
            noise = _draw_noise(cfg["noise_db"], n_out)
            f0, sil, crop, start, count, first = ds._labels_and_window(curve.astype(np.float32), n_out)
            # the time base consumes no draw: with ``time_base: device`` the device stage computes the batch's tables
            table = world.no_table() if cfg.get("time_base", "host") == "device" else \
                world.time_base(curve, ds.sr, frame_period, fft_size)
            req = ResynthesisRequest(base_path, float(gain), int(n), crop, start, count, first, base, curve,
                                     table.index, table.shift, table.vuv, noise_seed(curve),
                                     _noise_window(noise, start, count),
                                     None if transform is None else tuple(transform), positions)
            return torch.from_numpy(wave), torch.from_numpy(f0), torch.from_numpy(sil), first, int(wave_sr), req
        return None

    def collate(self, batch, rows, row_rates, mixed):
        reqs = [batch[i][-1] for i in rows]
        return ResynthesisBatch(_i64(rows), torch.cat([batch[i][0].reshape(-1) for i in rows]),
                                _i64([int(batch[i][0].shape[0]) for i in rows]), _i64([r.n for r in reqs]),
                                torch.from_numpy(np.concatenate([r.base_curve for r in reqs]).astype(np.float32)),
                                _f32([r.gain for r in reqs]), _i64([r.out_len for r in reqs]), _window_noise(reqs),
                                torch.tensor([row_rates[i] for i in rows], dtype=torch.int32),
                                np.array([r.out_start for r in reqs], dtype=np.int64), tuple(r.curve for r in reqs),
                                tuple((r.index, r.shift, r.vuv) for r in reqs), tuple(r.seed for r in reqs),
                                *((tuple(r.transform for r in reqs), tuple(r.positions for r in reqs),
                                   tuple(len(r.base_curve) for r in reqs))
                                  if any(r.transform is not None for r in reqs) else ()))

    def run(self, loader, waves, lengths, pack, host, src_sr):
        """Bring the rows' packed base files to the model rate (if needed), estimate the envelope of the frames each
        row's window reads and synthesize the window on the row's new curve."""
        cfg = loader.dataset.synthetic_resynthesis_config
        src = _base_files_at_model_rate(loader, pack.src, host.src_sr.tolist(), host.src_len.tolist())
        ap = None
        if cfg["aperiodicity"] == "d4c":
            ap = "d4c"                                           # the window's frames, analysed after CheapTrick
        elif cfg["aperiodicity"] > 0:
            ap = torch.full((cfg["fft_size"] // 2 + 1,), cfg["aperiodicity"], dtype=torch.float32, device=waves.device)
        base_len = [len(c) for c in host.curves] if host.base_len is None else list(host.base_len)
        resynthesize_ragged(src, host.n.tolist(), pack.base.split(base_len), host.curves,
                            loader.mel.sample_rate, cfg["frame_period"], ap=ap, seeds=host.seeds, gains=pack.gains,
                            out=waves, out_rows=host.rows.numpy(), out_start=host.out_start, out_noise=pack.noise,
                            out_len=host.out_len.numpy(), q1=cfg["q1"], fft_size=cfg["fft_size"],
                            tables="device" if cfg.get("time_base", "host") == "device" else host.tables,
                            d4c_threshold=cfg.get("d4c_threshold", 0.0), transforms=host.transforms,
                            positions=None if host.transforms is None else
                            [source_positions(len(c), 1.0, len(c)) if p is None else p
                             for c, p in zip(host.curves, host.positions)])
        return waves, lengths


PITCH_SHIFT, WORLD_VOCODER, WORLD_RESYNTHESIS = KINDS = [PitchShift(), WorldVocoder(), WorldResynthesis()]
