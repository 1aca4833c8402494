"""Data layer drop-in for the reference's ``meldataset.py`` with the mel transform on the GPU.

Public surface kept: ``DEFAULT_MEL_PARAMS``, ``MelDataset`` (same constructor keywords,
``to_melspec``, ``mean/std = -4/4``, ``max_mel_length = 192``, ``path|label`` list lines),
``Collater`` and ``build_dataloader(path_list, validation, batch_size, num_workers, device,
collate_config, dataset_config)`` yielding ``(mels (B,1,80,192), f0s (B,192), is_silences (B,192))``.

What moved: in the reference every item runs the mel transform on the CPU inside a DataLoader
worker (meldataset.py:644).  Here workers only read audio and labels; the batch's raw audio goes
to HBM once and ONE launch of the fused mel kernel does framing + FFT + mel + log + the random
192-frame crop (meldataset.py:668-672, applied as a per-item frame offset) + zero padding
(meldataset.py:806-816).  All index arithmetic -- segment pre-crop (meldataset.py:178-201), F0
alignment (f0_backends.py:788-806), crop offsets -- is reproduced exactly and runs on the host.

Out of scope here: the pyworld harvest / CREPE / SwiftF0 tracker backends (packages or weights that
are not available; pyworld's ``algorithm: dio`` is native, ``f0_tracker.WorldDioTracker``).
The synthetic augmentations run on the GPU, one kind each behind one protocol in ``pitchextractor_amd.synthetic_items``:
``synthetic_data.pitch_shift`` (meldataset.py:324-517), ``world_vocoder`` (Utils/synthetic.py; with ``backend: hip``,
else logged as disabled, as the reference does without pyworld) and ``world_resynthesis`` (not a key of the reference;
``backend: hip``).  A worker makes the kind's draws in the reference's order, builds the labels and ships a ``Request``;
the device writes only the samples the cropped 192 mel frames read into the batch row.  Only ``MelDataset``'s gating and
its fallback ladder (``_generate_synthetic_sample``, the reference's) name a kind; the rest asks the registry.
F0 labels come from the reference's cache files under the reference's own
contract (meldataset.py:519-604): ``<wav>_f0<cache_identifier>.npy`` validated by its sibling ``.json``
(cache_identifier, sample_rate, hop_length), then the legacy ``<wav>_f0.npy``; or from an ``f0_provider`` callable.
When the enabled backend chain of ``f0_params`` holds a ``praat`` / ``parselmouth`` entry (method ``ac``), the caches
need not exist beforehand: ``prepare_f0_caches`` -- run once by ``build_dataloader`` in the main process, before any
worker starts -- reads every listed file that has no valid cache, resamples it to the dataset rate on the device,
tracks whole batches of files with the on-device trackers (``pitchextractor_amd.f0_tracker``: praat ``ac``, pyworld
``dio``), applies
the reference's acceptance rule (fewer than ``bad_f0_threshold`` non-zero frames = that backend failed; every native
entry failed = empty track) and writes ``.npy`` + ``.json`` as meldataset.py:606-619 does, through temporary names.
Workers keep reading caches only.  Entries of the chain that need pyworld harvest / CREPE / SwiftF0 are skipped with a
warning each, as the reference skips a backend whose package is missing.  Existing valid caches are never recomputed,
overwritten or deleted.  A cache whose metadata does not match is skipped with a warning and left on disk (the
reference deletes and recomputes it; this build recomputes only under a name that is free).  Without a native entry
an item with no usable label source fails loudly, as the reference does when no backend is usable
(meldataset.py:80-88).  ``<wav>_mel.npy`` caches
(meldataset.py:679-741) are honoured read-only under the reference's rule: whole-file items without
augmentation whose ``<wav>_mel_meta.json`` equals the expected metadata (audio/dataset sample rate, sample
count, channel count, mel_params) take their spectrogram from the cache -- normalised on the host with the
reference's own float32 expression, cropped, and written over that batch row after the mel launch -- so a
dataset trained with cached spectrograms keeps seeing exactly those values.  Caches are never written (the
device recomputes the mel in one launch per batch) and a mismatching cache is skipped with a warning, not
deleted (the reference clears every cache of the dataset on the first mismatch, :743-767).  Files at another sample rate are resampled on the GPU
(meldataset.py:621-627 -> ``pitchextractor_amd.resample``) right before the mel launch; a batch may mix source
rates: it is then resampled by one ragged launch at each row's own rate (``RaggedResampler``), every row bit-identical
to resampling that item alone.
``dataset_config["augmentation"]`` (not a key of the reference) is taken out by ``build_dataloader`` before the dataset
is built and becomes the loader's ``augment.Augmenter``: reverb, noise, a per-row biquad cascade, clipping, gain and
polarity on the device after the stages above and before the mel launch, drawn from a generator of its own; without
the key, or with ``enabled: false``, every batch is what it was.  Rows with a cached spectrogram are not augmented.
``dataset_config["pitch_modulation"]`` (not a key of the reference either) becomes the loader's
``pitch_mod.PitchModulator``, the stage ahead of the ``Augmenter``: a time warp of the selected rows over their kept
label frames (vibrato, flutter, drift, glide) that moves ``f0s`` and ``is_silences`` with the audio.
"""
from __future__ import annotations

import json
import logging
import math
import os
import random
import re
import struct

import numpy as np
import torch
from torch.utils.data import DataLoader

from .mel import DEFAULT_MEL_PARAMS, MAX_MEL_LENGTH, MEL_MEAN, MEL_STD, LOG_EPS, MelSpectrogram
from . import f0_tracker, synthetic_items
from .pitch_shift import check_res_type
from .resample import RaggedResampler, Resampler
from .synthetic_items import (PITCH_SHIFT, WORLD_RESYNTHESIS, WORLD_VOCODER, PitchShiftBatch,  # noqa: F401
                              PitchShiftRequest, ResynthesisBatch, ResynthesisRequest, WorldBatch, WorldRequest,
                              synthetic_window)
from .world import WorldGenerator

_SYNTHETIC_BATCHES = tuple(kind.Batch for kind in synthetic_items.KINDS)     # of the built-in kinds

logger = logging.getLogger(__name__)
logger.setLevel(logging.DEBUG)

np.random.seed(1)      # meldataset.py:31-32
random.seed(1)


# --------------------------------------------------------------------------- host-side arithmetic
def align_length(values, target_frames: int) -> np.ndarray:
    """``F0Extractor.align_length`` (f0_backends.py:788-806): float64 linear interpolation to
    ``target_frames`` points, then zero each frame whose nearest (round-half-even) source frame is 0."""
    values = np.asarray(values, dtype=np.float64)
    if target_frames <= 0:
        return np.zeros((0,), dtype=np.float32)
    if values.size == target_frames:
        return values.astype(np.float32)
    if values.size == 0:
        return np.zeros((target_frames,), dtype=np.float32)
    last = values.size - 1
    grid = np.linspace(0.0, last, num=target_frames)
    out = np.interp(grid, np.linspace(0.0, last, num=values.size), values)
    zeros = values == 0.0
    if np.any(zeros):
        out[zeros[np.clip(np.round(grid).astype(int), 0, last)]] = 0.0
    return out.astype(np.float32)


def segment_plan(total_frames: int, source_sr: int, target_sr: int, hop: int, win: int, target_frames: int,
                 rng=random):
    """Pre-crop of meldataset.py:178-201 -> (start_frame, num_frames or None, use_full_file)."""
    if target_frames > 0 and source_sr and total_frames > 0:
        requested = (target_frames * hop) / float(target_sr) + max(win, hop) / float(target_sr)
        seg = int(np.ceil(requested * float(source_sr)))
        if seg > 0 and seg < total_frames:
            max_start = max(0, total_frames - seg)
            start = rng.randint(0, max_start) if max_start > 0 else 0
            return start, seg, False
        if seg > 0:
            return 0, seg, True
    return 0, None, True


def read_wav(path, start: int = 0, frames: int | None = None):
    """Minimal RIFF/WAVE reader (PCM 8/16/24/32-bit and IEEE float32/64) -> (float32 [n, ch] or [n], sr).
    Stands in for ``soundfile`` (absent from this image); uses it when importable."""
    try:
        import soundfile as sf  # pragma: no cover - optional
        with sf.SoundFile(path, mode="r") as f:
            if start:
                f.seek(int(start))
            data = f.read(frames=-1 if frames is None else int(frames), dtype="float32", always_2d=False)
            return np.asarray(data, dtype=np.float32), f.samplerate
    except ImportError:
        pass
    with open(path, "rb") as fh:
        riff, _, wave_id = struct.unpack("<4sI4s", fh.read(12))
        if riff != b"RIFF" or wave_id != b"WAVE":
            raise RuntimeError(f"Failed to load audio file '{path}': not a RIFF/WAVE file")
        fmt = None
        while True:
            head = fh.read(8)
            if len(head) < 8:
                raise RuntimeError(f"Failed to load audio file '{path}': no data chunk")
            cid, size = struct.unpack("<4sI", head)
            if cid == b"fmt ":
                raw = fh.read(size + (size & 1))
                tag, ch, sr, _, align, bits = struct.unpack("<HHIIHH", raw[:16])
                if tag == 0xFFFE and size >= 26:
                    tag = struct.unpack("<H", raw[24:26])[0]
                fmt = (tag, ch, sr, align, bits)
            elif cid == b"data":
                if fmt is None:
                    raise RuntimeError(f"Failed to load audio file '{path}': data before fmt")
                tag, ch, sr, align, bits = fmt
                total = size // align
                start = min(int(start or 0), total)
                n = total - start if frames is None else min(int(frames), total - start)
                fh.seek(start * align, 1)
                buf = fh.read(n * align)
                if tag == 3:
                    data = np.frombuffer(buf, dtype="<f4" if bits == 32 else "<f8").astype(np.float32)
                elif tag == 1 and bits == 16:
                    data = np.frombuffer(buf, dtype="<i2").astype(np.float32) / 32768.0
                elif tag == 1 and bits == 32:
                    data = np.frombuffer(buf, dtype="<i4").astype(np.float32) / 2147483648.0
                elif tag == 1 and bits == 8:
                    data = (np.frombuffer(buf, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
                elif tag == 1 and bits == 24:
                    b = np.frombuffer(buf, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
                    v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
                    data = (np.where(v >= 1 << 23, v - (1 << 24), v)).astype(np.float32) / 8388608.0
                else:
                    raise RuntimeError(f"Failed to load audio file '{path}': unsupported format {tag}/{bits}")
                return (data.reshape(-1, ch) if ch > 1 else data), sr
            else:
                fh.seek(size + (size & 1), 1)


def wav_info(path):
    """(frames, sample_rate, channels) without reading the samples."""
    with open(path, "rb") as fh:
        riff, _, wave_id = struct.unpack("<4sI4s", fh.read(12))
        if riff != b"RIFF" or wave_id != b"WAVE":
            raise RuntimeError("not a RIFF/WAVE file")
        fmt = None
        while True:
            head = fh.read(8)
            if len(head) < 8:
                raise RuntimeError("no data chunk")
            cid, size = struct.unpack("<4sI", head)
            if cid == b"fmt ":
                raw = fh.read(size + (size & 1))
                _, ch, sr, _, align, _ = struct.unpack("<HHIIHH", raw[:16])
                fmt = (ch, sr, align)
            elif cid == b"data":
                ch, sr, align = fmt
                return size // align, sr, ch
            else:
                fh.seek(size + (size & 1), 1)


# --------------------------------------------------------------------------- F0 cache naming
_BACKEND_TYPES = ("pyworld", "crepe", "swiftf0", "praat", "parselmouth")            # f0_backends.py:587-593
_DEFAULT_BACKENDS = [{"name": "pyworld_harvest", "type": "pyworld"}, {"name": "pyworld_dio", "type": "pyworld"}]


def _norm_backend(name) -> str:
    return re.sub(r"[^a-z0-9]+", "_", str(name).lower()).strip("_")               # f0_backends.py:596-597


def _enabled(value) -> bool:
    if isinstance(value, str):                                                      # f0_backends.py:619-631
        v = value.strip().lower()
        if not v or v in {"0", "false", "no", "off"}:
            return False
        if v in {"1", "true", "yes", "on"}:
            return True
    return bool(value)


def f0_backend_chain(f0_params: dict | None):
    """The enabled backend chain of an ``f0_params`` block as the reference builds it (f0_backends.py:661-757):
    list of (normalised name, type, config dict) in chain order."""
    cfg = f0_params or {}
    backends = cfg.get("backends") or {}
    if cfg.get("backend_order"):
        sequence = list(cfg["backend_order"])
    elif backends:
        sequence = list(backends.keys())
    else:
        sequence = [e["name"] for e in _DEFAULT_BACKENDS]
    defaults = {e["name"]: e for e in _DEFAULT_BACKENDS}
    chain = []
    for raw in sequence:
        if isinstance(raw, dict):
            entry = dict(raw)
        else:
            name = str(raw)
            bcfg, bkey = None, name
            if backends:
                if name in backends:
                    bcfg = backends[name]
                else:
                    for k, v in backends.items():
                        if _norm_backend(k) == _norm_backend(name):
                            bcfg, bkey = v, k
                            break
                if bcfg is None:
                    continue                                   # declared order names an unconfigured backend
            entry = {**defaults.get(bkey, defaults.get(name, {"name": name, "type": name})), **(bcfg or {})}
            entry.setdefault("name", bkey or name)
            entry.setdefault("type", entry.get("backend", entry.get("type", name)))
        if not _enabled(entry.get("enabled", True)):
            continue
        btype = str(entry.get("type") or entry.get("backend") or "pyworld").lower()
        if btype not in _BACKEND_TYPES:
            continue
        name = _norm_backend(entry.get("name") or entry.get("type") or "backend")
        bconf = entry.get("config") or {k: v for k, v in entry.items()
                                        if k not in {"name", "type", "backend", "enabled"}}
        chain.append((name, btype, bconf))
    return chain


def f0_cache_identifier(f0_params: dict | None) -> str:
    """The reference's ``F0Extractor.cache_identifier`` (f0_backends.py:661-757) for an ``f0_params``
    block: "-" + the cache keys of the enabled backends in chain order, joined by "_" (the shipped
    config.yml -> "-swiftf0").  The reference drops backends whose package is missing on the machine that
    computed the cache; set ``f0_params['cache_identifier']`` to name such a cache explicitly."""
    cfg = f0_params or {}
    if cfg.get("cache_identifier") is not None:
        return str(cfg["cache_identifier"])
    keys = []
    for name, _, bconf in f0_backend_chain(cfg):
        suffix = bconf.get("cache_key_suffix") if isinstance(bconf, dict) else None
        keys.append(_norm_backend(f"{name}-{suffix}" if suffix else name))
    return ("-" + "_".join(keys)) if keys else ""


# --------------------------------------------------------------------------- dataset
class MelDataset(torch.utils.data.Dataset):
    def __init__(self, data_list, sr=DEFAULT_MEL_PARAMS["sample_rate"], mel_params=None, f0_params=None,
                 data_augmentation=False, validation=False, verbose=True, synthetic_data=None,
                 f0_provider=None):
        self.verbose = verbose
        self.data_list = [line[:-1].split("|")[0] for line in data_list]        # meldataset.py:55-56

        mel_params = dict(mel_params or {})
        if "win_len" in mel_params and "win_length" not in mel_params:
            mel_params["win_length"] = mel_params.pop("win_len")                # meldataset.py:59-60
        self.mel_params = DEFAULT_MEL_PARAMS.copy()
        self.mel_params.update(mel_params)
        self.sr = sr if sr is not None else self.mel_params.get("sample_rate", DEFAULT_MEL_PARAMS["sample_rate"])
        self.mel_params["sample_rate"] = self.sr
        if self.verbose:
            print(f"[MelDataset] Using mel-spectrogram parameters: {self.mel_params}")
        self.to_melspec = MelSpectrogram(**self.mel_params)                     # HIP transform, (N,) -> (80, L)

        self.f0_params = f0_params or {}
        self.f0_provider = f0_provider
        self.f0_cache_identifier = f0_cache_identifier(self.f0_params)
        self.f0_cache_suffix = f"_f0{self.f0_cache_identifier}.npy"               # meldataset.py:91-92
        self.f0_meta_suffix = self.f0_cache_suffix.replace(".npy", ".json")
        self.mean, self.std = MEL_MEAN, MEL_STD
        self.data_augmentation = data_augmentation and (not validation)
        self.max_mel_length = MAX_MEL_LENGTH
        self.zero_value = float(self.f0_params.get("zero_fill_value", 0.0))
        self.bad_F0 = int(self.f0_params.get("bad_f0_threshold", 5))
        self.requires_cuda_backend = False
        # native (on-device) entries of the backend chain: validated now, run by prepare_f0_caches
        self._f0_chain = f0_backend_chain(self.f0_params)
        hop = int(self.mel_params["hop_length"])
        rows = [(name, f0_tracker.native_backend(btype, cfg), cfg if isinstance(cfg, dict) else {})
                for name, btype, cfg in self._f0_chain]
        # (name, tracker class name, validated config), chain order
        self._native_f0 = [(name, row.tracker.__name__, row.check(cfg, self.sr, hop)) for name, row, cfg in rows if row]
        self._audio_metadata_cache = {}
        self._invalid_paths = set()
        self._mel_cache_suffix, self._mel_meta_suffix = "_mel.npy", "_mel_meta.json"      # meldataset.py:102-103
        self._cache_enabled = True
        self._mel_cache_warned = False
        # synthetic augmentation (meldataset.py:139-143,324-381)
        self._base_length = len(self.data_list)
        self.synthetic_config = synthetic_data or {}
        self.synthetic_enabled = bool(self.synthetic_config.get("enabled", False))
        self.synthetic_apply_to_validation = bool(self.synthetic_config.get("apply_to_validation", False))
        if validation and not self.synthetic_apply_to_validation:
            self.synthetic_enabled = False
        self._synthetic_generators = []
        self._synthetic_count = 0
        self.synthetic_pitch_shift_config = {}
        if self.synthetic_enabled:
            self._initialise_synthetic_generators()
        if self.verbose and self.synthetic_enabled:
            print(f"[MelDataset] Synthetic data enabled: {{'count': {self._synthetic_count}, "
                  f"'strategies': {self._synthetic_generators}}}")

    def __len__(self):
        if not self.synthetic_enabled:
            return self._base_length
        return self._base_length + self._synthetic_count

    # ---- synthetic items ------------------------------------------------------------------
    def _initialise_synthetic_generators(self):
        config = self.synthetic_config
        ratio = float(config.get("ratio", 0.0))
        absolute_count = config.get("absolute_count")
        max_items = config.get("max_items")
        min_items = config.get("min_items", 0)
        if absolute_count is not None:
            self._synthetic_count = max(0, int(absolute_count))
        else:
            target = int(round(self._base_length * ratio))
            if ratio > 0 and target == 0 and self._base_length > 0:
                target = 1
            self._synthetic_count = max(0, target)
        if max_items is not None:
            self._synthetic_count = min(self._synthetic_count, int(max_items))
        if min_items:
            self._synthetic_count = max(self._synthetic_count, int(min_items))

        pitch_shift_cfg = config.get("pitch_shift", {}) or {}
        if pitch_shift_cfg.get("enabled", True):
            check_res_type(pitch_shift_cfg.get("resample_type", "kaiser_best"))
            if not self.data_list:
                if self.verbose:
                    print("[MelDataset] Pitch-shift augmentation disabled: no base samples available.")
            else:
                self._synthetic_generators.append("pitch_shift")
        self.synthetic_pitch_shift_config = pitch_shift_cfg

        world_cfg = config.get("world_vocoder", {}) or {}
        self._world_generator = None
        if world_cfg.get("enabled", False):
            if str(world_cfg.get("backend", "")).lower() == "hip":
                # the reference builds its WorldSynthesizer here (meldataset.py:357-373); a configuration it would
                # refuse, or an fft_size the kernel lacks, is an error rather than a silently missing generator
                self._world_generator = WorldGenerator(self.sr, int(self.mel_params["hop_length"]),
                                                       self.mel_params.get("n_fft", 1024), world_cfg)
                self._synthetic_generators.append("world_vocoder")
            else:
                logger.warning("[MelDataset] WORLD vocoder synthetic generation disabled: pyworld unavailable")

        self.synthetic_resynthesis_config = None
        resyn_cfg = config.get("world_resynthesis", {}) or {}
        if resyn_cfg.get("enabled", False):
            if str(resyn_cfg.get("backend", "")).lower() != "hip":
                logger.warning("[MelDataset] WORLD analysis / resynthesis disabled: it exists with `backend: hip` only")
            elif not self.data_list:
                logger.warning("[MelDataset] WORLD analysis / resynthesis disabled: no base samples available")
            else:
                self.synthetic_resynthesis_config = WORLD_RESYNTHESIS.check_config(self, resyn_cfg)
                self._synthetic_generators.append("world_resynthesis")

        if not self._synthetic_generators or self._synthetic_count <= 0:
            self.synthetic_enabled = False
            self._synthetic_generators = []
            self._synthetic_count = 0
            if self.verbose:
                print("[MelDataset] Synthetic data disabled: no valid generators or count is zero.")

    def _generate_synthetic_sample(self):
        """meldataset.py:382-418, draw for draw: which kind makes the item, and which one steps in when it cannot."""
        if not self._synthetic_generators:
            raise RuntimeError("Synthetic generation requested but no generators are available")
        generator_name = random.choice(self._synthetic_generators)
        if generator_name == "pitch_shift":
            result = PITCH_SHIFT.generate(self)
            if result is not None:
                return result
            remaining = [g for g in self._synthetic_generators if g != "pitch_shift"]
            if remaining:
                generator_name = random.choice(remaining)
            else:
                result = PITCH_SHIFT.generate(self, force=True)
                if result is not None:
                    return result
                raise RuntimeError("Unable to produce synthetic pitch-shift sample")
        if generator_name == "world_resynthesis":
            result = WORLD_RESYNTHESIS.generate(self)
            if result is not None:
                return result
            if "world_vocoder" not in self._synthetic_generators:
                raise RuntimeError("Unable to produce synthetic resynthesis sample")
            generator_name = "world_vocoder"                  # the one generator that needs no file; no draw for it
        if generator_name == "world_vocoder" and self._world_generator is not None:
            return WORLD_VOCODER.generate(self)
        raise RuntimeError(f"Unknown synthetic generator '{generator_name}'")

    align_length = staticmethod(align_length)

    def _base_file_attempt(self, available_paths, min_voiced_fraction):
        """One attempt of a kind that starts from a listed file (meldataset.py:437-466): draws the file
        (``random.choice``), reads it as mono float32 and fetches its F0 track -> (path, wave, wave_sr, n = its length
        at the model rate, base_f0), or None for "next attempt": unreadable (and from now on invalid), unlabelled or
        voiced in less than ``min_voiced_fraction`` of its frames."""
        base_path = random.choice(available_paths)
        try:
            wave, wave_sr = read_wav(base_path)
        except (RuntimeError, OSError, ValueError, struct.error) as exc:
            self._invalid_paths.add(base_path)
            logger.warning("[MelDataset] Skipping unreadable audio file: %s (%s)", base_path, exc)
            return None
        if wave.ndim > 1:
            wave = np.mean(wave, axis=-1)
        wave = wave.astype(np.float32)
        n = Resampler(wave_sr, self.sr).out_len(len(wave)) if wave_sr != self.sr else len(wave)
        try:
            base_f0 = self._f0_for(base_path, wave, 0, None)
        except RuntimeError as exc:          # the reference falls back to an empty track when F0 fails
            logger.warning("[MelDataset] %s", exc)
            base_f0 = np.zeros((0,), dtype=np.float32)
        if base_f0.size == 0 or float(np.count_nonzero(base_f0 > 0)) / base_f0.size < min_voiced_fraction:
            return None
        return base_path, wave, wave_sr, n, base_f0

    def _labels_and_window(self, curve, n):
        """_build_training_example (meldataset.py:629-677) with caches off, for a synthetic item of ``n`` samples whose
        F0 track is ``curve`` (float32): labels per mel frame, the crop draw (``np.random.randint``, beyond 192 frames),
        the samples the kept frames read -> (f0, is_silence, crop, out_start, out_len, frame_start), NaNs left in."""
        hop = int(self.mel_params["hop_length"])
        mel_len = 1 + n // hop
        f0 = align_length(curve, mel_len)
        sil = (f0 == 0).astype(np.float32)
        crop = 0
        if mel_len > self.max_mel_length:
            crop = int(np.random.randint(0, mel_len - self.max_mel_length))
            f0 = f0[crop:crop + self.max_mel_length]
            sil = sil[crop:crop + self.max_mel_length]
        return (f0, sil, crop) + synthetic_window(n, crop, hop, int(self.mel_params["n_fft"]), self.max_mel_length)

    # ---- labels ---------------------------------------------------------------------------
    def _f0_cache_paths(self, path):
        return path + self.f0_cache_suffix, path + self.f0_meta_suffix, path + "_f0.npy"

    def _f0_cache_metadata(self, path):
        """(metadata of the identifier-named cache or None, the metadata this dataset expects)."""
        meta_path = self._f0_cache_paths(path)[1]
        metadata = None
        if os.path.isfile(meta_path):
            try:
                with open(meta_path, "r", encoding="utf-8") as fh:
                    metadata = json.load(fh)
            except (OSError, json.JSONDecodeError):
                metadata = None
        expected = {"cache_identifier": self.f0_cache_identifier, "sample_rate": int(self.sr),
                    "hop_length": int(self.mel_params["hop_length"])}
        return metadata, expected

    def _load_cached_f0(self, path):
        """meldataset.py:566-604: the identifier-named cache if its .json agrees on (cache_identifier,
        sample_rate, hop_length); else the legacy ``_f0.npy``; else None.  Nothing is deleted."""
        data_path, meta_path, legacy_path = self._f0_cache_paths(path)
        if os.path.isfile(data_path) and data_path != legacy_path:
            metadata, expected = self._f0_cache_metadata(path)
            if metadata and all(metadata.get(k) == v for k, v in expected.items()):
                try:
                    return np.load(data_path).astype(np.float32)
                except (OSError, ValueError):
                    logger.warning("[MelDataset] unreadable F0 cache %s: skipped", data_path)
            else:
                logger.warning("[MelDataset] F0 cache %s %s: skipped (the reference would recompute it)", data_path,
                               "has no readable metadata" if not metadata else
                               f"was computed for {({k: metadata.get(k) for k in expected})}, expected {expected}")
        if os.path.isfile(legacy_path):
            try:
                return np.load(legacy_path).astype(np.float32)
            except (OSError, ValueError):
                logger.warning("[MelDataset] unreadable legacy F0 cache %s: skipped", legacy_path)
        return None

    # ---- label pre-pass (meldataset.py:525-564,606-619 for whole files, on the device) ---------------------
    @property
    def has_native_f0(self) -> bool:
        """True when the enabled backend chain holds a ``praat`` / ``parselmouth`` entry this build can run."""
        return bool(self._native_f0)

    def _save_f0_cache(self, path, f0, backend_name):
        """meldataset.py:606-619 through temporary names.  After a return or an exception both files exist under their
        final names or neither does.  The .json goes first: a process killed between the two renames leaves a lone
        .json, which is not a cache (the loader asks for the .npy first) and is replaced by the next pass."""
        data_path, meta_path, _ = self._f0_cache_paths(path)
        metadata = {"cache_identifier": self.f0_cache_identifier, "backend": backend_name,
                    "sample_rate": int(self.sr), "hop_length": int(self.mel_params["hop_length"])}
        tmp = [f"{data_path}.tmp{os.getpid()}", f"{meta_path}.tmp{os.getpid()}"]
        had_meta = os.path.exists(meta_path)
        placed = False
        try:
            with open(tmp[0], "wb") as fh:
                np.save(fh, np.asarray(f0, dtype=np.float32))
            with open(tmp[1], "w", encoding="utf-8") as fh:
                json.dump(metadata, fh, sort_keys=True)
            os.replace(tmp[1], meta_path)
            placed = True
            os.replace(tmp[0], data_path)
        except BaseException:
            if placed and not had_meta:                # only what this call put there
                os.remove(meta_path)
            raise
        finally:
            for t in tmp:
                if os.path.exists(t):
                    os.remove(t)

    def files_to_label(self, rank: int = 0, world: int = 1):
        """Listed files (each once, in list order) of shard ``rank::world`` that have no valid F0 cache and whose
        cache name is free."""
        todo = []
        for path in list(dict.fromkeys(self.data_list))[int(rank)::max(int(world), 1)]:
            data_path, _, legacy_path = self._f0_cache_paths(path)
            if os.path.isfile(data_path) and data_path != legacy_path:
                metadata, expected = self._f0_cache_metadata(path)           # the metadata alone; no array is read
                if not (metadata and all(metadata.get(k) == v for k, v in expected.items())) and \
                        not os.path.isfile(legacy_path):
                    logger.warning("[MelDataset] %s does not match this dataset and is in the way: %s is not labelled",
                                   data_path, path)
                continue
            if os.path.isfile(legacy_path) or os.path.exists(data_path):
                continue
            todo.append(path)
        return todo

    def prepare_f0_caches(self, device="cuda", files_per_batch: int = 16, rank: int = 0, world: int = 1,
                          tracker_factory=None):
        """Label every listed file without a valid cache with the native backend chain and write its cache.
        Whole files are read, packed, resampled to ``self.sr`` in one ragged launch per batch and tracked in a fixed
        number of launches per batch.  Each native entry runs its own tracker class (``PraatACTracker`` for praat /
        parselmouth, ``WorldDioTracker`` for a pyworld entry with ``algorithm: dio``), in the chain's order;
        ``tracker_factory(sr, hop, **config)`` replaces all of them (a test's stub).  Returns the files labelled."""
        if not self._native_f0:
            raise RuntimeError("prepare_f0_caches: f0_params enables no praat / parselmouth backend; the other "
                               "backends are outside this build")
        for name, btype, cfg in self._f0_chain:
            if f0_tracker.native_backend(btype, cfg) is None:
                logger.warning("[MelDataset] F0 backend '%s' (%s) is not part of this build: skipped", name, btype)
        todo = self.files_to_label(rank, world)
        if not todo:
            return []
        hop = int(self.mel_params["hop_length"])
        trackers = [(name, (tracker_factory or getattr(f0_tracker, cls))(self.sr, hop, **cfg))
                    for name, cls, cfg in self._native_f0]
        resampler = RaggedResampler(self.sr)
        done = []
        for lo in range(0, len(todo), max(int(files_per_batch), 1)):
            paths, waves, rates = [], [], []
            for path in todo[lo:lo + max(int(files_per_batch), 1)]:
                try:
                    wave, wave_sr = read_wav(path)
                except (RuntimeError, OSError, ValueError, struct.error) as exc:
                    logger.warning("[MelDataset] Skipping unreadable audio file: %s (%s)", path, exc)
                    continue
                if wave.ndim > 1:
                    wave = np.mean(wave, axis=-1)
                paths.append(path)
                waves.append(np.ascontiguousarray(wave, dtype=np.float32))
                rates.append(int(wave_sr))
            if not paths:
                continue
            lengths = [int(w.shape[0]) for w in waves]
            flat = torch.from_numpy(np.concatenate(waves)).to(device)
            if any(r != self.sr for r in rates):
                flat, _ = resampler(flat, rates, lengths)                  # (B, width), each row at its own rate
                lengths = [resampler.out_len(r, n) for r, n in zip(rates, lengths)]
            result = [(np.zeros((0,), dtype=np.float32), "")] * len(paths)
            pending = list(range(len(paths)))
            for name, tracker in trackers:
                if not pending:
                    break
                if flat.dim() == 2:
                    sub, sub_len = flat[pending].contiguous(), [lengths[i] for i in pending]
                elif len(pending) == len(paths):
                    sub, sub_len = flat, lengths
                else:
                    off = np.concatenate([[0], np.cumsum(lengths)])
                    sub = torch.cat([flat[off[i]:off[i + 1]] for i in pending])
                    sub_len = [lengths[i] for i in pending]
                contours = tracker.track(sub, sub_len)
                still = []
                for i, f0 in zip(pending, contours):
                    f0 = np.asarray(f0, dtype=np.float32)
                    if np.count_nonzero(f0) < self.bad_F0:                 # f0_backends.py:776-782
                        logger.warning("Backend '%s' returned only %d voiced frames for %s; attempting next backend.",
                                       name, int(np.count_nonzero(f0)), paths[i])
                        still.append(i)
                    else:
                        result[i] = (f0, name)
                pending = still
            for i in pending:
                logger.warning("All configured F0 backends failed for %s", paths[i])
            for path, (f0, name) in zip(paths, result):
                try:
                    self._save_f0_cache(path, f0, name)
                    done.append(path)
                except OSError as exc:
                    logger.warning("Failed to cache F0 for %s: %s", path, exc)
        if self.verbose:
            print(f"[MelDataset] F0 labels written for {len(done)} file(s) "
                  f"(backends: {', '.join(n for n, _, _ in self._native_f0)})")
        return done

    def _f0_for(self, path, waveform, start_sample, expected_frames):
        cached = self._load_cached_f0(path)
        if cached is not None:
            if expected_frames is None:
                return cached
            hop = max(int(self.mel_params["hop_length"]), 1)
            lo = max(0, int(math.floor(start_sample / float(hop))))              # meldataset.py:532-537
            if lo >= cached.shape[0]:
                return np.zeros((0,), dtype=np.float32)
            return cached[lo:min(cached.shape[0], lo + int(expected_frames) + 4)]
        if self.f0_provider is not None:
            return np.asarray(self.f0_provider(path, waveform, self.sr), dtype=np.float32)
        raise RuntimeError(f"no F0 labels for {path}: no valid '{os.path.basename(path)}{self.f0_cache_suffix}' "
                           "(+ .json) cache, no legacy '_f0.npy' and no f0_provider (of the reference's tracker "
                           "backends only praat / parselmouth with method 'ac' and pyworld with algorithm 'dio' are "
                           "part of this build)")

    # ---- cached spectrograms (meldataset.py:679-741), read-only ------------------------------
    def _build_mel_metadata(self, num_samples: int, wave_sr: int) -> dict:
        """meldataset.py:679-701 for the mono float waveform handed to ``_build_training_example``."""
        def plain(v):
            if isinstance(v, np.ndarray):
                return v.tolist()
            if isinstance(v, np.generic):
                return v.item()
            if isinstance(v, torch.Tensor):
                v = v.detach().cpu()
                return v.item() if v.numel() == 1 else v.tolist()
            return v
        return {"audio_sample_rate": int(wave_sr), "audio_num_samples": int(num_samples), "audio_num_channels": 1,
                "dataset_sample_rate": int(self.sr), "mel_params": {k: plain(v) for k, v in self.mel_params.items()}}

    def _mel_cache_paths(self, path):
        return path + self._mel_cache_suffix, path + self._mel_meta_suffix

    def _load_cached_mel(self, path, expected_metadata):
        """meldataset.py:706-741: the cached power-mel (n_mels, L) if its metadata file equals
        ``expected_metadata``; None otherwise.  Nothing is deleted."""
        if not self._cache_enabled or self.data_augmentation:
            return None
        mel_path, meta_path = self._mel_cache_paths(path)
        if not os.path.isfile(mel_path):
            return None
        why = None
        if not os.path.isfile(meta_path):
            why = "has no metadata file"
        else:
            try:
                with open(meta_path, "r", encoding="utf-8") as fh:
                    cached = json.load(fh)
            except (OSError, json.JSONDecodeError):
                cached, why = None, "has unreadable metadata"
            if why is None and cached != expected_metadata:
                why = "was computed for other audio / mel parameters"
        if why is None:
            try:
                mel = np.load(mel_path)
                if mel.ndim == 2 and mel.shape[0] == int(self.mel_params["n_mels"]):
                    return np.ascontiguousarray(mel, dtype=np.float32)
                why = f"has shape {mel.shape}"
            except (OSError, ValueError):
                why = "is unreadable"
        if not self._mel_cache_warned:          # once per dataset, like the reference's one-shot invalidation
            self._mel_cache_warned = True
            logger.warning("[MelDataset] mel cache %s %s: skipped, the device recomputes it (the reference would clear "
                           "the dataset's caches here)", mel_path, why)
        return None

    # ---- one item -------------------------------------------------------------------------
    def _metadata(self, path):
        md = self._audio_metadata_cache.get(path)
        if md is None:
            frames, sr, ch = wav_info(path)
            md = {"frames": frames, "sample_rate": sr, "channels": ch}
            self._audio_metadata_cache[path] = md
        return md

    def path_to_wave_and_label(self, path):
        """Everything of meldataset.py:178-245 + :629-677 except the mel transform itself.
        Returns (waveform f32 (N,), f0 (L,), is_silence (L,), crop_start) with L = min(mel_len, 192)."""
        md = self._metadata(path)
        hop = int(self.mel_params["hop_length"])
        win = int(self.mel_params.get("win_length") or self.mel_params.get("n_fft", hop))
        start, seg, full = segment_plan(int(md["frames"]), md["sample_rate"], self.sr, hop, win,
                                        int(self.max_mel_length))
        wave, wave_sr = read_wav(path, start, seg)
        if wave.ndim > 1:
            wave = np.mean(wave, axis=-1)
        wave = wave.astype(np.float32)
        # the device resamples; everything below only needs the resampled LENGTH: ceil(new * L / orig)
        n_target = Resampler(wave_sr, self.sr).out_len(len(wave)) if wave_sr != self.sr else len(wave)
        start_sample = 0 if full else int(round(start / float(md["sample_rate"]) * self.sr))
        expected = None if full else int(np.ceil(n_target / max(hop, 1))) + 2
        f0 = self._f0_for(path, wave, start_sample, expected)
        if self.data_augmentation:
            wave = (0.5 + 0.5 * np.random.random()) * wave                        # meldataset.py:232-234
            wave = wave.astype(np.float32)
        mel_len = 1 + n_target // hop
        # meldataset.py:236-237,640-642: whole-file items without augmentation may come from the spectrogram cache
        self._last_cached_mel = None
        if full and not self.data_augmentation:
            cached = self._load_cached_mel(path, self._build_mel_metadata(n_target, self.sr))
            if cached is not None:
                mel_len = cached.shape[1]                                         # meldataset.py:651
                self._last_cached_mel = cached
        f0 = align_length(f0, mel_len)
        sil = (f0 == 0).astype(np.float32)
        crop = 0
        if mel_len > self.max_mel_length:
            crop = int(np.random.randint(0, mel_len - self.max_mel_length))       # meldataset.py:668-672
            f0 = f0[crop:crop + self.max_mel_length]
            sil = sil[crop:crop + self.max_mel_length]
        f0 = np.where(np.isnan(f0), np.float32(self.zero_value), f0).astype(np.float32)
        self._last_sr = wave_sr
        if self._last_cached_mel is not None:
            # meldataset.py:650,668-670 in the reference's own float32 torch arithmetic, on the host
            m = (torch.log(LOG_EPS + torch.from_numpy(self._last_cached_mel)) - self.mean) / self.std
            self._last_cached_mel = m[:, crop:crop + self.max_mel_length].contiguous()
        return wave, f0, sil, crop

    def __getitem__(self, idx):
        if self.synthetic_enabled and idx >= self._base_length:
            return self._generate_synthetic_sample()
        total = len(self.data_list)
        if total == 0:
            raise IndexError("MelDataset is empty")
        for attempt in range(total):
            path = self.data_list[(idx + attempt) % total]
            if path in self._invalid_paths:
                continue
            try:
                wave, f0, sil, crop = self.path_to_wave_and_label(path)
            except (FileNotFoundError, RuntimeError, OSError, ValueError, struct.error) as exc:
                if isinstance(exc, NotImplementedError):
                    raise
                self._invalid_paths.add(path)
                logger.warning("[MelDataset] Skipping unreadable audio file: %s (%s)", path, exc)
                continue
            item = (torch.from_numpy(wave), torch.from_numpy(f0), torch.from_numpy(sil), crop, int(self._last_sr))
            return item if self._last_cached_mel is None else item + (self._last_cached_mel,)
        raise RuntimeError("No valid audio files could be loaded from the dataset")

    def path_to_mel_and_label(self, path, device="cuda"):
        """Reference-shaped single item: (mel (80, L<=192) normalised log-mel on the device, f0, is_silence)."""
        wave, f0, sil, crop = self.path_to_wave_and_label(path)
        if self._last_cached_mel is not None:
            return self._last_cached_mel.to(device), torch.from_numpy(f0), torch.from_numpy(sil)
        wave_dev = torch.from_numpy(wave).to(device)
        if self._last_sr != self.sr:
            wave_dev = Resampler(self._last_sr, self.sr)(wave_dev)
        mel = self.to_melspec(wave_dev)
        mel = (torch.log(LOG_EPS + mel) - self.mean) / self.std
        return mel[:, crop:crop + self.max_mel_length], torch.from_numpy(f0), torch.from_numpy(sil)


class Collater(object):
    """Zero-pads items to 192 frames (meldataset.py:790-826).

    Accepts the reference's ``(mel (80,L), f0, is_silence)`` items, or this build's raw-audio items
    ``(wave (N,), f0, is_silence, crop_start[, source_sr[, cached_mel (80,L<=192)]])``; for the latter it returns
    host tensors ``(waves (B,Nmax), lengths, crop_starts, f0s, is_silences, source_sr)`` for the device mel stage,
    where ``source_sr`` is the batch's one source rate (``int``, 0 if unknown) or, when its items carry different
    rates, an int32 ``(B,)`` tensor of per-row rates (0 for an item without one),
    followed by ``(cached_rows (K,), cached_mels (K,80,192))`` when any item carries a cached spectrogram, then by one
    ``Batch`` per synthetic kind with items in the batch (their last element is the kind's ``Request``), in the order of
    ``synthetic_items.KINDS``: pitch shift, WORLD vocoder, WORLD resynthesis.  A synthetic row's waveform is left zero
    (the device writes its window there) and its length is that window's; the rest travels in the kind's ``Batch``."""

    def __init__(self, return_wave=False):
        self.return_wave = return_wave
        self.min_mel_length = MAX_MEL_LENGTH
        self.max_mel_length = MAX_MEL_LENGTH

    def __call__(self, batch):
        B = len(batch)
        L = self.max_mel_length
        f0s = torch.zeros((B, L)).float()
        sils = torch.zeros((B, L)).float()
        if len(batch[0]) == 3:
            n_mels = batch[0][0].size(0)
            mels = torch.zeros((B, n_mels, L), dtype=torch.float32, device=batch[0][0].device)
            for i, (mel, f0, sil) in enumerate(batch):
                n = mel.size(1)
                mels[i, :, :n] = mel
                f0s[i, :n] = f0
                sils[i, :n] = sil
            return mels.unsqueeze(1), f0s, sils
        rows_of = {}                                   # type of an item's last element -> rows, in one pass
        for i, item in enumerate(batch):
            rows_of.setdefault(type(item[-1]), []).append(i)
        kinds = [kind for kind in synthetic_items.KINDS if kind.Request in rows_of]
        synthetic = {i for kind in kinds for i in rows_of[kind.Request]}
        n_max = max(int(item[-1].out_len) if i in synthetic else int(item[0].shape[0])
                    for i, item in enumerate(batch))
        waves = torch.zeros((B, n_max), dtype=torch.float32)
        lengths = torch.zeros((B,), dtype=torch.int32)
        crops = torch.zeros((B,), dtype=torch.int32)
        row_rates = [int(item[4]) if len(item) > 4 else 0 for item in batch]
        rates = {int(item[4]) for item in batch if len(item) > 4}
        mixed = len(rates) > 1
        for i, item in enumerate(batch):
            wave, f0, sil, crop = item[:4]
            if i in synthetic:
                n = item[-1].out_len
            else:
                n = wave.shape[0]
                waves[i, :n] = wave
            lengths[i] = n
            crops[i] = int(crop)
            f0s[i, :f0.shape[0]] = f0
            sils[i, :sil.shape[0]] = sil
        source_sr = torch.tensor(row_rates, dtype=torch.int32) if mixed else (rates.pop() if rates else 0)
        out = (waves, lengths, crops, f0s, sils, source_sr)
        rows = [i for i, item in enumerate(batch) if len(item) > 5 and torch.is_tensor(item[5])]
        if rows:                                       # normalised, cropped cache rows, zero-padded like :812-816
            cached = torch.zeros((len(rows), batch[rows[0]][5].shape[0], L), dtype=torch.float32)
            for k, i in enumerate(rows):
                m = batch[i][5]
                cached[k, :, :m.shape[1]] = m
            out += (torch.tensor(rows, dtype=torch.int64), cached)
        return out + tuple(kind.collate(batch, rows_of[kind.Request], row_rates, mixed) for kind in kinds)


class H2DPrefetcher:
    """Host->device copies on a side HIP stream so the next batch's raw audio (49 MB at B = 256) crosses PCIe
    underneath the current step.  ``submit`` starts the copies of a tuple of (pinned) host tensors and returns a
    ticket; ``acquire`` makes the compute stream wait for that ticket only.  ``stream``: issue the copies from an
    existing stream instead of a private one -- data-parallel runs pass the model's weight-gradient side stream, which
    is idle during the forward pass when the next batch is submitted, because those runs cap the HIP hardware queues
    at three (compute, side, RCCL) and a fourth stream would share one of them (+1.7 ms per step, measured)."""

    def __init__(self, device, stream=None):
        self.device = torch.device(device)
        self.stream = stream if stream is not None else torch.cuda.Stream(device=self.device)

    def submit(self, host_items):
        def to_dev(t):
            return t.to(self.device, non_blocking=True) if torch.is_tensor(t) else t
        with torch.cuda.stream(self.stream):
            # a tuple among the items is a synthetic kind's Batch: rebuilt field by field, as pin_memory does
            dev = tuple(type(t)(*map(to_dev, t)) if isinstance(t, tuple) else to_dev(t) for t in host_items)
            ready = torch.cuda.Event()
            ready.record(self.stream)
        return dev, ready

    def acquire(self, ticket):
        dev, ready = ticket
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ready)
        for t in dev:
            for x in (t if isinstance(t, tuple) else (t,)):
                if torch.is_tensor(x) and x.is_cuda:
                    x.record_stream(cur)          # allocated on the side stream, consumed on the compute stream
        return dev


class DeviceMelLoader:
    """Iterates a host DataLoader of raw-audio batches and yields the reference's batch tuple
    ``(mels (B,1,80,192), f0s, is_silences)`` with the mel computed on the GPU in one launch."""

    def __init__(self, loader: DataLoader, mel: MelSpectrogram, device, augmenter=None, modulator=None):
        self.loader, self.mel, self.device = loader, mel, torch.device(device)
        self.dataset = loader.dataset
        self.augmenter = augmenter                 # augment.Augmenter or None: the stage ahead of the mel launch
        self.modulator = modulator                 # pitch_mod.PitchModulator or None: the stage ahead of the Augmenter
        self._ragged = RaggedResampler(mel.sample_rate)
        self._h2d, self._host = None, []

    def __len__(self):
        return len(self.loader)

    def set_epoch(self, epoch: int):
        """Data-parallel runs: re-seed the cross-rank permutation (distributed.EpochShardSampler)."""
        sampler = getattr(self.loader, "sampler", None)
        if hasattr(sampler, "set_epoch"):
            sampler.set_epoch(epoch)

    def _run_stage(self, kind, waves, lengths, dev_batch, host_batch, src_sr):
        """One synthetic kind's device stage: ``waves`` widened to the kind's largest window, the kind's ``run``, then
        its rows' lengths set to their windows'."""
        need = int(host_batch.out_len.max())
        if waves.shape[1] < need:
            waves = torch.nn.functional.pad(waves, (0, need - waves.shape[1]))
        waves, lengths = kind.run(self, waves.contiguous(), lengths, dev_batch, host_batch, src_sr)
        return waves, lengths.index_copy(0, dev_batch.rows, dev_batch.out_len.to(torch.int32))

    def _submit(self, host):
        """Start a collated batch's copies on the side stream -> ticket for ``_finish``.  What ``_finish`` reads on the
        host waits in a FIFO: (lengths, per-row rates or None, {Batch type: host batch}, crops, cached-mel rows)."""
        if self._h2d is None:
            from . import distributed as pdist
            shared = None
            if torch.distributed.is_available() and torch.distributed.is_initialized() and \
                    (torch.distributed.get_world_size() > 1 or pdist.rehearse_single_rank()):
                from .model import _side_stream
                shared = _side_stream(self.device)
            self._h2d = H2DPrefetcher(self.device, stream=shared)
        self._host.append((host[1].tolist(), host[5].tolist() if torch.is_tensor(host[5]) else None,
                           {type(t): t for t in host[6:] if isinstance(t, tuple)}, host[2].tolist(),
                           host[6].tolist() if len(host) > 6 and torch.is_tensor(host[6]) else []))
        return self._h2d.submit(host)

    def _finish(self, ticket):
        waves, lengths, crops, f0s, sils, src_sr, *rest = self._h2d.acquire(ticket)
        host_lengths, host_rates, host_batches, host_crops, cached_rows = self._host.pop(0)
        batches = {type(t): (t, host_batches[type(t)]) for t in rest if type(t) in host_batches}
        cached = [t for t in rest if type(t) not in host_batches]
        sr = self.mel.sample_rate
        rates = host_rates if host_rates is not None else [src_sr] * len(host_lengths)
        if any(r and r != sr for r in rates):
            # one ragged launch, each row at its own rate and bit-identical to that item resampled alone; synthetic
            # rows are left zero (length 0): their stages write them, and resample their base files themselves
            synthetic = {i for t in host_batches.values() for i in t.rows.tolist()}
            host_lengths = [0 if i in synthetic else int(n) for i, n in enumerate(host_lengths)]
            waves, lengths = self._ragged(waves, [r or sr for r in rates], host_lengths)
            host_lengths = [self._ragged.out_len(r or sr, n) for r, n in zip(rates, host_lengths)]
        for kind in synthetic_items.KINDS:                    # after the resampler, before the one mel launch
            if kind.Batch in batches:
                waves, lengths = self._run_stage(kind, waves, lengths, *batches[kind.Batch], src_sr)
        staged = (self.modulator is not None and self.modulator.active) or \
            (self.augmenter is not None and self.augmenter.active)
        if staged:
            # the whole rows at their lengths after the stages above
            synthetic = [i for t in host_batches.values() for i in t.rows.tolist()]
            for t in host_batches.values():
                for i, n in zip(t.rows.tolist(), t.out_len.tolist()):
                    host_lengths[i] = int(n)
        if self.modulator is not None and self.modulator.active:
            # the time warp moves the labels with the audio; reverb and noise then land on the modulated voice.  Rows
            # with a cached spectrogram keep it, so they and their labels are left alone
            mod_plan = self.modulator.draw(len(host_lengths)).without(cached_rows)
            if synthetic and not self.modulator.config["apply_to_synthetic"]:
                mod_plan = mod_plan.without(synthetic)
            waves, f0s, sils = self.modulator.apply(waves, host_lengths, host_crops, f0s, sils, mod_plan)
        if self.augmenter is not None and self.augmenter.active:
            # labels, crops and cached mels are not touched
            plan = self.augmenter.draw(len(host_lengths))
            if synthetic and not self.augmenter.config["apply_to_synthetic"]:
                plan = plan.without(synthetic)
            waves = self.augmenter.apply(waves, host_lengths, plan)
        mels = self.mel.log_mel_ragged(waves, lengths, crops, max_frames=MAX_MEL_LENGTH)
        if cached:                                            # rows whose spectrogram came from <wav>_mel.npy
            rows, cached_mels = cached
            mels[:, 0].index_copy_(0, rows, cached_mels)
        return mels, f0s, sils

    def __iter__(self):
        """Double-buffered: batch k+1's H2D is in flight on the side stream while batch k is being consumed."""
        self._host.clear()
        pending = None
        for host in self.loader:
            ticket = self._submit(host)
            if pending is not None:
                yield self._finish(pending)
            pending = ticket
        if pending is not None:
            yield self._finish(pending)


def build_dataloader(path_list, validation=False, batch_size=4, num_workers=1, device="cpu", collate_config=None,
                     dataset_config=None, shard=None):
    """Reference signature (meldataset.py:829-875) plus ``shard=(rank, world, seed)`` for data-parallel runs:
    the loader then draws its indices from ``distributed.EpochShardSampler`` (equal contiguous per-rank shards
    of a per-epoch permutation) instead of the single-process shuffle."""
    dataset_config = dict(dataset_config or {})
    dataloader_options = dataset_config.pop("dataloader", {}) or {}
    augmentation = dataset_config.pop("augmentation", None)      # the device stage's block: the dataset never sees it
    pitch_modulation = dataset_config.pop("pitch_modulation", None)       # likewise
    if torch.device(device).type != "cuda":
        raise RuntimeError("build_dataloader (HIP path): device must be a HIP ('cuda') device; the mel stage has "
                           "no CPU fallback")
    dataset = MelDataset(path_list, validation=validation, **dataset_config)
    if dataset.has_native_f0:
        # label pass: once, in this process, before any worker exists (workers only ever read caches); in
        # data-parallel runs every rank labels its share of the files and the ranks meet before the first batch
        rank, world = (int(shard[0]), int(shard[1])) if shard is not None else (0, 1)
        dataset.prepare_f0_caches(device, files_per_batch=int(dataloader_options.get("f0_files_per_batch", 16)),
                                  rank=rank, world=world)
        if world > 1 and torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.barrier()
    collate_fn = Collater(**(collate_config or {}))
    kwargs = dict(batch_size=batch_size, shuffle=(not validation), num_workers=num_workers,
                  drop_last=(not validation), collate_fn=collate_fn, pin_memory=True)
    if shard is not None:
        from .distributed import EpochShardSampler
        rank, world, seed = shard
        kwargs["sampler"] = EpochShardSampler(len(dataset), batch_size, rank, world, seed=seed,
                                              shuffle=(not validation), drop_last=(not validation))
        kwargs["shuffle"] = False
    start_method = dataloader_options.get("start_method")
    if start_method and num_workers > 0:
        kwargs["multiprocessing_context"] = torch.multiprocessing.get_context(start_method)
    if dataloader_options.get("persistent_workers") is not None and num_workers > 0:
        kwargs["persistent_workers"] = bool(dataloader_options["persistent_workers"])
    if dataloader_options.get("prefetch_factor") is not None and num_workers > 0:
        kwargs["prefetch_factor"] = int(dataloader_options["prefetch_factor"])
    augmenter = None
    if augmentation is not None:
        from .augment import Augmenter
        augmenter = Augmenter(augmentation, dataset.sr, seed=int((augmentation or {}).get("seed", 0)),
                              rank=int(shard[0]) if shard is not None else 0)
        if not augmenter.active or (validation and not augmenter.config["apply_to_validation"]):
            augmenter = None
        else:
            augmenter.prepare(device)
    modulator = None
    if pitch_modulation is not None:
        from .pitch_mod import PitchModulator
        modulator = PitchModulator(pitch_modulation, dataset.sr, dataset.to_melspec.hop_length,
                                   seed=int((pitch_modulation or {}).get("seed", 0)),
                                   rank=int(shard[0]) if shard is not None else 0)
        if not modulator.active or (validation and not modulator.config["apply_to_validation"]):
            modulator = None
    return DeviceMelLoader(DataLoader(dataset, **kwargs), dataset.to_melspec, device, augmenter, modulator)
