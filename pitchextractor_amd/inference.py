"""Inference recipe of the reference's evaluation notebooks (Utils/dynamic_pitch_behavior.ipynb, code
cell 5: ``load_model`` / ``waveform_to_mel`` / ``predict_f0``) on the HIP path.

``predict_f0`` keeps the notebook's semantics exactly -- mel -> chunks of ``chunk_size`` frames every
``chunk_size - overlap`` frames, the last chunk zero-padded, every chunk contributing its first
``end - start`` predictions, overlaps NOT blended (so the result is longer than the frame count) -- but
runs all chunks of an utterance as ONE batch through the network instead of one forward per chunk
(eval-mode BatchNorm makes samples independent, bit for bit).
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import torch

from . import ops
from .mel import DEFAULT_MEL_PARAMS, LOG_EPS, MEL_MEAN, MEL_STD, MelSpectrogram
from .model import JDCNet


def infer_model_config(model_state: dict) -> tuple[int, dict]:
    """(num_class, sequence_model_config) read off a reference-format ``state_dict``."""
    num_class = int(model_state["classifier.weight"].shape[0]) if "classifier.weight" in model_state else 722
    keys = list(model_state)
    if any(k.startswith("sequence_classifier.model.weight_ih_l") for k in keys):
        layers = 1 + max(int(re.search(r"weight_ih_l(\d+)", k).group(1)) for k in keys
                         if k.startswith("sequence_classifier.model.weight_ih_l"))
        hidden = int(model_state["sequence_classifier.model.weight_hh_l0"].shape[1])
        bidir = "sequence_classifier.model.weight_ih_l0_reverse" in model_state
        cfg = {"model_type": "bilstm", "hidden_size": hidden, "num_layers": layers, "bidirectional": bidir}
    elif any(k.startswith("sequence_classifier.model.layers.") for k in keys):
        layers = 1 + max(int(re.search(r"layers\.(\d+)\.", k).group(1)) for k in keys
                         if k.startswith("sequence_classifier.model.layers."))
        ff = int(model_state["sequence_classifier.model.layers.0.linear1.weight"].shape[0])
        max_len = int(model_state["sequence_classifier.pos_encoding.pe"].shape[1])
        cfg = {"model_type": "transformer", "num_layers": layers, "dim_feedforward": ff, "max_len": max_len,
               "nhead": 8}
    else:
        raise RuntimeError("checkpoint has neither a BiLSTM nor a Transformer temporal head")
    return num_class, cfg


def load_model(checkpoint_path, device="cuda", sequence_model_config: dict | None = None) -> JDCNet:
    """Build a ``JDCNet`` for a reference-format checkpoint ({"model": state_dict, ...} or a bare state dict),
    load it non-strictly and put it in eval mode on ``device``."""
    path = Path(checkpoint_path)
    if not path.is_file():
        raise FileNotFoundError(f"Checkpoint not found: {path}")
    blob = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(blob, dict):
        raise RuntimeError("Unexpected checkpoint format")
    state = blob.get("model", blob.get("state_dict", blob))
    if not isinstance(state, dict):
        raise RuntimeError("Checkpoint is missing a valid model state")
    num_class, cfg = infer_model_config(state)
    cfg.update(sequence_model_config or {})
    model = JDCNet(num_class=num_class, sequence_model_config=cfg)
    model.load_state_dict(state, strict=False)
    return model.to(device).eval()


def waveform_to_mel(audio, mel_transform: MelSpectrogram | None = None, device="cuda") -> torch.Tensor:
    """(N,) float audio at the model rate -> (n_mels, L) normalised log-mel on the device."""
    tf = mel_transform or MelSpectrogram(**DEFAULT_MEL_PARAMS)
    wave = torch.as_tensor(np.asarray(audio, dtype=np.float32)).to(device)
    mel = tf(wave)
    return (torch.log(mel + LOG_EPS) - MEL_MEAN) / MEL_STD


@torch.no_grad()
def predict_f0(model: JDCNet, audio, chunk_size: int = 192, overlap: int = 48,
               mel_transform: MelSpectrogram | None = None, *, decoder: str | None = None,
               silence_threshold: float | None = None, return_confidence: bool = False):
    """The notebook's recipe.  With the keyword arguments left alone it returns what the notebook returns: Hz for a
    regression model (``num_class == 1``), the raw ``(frames, num_class)`` logits otherwise.

    ``decoder`` ("argmax", "weighted", "viterbi", "weighted_viterbi"; ``ops.decode_f0_bins``) turns a classifier's
    logits into Hz on the device: every chunk is one sequence of ``end - start`` frames (chunks are independent and
    the un-blended concatenation repeats ``overlap`` frames at each seam, so no path runs across seams), all chunks
    are decoded in one call and concatenated as the Hz of a regression model are.  ``silence_threshold=p`` returns
    0 Hz where ``sigmoid(detector logit) > p`` (the detector head predicts ``is_silence``).
    ``return_confidence=True`` returns ``(f0, confidence)``, confidence = softmax(frame)[decoded bin]."""
    if decoder is not None and decoder not in ops.F0_DECODERS:
        raise ValueError(f"decoder must be one of {ops.F0_DECODERS}, got {decoder!r}")
    if decoder is not None and model.num_class == 1:
        raise ValueError("decoder: the model is a regression model (num_class == 1), there are no bins to decode")
    if return_confidence and decoder is None:
        raise ValueError("return_confidence needs a decoder")
    if silence_threshold is not None and decoder is None and model.num_class != 1:
        raise ValueError("silence_threshold on a classifier needs a decoder")
    device = model.flat_parameters.device
    mel = waveform_to_mel(audio, mel_transform, device)
    total = mel.shape[-1]
    step = max(chunk_size - overlap, 1)
    starts = list(range(0, total, step))
    if not starts:
        return np.zeros((0,), dtype=np.float32)
    batch = torch.zeros((len(starts), 1, mel.shape[0], chunk_size), dtype=torch.float32, device=device)
    for i, s in enumerate(starts):
        e = min(s + chunk_size, total)
        batch[i, 0, :, :e - s] = mel[:, s:e]
    was_training = model.training
    model.eval()
    f0, sil = model(batch.transpose(-1, -2))
    if ops.persistent_lstm_error(device):          # a timed-out group barrier voids the outputs: redo on the safe kernels
        ops.clear_persistent_lstm_error(device)
        ops.USE_PERSISTENT_LSTM = False
        f0, sil = model(batch.transpose(-1, -2))
    if was_training:
        model.train()
    if decoder is not None or silence_threshold is not None:
        ends = [min(s + chunk_size, total) - s for s in starts]
        conf = None
        if decoder is not None:
            lengths = torch.tensor(ends, dtype=torch.int32, device=device)
            hz, conf, _ = ops.decode_f0_bins(f0.detach().contiguous(), lengths, decoder)
        else:
            hz = f0[..., 0]
        if silence_threshold is not None:
            # sigmoid(z) > p  <=>  z > logit(p); the comparison is exact, the zeros are written on the device
            p = float(silence_threshold)
            cut = -np.inf if p <= 0.0 else (np.inf if p >= 1.0 else float(np.log(p) - np.log1p(-p)))
            hz = torch.where(sil.reshape(hz.shape) > cut, torch.zeros_like(hz), hz)
        hz = hz.cpu().numpy()
        out = np.concatenate([hz[i][:e] for i, e in enumerate(ends)])
        if not return_confidence:
            return out
        conf = conf.cpu().numpy()
        return out, np.concatenate([conf[i][:e] for i, e in enumerate(ends)])
    f0 = f0[..., 0].cpu().numpy() if f0.shape[-1] == 1 else f0.cpu().numpy()
    return np.concatenate([f0[i][:min(s + chunk_size, total) - s] for i, s in enumerate(starts)])


_TRACKERS = {}


def track_f0(wave, *, sr: int, hop_length: int, device="cuda", backend: str = "praat", **config) -> np.ndarray:
    """F0 contour (Hz, 0 = unvoiced; float32) of one wave at ``sr`` by an on-device tracker: ``backend="praat"``, the
    Praat-style autocorrelation tracker (``f0_tracker.PraatACTracker``; ``config``: the reference's ``praat`` backend
    keys), or ``backend="dio"``, WORLD's DIO + StoneMask (``f0_tracker.WorldDioTracker``; the ``pyworld`` keys).  One
    value every ``hop_length / sr`` seconds -- praat: over the frames whose window lies inside the wave; dio: from
    time 0 -- not the mel frame count: ``pitch_metrics(predict_f0(...), align_length(track_f0(...), L))`` scores a
    model against it."""
    from .f0_tracker import NATIVE_BACKENDS
    classes = {row.key: row.tracker for row in NATIVE_BACKENDS}
    if backend not in classes:
        raise ValueError(f"track_f0: backend {backend!r} is not one of {sorted(classes)}")
    key = (backend, int(sr), int(hop_length), tuple(sorted((k, str(v)) for k, v in config.items())))
    if key not in _TRACKERS:
        _TRACKERS[key] = classes[backend](sr, hop_length, **config)
    if isinstance(wave, torch.Tensor):
        w = wave.detach().reshape(-1).to(device, torch.float32).contiguous()
    else:
        w = torch.from_numpy(np.ascontiguousarray(np.asarray(wave, dtype=np.float32).reshape(-1))).to(device)
    return _TRACKERS[key].track(w)[0]


def pitch_metrics(f0_pred, f0_ref, *, threshold_cents: float = 50.0, device="cuda") -> dict:
    """How far a predicted F0 track (Hz, 0 = unvoiced) is from a reference track, over their first ``min(len)``
    frames, reduced on the device.  Device tensors or arrays.  With ``voiced = f0_ref > 0`` and cents re 55 Hz:

    * ``rms_cents``: the reference's ``rms_cents_error`` (Utils/dynamic_pitch_tools.py:92-104): RMS cents error over
      the voiced frames, the prediction clipped below at 1e-5; NaN when no frame is voiced;
    * ``rpa``: share of voiced frames predicted within ``threshold_cents`` (a predicted 0 Hz is a miss);
      ``rca``: the same on ``circular_cents_distance`` (octave errors forgiven);
    * ``vuv_error``: share of all frames whose voicing decision differs; ``n_voiced``, ``n_frames``."""
    def as_track(x):
        if isinstance(x, torch.Tensor):
            return x.detach().reshape(-1)
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1)))

    pred, ref = as_track(f0_pred), as_track(f0_ref)
    n = min(pred.numel(), ref.numel())
    nan = float("nan")
    if n == 0:
        return dict(rms_cents=nan, rpa=nan, rca=nan, vuv_error=nan, n_voiced=0, n_frames=0)
    dev = pred.device if pred.is_cuda else (ref.device if ref.is_cuda else torch.device(device))
    pred = pred[:n].to(dev, torch.float32).contiguous()
    ref = ref[:n].to(dev, torch.float32).contiguous()
    out = ops.pitch_metrics(pred, ref, threshold_cents).cpu().tolist()
    return dict(rms_cents=out[0], rpa=out[1], rca=out[2], vuv_error=out[3], n_voiced=int(out[4]),
                n_frames=int(out[5]))


def melody_metrics(pred, ref, baseline=None, voicing_threshold_hz: float = 10.0, device="cuda") -> dict:
    """The evaluation notebooks' ``compute_metrics`` (e.g. Utils/room_and_microphone_stress.ipynb) of one predicted
    track against its reference over their first ``min(len)`` frames, reduced on the device in double:
    ``{RPA, RCA, VUV, OctaveError, VUV_flips, n_voiced, n_frames}``.  ``voiced = ref > 0``, predicted voiced =
    ``pred > voicing_threshold_hz``; cents re 55 Hz with the prediction clipped below at 1e-5; RPA / RCA: share of
    voiced frames within 50 cents (RCA: on the circular distance); VUV: share of frames whose voicing agrees;
    OctaveError: share of voiced frames that miss but lie within 50 cents of a non-zero whole number of octaves.  The
    three shares over voiced frames are NaN when none is voiced.  ``VUV_flips`` (Utils/amplitude_pathologies.ipynb):
    share of frames whose predicted voicing differs from ``baseline``'s (the clean run's prediction); NaN without one."""
    from .stress import melody_metrics_rows
    return melody_metrics_rows([pred], [ref], None if baseline is None else [baseline], voicing_threshold_hz, device)[0]


@torch.no_grad()
def stress_sweep(model: JDCNet, items, conditions, *, sr: int | None = None, voicing_threshold_hz: float = 10.0,
                 **predict_kwargs) -> dict:
    """The notebooks' sweep: ``items`` (a list of ``{"audio", "reference_f0"}`` at the model rate ``sr``, default the
    mel front end's) are scored clean, then every ``stress.Condition`` degrades the whole set as one ragged batch on
    the device and each degraded row goes through ``predict_f0`` (``predict_kwargs``: its keyword arguments; a
    classifier needs a ``decoder``).  Returns ``{"baseline": [...], "conditions": [...]}``: one record per item, and
    one per (condition, item) in order, each ``{"condition", "kind", "item"}`` plus ``melody_metrics``; a condition's
    ``VUV_flips`` is measured against the item's clean prediction, the baseline's own is 0."""
    from . import stress
    device = model.flat_parameters.device
    sr = int(sr or DEFAULT_MEL_PARAMS["sample_rate"])
    waves = [np.ascontiguousarray(np.asarray(it["audio"], dtype=np.float32).reshape(-1)) for it in items]
    refs = [np.asarray(it["reference_f0"], dtype=np.float32).reshape(-1) for it in items]
    lengths = [int(w.size) for w in waves]
    batch = torch.zeros((len(waves), max(lengths, default=0)), dtype=torch.float32, device=device)
    for r, w in enumerate(waves):
        batch[r, :w.size] = torch.from_numpy(w).to(device)

    def run(rows, row_lengths):
        return [np.asarray(predict_f0(model, rows[r, :n].cpu().numpy(), **predict_kwargs), dtype=np.float32)
                for r, n in enumerate(row_lengths)]

    def records(cond, preds):
        ms = stress.melody_metrics_rows(preds, refs, clean, voicing_threshold_hz, device) if preds else []
        return [dict(condition=cond.label if cond else "clean", kind=cond.kind if cond else "clean", item=i, **m)
                for i, m in enumerate(ms)]

    clean = run(batch, lengths)
    out = {"baseline": records(None, clean), "conditions": []}
    for cond in conditions:
        degraded, row_lengths = stress.apply_condition(cond, batch, sr, lengths)
        out["conditions"] += records(cond, run(degraded, row_lengths))
    return out
