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

from . import ops, ragged
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


def load_model(checkpoint_path, device="cuda", sequence_model_config: dict | None = None, frozen=False) -> JDCNet:
    """Build a ``JDCNet`` for a reference-format checkpoint ({"model": state_dict, ...} or a bare state dict),
    load it non-strictly and put it in eval mode on ``device``.  ``frozen``: also ``requires_grad_(False)``, the
    form a loss network takes (StyleTTS / StarGANv2-VC): a backward through it then computes the gradient with respect to
    its input and nothing else (``JDCNet.is_frozen``)."""
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
    model = model.to(device).eval()
    return model.requires_grad_(False) if frozen else model


def waveform_to_mel(audio, mel_transform: MelSpectrogram | None = None, device="cuda") -> torch.Tensor:
    """(N,) float audio at the model rate -> (n_mels, L) normalised log-mel on the device."""
    tf = mel_transform or MelSpectrogram(**DEFAULT_MEL_PARAMS)
    wave = torch.as_tensor(np.asarray(audio, dtype=np.float32)).to(device)
    return _normalised_log(tf(wave))


def f0_from_wave(model: JDCNet, waves: torch.Tensor, lengths: torch.Tensor | None = None,
                 mel_transform: MelSpectrogram | None = None, *, max_frames: int | None = None,
                 frame_start: torch.Tensor | None = None, sample_rate: int | None = None, rates=None):
    """The model's outputs for (B, N) float32 device audio with the autograd graph intact: ``log_mel_batch`` (or
    ``log_mel_ragged`` with int32 device ``lengths``), the transpose to the model's (B, 1, T, n_mels) input, the
    model.  With a frozen ``model`` (``load_model(..., frozen=True)``) and ``waves`` that require grad, a loss on the
    result back-propagates to the waveform through native kernels only (the F0 loss of something that emits audio).
    ``max_frames``: frames per row, padded or truncated (default: the frames of N samples).

    Audio at another rate than the mel transform's: ``sample_rate=R`` for (B, N) rows all at rate ``R`` (``Resampler``
    to the model rate, then ``log_mel_batch``), or ``rates=[...]`` with ``lengths`` as host sequences for a batch
    that mixes rates, padded (B, N) or packed 1-D (``RaggedResampler``, then ``log_mel_ragged`` on the resampler's
    ``out_lengths``).  Both resamplers are differentiable, so the gradient reaches the audio at its own rate.
    ``max_frames`` then defaults to the frames of the longest resampled row."""
    tf = mel_transform or _default_mel()
    if sample_rate is not None and rates is not None:
        raise ValueError("f0_from_wave: give sample_rate (one rate) or rates (one per row), not both")
    if sample_rate is not None:
        if lengths is not None:
            raise ValueError("f0_from_wave: sample_rate takes whole rows; pass rates= with lengths for ragged rows")
        waves = _resampler(int(sample_rate), tf.sample_rate)(waves)
    elif rates is not None:
        if lengths is None or isinstance(lengths, torch.Tensor) and lengths.is_cuda:
            raise ValueError("f0_from_wave: rates needs the rows' lengths as a host sequence")
        waves, lengths = _ragged_resampler(tf.sample_rate)(waves, rates, [int(n) for n in lengths])
    T = int(max_frames) if max_frames is not None else tf.num_frames(waves.shape[1])
    if lengths is None:
        mel = tf.log_mel_batch(waves, max_frames=T)
    else:
        mel = tf.log_mel_ragged(waves, lengths, frame_start, max_frames=T)
    return model(mel.transpose(-1, -2))


def _normalised_log(mel: torch.Tensor) -> torch.Tensor:
    """meldataset.py:650 as the notebooks apply it to a mel power tensor."""
    return (torch.log(mel + LOG_EPS) - MEL_MEAN) / MEL_STD


def _silence_cut(p) -> float:
    """logit(p), the detector logit above which ``sigmoid(z) > p``."""
    p = float(p)
    return -np.inf if p <= 0.0 else (np.inf if p >= 1.0 else float(np.log(p) - np.log1p(-p)))


def _check_decoding(model, decoder, silence_threshold, return_confidence):
    if decoder is not None and decoder not in ops.F0_DECODERS:
        raise ValueError(f"decoder must be one of {ops.F0_DECODERS}, got {decoder!r}")
    if decoder is not None and model.num_class == 1:
        raise ValueError("decoder: the model is a regression model (num_class == 1), there are no bins to decode")
    if return_confidence and decoder is None:
        raise ValueError("return_confidence needs a decoder")
    if silence_threshold is not None and decoder is None and model.num_class != 1:
        raise ValueError("silence_threshold on a classifier needs a decoder")


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
    ``return_confidence=True`` returns ``(f0, confidence)``, confidence = softmax(frame)[decoded bin].

    A Transformer model needs ``chunk_size % 4 == 0`` and ``chunk_size <= max_len`` (its positional table); the
    model raises otherwise."""
    _check_decoding(model, decoder, silence_threshold, return_confidence)
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
            hz = torch.where(sil.reshape(hz.shape) > _silence_cut(silence_threshold), torch.zeros_like(hz), hz)
        hz = hz.cpu().numpy()
        out = np.concatenate([hz[i][:e] for i, e in enumerate(ends)])
        if not return_confidence:
            return out
        conf = conf.cpu().numpy()
        return out, np.concatenate([conf[i][:e] for i, e in enumerate(ends)])
    f0 = f0[..., 0].cpu().numpy() if f0.shape[-1] == 1 else f0.cpu().numpy()
    return np.concatenate([f0[i][:min(s + chunk_size, total) - s] for i, s in enumerate(starts)])

# ---------------------------------------------------------------------------------------- batched ragged inference
STITCH_MODES = ("concat", "center", "crossfade")
# columns of a stitch run (include/pitchextractor_hip.h, pe_stitch_chunks)
RUN_A, RUN_FA, RUN_DST, RUN_LEN, RUN_NOV, RUN_J0, RUN_B, RUN_FB = range(8)


def _row_runs(starts, ends, n_frames, chunk_size, stitch):
    """``(kept, runs)`` of one row: the chunks (indices into ``starts``) that own an output frame, and its stitch runs
    as 8-column rows whose chunk columns count in ``kept`` and whose destination counts from the row's first frame."""
    K = len(starts)
    runs = []
    if K == 0:
        return [], runs
    if stitch == "concat":
        at = 0
        for k in range(K):
            runs.append((k, 0, at, ends[k] - starts[k], 0, 0, 0, 0))
            at += ends[k] - starts[k]
        return list(range(K)), runs
    if stitch == "center":
        owner = np.zeros(n_frames, np.int64)
        best = np.full(n_frames, np.iinfo(np.int64).max, np.int64)
        for k in range(K):                              # ascending k and a strict "<": ties go to the smaller k
            t = np.arange(starts[k], ends[k], dtype=np.int64)
            cost = np.abs(2 * (t - starts[k]) - (chunk_size - 1))
            win = cost < best[starts[k]:ends[k]]
            owner[starts[k]:ends[k]][win] = k
            best[starts[k]:ends[k]][win] = cost[win]
        cuts = [0] + (np.flatnonzero(np.diff(owner)) + 1).tolist() + [n_frames]
        kept = sorted(set(owner.tolist()))
        index = {k: i for i, k in enumerate(kept)}
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            k = int(owner[lo])
            runs.append((index[k], lo - starts[k], lo, hi - lo, 0, 0, 0, 0))
        return kept, runs
    for k in range(K):                                  # crossfade: a chunk's own frames, then its seam with the next
        lo = max(starts[k], ends[k - 1]) if k else starts[k]
        hi = min(ends[k], starts[k + 1]) if k + 1 < K else ends[k]
        if hi > lo:
            runs.append((k, lo - starts[k], lo, hi - lo, 0, 0, 0, 0))
        if k + 1 < K and ends[k] > starts[k + 1]:
            n_ov = ends[k] - starts[k + 1]
            runs.append((k, starts[k + 1] - starts[k], starts[k + 1], n_ov, n_ov, 0, k + 1, 0))
    return list(range(K)), runs


def chunk_plan(n_frames, chunk_size: int = 192, overlap: int = 48, stitch: str = "concat", *, sample_offsets=None,
               sample_counts=None) -> dict:
    """Host plan of chunked inference over rows of ``n_frames`` mel frames (an int, or one per row).

    Chunks start every ``max(chunk_size - overlap, 1)`` frames from 0 (the notebook's rule) and chunk k is valid over
    ``[s_k, e_k)``, ``e_k = min(s_k + chunk_size, n_frames)``.  ``stitch`` makes a row's output of them:
    "concat", the valid frames of every chunk back to back (``sum(e_k - s_k)`` values, ``overlap`` frames repeated at
    every seam); "center", ``n_frames`` values, frame t copied from the covering chunk that minimises
    ``|2 (t - s_k) - (chunk_size - 1)|`` (ties: the smaller k), chunks that own no frame left out; "crossfade"
    (``2 * overlap <= chunk_size``), ``n_frames`` values, the ``n_ov = e_k - s_{k+1}`` frames two chunks share
    blended as ``a + w (b - a)``, ``w = (j + 1) / (n_ov + 1)`` for the j-th of them, the others copied.

    Returns ``rows`` (per row: ``starts``, ``valid``, ``kept``, ``out_len``, ``out_offset``, ``chunks`` and ``runs``
    as (first, end) positions in the two tables) and, for the batch in row-major order, ``meta`` (n_chunks, 3) int64
    {sample offset, sample count (``sample_offsets`` / ``sample_counts`` per row; 0 without), first frame},
    ``chunk_valid`` (n_chunks,), ``runs`` (n_runs, 8) int64 {chunk, frame in it, destination, length, n_ov, first j,
    second chunk, frame in it} with rows packed back to back in the destination, and ``n_out``."""
    chunk_size, overlap = int(chunk_size), int(overlap)
    if stitch not in STITCH_MODES:
        raise ValueError(f"stitch must be one of {STITCH_MODES}, got {stitch!r}")
    if chunk_size < 1 or not 0 <= overlap < chunk_size:
        raise ValueError("chunk_plan: need chunk_size >= 1 and 0 <= overlap < chunk_size")
    if stitch == "crossfade" and 2 * overlap > chunk_size:
        raise ValueError("chunk_plan: crossfade needs 2 * overlap <= chunk_size (at most two chunks per frame)")
    frames = [int(n_frames)] if np.ndim(n_frames) == 0 else [int(n) for n in n_frames]
    if any(n < 0 for n in frames):
        raise ValueError("chunk_plan: a frame count is negative")
    R = len(frames)
    offs = np.zeros(R, np.int64) if sample_offsets is None else ragged.i64(sample_offsets)
    counts = np.zeros(R, np.int64) if sample_counts is None else ragged.i64(sample_counts)
    if offs.size != R or counts.size != R:
        raise ValueError("chunk_plan: one sample offset and one sample count per row")
    step = max(chunk_size - overlap, 1)
    rows, meta, valid, runs = [], [], [], []
    n_out = 0
    for r, L in enumerate(frames):
        starts = list(range(0, L, step))
        ends = [min(s + chunk_size, L) for s in starts]
        kept, row_runs = _row_runs(starts, ends, L, chunk_size, stitch)
        out_len = sum(run[RUN_LEN] for run in row_runs)
        base = len(meta)
        rows.append(dict(starts=starts, valid=[e - s for s, e in zip(starts, ends)], kept=kept, out_len=out_len,
                         out_offset=n_out, chunks=(base, base + len(kept)), runs=(len(runs), len(runs) + len(row_runs))))
        meta += [(offs[r], counts[r], starts[k]) for k in kept]
        valid += [ends[k] - starts[k] for k in kept]
        runs += [(a + base, fa, dst + n_out, n, n_ov, j0, b + base if n_ov else 0, fb)
                 for a, fa, dst, n, n_ov, j0, b, fb in row_runs]
        n_out += out_len
    return dict(rows=rows, n_out=n_out, chunk_size=chunk_size, overlap=overlap, stitch=stitch,
                meta=np.array(meta, np.int64).reshape(-1, 3), chunk_valid=np.array(valid, np.int64),
                runs=np.array(runs, np.int64).reshape(-1, 8))


def _moved_runs(plan: dict, order, dst_starts) -> np.ndarray:
    """The stitch runs of rows ``order`` with row ``order[i]`` written from destination frame ``dst_starts[i]``
    (ascending) instead of its packed place."""
    parts = []
    for r, at in zip(order, dst_starts):
        row = plan["rows"][r]
        part = plan["runs"][row["runs"][0]:row["runs"][1]].copy()
        part[:, RUN_DST] += at - row["out_offset"]
        parts.append(part)
    return np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, 8), np.int64)


def _length_groups(lengths, row_bytes: int, budget: int):
    """Rows in order of length cut into groups whose padded size ``rows * longest * row_bytes`` stays within ``budget``
    (a row that is over it alone is a group of its own)."""
    order = sorted(range(len(lengths)), key=lambda r: (lengths[r], r))
    groups, cur = [], []
    for r in order:
        if cur and (len(cur) + 1) * lengths[r] * row_bytes > budget:
            groups.append(cur)
            cur = []
        cur.append(r)
    return groups + ([cur] if cur else [])


_DEFAULT_MEL = None


def _default_mel() -> MelSpectrogram:
    global _DEFAULT_MEL
    if _DEFAULT_MEL is None:
        _DEFAULT_MEL = MelSpectrogram(**DEFAULT_MEL_PARAMS)
    return _DEFAULT_MEL


_RESAMPLERS: dict = {}


def _resampler(orig: int, target: int):
    """The cached ``Resampler(orig, target)`` (its plan owns a device table)."""
    from .resample import Resampler
    if (orig, target) not in _RESAMPLERS:
        _RESAMPLERS[orig, target] = Resampler(orig, target)
    return _RESAMPLERS[orig, target]


def _ragged_resampler(target: int):
    from .resample import RaggedResampler
    if target not in _RESAMPLERS:
        _RESAMPLERS[target] = RaggedResampler(target)
    return _RESAMPLERS[target]


def mel_chunks(waves, plan: dict, mel_transform: MelSpectrogram | None = None) -> torch.Tensor:
    """The model input ``(n_chunks, 1, chunk_size, n_mels)`` of a ``chunk_plan`` with its device copy (``meta_d``): one
    launch writes the mel power of every chunk of every row in that layout (``ops.mel_forward_chunks``), zero past a
    row's frames; log and normalisation are then ``waveform_to_mel``'s own expression, in place of the kernel's fused
    form, whose logarithm rounds differently -- so a chunk is, bit for bit, a slice of ``waveform_to_mel`` of its row
    alone, which is what makes the batched path comparable with the notebook's on the same chunks."""
    tf = mel_transform or _default_mel()
    x = ops.mel_forward_chunks(tf, waves, plan["meta"], plan["meta_d"], plan["chunk_size"], log=False)
    valid = torch.from_numpy(plan["chunk_valid"]).to(x.device)
    frame = torch.arange(plan["chunk_size"], device=x.device)
    return _normalised_log(x).masked_fill_((frame[None, :] >= valid[:, None])[:, None, :, None], 0.0)


def _stitch(x, runs, n_dst, det=None):
    """``ops.stitch_chunks`` into a fresh destination of ``n_dst`` frames: ``(out, det_out)``."""
    out = torch.empty((n_dst,) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    det_out = None if det is None else torch.empty((n_dst,), dtype=torch.float32, device=x.device)
    ops.stitch_chunks(x, runs, torch.from_numpy(runs).to(x.device), out, det, det_out)
    return out, det_out


@torch.no_grad()
def predict_f0_batch(model: JDCNet, waves, lengths=None, *, chunk_size: int = 192, overlap: int = 48,
                     stitch: str = "center", max_chunks: int = 256, mel_transform: MelSpectrogram | None = None,
                     decoder: str | None = None, silence_threshold: float | None = None,
                     return_confidence: bool = False, group_bytes: int = 1 << 30):
    """``predict_f0`` for a whole ragged batch without leaving the device, and with a choice of how chunks become a
    row (``chunk_plan``): the default "center" returns one value per mel frame.

    ``waves`` is float32 device audio at the model rate in the layouts of ``ragged.device_plan`` (one 1-D wave, packed
    rows with ``lengths``, padded 2-D rows) or a list of numpy arrays, uploaded once.  One launch takes the mel of
    every chunk of every row into the model's input layout (``mel_chunks``), the model runs in eval mode over
    consecutive sub-batches of at most ``max_chunks`` chunks (row-major), one launch stitches.  Returns one device
    tensor per row, views of one buffer: Hz for a regression model, the stitched ``(L, num_class)`` logits for a
    classifier without a ``decoder``.
    With a ``decoder`` and "concat" every chunk is decoded on its own as in ``predict_f0``; with "center" or
    "crossfade" a row's stitched logits are ONE sequence for ``ops.decode_f0_bins``, so a Viterbi path crosses seams
    (rows go through it in padded groups by length of at most ``group_bytes``).  ``silence_threshold`` and
    ``return_confidence`` as in ``predict_f0``, on the stitched detector logit.  A chunk's output depends at rounding
    level on the chunks that share its forward (the h2 products scale by tensor maxima), so the result is not
    bit-equal to a ``predict_f0`` loop in any mode.  A Transformer model needs ``chunk_size % 4 == 0`` and
    ``chunk_size <= max_len`` (its positional table); the model raises otherwise."""
    _check_decoding(model, decoder, silence_threshold, return_confidence)
    device = model.flat_parameters.device
    if isinstance(waves, (list, tuple)):
        host = [np.ascontiguousarray(np.asarray(w, dtype=np.float32).reshape(-1)) for w in waves]
        if not host:
            return ([], []) if return_confidence else []
        lengths = [int(w.size) for w in host]
        waves = torch.from_numpy(np.concatenate(host)).to(device)
    tf = mel_transform or _default_mel()
    frames = []

    def plan(row_lengths, offsets):
        if any(n <= tf.n_fft // 2 for n in row_lengths):
            raise ValueError(f"predict_f0_batch: a row has at most n_fft / 2 = {tf.n_fft // 2} samples; the mel front "
                             "end cannot reflect-pad it")
        frames[:] = [tf.num_frames(n) for n in row_lengths]
        return chunk_plan(frames, chunk_size, overlap, stitch, sample_offsets=offsets, sample_counts=row_lengths)

    pl = ragged.device_plan(waves, lengths, plan, "predict_f0_batch")
    rows, n_chunks, C = pl["rows"], int(pl["meta"].shape[0]), model.num_class
    if not rows:
        return ([], []) if return_confidence else []
    mel = mel_chunks(waves, pl, tf)

    was_training = model.training
    model.eval()
    max_chunks = max(int(max_chunks), 1)
    logits = det = None
    if n_chunks > max_chunks:
        logits = torch.empty((n_chunks, chunk_size, C), dtype=torch.float32, device=device)
        det = torch.empty((n_chunks, chunk_size), dtype=torch.float32, device=device)
    for lo in range(0, n_chunks, max_chunks):
        x = mel[lo:lo + max_chunks]
        f0, sil = model(x)
        if ops.persistent_lstm_error(device):          # a timed-out group barrier voids the outputs: redo
            ops.clear_persistent_lstm_error(device)
            ops.USE_PERSISTENT_LSTM = False
            f0, sil = model(x)
        if logits is None:
            logits, det = f0.detach().reshape(n_chunks, chunk_size, C), sil.detach().reshape(n_chunks, chunk_size)
        else:
            logits[lo:lo + max_chunks] = f0.reshape(-1, chunk_size, C)
            det[lo:lo + max_chunks] = sil.reshape(-1, chunk_size)
    if was_training:
        model.train()
    logits, det = logits.contiguous(), det.contiguous()

    gate = None if silence_threshold is None else _silence_cut(silence_threshold)
    want_det = det if gate is not None else None
    conf = None
    if decoder is None:
        out, sil = _stitch(logits, pl["runs"], pl["n_out"], want_det)
        hz = out[:, 0] if C == 1 else out
        offsets = [row["out_offset"] for row in rows]
    elif stitch == "concat":
        valid = torch.from_numpy(pl["chunk_valid"].astype(np.int32)).to(device)
        hz, conf, _ = ops.decode_f0_bins(logits, valid, decoder)
        hz, sil = _stitch(hz, pl["runs"], pl["n_out"], want_det)
        if return_confidence:
            conf, _ = _stitch(conf, pl["runs"], pl["n_out"])
        offsets = [row["out_offset"] for row in rows]
    else:
        # one sequence per row: padded groups by length for the decoder, gathered into one packed buffer group by group
        n_out = pl["n_out"]
        hz = torch.empty((n_out,), dtype=torch.float32, device=device)
        conf = torch.empty((n_out,), dtype=torch.float32, device=device) if return_confidence else None
        sil = None
        offsets = [0] * len(rows)
        at = 0
        for group in _length_groups(frames, 4 * C, int(group_bytes)):
            G, width = len(group), max(frames[r] for r in group)
            runs = _moved_runs(pl, group, [i * width for i in range(G)])
            padded, sil_g = _stitch(logits, runs, G * width, want_det)
            row_frames = torch.tensor([frames[r] for r in group], dtype=torch.int32, device=device)
            hz_g, conf_g, _ = ops.decode_f0_bins(padded.view(G, width, C), row_frames, decoder)
            if gate is not None:
                hz_g = torch.where(sil_g.view(G, width) > gate, torch.zeros_like(hz_g), hz_g)
            gather = np.zeros((G, 8), np.int64)
            total = 0
            for i, r in enumerate(group):
                gather[i, [RUN_A, RUN_DST, RUN_LEN]] = (i, total, frames[r])
                offsets[r] = at + total
                total += frames[r]
            gather_d = torch.from_numpy(gather).to(device)
            ops.stitch_chunks(hz_g, gather, gather_d, hz[at:at + total])
            if return_confidence:
                ops.stitch_chunks(conf_g, gather, gather_d, conf[at:at + total])
            at += total
        gate = None                                    # applied per group above
    if gate is not None:
        hz = torch.where(sil > gate, torch.zeros_like(hz), hz)
    out_rows = [hz[o:o + row["out_len"]] for o, row in zip(offsets, rows)]
    if not return_confidence:
        return out_rows
    return out_rows, [conf[o:o + row["out_len"]] for o, row in zip(offsets, rows)]


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
                 batched: bool = False, **predict_kwargs) -> dict:
    """The notebooks' sweep: ``items`` (``{"audio", "reference_f0"}`` each, arrays or device tensors, at the model rate
    ``sr``, default the mel front end's) are scored clean, then every ``stress.Condition`` degrades the whole set as one
    ragged batch on the device and each degraded row goes through ``predict_f0`` (``predict_kwargs``: its keyword
    arguments; a classifier needs a ``decoder``).  Returns ``{"baseline": [...], "conditions": [...]}``: one record per item, and
    one per (condition, item) in order, each ``{"condition", "kind", "item"}`` plus ``melody_metrics``; a condition's
    ``VUV_flips`` is measured against the item's clean prediction, the baseline's own is 0.  ``batched=True``: the
    clean set and every degraded set go through ``predict_f0_batch(..., stitch="concat")`` without leaving the device;
    the records keep their shape, the predictions differ from the per-row ones at rounding level."""
    from . import stress
    device = model.flat_parameters.device
    sr = int(sr or DEFAULT_MEL_PARAMS["sample_rate"])

    def track(x):                                       # device tensors (``stimuli.StimulusSet.items``) stay there
        if isinstance(x, torch.Tensor):
            return x.detach().reshape(-1).to(device, torch.float32)
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1)))

    items = list(items)
    waves = [track(it["audio"]) for it in items]
    refs = [track(it["reference_f0"]) for it in items]
    lengths = [int(w.numel()) for w in waves]
    batch = torch.zeros((len(waves), max(lengths, default=0)), dtype=torch.float32, device=device)
    for r, w in enumerate(waves):
        batch[r, :w.numel()] = w.to(device)

    def run(rows, row_lengths):
        if batched:
            return predict_f0_batch(model, rows, row_lengths, **{"stitch": "concat", **predict_kwargs})
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


SUMMARY_METRICS = ("RPA", "RCA", "VUV", "OctaveError")
_LOWER_IS_BETTER = ("OctaveError",)


def summarize_with_drop(records, baseline_records, group_keys, metrics=SUMMARY_METRICS) -> list:
    """The summary table the evaluation notebooks print under every sweep (Utils/codec_and_bandwidth_torture.ipynb's
    ``_summarize_with_drop``), on the host: the records (of ``stress_sweep`` or any list of dicts) grouped by
    ``group_keys``, one row per group in order of first appearance with the group's keys and per metric
    ``<metric>_mean`` (NaN left out), ``<metric>_std`` (NaN left out, ddof 1, NaN below two values) and
    ``<metric>_drop`` against the NaN-skipping mean over ``baseline_records``: baseline - mean where higher is better,
    mean - baseline for ``OctaveError``."""
    group_keys = [group_keys] if isinstance(group_keys, str) else list(group_keys)

    def column(rows, metric):
        vals = np.asarray([float(r[metric]) for r in rows], dtype=np.float64)
        return vals[~np.isnan(vals)]

    baseline = {}
    for metric in metrics:
        vals = column(baseline_records, metric)
        baseline[metric] = float(np.mean(vals)) if vals.size else float("nan")
    groups = {}
    for rec in records:
        groups.setdefault(tuple(rec[k] for k in group_keys), []).append(rec)
    table = []
    for key, rows in groups.items():
        line = dict(zip(group_keys, key))
        for metric in metrics:
            vals = column(rows, metric)
            line[metric + "_mean"] = float(np.mean(vals)) if vals.size else float("nan")
            line[metric + "_std"] = float(np.std(vals, ddof=1)) if vals.size >= 2 else float("nan")
        for metric in metrics:
            mean = line[metric + "_mean"]
            line[metric + "_drop"] = mean - baseline[metric] if metric in _LOWER_IS_BETTER else baseline[metric] - mean
        table.append(line)
    return table


def noise_sweep(model: JDCNet, items, snrs_db=(30, 20, 10, 5, 0, -5), sources=("white", "pink", "brown"), seed=0,
                batched: bool = True, **predict_kwargs) -> dict:
    """The noise-robustness curve (what the reference's Utils/noise_robustness_evaluation.ipynb is meant to draw): one
    ``stress.Condition("additive_noise", ...)`` per (source, SNR), sources outermost, run by ``stress_sweep`` (its
    ``items``, ``batched`` and other keyword arguments).  ``sources``: colour names or custom colours of
    ``noise.colour_sections``, ``noise.NoiseSet`` beds, or ``(name, source)`` pairs; item r of every condition draws its
    noise from ``seed + r``.  Returns ``stress_sweep``'s dict, whose condition records also carry ``source`` and
    ``snr_db``, plus ``"summary"``: ``summarize_with_drop`` of them by ``("source", "snr_db")``."""
    from . import stress
    conditions, labels = [], {}
    for k, source in enumerate(sources):
        if isinstance(source, tuple) and len(source) == 2 and isinstance(source[0], str):
            name, source = source
        else:
            name = source if isinstance(source, str) else f"source {k}"
        for snr in snrs_db:
            cond = stress.Condition("additive_noise", f"{name} {float(snr):g} dB", snr_db=float(snr), source=source,
                                    seed=seed)
            conditions.append(cond)
            labels[cond.label] = (name, float(snr))
    if len(labels) != len(conditions):
        raise ValueError("noise_sweep: two conditions share a source name and an SNR")
    out = stress_sweep(model, items, conditions, batched=batched, **predict_kwargs)
    for rec in out["conditions"]:
        rec["source"], rec["snr_db"] = labels[rec["condition"]]
    out["summary"] = summarize_with_drop(out["conditions"], out["baseline"], ("source", "snr_db"))
    return out


def codec_sweep(model: JDCNet, items, bitrates_kbps=(16, 32, 64, 128), codecs=("transform",), frame: int = 1024,
                batched: bool = True, **predict_kwargs) -> dict:
    """The codec sweep of the reference's Utils/codec_and_bandwidth_torture.ipynb with the codecs this project builds
    (``codec.py``): one ``codec.CodecCondition`` per (codec, bitrate), codecs outermost, run by ``stress_sweep`` (its
    ``items``, ``batched`` and other keyword arguments).  ``"transform"`` is the build-defined MDCT codec at every
    bitrate (its kbps are those of its own cost model, not of opus, mp3 or aac); ``"g711u"`` is one condition, G.711
    mu-law at 8 kHz, recorded at 64 kbps.  Returns ``stress_sweep``'s dict, whose condition records also carry
    ``codec`` and ``bitrate_kbps``, plus ``"summary"``: ``summarize_with_drop`` of them by ``("codec",
    "bitrate_kbps")``, the grouping of the notebook's table."""
    from .codec import CodecCondition
    conditions, labels = [], {}
    for name in codecs:
        if name == "g711u":
            conditions.append(CodecCondition("g711u 64 kbps", codec="g711u"))
        else:
            conditions += [CodecCondition(f"{name} {float(kbps):g} kbps", codec=name, bitrate_kbps=float(kbps),
                                          frame=frame) for kbps in bitrates_kbps]
    for cond in conditions:
        labels[cond.label] = (cond.codec, cond.bitrate_kbps)
    if len(labels) != len(conditions):
        raise ValueError("codec_sweep: two conditions share a codec and a bitrate")
    out = stress_sweep(model, items, conditions, batched=batched, **predict_kwargs)
    for rec in out["conditions"]:
        rec["codec"], rec["bitrate_kbps"] = labels[rec["condition"]]
    out["summary"] = summarize_with_drop(out["conditions"], out["baseline"], ("codec", "bitrate_kbps"))
    return out


# ------------------------------------------------------------------------------------------- synthesized-stimulus sweeps
def _score_set(model, st, stitch, voicing_threshold_hz, predict_kwargs):
    """One ``predict_f0_batch`` call over a ``stimuli.StimulusSet`` and its scores: ``(melody metrics, dynamic
    metrics)``, the reference sampled at each prediction's own length as the notebooks do."""
    from . import stimuli, stress
    if model.num_class != 1 and predict_kwargs.get("decoder") is None:
        raise ValueError("a classifier needs a decoder (predict_kwargs) to be scored in Hz")
    device = model.flat_parameters.device
    preds = predict_f0_batch(model, st.audio, st.lengths, **{"stitch": stitch, **predict_kwargs})
    refs = st.reference_f0([int(p.numel()) for p in preds])
    melody = stress.melody_metrics_rows(preds, refs, None, voicing_threshold_hz, device)
    return melody, stimuli.dynamic_metrics_rows(preds, refs, device)


def _frame_period_ms(predict_kwargs, sr) -> float:
    tf = predict_kwargs.get("mel_transform") or _default_mel()
    return tf.hop_length * 1000.0 / sr


_MELODY_COLUMNS = ("RPA", "RCA", "VUV", "OctaveError")


@torch.no_grad()
def dynamic_pitch_sweep(model: JDCNet, *, sr: int | None = None, vibrato: dict | None = None, glide: dict | None = None,
                        stitch: str = "concat", voicing_threshold_hz: float = 10.0, **predict_kwargs) -> dict:
    """Utils/dynamic_pitch_behavior.ipynb without the host touching a sample: the vibrato grid and the glides are
    synthesized on the device (``stimuli.vibratos``, ``stimuli.glides``; ``vibrato`` / ``glide``: the notebook's CONFIG
    sections, default ``stimuli.VIBRATO_GRID`` / ``stimuli.GLIDE_GRID``), each set is one ``predict_f0_batch`` call
    (``stitch="concat"`` is the notebooks' ``predict_f0``; ``predict_kwargs``: its other keyword arguments, a classifier
    needs a ``decoder``) and the reference is sampled at the prediction's own length.  Returns ``{"vibrato": [...],
    "glide": [...]}`` with the notebook's columns: ``rate_hz, depth_cents, RPA, RCA, VUV, OctaveError, RMSE_cents`` and
    ``duration_s, RPA, RCA, VUV, OctaveError, RMSE_cents, Lag_ms, Overshoot_cents, Final_error_cents``."""
    from . import stimuli
    device = model.flat_parameters.device
    sr = int(sr or DEFAULT_MEL_PARAMS["sample_rate"])
    v, g = {**stimuli.VIBRATO_GRID, **(vibrato or {})}, {**stimuli.GLIDE_GRID, **(glide or {})}
    period = _frame_period_ms(predict_kwargs, sr)
    out = {"vibrato": [], "glide": []}
    st = stimuli.vibratos([float(r) for r in v["rates_hz"]], [float(d) for d in v["depth_cents"]],
                          float(v["base_frequency_hz"]), float(v["duration_seconds"]), sr, device=device)
    melody, dynamic = _score_set(model, st, stitch, voicing_threshold_hz, predict_kwargs)
    for label, m, d in zip(st.labels, melody, dynamic):
        out["vibrato"].append(dict(rate_hz=label["rate_hz"], depth_cents=label["depth_cents"],
                                   **{k: m[k] for k in _MELODY_COLUMNS}, RMSE_cents=d["RMSE_cents"]))
    st = stimuli.glides([float(d) for d in g["durations_seconds"]], float(g["start_hz"]), float(g["end_hz"]), sr,
                        device=device)
    melody, dynamic = _score_set(model, st, stitch, voicing_threshold_hz, predict_kwargs)
    for label, m, d in zip(st.labels, melody, dynamic):
        out["glide"].append(dict(duration_s=label["duration_s"], **{k: m[k] for k in _MELODY_COLUMNS},
                                 RMSE_cents=d["RMSE_cents"], Lag_ms=d["Lag_frames"] * period,
                                 Overshoot_cents=d["Overshoot_cents"], Final_error_cents=d["Final_error_cents"]))
    return out


@torch.no_grad()
def timbre_coverage_sweep(model: JDCNet, *, sr: int | None = None, ranges=None, profiles: dict | None = None,
                          duration: float | None = None, frequencies_per_range: int | None = None,
                          edge_band_fraction: float | None = None, seed: int | None = None, noise: str = "numpy",
                          stitch: str = "concat", voicing_threshold_hz: float = 10.0, **predict_kwargs) -> dict:
    """Utils/pitch_range_and_timbre_coverage.ipynb on the device: every range x frequency x timbre profile is one row of
    one ``stimuli.timbre_tones`` set (the notebook's order, so the noisy profile draws the notebook's noise), scored by
    one ``predict_f0_batch`` call.  Defaults: ``stimuli.VOCAL_RANGES``, ``stimuli.TIMBRE_PROFILES``,
    ``stimuli.TIMBRE_STIMULUS``.  Returns ``{"records": [...], "per_range": {...}}``: records with the notebook's columns
    ``range, frequency_hz, timbre, edge_region, RPA, RCA, VUV, OctaveError``, and per range the means
    ``RPA_mean, RCA_mean, VUV_mean, OctaveError_mean`` (NaN records left out, as a data frame's mean leaves them)."""
    from . import stimuli
    device = model.flat_parameters.device
    sr = int(sr or DEFAULT_MEL_PARAMS["sample_rate"])
    cfg = stimuli.TIMBRE_STIMULUS
    ranges = stimuli.VOCAL_RANGES if ranges is None else ranges
    count = int(cfg["frequencies_per_range"] if frequencies_per_range is None else frequencies_per_range)
    fraction = float(cfg["edge_band_fraction"] if edge_band_fraction is None else edge_band_fraction)
    freqs, labels = [], []
    for rng in ranges:
        lo, hi = float(rng["min_hz"]), float(rng["max_hz"])
        for f in stimuli.frequency_grid(lo, hi, count):
            freqs.append(float(f))
            labels.append({"range": rng["name"], "edge_region": stimuli.edge_region(float(f), lo, hi, fraction)})
    st = stimuli.timbre_tones(freqs, profiles, float(cfg["duration_seconds"] if duration is None else duration), sr,
                              int(cfg["random_seed"] if seed is None else seed), noise, device=device, labels=labels)
    melody, _ = _score_set(model, st, stitch, voicing_threshold_hz, predict_kwargs)
    records = [dict(range=label["range"], frequency_hz=label["frequency_hz"], timbre=label["timbre"],
                    edge_region=label["edge_region"], **{k: m[k] for k in _MELODY_COLUMNS})
               for label, m in zip(st.labels, melody)]
    per_range = {}
    for rng in ranges:
        rows = [r for r in records if r["range"] == rng["name"]]
        means = {}
        for k in _MELODY_COLUMNS:
            vals = [r[k] for r in rows if not np.isnan(r[k])]
            means[k + "_mean"] = float(np.mean(vals)) if vals else float("nan")
        per_range[rng["name"]] = means
    return {"records": records, "per_range": per_range}
