"""Synthesized evaluation stimuli of the reference's notebooks on the device (``csrc/stimuli.hip``): the glides and the
vibrato grid of Utils/dynamic_pitch_behavior.ipynb (``Utils/dynamic_pitch_tools.py``), the harmonic tones of
Utils/pitch_range_and_timbre_coverage.ipynb, the clean tones of Utils/amplitude_pathologies.ipynb, their analytic
reference at frame rate (``sample_reference_f0``) and the dynamic metrics (``rms_cents_error``,
``estimate_tracking_delay_ms``, ``compute_overshoot_cents``, the final-frame error).  There is no CPU path.
``tests/stimuli_ref.py`` is the float64 restatement that pins every stage.

A builder (``glides``, ``vibratos``, ``tones``, ``from_f0_curves``, ``timbre_tones``) returns a ``StimulusSet``: one
ragged device batch (``audio``, a packed 1-D float32 tensor, and ``lengths``) that goes to
``inference.predict_f0_batch`` as it is, and ``reference_f0(num_frames)``.  The stages (``phase``, ``synth``, ``tone``,
``finish``, ``reference``) are also callable one by one on a ``plan_rows`` plan in any layout; a row's output is
bit-identical whether the row is produced alone, packed at an odd offset or padded, and a stage's launch count does not
depend on the rows.  ``inference.dynamic_pitch_sweep`` and ``inference.timbre_coverage_sweep`` run the notebooks.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, ops
from .noise import STAT_KEYS  # noqa: F401  (the mix at an SNR is one implementation; finish returns its stats)
from .ragged import (check_device_tensor, check_waves, host_ptrs, pack_tracks, per_row, plan_arrays, plan_output,
                     row_layout, to_device, workspace)

KINDS = ("curve", "glide", "vibrato", "tone")
K_CURVE, K_GLIDE, K_VIBRATO, K_TONE = range(4)
MAX_PARTIALS = 16
FADE_TIME = 0.02
# Utils/pitch_range_and_timbre_coverage.ipynb, CONFIG
TIMBRE_PROFILES = {
    "Pure Sine": {"partials": {1: 1.0}},
    "Warm Vocal": {"partials": {1: 1.0, 2: 0.45, 3: 0.2}},
    "Bright Belt": {"partials": {1: 1.0, 2: 0.9, 3: 0.75, 4: 0.5, 5: 0.35}},
    "Breathy Head": {"partials": {1: 1.0, 2: 0.5, 3: 0.35}, "snr_db": 25.0},
}
VOCAL_RANGES = (
    {"name": "Bass", "min_hz": 70.0, "max_hz": 120.0},
    {"name": "Baritone/Tenor", "min_hz": 120.0, "max_hz": 220.0},
    {"name": "Alto", "min_hz": 220.0, "max_hz": 350.0},
    {"name": "Child/Falsetto", "min_hz": 350.0, "max_hz": 1000.0},
)
TIMBRE_STIMULUS = {"duration_seconds": 2.5, "frequencies_per_range": 15, "edge_band_fraction": 0.15,
                   "random_seed": 1337}
# Utils/dynamic_pitch_behavior.ipynb, CONFIG
VIBRATO_GRID = {"base_frequency_hz": 220.0, "duration_seconds": 3.0, "rates_hz": (4.0, 6.0, 8.0),
                "depth_cents": (20.0, 60.0, 120.0, 200.0)}
GLIDE_GRID = {"start_hz": 60.0, "end_hz": 500.0, "durations_seconds": (0.4, 0.8, 1.6, 3.2)}
DYNAMIC_KEYS = ("RMSE_cents", "Lag_frames", "Overshoot_cents", "Final_error_cents")


def fade_samples(sr) -> int:
    """``_apply_fade``'s ``int(max(fade_time * sr, 0))``."""
    return int(max(FADE_TIME * sr, 0))


def num_samples(duration: float, sr) -> int:
    """The reference's ``int(duration * sr)``."""
    return int(duration * sr)


# ------------------------------------------------------------------------------------------------------------ row specs
def _positive(value, what: str) -> float:
    value = float(value)
    if not (math.isfinite(value) and value > 0.0):
        raise ValueError(f"stimuli: {what} must be positive and finite, got {value!r}")
    return value


def _finite(value, what: str) -> float:
    value = float(value)
    if not math.isfinite(value):
        raise ValueError(f"stimuli: {what} must be finite, got {value!r}")
    return value


def _row(kind, n, amplitude, a=0.0, b=0.0, c=0.0, duration=0.0, snr_db=None, partials=(), curve=(0, 0), **label):
    return dict(kind=int(kind), n=int(n), amplitude=_finite(amplitude, "amplitude"), a=float(a), b=float(b), c=float(c),
                duration=_positive(duration, "duration"), snr_db=None if snr_db is None else _finite(snr_db, "snr_db"),
                partials=list(partials), curve=(int(curve[0]), int(curve[1])), label=label)


def glide_row(duration, start_hz, end_hz, sr, amplitude: float = 0.8) -> dict:
    return _row(K_GLIDE, num_samples(duration, sr), amplitude, _positive(start_hz, "start_hz"),
                _positive(end_hz, "end_hz"), duration=duration, duration_s=float(duration))


def vibrato_row(rate_hz, depth_cents, base_hz, duration, sr, amplitude: float = 0.8) -> dict:
    return _row(K_VIBRATO, num_samples(duration, sr), amplitude, _positive(base_hz, "base_hz"),
                _finite(depth_cents, "depth_cents"), _finite(rate_hz, "rate_hz"), duration=duration,
                rate_hz=float(rate_hz), depth_cents=float(depth_cents))


def curve_row(n, sr, amplitude, curve_offset, curve_length, duration=None, **label) -> dict:
    """A row that follows ``curve_length`` (1: a constant tone, else ``n``) float32 values at ``curve_offset`` of the
    curve tensor; its time axis is ``linspace(0, duration, n, endpoint=False)``, ``duration`` defaulting to ``n / sr``."""
    if int(n) < 1:
        raise ValueError("stimuli: a row needs at least one sample")
    duration = int(n) / float(sr) if duration is None else duration
    return _row(K_CURVE, n, amplitude, duration=duration, curve=(curve_offset, curve_length), **label)


def timbre_row(frequency, profile: dict, duration, sr, **label) -> dict:
    """``synthesize_timbre_waveform``'s row: the partials of ``profile`` in dict order without the zero amplitudes,
    noise when it has an ``snr_db``.  A callable ``envelope`` is not built."""
    if callable(profile.get("envelope")):
        raise ValueError("stimuli: a callable envelope is not supported")
    partials = [(float(h), float(a)) for h, a in profile.get("partials", {1: 1.0}).items() if a != 0]
    if not 1 <= len(partials) <= MAX_PARTIALS:
        raise ValueError(f"stimuli: a timbre profile has 1 .. {MAX_PARTIALS} non-zero partials, got {len(partials)}")
    for h, a in partials:
        _finite(h, "harmonic"), _finite(a, "partial amplitude")
    f = _positive(frequency, "frequency")
    return _row(K_TONE, num_samples(duration, sr), 1.0, f, duration=duration, snr_db=profile.get("snr_db"),
                partials=partials, frequency_hz=f, **label)


# ------------------------------------------------------------------------------------------------------------ the plan
def plan_rows(rows, sr, offsets=None) -> dict:
    """``pe_stim_plan`` (host only) of row specs (``glide_row`` ...): the row plan, the derived parameters and the
    constants.  ``offsets``: where each row lies in the output (default: packed).  Rows with noise take their noise
    packed back to back in row order.  ``ValueError`` for a row the reference cannot make: ``n = 0``, ``n`` below the
    fade length, more than 16 partials, a non-positive or non-finite frequency, duration or ``sr``."""
    sr = _positive(sr, "sr")
    rows = list(rows)
    fade = fade_samples(sr)
    for row in rows:
        if row["n"] < 1:
            raise ValueError("stimuli: a row needs at least one sample")
        if 0 < fade and row["n"] < fade:
            raise ValueError(f"stimuli: a row of {row['n']} samples is shorter than the fade of {fade}")
    lib = _lib.load()
    R, n, off, meta = plan_arrays("pe_stim_plan_fields", [row["n"] for row in rows], offsets,
                                  "stimuli plan: one offset per row")
    kind = np.asarray([row["kind"] for row in rows], np.int32).reshape(-1)
    raw = np.zeros((max(R, 1), 6), np.float64)
    partials = np.zeros((max(R, 1), 2 * MAX_PARTIALS), np.float64)
    n_part = np.zeros(max(R, 1), np.int32)
    coff, clen, noff = np.zeros(max(R, 1), np.int64), np.zeros(max(R, 1), np.int64), np.full(max(R, 1), -1, np.int64)
    at = 0
    for r, row in enumerate(rows):
        raw[r] = (row["amplitude"], row["a"], row["b"], row["c"], row["duration"],
                  0.0 if row["snr_db"] is None else row["snr_db"])
        n_part[r] = len(row["partials"])
        for h, (harmonic, amp) in enumerate(row["partials"][:MAX_PARTIALS]):
            partials[r, 2 * h:2 * h + 2] = (harmonic, amp)
        coff[r], clen[r] = row["curve"]
        if row["snr_db"] is not None:
            noff[r] = at
            at += row["n"]
    params = np.zeros((max(R, 1), lib.pe_stim_param_fields()), np.float64)
    consts, totals = np.zeros(4, np.int64), np.zeros(2, np.int64)
    status = lib.pe_stim_plan(R, *host_ptrs(n, off, kind, raw, partials, n_part, coff, clen, noff), sr,
                              *host_ptrs(consts, meta, params, totals))
    if status == -1:
        raise ValueError("stimuli plan: pe_stim_plan refused a row (PE_E_ARG)")
    _lib.check(status, "pe_stim_plan")
    return dict(rows=R, specs=rows, sr=sr, lengths=n, offsets=off, meta=meta, params=params, piece=int(consts[0]),
                fade=int(consts[1]), stat_fields=int(consts[3]), n_samples=int(totals[0]), n_pieces=int(totals[1]),
                n_noise=at, has_curves=bool(np.any(kind == K_CURVE)), has_tones=bool(np.any(kind == K_TONE)),
                has_phases=bool(np.any(kind != K_TONE)))


def _curves_ptr(pl, curves, who):
    if not pl["has_curves"]:
        return 0
    check_device_tensor(curves, who)
    need = max(int(row["curve"][0]) + int(row["curve"][1]) for row in pl["specs"] if row["kind"] == K_CURVE)
    if curves.numel() < need:
        raise ValueError(f"{who}: the curve tensor is shorter than the rows' curves")
    return curves.data_ptr()


def _ws(pl, device):
    n_bytes = _lib.load().pe_stim_workspace_bytes(pl["n_pieces"])
    return workspace(n_bytes, device), n_bytes


# -------------------------------------------------------------------------------------------------------------- stages
def phase(pl: dict, curves=None, device="cuda") -> torch.Tensor:
    """``pe_stim_phase``: ``cumsum(((2 pi) curve) / sr)`` of every curve, glide and vibrato row as float64, rows back to
    back in plan order (a tone row's stretch is left as it is).  Three launches."""
    device = curves.device if isinstance(curves, torch.Tensor) and curves.is_cuda else torch.device(device)
    to_device(pl, device)
    out = torch.zeros((max(pl["n_samples"], 1),), dtype=torch.float64, device=device)
    ws, n_bytes = _ws(pl, device)
    with torch.cuda.device(device):
        ops._call("pe_stim_phase", pl["meta_d"].data_ptr(), pl["meta"].ctypes.data, pl["params_d"].data_ptr(),
                  _curves_ptr(pl, curves, "stimuli.phase"), pl["rows"], out.data_ptr(), ws.data_ptr(), n_bytes,
                  _lib.stream_ptr())
    return out


def _check_out(pl, y, who):
    check_device_tensor(y, who)
    to_device(pl, plan_output(pl, y, y.device, who).device)


def synth(pl: dict, phases: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """``pe_stim_synth``: ``float32(amplitude * sin(phase))`` into the rows of ``y``.  One launch."""
    _check_out(pl, y, "stimuli.synth")
    check_device_tensor(phases, "stimuli.synth", torch.float64)
    if phases.numel() < pl["n_samples"]:
        raise ValueError("stimuli.synth: one phase per sample")
    with torch.cuda.device(y.device):
        ops._call("pe_stim_synth", pl["meta_d"].data_ptr(), pl["meta"].ctypes.data, pl["params_d"].data_ptr(),
                  phases.data_ptr(), pl["rows"], y.data_ptr(), _lib.stream_ptr())
    return y


def tone(pl: dict, y: torch.Tensor) -> torch.Tensor:
    """``pe_stim_tone``: the harmonic-tone rows of the plan into ``y``.  One launch."""
    _check_out(pl, y, "stimuli.tone")
    with torch.cuda.device(y.device):
        ops._call("pe_stim_tone", pl["meta_d"].data_ptr(), pl["meta"].ctypes.data, pl["params_d"].data_ptr(),
                  pl["rows"], y.data_ptr(), _lib.stream_ptr())
    return y


def finish(pl: dict, y: torch.Tensor, noise=None, return_stats: bool = False):
    """``pe_stim_finish`` in place on ``y``: fade, noise mix (``noise``: the packed noise of the rows that have one) and
    peak normalisation: the mix of ``csrc/snr_mix.h``, which ``noise.mix_at_snr`` runs without a fade.  Four launches.
    ``return_stats``: also the ``(rows, 4)`` float64 ``STAT_KEYS``."""
    _check_out(pl, y, "stimuli.finish")
    if pl["n_noise"]:
        check_device_tensor(noise, "stimuli.finish")
        if noise.numel() < pl["n_noise"]:
            raise ValueError("stimuli.finish: the noise tensor is shorter than the rows that mix it")
    stats = torch.zeros((max(pl["rows"], 1), pl["stat_fields"]), dtype=torch.float64, device=y.device)
    ws, n_bytes = _ws(pl, y.device)
    with torch.cuda.device(y.device):
        ops._call("pe_stim_finish", pl["meta_d"].data_ptr(), pl["meta"].ctypes.data, pl["params_d"].data_ptr(),
                  noise.data_ptr() if pl["n_noise"] else 0, pl["rows"], y.data_ptr(), stats.data_ptr(), ws.data_ptr(),
                  n_bytes, _lib.stream_ptr())
    return (y, stats[:pl["rows"]]) if return_stats else y


def frame_times(n: int, tstep: float, num_frames: int) -> np.ndarray:
    """``sample_reference_f0``'s frame times for a time axis ``float32(i * tstep)``, made by NumPy itself: the stop is a
    float32 scalar, and what ``np.linspace`` does with it is the installed NumPy's business."""
    t32 = lambda i: np.float32(np.float64(i) * np.float64(tstep))  # noqa: E731
    duration = t32(n - 1)
    if n > 1:
        duration = duration + (t32(1) - t32(0))
    return np.linspace(0.0, duration, num=int(num_frames), endpoint=False, dtype=np.float64)


def reference(pl: dict, num_frames, curves=None, device="cuda"):
    """``pe_stim_reference``: ``sample_reference_f0`` of every row at ``num_frames`` (an int, or one per row) frames,
    one launch, no per-sample curve in memory.  Returns ``(ref, frame offsets)``: a packed float32 device tensor."""
    device = curves.device if isinstance(curves, torch.Tensor) and curves.is_cuda else torch.device(device)
    to_device(pl, device)
    R = pl["rows"]
    one_each = "stimuli.reference: one non-negative frame count per row"
    nf = per_row(num_frames, R, one_each).tolist()
    if any(v < 0 for v in nf):
        raise ValueError(one_each)
    table = np.zeros((max(R, 1), 2), np.int64)
    table[:R, 1] = nf
    table[:R, 0] = np.cumsum([0] + nf[:-1]) if R else 0
    tstep = pl["params"][:, 6]
    taus = [frame_times(int(pl["lengths"][r]), float(tstep[r]), nf[r]) for r in range(R)]
    tau = np.concatenate(taus + [np.zeros(1)])
    out = torch.zeros((max(sum(nf), 1),), dtype=torch.float32, device=device)
    table_d, tau_d = torch.from_numpy(table).to(device), torch.from_numpy(tau).to(device)
    with torch.cuda.device(device):
        ops._call("pe_stim_reference", pl["meta_d"].data_ptr(), pl["meta"].ctypes.data, pl["params_d"].data_ptr(),
                  _curves_ptr(pl, curves, "stimuli.reference"), table_d.data_ptr(), table.ctypes.data,
                  tau_d.data_ptr(), R, out.data_ptr(), _lib.stream_ptr())
    return out, table[:R, 0].tolist()


def dynamic_metrics_rows(preds, refs, device="cuda"):
    """``pe_dynamic_metrics`` for R rows in one launch: ``preds[r]`` against ``refs[r]`` (tensors or arrays of Hz) over
    their first ``min(len)`` frames.  One dict of ``DYNAMIC_KEYS`` per row; the lag is in frames."""
    R = len(preds)
    if len(refs) != R:
        raise ValueError("dynamic_metrics: one reference per prediction")
    if R == 0:
        return []
    (pred, po, pn), (ref, ro, rn) = pack_tracks(preds, device), pack_tracks(refs, device)
    tracks = np.zeros((R, _lib.load().pe_dynamic_metrics_fields()), np.int64)
    for r in range(R):
        tracks[r] = (po[r], min(pn[r], rn[r]), ro[r])
    dev = pred.device
    out = torch.empty((R, 4), dtype=torch.float64, device=dev)
    tracks_d = torch.from_numpy(tracks).to(dev)
    with torch.cuda.device(dev):
        ops._call("pe_dynamic_metrics", pred.data_ptr(), ref.data_ptr(), tracks_d.data_ptr(), tracks.ctypes.data, R,
                  out.data_ptr(), _lib.stream_ptr())
    return [dict(zip(DYNAMIC_KEYS, v)) for v in out.cpu().tolist()]


# ------------------------------------------------------------------------------------------------------------ builders
class StimulusSet:
    """One ragged device batch of stimuli: ``audio`` (packed 1-D float32), ``lengths``, ``sr``, ``labels`` (one dict per
    row: the parameters the notebooks tabulate) and ``stats`` (``(rows, 4)`` float64 ``STAT_KEYS``, on the device)."""

    def __init__(self, plan, audio, stats, curves=None):
        self.plan, self.audio, self.stats, self.curves = plan, audio, stats, curves
        self.sr = plan["sr"]
        self.lengths = [int(n) for n in plan["lengths"]]
        self.labels = [dict(row["label"]) for row in plan["specs"]]

    def __len__(self):
        return self.plan["rows"]

    def rows(self):
        """The rows of ``audio`` as views."""
        return [self.audio[o:o + n] for o, n in zip(self.plan["offsets"].tolist(), self.lengths)]

    def reference_f0(self, num_frames):
        """One float32 device tensor per row: the analytic F0 at ``num_frames`` (an int, or one per row) frames, as the
        reference's ``sample_reference_f0`` samples it."""
        ref, offsets = reference(self.plan, num_frames, self.curves, self.audio.device)
        nf = per_row(num_frames, len(self), "stimuli.reference: one non-negative frame count per row").tolist()
        return [ref[o:o + n] for o, n in zip(offsets, nf)]

    def items(self, hop_length: int = 300):
        """``{"audio", "reference_f0"}`` per row (device tensors), the reference at the mel front end's
        ``1 + n // hop_length`` frames: what ``inference.stress_sweep`` takes."""
        refs = self.reference_f0([1 + n // int(hop_length) for n in self.lengths])
        for wave, ref in zip(self.rows(), refs):
            yield {"audio": wave, "reference_f0": ref}


def build(rows, sr, curves=None, noise=None, device="cuda") -> StimulusSet:
    """The row specs as one packed batch: phase and synthesis for the curve rows, the partial sums for the tone rows,
    then ``finish``."""
    if curves is not None:
        check_device_tensor(curves, "stimuli.build")
        device = curves.device
    pl = to_device(plan_rows(rows, sr), device)
    y = torch.zeros((max(pl["n_samples"], 1),), dtype=torch.float32, device=device)
    if pl["has_phases"]:
        synth(pl, phase(pl, curves, device), y)
    if pl["has_tones"]:
        tone(pl, y)
    y, stats = finish(pl, y, noise, return_stats=True)
    return StimulusSet(pl, y[:pl["n_samples"]], stats, curves)


def glides(durations, start_hz, end_hz, sr, amplitude: float = 0.8, device="cuda") -> StimulusSet:
    """``generate_glide_waveform`` for every duration: a linear glide from ``start_hz`` to ``end_hz``."""
    return build([glide_row(d, start_hz, end_hz, sr, amplitude) for d in durations], sr, device=device)


def vibratos(rates_hz, depths_cents, base_hz, duration, sr, amplitude: float = 0.8, device="cuda") -> StimulusSet:
    """``generate_vibrato_waveform`` over the grid rates x depths (rates outermost, as the notebook loops)."""
    return build([vibrato_row(rate, depth, base_hz, duration, sr, amplitude)
                  for rate in rates_hz for depth in depths_cents], sr, device=device)


def tones(freqs_hz, duration, sr, amplitude: float = 0.8, device="cuda") -> StimulusSet:
    """Constant tones (the clean stimuli of Utils/amplitude_pathologies.ipynb): ``synthesize_from_f0_curve`` of a
    curve of one value, with a free amplitude."""
    freqs = [_positive(f, "frequency") for f in freqs_hz]
    n = num_samples(duration, sr)
    curves = torch.from_numpy(np.asarray(freqs + [0.0], np.float32)).to(device)
    rows = [curve_row(n, sr, amplitude, k, 1, duration, frequency_hz=f) for k, f in enumerate(freqs)]
    return build(rows, sr, curves=curves, device=device)


def from_f0_curves(curves, lengths=None, sr=24000, amplitude: float = 0.8) -> StimulusSet:
    """``synthesize_from_f0_curve`` of given per-sample F0 curves: a float32 device tensor, rows packed with ``lengths``
    or padded 2-D.  Host arrays are refused."""
    check_waves(curves, "from_f0_curves")
    row_lengths, offsets = row_layout(curves, lengths, whole_by_default=True)
    return build([curve_row(n, sr, amplitude, o, n) for n, o in zip(row_lengths, offsets)], sr, curves=curves)


def timbre_tones(freqs_hz, profiles=None, duration: float = 2.5, sr=24000, seed: int = 1337, noise: str = "numpy",
                 device="cuda", labels=None) -> StimulusSet:
    """``synthesize_timbre_waveform`` for every frequency (outer) and profile (inner; a dict name -> profile, default
    ``TIMBRE_PROFILES``): the notebook's sweep order, in which the rows with an ``snr_db`` draw their noise from one
    generator.  ``noise="numpy"``: ``np.random.default_rng(seed).standard_normal(n).astype(float32)`` per such row,
    drawn on the host and uploaded once; ``noise="device"``: one seeded torch generator on the device.  ``labels``:
    one dict per frequency, merged into the rows' labels."""
    if noise not in ("numpy", "device"):
        raise ValueError("timbre_tones: noise is 'numpy' or 'device'")
    profiles = TIMBRE_PROFILES if profiles is None else profiles
    freqs = list(freqs_hz)
    rows = [timbre_row(f, profile, duration, sr, timbre=name, **(labels[k] if labels else {}))
            for k, f in enumerate(freqs) for name, profile in profiles.items()]
    noisy = [row["n"] for row in rows if row["snr_db"] is not None]
    noise_d = None
    if noisy:
        if noise == "numpy":
            rng = np.random.default_rng(seed)
            host = np.concatenate([rng.standard_normal(n).astype(np.float32) for n in noisy])
            noise_d = torch.from_numpy(host).to(device)
        else:
            gen = torch.Generator(device=device)
            gen.manual_seed(int(seed))
            noise_d = torch.randn((sum(noisy),), dtype=torch.float32, device=device, generator=gen)
    return build(rows, sr, noise=noise_d, device=device)


def frequency_grid(min_hz: float, max_hz: float, count: int) -> np.ndarray:
    """The timbre notebook's ``_frequency_grid``."""
    if count <= 1:
        return np.array([(min_hz + max_hz) / 2.0], dtype=np.float64)
    return np.linspace(min_hz, max_hz, count, dtype=np.float64)


def edge_region(frequency: float, min_hz: float, max_hz: float, edge_band_fraction: float) -> str:
    """The timbre notebook's ``low_cut`` / ``high_cut`` rule."""
    low_cut = min_hz + (max_hz - min_hz) * edge_band_fraction
    high_cut = max_hz - (max_hz - min_hz) * edge_band_fraction
    return "low" if frequency <= low_cut else ("high" if frequency >= high_cut else "mid")
