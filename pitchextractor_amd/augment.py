"""Training-time augmentation on the device (``csrc/augment.hip`` and the stress / noise kernels): reverb, additive
noise, a per-row biquad cascade, clipping, gain and polarity, drawn per row on the host and applied to a ragged batch
between the loader's synthetic stages and its one mel launch.  It is what the reference leaves to its users ("add your
own data augmentation in meldataset.py with audiomentations").  There is no CPU path.  ``tests/augment_ref.py`` is the
float64 restatement of the cascade and of the designers.

``biquad_cascade`` is the new kernel's wrapper: per row up to 8 second-order sections ``{b0, b1, b2, a1, a2}`` (``a0 =
1``), the row's float32 samples widened to double, the sections chained in double in transposed direct form II from a
zero state with neither a clamp nor a rounding between them, one rounding to float32 at the end:
``scipy.signal.sosfilt`` in float64 and a cast.  (``stress.apply_microphone_eq`` keeps torchaudio's clamp per stage.)
A stage's poles may lie no further out than ``MAX_POLE_RADIUS = 1 - 2^-12``.

``Augmenter`` holds a checked config.  ``draw(n_rows)`` makes an ``AugmentPlan`` on the host from the Augmenter's own
``numpy.random.Generator``: every value of every transform for every row, in one fixed order, whatever is enabled and
whatever a row was selected for, so that switching a transform off leaves the others' values alone; ``random`` and
``numpy.random`` are never touched, so the items of a run and the workers' draw orders are the same with and without
augmentation.  ``apply(waves, lengths, plan)`` runs the chain in the fixed order reverb, noise, filter, clipping, gain
and polarity; a row that a transform did not select passes through it bit-identical.  Labels are not moved: nothing here
shifts, stretches or transposes."""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

import numpy as np
import torch

from . import _lib, ops
from .ragged import check_waves, host_ptrs, i64, per_row, row_layout, workspace

MAX_STAGES = 8
MAX_POLE_RADIUS = 1.0 - 2.0 ** -12          # csrc/augment.hip's kMaxPoleRadius: the error bound stands on it
TRANSFORMS = ("reverb", "noise", "filter", "clipping", "gain", "polarity")      # the order of the chain
CONFIG_KEYS = ("enabled", "seed", "apply_to_validation", "apply_to_synthetic") + TRANSFORMS
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0)
_SQRT_HALF = 1.0 / math.sqrt(2.0)


# ------------------------------------------------------------------------------------------------------------ designers
def pole_radius(stage) -> float:
    """Largest pole modulus of a normalised stage ``{b0, b1, b2, a1, a2}``, as the kernel's argument check computes
    it: ``sqrt(a2)`` for a complex pair, ``(|a1| + sqrt(a1^2 - 4 a2)) / 2`` for real poles."""
    a1, a2 = float(stage[3]), float(stage[4])
    disc = a1 * a1 - 4.0 * a2
    return math.sqrt(a2) if disc < 0.0 else 0.5 * (abs(a1) + math.sqrt(disc))


def _stage_error(c):
    """Why the kernel would refuse the five floats ``c``, or None."""
    if not all(math.isfinite(v) for v in c):
        return "a stage is five finite coefficients {b0, b1, b2, a1, a2}"
    if not (abs(c[4]) < 1.0 and abs(c[3]) < 1.0 + c[4]):
        return "the poles lie outside the unit circle"
    radius = pole_radius(c)
    if not radius <= MAX_POLE_RADIUS:
        return f"pole radius {radius!r} exceeds 1 - 2^-12, the kernel's limit"
    return None


def check_stage(stage, name: str = "stage") -> np.ndarray:
    """The stage as five float64, or ``ValueError`` naming it: a non-finite coefficient, poles outside the stability
    triangle, or a pole radius above ``MAX_POLE_RADIUS``."""
    c = np.asarray(stage, dtype=np.float64).reshape(-1)
    error = "a stage is five finite coefficients {b0, b1, b2, a1, a2}" if c.size != 5 else _stage_error(c.tolist())
    if error is not None:
        raise ValueError(f"{name}: {error}")
    return c


def _rbj(name, sr, f, Q, gain_db=0.0):
    sr, f, Q, gain_db = float(sr), float(f), float(Q), float(gain_db)
    if not (math.isfinite(sr) and math.isfinite(f) and math.isfinite(Q) and math.isfinite(gain_db)) or \
            not (sr > 0.0 and 0.0 < f < sr / 2.0 and Q > 0.0):
        raise ValueError(f"{name}: needs sr > 0, 0 < f < sr / 2, Q > 0 and a finite gain")
    w0 = 2.0 * math.pi * f / sr
    return math.cos(w0), math.sin(w0) / (2.0 * Q), 10.0 ** (gain_db / 40.0)


def _stage(kind, args, b, a):
    c = [b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]]
    error = _stage_error(c)
    if error is not None:
        names = ("sr", "f", "gain_db", "Q") if len(args) == 4 else ("sr", "f", "Q")
        raise ValueError(f"{kind}({', '.join(f'{k}={v}' for k, v in zip(names, args))}): {error}")
    return np.array(c, dtype=np.float64)


def lowpass(sr, f, Q=_SQRT_HALF) -> np.ndarray:
    """The RBJ cookbook's low-pass as one normalised float64 stage ``{b0, b1, b2, a1, a2}``."""
    c, alpha, _ = _rbj("lowpass", sr, f, Q)
    return _stage("lowpass", (sr, f, Q), ((1.0 - c) / 2.0, 1.0 - c, (1.0 - c) / 2.0),
                  (1.0 + alpha, -2.0 * c, 1.0 - alpha))


def highpass(sr, f, Q=_SQRT_HALF) -> np.ndarray:
    """The RBJ cookbook's high-pass."""
    c, alpha, _ = _rbj("highpass", sr, f, Q)
    return _stage("highpass", (sr, f, Q), ((1.0 + c) / 2.0, -(1.0 + c), (1.0 + c) / 2.0),
                  (1.0 + alpha, -2.0 * c, 1.0 - alpha))


def peaking(sr, f, gain_db, Q=_SQRT_HALF) -> np.ndarray:
    """The RBJ cookbook's peaking equaliser (``stress.peaking_biquad``'s form)."""
    c, alpha, A = _rbj("peaking", sr, f, Q, gain_db)
    return _stage("peaking", (sr, f, gain_db, Q), (1.0 + alpha * A, -2.0 * c, 1.0 - alpha * A),
                  (1.0 + alpha / A, -2.0 * c, 1.0 - alpha / A))


def lowshelf(sr, f, gain_db, Q=_SQRT_HALF) -> np.ndarray:
    """The RBJ cookbook's low shelf: ``gain_db`` at 0 Hz, 0 dB at Nyquist."""
    c, alpha, A = _rbj("lowshelf", sr, f, Q, gain_db)
    k = 2.0 * math.sqrt(A) * alpha
    return _stage("lowshelf", (sr, f, gain_db, Q),
                  (A * ((A + 1.0) - (A - 1.0) * c + k), 2.0 * A * ((A - 1.0) - (A + 1.0) * c),
                   A * ((A + 1.0) - (A - 1.0) * c - k)),
                  ((A + 1.0) + (A - 1.0) * c + k, -2.0 * ((A - 1.0) + (A + 1.0) * c), (A + 1.0) + (A - 1.0) * c - k))


def highshelf(sr, f, gain_db, Q=_SQRT_HALF) -> np.ndarray:
    """The RBJ cookbook's high shelf: 0 dB at 0 Hz, ``gain_db`` at Nyquist."""
    c, alpha, A = _rbj("highshelf", sr, f, Q, gain_db)
    k = 2.0 * math.sqrt(A) * alpha
    return _stage("highshelf", (sr, f, gain_db, Q),
                  (A * ((A + 1.0) + (A - 1.0) * c + k), -2.0 * A * ((A - 1.0) + (A + 1.0) * c),
                   A * ((A + 1.0) + (A - 1.0) * c - k)),
                  ((A + 1.0) - (A - 1.0) * c + k, 2.0 * ((A - 1.0) - (A + 1.0) * c), (A + 1.0) - (A - 1.0) * c - k))


# ------------------------------------------------------------------------------------------------------------ the kernel
def kernel_consts() -> dict:
    """``pe_augment_biquad_consts`` (host only): the kernel's piece, block and stage limit."""
    consts = np.zeros(3, np.int64)
    _lib.check(_lib.load().pe_augment_biquad_consts(*host_ptrs(consts)), "pe_augment_biquad_consts")
    return dict(piece=int(consts[0]), block=int(consts[1]), max_stages=int(consts[2]))


def _row_plan(x, lengths, who):
    """The two-field row plan {offset, length} of ``x`` in one of the three wave layouts, and its device copy."""
    check_waves(x, who)
    n, off = row_layout(x, lengths, whole_by_default=True)
    meta = np.zeros((max(len(n), 1), 2), np.int64)
    meta[:len(n), 0], meta[:len(n), 1] = off, n
    return len(n), meta, torch.from_numpy(meta).to(x.device)


def _output(x, out, who):
    if out is None:
        return torch.zeros(tuple(x.shape), dtype=torch.float32, device=x.device)
    check_waves(out, who)
    if tuple(out.shape) != tuple(x.shape) or out.stride() != x.stride() or out.device != x.device:
        raise ValueError(f"{who}: out has x's shape, strides and device")
    return out


def cascade_table(sos, n_stages, R: int):
    """``(sos (R, 8, 5) float64, n_stages (R,) int32)`` of a cascade given per row (``(R, S, 5)``, S <= 8) or once for
    every row (``(S, 5)``); ``n_stages`` defaults to S.  The unused stages are the identity.  ``ValueError`` for a shape
    that is neither, a count outside 0 .. S, or a used stage that ``check_stage`` refuses."""
    sos = np.asarray(sos, dtype=np.float64)
    if sos.ndim == 2:
        sos = np.broadcast_to(sos, (R,) + sos.shape)
    if sos.ndim != 3 or sos.shape[0] != R or sos.shape[1] > MAX_STAGES or sos.shape[2] != 5:
        raise ValueError(f"biquad_cascade: sos is (rows, stages <= {MAX_STAGES}, 5) or (stages, 5)")
    S = int(sos.shape[1])
    count = per_row(S if n_stages is None else n_stages, R, "biquad_cascade: one stage count per row", np.int32)
    if np.any(count < 0) or np.any(count > S):
        raise ValueError(f"biquad_cascade: a stage count lies outside 0 .. {S}")
    table = np.tile(np.asarray(IDENTITY, np.float64), (max(R, 1), MAX_STAGES, 1))
    used = np.arange(S)[None, :] < count[:, None]
    table[:R, :S][used] = sos[used]
    a1, a2 = table[..., 3], table[..., 4]
    disc = a1 * a1 - 4.0 * a2
    with np.errstate(invalid="ignore"):
        radius = np.where(disc < 0.0, np.sqrt(np.abs(a2)), 0.5 * (np.abs(a1) + np.sqrt(np.abs(disc))))
        fine = np.isfinite(table).all(-1) & (np.abs(a2) < 1.0) & (np.abs(a1) < 1.0 + a2) & (radius <= MAX_POLE_RADIUS)
    for r, s in np.argwhere(~fine):                            # names the first stage the kernel would refuse
        check_stage(table[r, s], f"biquad_cascade: row {r} stage {s}")
    return table, np.ascontiguousarray(count, dtype=np.int32)


def biquad_cascade(x: torch.Tensor, sos, n_stages=None, lengths=None, out=None) -> torch.Tensor:
    """``pe_augment_biquad``: row r of ``x`` (one 1-D wave, rows packed with ``lengths``, or padded 2-D rows) through
    its own cascade ``sos[r, :n_stages[r]]`` (``cascade_table``), as the module's head defines it.  The result has
    ``x``'s shape, zero outside the rows, or is written to ``out`` (``x`` itself: in place).  A row's result is
    bit-identical alone, packed at any offset, padded or in place, whatever the other rows' cascades.  One launch."""
    R, meta, meta_d = _row_plan(x, lengths, "biquad_cascade")
    y = _output(x, out, "biquad_cascade")
    table, count = cascade_table(sos, n_stages, R)
    if R == 0 or int(meta[:, 1].sum()) == 0:
        return y
    table_d, count_d = torch.from_numpy(table).to(x.device), torch.from_numpy(count).to(x.device)
    with torch.cuda.device(x.device):
        ops._call("pe_augment_biquad", x.data_ptr(), meta_d.data_ptr(), meta.ctypes.data, 2, R, table_d.data_ptr(),
                  table.ctypes.data, count_d.data_ptr(), count.ctypes.data, y.data_ptr(), _lib.stream_ptr())
    return y


def apply_gain(x: torch.Tensor, gains, lengths=None, out=None) -> torch.Tensor:
    """``pe_augment_gain``: ``float32(x * float32(gains[r]))`` over row r (a gain and a polarity in one multiply).  One
    launch."""
    R, meta, meta_d = _row_plan(x, lengths, "apply_gain")
    y = _output(x, out, "apply_gain")
    g = per_row(gains, R, "apply_gain: one gain per row", np.float32)
    if not np.all(np.isfinite(g)):
        raise ValueError("apply_gain: a gain is not finite")
    if R == 0 or int(meta[:, 1].sum()) == 0:
        return y
    g_d = torch.from_numpy(g).to(x.device)
    with torch.cuda.device(x.device):
        ops._call("pe_augment_gain", x.data_ptr(), meta_d.data_ptr(), meta.ctypes.data, 2, R, g_d.data_ptr(),
                  g.ctypes.data, y.data_ptr(), _lib.stream_ptr())
    return y


# ------------------------------------------------------------------------------------------------------------ the config
DEFAULTS = {
    "reverb": {"p": 0.0, "library": None, "files": None, "responses": None},
    "noise": {"p": 0.0, "colours": ("white", "pink", "brown"), "snr_db": (5.0, 40.0), "warmup": 4096},
    # every default range keeps every stage inside MAX_POLE_RADIUS at 16 to 48 kHz (see check_config)
    "filter": {"p": 0.0,
               "highpass": {"p": 0.5, "f": (40.0, 400.0), "Q": (0.5, 1.0)},
               "lowpass": {"p": 0.5, "f": (2000.0, 7000.0), "Q": (0.5, 1.0)},
               "peaking": {"count": (0, 3), "f": (100.0, 6000.0), "gain_db": (-9.0, 9.0), "Q": (0.5, 3.0)},
               "shelf": {"p": 0.5, "f": (100.0, 5000.0), "gain_db": (-9.0, 9.0), "Q": (0.5, 1.0)}},
    "clipping": {"p": 0.0, "percent": (0.1, 10.0)},
    "gain": {"p": 0.0, "gain_db": (-12.0, 6.0)},
    "polarity": {"p": 0.0},
}
_FILTER_KINDS = ("highpass", "lowpass", "peaking", "shelf")


def _range(value, what, positive=False, integer=False):
    try:
        lo, hi = (value, value) if np.ndim(value) == 0 else value
        lo, hi = (int(lo), int(hi)) if integer else (float(lo), float(hi))
    except (TypeError, ValueError):
        raise ValueError(f"augmentation: {what} must be a number or [lo, hi]") from None
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi or (positive and lo <= 0):
        raise ValueError(f"augmentation: {what} must be a finite {'positive ' if positive else ''}range lo <= hi, "
                         f"got {value!r}")
    return lo, hi


def _probability(value, what):
    try:
        p = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"augmentation: {what} must be a probability") from None
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"augmentation: {what} must lie in [0, 1], got {value!r}")
    return p


def _block(name, given, defaults):
    if given is None:
        given = {}
    if not isinstance(given, dict):
        raise ValueError(f"augmentation: {name} must be a mapping")
    for k in given:
        if k not in defaults:
            raise ValueError(f"augmentation: {name} has no option {k!r} (it has {sorted(defaults)})")
    return {**defaults, **given}


def check_config(config, sr) -> dict:
    """The augmentation block with its defaults filled in.  ``ValueError``: an unknown transform or option, a
    probability outside [0, 1], a range that is not finite ``lo <= hi``, an unknown noise colour, a frequency range that
    reaches Nyquist, or filter ranges none of whose corners gives a stage the kernel takes."""
    from . import noise
    if config is None:
        config = {}
    if not isinstance(config, dict):
        raise ValueError("augmentation: the config must be a mapping")
    for k in config:
        if k not in CONFIG_KEYS:
            raise ValueError(f"augmentation: {k!r} is not a transform or an option (known: {CONFIG_KEYS})")
    sr = float(sr)
    out = {"enabled": bool(config.get("enabled", True)), "seed": int(config.get("seed", 0)),
           "apply_to_validation": bool(config.get("apply_to_validation", False)),
           "apply_to_synthetic": bool(config.get("apply_to_synthetic", True))}
    for name in TRANSFORMS:
        blk = _block(name, config.get(name), DEFAULTS[name])
        blk["p"] = _probability(blk["p"], f"{name}.p")
        out[name] = blk
    rv = out["reverb"]
    if sum(rv[k] is not None for k in ("library", "files", "responses")) > 1:
        raise ValueError("augmentation: reverb takes one of library, files, responses")
    if rv["library"] is not None and rv["library"] != "shoebox":
        raise ValueError(f"augmentation: reverb.library {rv['library']!r} is not 'shoebox'")
    for k in ("files", "responses"):
        if rv[k] is not None and (isinstance(rv[k], (str, bytes)) or len(rv[k]) == 0):
            raise ValueError(f"augmentation: reverb.{k} must be a non-empty list")
    if rv["p"] > 0 and all(rv[k] is None for k in ("library", "files", "responses")):
        raise ValueError("augmentation: reverb needs library: shoebox, files or responses")
    ns = out["noise"]
    ns["colours"] = tuple(ns["colours"]) if not isinstance(ns["colours"], str) else (ns["colours"],)
    if not ns["colours"] or any(c not in noise.NOISE_COLOURS for c in ns["colours"]):
        raise ValueError(f"augmentation: noise.colours must be a non-empty subset of {noise.NOISE_COLOURS}")
    ns["snr_db"] = _range(ns["snr_db"], "noise.snr_db")
    ns["warmup"] = int(ns["warmup"])
    if ns["warmup"] < 0:
        raise ValueError("augmentation: noise.warmup must not be negative")
    fl = out["filter"]
    for kind in _FILTER_KINDS:
        sub = _block(f"filter.{kind}", fl[kind], DEFAULTS["filter"][kind])
        if "p" in sub:
            sub["p"] = _probability(sub["p"], f"filter.{kind}.p")
        if "count" in sub:
            sub["count"] = _range(sub["count"], f"filter.{kind}.count", integer=True)
            if sub["count"][0] < 0 or sub["count"][1] > MAX_STAGES - 3:
                raise ValueError(f"augmentation: filter.peaking.count must lie in 0 .. {MAX_STAGES - 3}")
        sub["f"] = _range(sub["f"], f"filter.{kind}.f", positive=True)
        if fl["p"] > 0 and sub["f"][1] >= sr / 2.0:
            raise ValueError(f"augmentation: filter.{kind}.f reaches Nyquist ({sr / 2.0} Hz)")
        sub["Q"] = _range(sub["Q"], f"filter.{kind}.Q", positive=True)
        if "gain_db" in sub:
            sub["gain_db"] = _range(sub["gain_db"], f"filter.{kind}.gain_db")
        fl[kind] = sub
        if fl["p"] > 0:                                        # a redraw must be able to end
            corners = [(f, q, g) for f in sub["f"] for q in sub["Q"] for g in sub.get("gain_db", (0.0,))]
            if not any(_try_stage(kind, sr, f, g, q, True) is not None for f, q, g in corners):
                raise ValueError(f"augmentation: no corner of filter.{kind}'s ranges gives a stage within the pole-radius "
                                 f"limit at {sr} Hz")
    out["clipping"]["percent"] = _range(out["clipping"]["percent"], "clipping.percent")
    if out["clipping"]["percent"][0] < 0 or out["clipping"]["percent"][1] > 100:
        raise ValueError("augmentation: clipping.percent must lie in [0, 100]")
    out["gain"]["gain_db"] = _range(out["gain"]["gain_db"], "gain.gain_db")
    return out


def _try_stage(kind, sr, f, gain_db, Q, low):
    try:
        if kind == "highpass":
            return highpass(sr, f, Q)
        if kind == "lowpass":
            return lowpass(sr, f, Q)
        if kind == "peaking":
            return peaking(sr, f, gain_db, Q)
        return (lowshelf if low else highshelf)(sr, f, gain_db, Q)
    except ValueError:
        return None


# ------------------------------------------------------------------------------------------------------------ the plan
@dataclass(frozen=True)
class AugmentPlan:
    """What ``Augmenter.draw`` drew for R rows, all on the host.  ``*_on``: the rows a transform selected (all False for
    a transform that is off).  Every value is drawn for every row, selected or not."""
    rows: int
    reverb_on: np.ndarray
    rir_index: np.ndarray           # int32, into the Augmenter's RirSet (0 without one)
    noise_on: np.ndarray
    noise_colour: np.ndarray        # int64, into the config's colours
    snr_db: np.ndarray              # float64
    noise_seed: np.ndarray          # int64
    filter_on: np.ndarray
    n_stages: np.ndarray            # int32, 0 .. 8
    sos: np.ndarray                 # float64 (R, 8, 5), the identity past n_stages
    clipping_on: np.ndarray
    clip_percent: np.ndarray        # float64
    gain_on: np.ndarray
    gain_db: np.ndarray             # float64
    polarity_on: np.ndarray

    def factors(self) -> np.ndarray:
        """float32 per row: the linear gain of a selected row, negated for a flipped one, 1 for neither."""
        g = np.where(self.gain_on, 10.0 ** (self.gain_db / 20.0), 1.0).astype(np.float32)
        return np.where(self.polarity_on, -g, g).astype(np.float32)

    def without(self, rows) -> "AugmentPlan":
        """The plan with ``rows`` selected by no transform."""
        keep = np.ones(self.rows, bool)
        keep[np.asarray(list(rows), dtype=np.int64)] = False
        return replace(self, **{f"{t}_on": getattr(self, f"{t}_on") & keep for t in TRANSFORMS})


def _uniform(u, lo_hi):
    return lo_hi[0] + (lo_hi[1] - lo_hi[0]) * u


def _log_uniform(u, lo_hi):
    return math.exp(_uniform(u, (math.log(lo_hi[0]), math.log(lo_hi[1]))))


class Augmenter:
    """``Augmenter(config, sr, seed=0, rank=0)``: the checked augmentation block of a loader at sample rate ``sr``; its
    generator is seeded with ``(seed, rank)``.  See the module's head."""

    def __init__(self, config, sr, seed=0, rank=0):
        self.sr = int(sr)
        self.config = check_config(config, sr)
        self.rng = np.random.Generator(np.random.PCG64([int(seed) & (2 ** 63 - 1), int(rank)]))
        self._rirs = None
        rv = self.config["reverb"]
        if rv["library"] is not None:
            from . import rir
            self.n_rirs = sum(len(v) for v in rir.LIBRARY_T60S.values())
        else:
            self.n_rirs = len(rv["files"] or rv["responses"] or ())

    @property
    def active(self) -> bool:
        return self.config["enabled"] and any(self.config[t]["p"] > 0 for t in TRANSFORMS)

    # ---- host
    def _draw_filter(self, word: int):
        """A row's stages from a generator of its own (seeded by one word of the main stream, so that a redraw never
        shifts what the other rows and transforms draw): high-pass, low-pass, the peaking stages, a shelf."""
        cfg, rng, stages = self.config["filter"], np.random.Generator(np.random.PCG64(int(word))), []

        def stage(kind):
            sub = cfg[kind]
            for _ in range(256):
                f, q = _log_uniform(rng.random(), sub["f"]), _log_uniform(rng.random(), sub["Q"])
                g, low = _uniform(rng.random(), sub.get("gain_db", (0.0, 0.0))), rng.random() < 0.5
                got = _try_stage(kind, self.sr, f, g, q, low)
                if got is not None:                            # else: past the pole-radius limit, drawn again
                    return got
            raise ValueError(f"augmentation: filter.{kind} found no stage within the pole-radius limit in 256 draws")

        take = [rng.random() < cfg[k]["p"] for k in ("highpass", "lowpass", "shelf")]
        count = int(rng.integers(cfg["peaking"]["count"][0], cfg["peaking"]["count"][1] + 1))
        if take[0]:
            stages.append(stage("highpass"))
        if take[1]:
            stages.append(stage("lowpass"))
        stages += [stage("peaking") for _ in range(count)]
        if take[2]:
            stages.append(stage("shelf"))
        return stages

    def draw(self, n_rows: int) -> AugmentPlan:
        """The plan of ``n_rows`` rows: per call one ``(n_rows, 12)`` block of uniforms and one ``(n_rows, 2)`` block of
        63-bit words from the Augmenter's generator, whatever the config holds."""
        R, cfg = int(n_rows), self.config
        u = self.rng.random((R, 12))
        words = self.rng.integers(0, 2 ** 63 - 1, size=(R, 2), dtype=np.int64)
        on = {t: (u[:, k] < cfg[t]["p"]) & cfg["enabled"] for k, t in enumerate(TRANSFORMS)}
        rir_index = np.minimum((u[:, 6] * max(self.n_rirs, 1)).astype(np.int32), max(self.n_rirs - 1, 0))
        colours = len(cfg["noise"]["colours"])
        colour = np.minimum((u[:, 7] * colours).astype(np.int64), colours - 1)
        sos = np.tile(np.asarray(IDENTITY, np.float64), (R, MAX_STAGES, 1))
        n_stages = np.zeros(R, np.int32)
        if cfg["filter"]["p"] > 0 and cfg["enabled"]:          # the stages come from the rows' own generators
            for r in range(R):
                stages = self._draw_filter(words[r, 1])
                n_stages[r] = len(stages)
                if stages:
                    sos[r, :len(stages)] = stages
        return AugmentPlan(
            rows=R, reverb_on=on["reverb"], rir_index=rir_index.astype(np.int32), noise_on=on["noise"],
            noise_colour=colour, snr_db=_uniform(u[:, 8], cfg["noise"]["snr_db"]), noise_seed=words[:, 0].copy(),
            filter_on=on["filter"], n_stages=n_stages, sos=sos, clipping_on=on["clipping"],
            clip_percent=_uniform(u[:, 9], cfg["clipping"]["percent"]), gain_on=on["gain"],
            gain_db=_uniform(u[:, 10], cfg["gain"]["gain_db"]), polarity_on=on["polarity"])

    # ---- device
    def prepare(self, device):
        """Build what ``apply`` needs beyond a plan, once: the reverb's ``stress.RirSet`` (``library: shoebox`` is
        ``rir.room_library(sr)`` calibrated on ``device``; ``files`` are read and normalised by ``stress.prepare_rir``
        and must be at ``sr``; ``responses`` are arrays taken the same way)."""
        rv = self.config["reverb"]
        if self._rirs is not None or not (self.config["enabled"] and rv["p"] > 0):
            return self
        from . import rir, stress
        if rv["library"] is not None:
            self._rirs = rir.room_library(self.sr, device=device).rir_set()
        elif rv["files"] is not None:
            from .meldataset import read_wav
            responses = []
            for path in rv["files"]:
                audio, rate = read_wav(path)
                if int(rate) != self.sr:
                    raise ValueError(f"augmentation: impulse response {path!r} is at {rate} Hz, the loader at {self.sr}")
                responses.append(stress.prepare_rir(audio if audio.ndim == 1 else audio[:, 0]))
            self._rirs = stress.RirSet(responses)
        else:
            self._rirs = stress.RirSet([stress.prepare_rir(h) for h in rv["responses"]])
        if len(self._rirs) != self.n_rirs:
            raise ValueError("augmentation: the reverb's responses are not as many as the plans index")
        return self

    def _reverb(self, x, n, off, plan):
        """``x`` with the selected rows convolved (``stress.apply_rir``'s three launches over those rows alone)."""
        from . import stress
        y = x.clone()
        rows = np.flatnonzero(plan.reverb_on & (n > 0))
        if rows.size == 0:
            return y
        self.prepare(x.device)
        pl = stress.plan_rows(n[rows], off[rows], off[rows])
        meta_d = torch.from_numpy(pl["meta"]).to(x.device)
        index = np.ascontiguousarray(plan.rir_index[rows], dtype=np.int32)
        index_d = torch.from_numpy(index).to(x.device)
        rir_meta_d, spectra = self._rirs.device_spectra(x.device)
        tables = stress._tables(x.device)
        ws_bytes = _lib.load().pe_stress_rir_workspace_bytes(pl["n_blocks"])
        ws = workspace(ws_bytes, x.device)
        with torch.cuda.device(x.device):
            ops._call("pe_stress_rir", x.data_ptr(), meta_d.data_ptr(), pl["meta"].ctypes.data, int(rows.size),
                      spectra.data_ptr(), rir_meta_d.data_ptr(), self._rirs.plan["meta"].ctypes.data, len(self._rirs),
                      index_d.data_ptr(), index.ctypes.data, tables.data_ptr(), tables.numel(), y.data_ptr(),
                      ws.data_ptr(), ws_bytes, _lib.stream_ptr())
        return y

    def _noise(self, x, n, off, lengths, plan):
        """``x`` plus noise at the selected rows' SNRs: the rows of one colour drawn together into one buffer of
        ``x``'s layout, then one ``noise.mix_at_snr`` over the batch without the peak rule (an unselected row's noise
        is silent, which makes the row a copy)."""
        from . import noise
        flat = torch.zeros((max(x.numel(), 1),), dtype=torch.float32, device=x.device)
        cfg = self.config["noise"]
        for k, colour in enumerate(cfg["colours"]):
            rows = np.flatnonzero(plan.noise_on & (plan.noise_colour == k) & (n > 0))
            if rows.size == 0:
                continue
            if colour == "white":
                noise.white(n[rows], plan.noise_seed[rows], offsets=off[rows], out=flat)
            else:
                noise.coloured(n[rows], colour, self.sr, seeds=plan.noise_seed[rows], warmup=cfg["warmup"],
                               offsets=off[rows], out=flat)
        snr = np.where(plan.noise_on, plan.snr_db, 0.0)
        return noise.mix_at_snr(x, flat[:x.numel()].view(x.shape), snr, lengths, peak_normalize=False)

    def apply(self, waves: torch.Tensor, lengths, plan: AugmentPlan, return_stages: bool = False):
        """The chain over a ragged batch (packed rows with ``lengths``, padded rows, or one wave): reverb, noise,
        filter, clipping, gain and polarity, each over the rows the plan selected for it; the result has ``waves``'
        shape and ``waves`` is left alone.  ``return_stages``: also a dict of the batch as it left each transform
        (``"input"`` and the names of ``TRANSFORMS`` but ``"polarity"``, which rides on the gain's multiply)."""
        from . import stress
        check_waves(waves, "Augmenter.apply")
        x = waves.contiguous()
        row_lengths, offsets = row_layout(x, lengths, whole_by_default=True)
        if len(row_lengths) != plan.rows:
            raise ValueError(f"Augmenter.apply: a plan of {plan.rows} rows for {len(row_lengths)}")
        n, off = i64(row_lengths), i64(offsets)
        stages = {"input": x}

        def keep(name, y):
            if return_stages:
                stages[name] = y.clone()
            return y

        y = keep("reverb", self._reverb(x, n, off, plan))
        if np.any(plan.noise_on):
            y = self._noise(y, n, off, row_lengths, plan)
        keep("noise", y)
        if np.any(plan.filter_on):
            biquad_cascade(y, plan.sos, np.where(plan.filter_on, plan.n_stages, 0), row_lengths, out=y)
        keep("filter", y)
        if np.any(plan.clipping_on):
            y = stress.apply_sample_clipping_rows(y, np.where(plan.clipping_on, plan.clip_percent, 0.0), row_lengths)
        keep("clipping", y)
        if np.any(plan.gain_on | plan.polarity_on):
            apply_gain(y, plan.factors(), row_lengths, out=y)
        keep("gain", y)
        return (y, stages) if return_stages else y
