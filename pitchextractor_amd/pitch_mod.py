"""Pitch modulation of real training audio on the device (``csrc/pitch_mod.hip``): a time warp ``y(t) = x(tau(t))``
over the span a row's kept label frames cover, so that every harmonic of the recording is multiplied by the local speed
``s(t) = tau'(t)`` and the exact label is ``s(t) * F0(tau(t))``; vibrato, flutter, drift and glides on a voice's own
samples, with no vocoder in the path.  There is no CPU path.  ``tests/pitch_mod_ref.py`` is the float64 restatement.

A ``Modulation`` is up to 4 sinusoids ``(d, rate in Hz, phi)`` and one ramp ``a``.  With ``u = t - t0``, ``T = t1 - t0``
and ``w_k = 2 pi rate_k / sr`` the map is closed form and evaluated in double on host and device::

    m(u)   = sum_k d_k sin(w_k u + phi_k) + a (2u/T - 1)
    mbar   = (1/T) sum_k d_k (cos phi_k - cos(w_k T + phi_k)) / w_k
    s(u)   = 1 + m(u) - mbar
    tau(u) = u (1 - mbar) + a (u^2/T - u) + sum_k d_k (cos phi_k - cos(w_k u + phi_k)) / w_k

``tau(0) = 0`` and ``tau(T) = T`` (both pinned), so every source position of a kept frame lies inside the kept frames
and every label the stage needs is one the batch holds; outside ``[t0, t1]`` the map is the identity.  The ramp is a
glide from speed ``1 - a`` to ``1 + a``.  A constant transposition cannot be expressed (``synthetic_data.pitch_shift``
has that).  ``2 sum|d_k| + |a| <= 0.5`` (``CAP``) keeps ``s`` within [0.5, 1.5] and ``tau`` monotone.

``modulate`` is the wave kernel's wrapper, ``modulate_labels`` the label kernel's.  ``PitchModulator`` holds a checked
config, draws a ``PitchModPlan`` per batch from a ``numpy.random.Generator`` of its own (``random`` and
``numpy.random`` are never touched) and applies it to a ragged batch and its labels; it is the loader's stage between
the synthetic kinds and the ``Augmenter``."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, replace

import numpy as np
import torch

from . import _lib, ops
from .pitch_shift import RES_TYPES, check_res_type, resample_filter
from .ragged import check_device_tensor, check_waves, host_ptrs, i64, plan_meta, row_layout

MAX_SINUSOIDS = 4
CAP = 0.5                                   # csrc/pitch_mod.hip's kCap: 2 sum|d| + |a| may not exceed it
MIN_RATE_HZ = 0.05
MAX_FRAMES = 192                            # the label frames a batch row keeps
PARAMS = 24                                 # doubles per row of the plan's parameter table
# where the wave kernel reads the filter table.  Both stay in L2: measured on 256 rows of 2 s (tools/bench_pitch_mod.py,
# profiles/bench_pitch_mod.json), kaiser_fast's 64 KiB table takes 0.48 ms read from L2 and 0.64 ms when every
# workgroup first copies it into LDS; kaiser_best's 256 KiB do not fit there
TABLE_IN_LDS = {"kaiser_fast": False, "kaiser_best": False}


@dataclass(frozen=True)
class Modulation:
    """Up to 4 sinusoids ``(d, rate_hz, phi)`` and the ramp ``a``.  A sinusoid with ``d == 0`` is absent."""
    sinusoids: tuple = ()
    ramp: float = 0.0

    def row(self) -> np.ndarray:
        """``{d[4], rate_hz[4], phi[4], a}`` as 13 float64, the absent sinusoids zero."""
        return self._row.copy()

    @functools.cached_property
    def _row(self) -> np.ndarray:
        comps = [tuple(float(v) for v in c) for c in self.sinusoids]
        if len(comps) > MAX_SINUSOIDS or any(len(c) != 3 for c in comps):
            raise ValueError(f"pitch modulation: at most {MAX_SINUSOIDS} sinusoids (d, rate_hz, phi)")
        out = np.zeros(13, np.float64)
        for k, (d, rate, phi) in enumerate(comps):
            out[k], out[4 + k], out[8 + k] = d, rate, phi
        out[12] = float(self.ramp)
        return out

    @functools.cached_property
    def identity(self) -> bool:
        g = self._row
        return not (np.any(g[:4] != 0.0) or g[12] != 0.0)


def check_modulation(mod: Modulation, T=None, hop=None) -> np.ndarray:
    """The modulation's row, or ``ValueError``: a non-finite value, ``2 sum|d| + |a| > 0.5``, a rate below 0.05 Hz, or
    (given ``T`` and ``hop``) a span shorter than one hop."""
    g = mod.row()
    if not np.all(np.isfinite(g)):
        raise ValueError("pitch modulation: a parameter is not finite")
    used = g[:4] != 0.0
    if np.any(g[4:8][used] < MIN_RATE_HZ):
        raise ValueError(f"pitch modulation: a rate lies below {MIN_RATE_HZ} Hz")
    total = 2.0 * float(np.abs(g[:4]).sum()) + abs(float(g[12]))
    if total > CAP:
        raise ValueError(f"pitch modulation: 2 sum|d| + |a| = {total!r} exceeds {CAP}")
    if T is not None and hop is not None and T < hop:
        raise ValueError(f"pitch modulation: the span of {T} samples is shorter than one hop ({hop})")
    return g


def time_map(mod: Modulation, T, u, sr):
    """``(tau, s)`` in float64 at ``u`` (samples from the span's start, within ``[0, T]``), as the kernels form them;
    ``tau`` is exactly ``u`` at 0 and ``T``."""
    g = check_modulation(mod)
    T = float(T)
    u = np.asarray(u, dtype=np.float64)
    mbar, m, c = 0.0, np.zeros_like(u), np.zeros_like(u)
    for k in range(MAX_SINUSOIDS):
        d = g[k]
        if d == 0.0:
            continue
        w, phi = 2.0 * math.pi * g[4 + k] / float(sr), g[8 + k]
        mbar += d * (math.cos(phi) - math.cos(w * T + phi)) / w
        arg = w * u + phi
        m = m + d * np.sin(arg)
        c = c + d * (math.cos(phi) - np.cos(arg)) / w
    mbar /= T
    a = g[12]
    s = 1.0 + m + a * (2.0 * u / T - 1.0) - mbar
    tau = u * (1.0 - mbar) + a * (u * u / T - u) + c
    tau = np.where(u <= 0.0, 0.0, np.where(u >= T, T, tau))
    return tau, s


def kernel_consts() -> dict:
    """``pe_pitch_mod_consts`` (host only): the wave kernel's tile, block, staged span and sinusoid limit."""
    consts = np.zeros(4, np.int64)
    _lib.check(_lib.load().pe_pitch_mod_consts(*host_ptrs(consts)), "pe_pitch_mod_consts")
    return dict(tile=int(consts[0]), block=int(consts[1]), span=int(consts[2]), max_sinusoids=int(consts[3]))


def frame_spans(lengths, crops, hop: int, max_frames: int = MAX_FRAMES):
    """``(spans (R, 2) int64, counts (R,) int64)``: the samples ``[t0, t1] = [crop hop, (crop + L - 1) hop]`` that the
    ``L = min(max_frames, 1 + n // hop - crop)`` kept label frames of each row cover (``L`` is 0 at the least)."""
    n, crop = i64(lengths), i64(crops)
    if n.size != crop.size:
        raise ValueError("pitch modulation: one crop per row")
    counts = np.maximum(np.minimum(int(max_frames), 1 + n // int(hop) - crop), 0)
    spans = np.stack([crop * int(hop), (crop + np.maximum(counts, 1) - 1) * int(hop)], axis=1)
    return spans.astype(np.int64), counts.astype(np.int64)


def _plan(lengths, x_off, y_off, spans, mods, sr, hop, who):
    """The C plan of R rows: ``mods[r]`` a ``Modulation`` or None (not selected).  Everything the plan refuses is a
    ``ValueError`` here first."""
    n, x_off, y_off = i64(lengths), i64(x_off), i64(y_off)
    R = int(n.size)
    spans = np.ascontiguousarray(spans, dtype=np.int64).reshape(-1, 2)
    mods = list(mods)
    if spans.shape[0] != R or len(mods) != R:
        raise ValueError(f"{who}: one span and one modulation (or None) per row")
    sr, hop = int(sr), int(hop)
    if sr <= 0 or hop <= 0:
        raise ValueError(f"{who}: sr and hop are positive")
    on = np.zeros(max(R, 1), np.int32)
    table = np.zeros((max(R, 1), 13), np.float64)
    for r, mod in enumerate(mods):
        if mod is None or mod.identity:
            continue
        t0, t1 = int(spans[r, 0]), int(spans[r, 1])
        table[r] = check_modulation(mod, t1 - t0, hop)
        if t0 < 0 or t1 > int(n[r]) or (t1 - t0) % hop:
            raise ValueError(f"{who}: row {r}'s span [{t0}, {t1}] is not whole hops within its {int(n[r])} samples")
        on[r] = 1
    t0s, t1s = np.ascontiguousarray(spans[:, 0]), np.ascontiguousarray(spans[:, 1])
    if R == 0:
        t0s = t1s = np.zeros(1, np.int64)
    meta = plan_meta("pe_pitch_mod_plan_fields", R)
    params = np.zeros((max(R, 1), PARAMS), np.float64)
    totals = np.zeros(2, np.int64)
    _lib.check(_lib.load().pe_pitch_mod_plan(R, *host_ptrs(n, x_off, y_off, t0s, t1s, on, table), sr, hop,
                                             *host_ptrs(meta, params, totals)), "pe_pitch_mod_plan")
    return dict(rows=R, meta=meta, params=params, tiles=int(totals[0]), warped=int(totals[1]), on=on[:R].astype(bool))


def filter_table(quality: str, device) -> torch.Tensor:
    """Device copy of ``pitch_shift.resample_filter(quality)`` as pairs ``{value, forward difference}`` (float32)."""
    def build():
        w = resample_filter(quality)
        d = np.zeros_like(w)
        d[:-1] = np.diff(w)
        return np.stack([w, d], axis=1).reshape(-1)
    return _lib.device_table(("pitch_mod", quality), device, build)


def modulate(waves: torch.Tensor, lengths, spans, mods, *, sr, hop, quality: str = "kaiser_fast", out=None,
             table_in_lds=None, return_plan: bool = False):
    """``pe_pitch_mod_wave``: row r of ``waves`` (one 1-D wave, rows packed with ``lengths``, or padded 2-D rows) read
    at ``t0 + tau(t - t0)`` over ``spans[r] = (t0, t1)`` under ``mods[r]`` (a ``Modulation``; None or an all-zero one:
    the row is copied), through ``pitch_shift.resample_filter(quality)`` with the cutoff ``min(1, 1 / s)`` per sample.
    The result has ``waves``' shape, zero outside the rows, or goes to ``out`` (another tensor, in any of the three
    layouts with the same row lengths: out of place).  Samples outside ``(t0, t1)`` are bit copies.  A row's result is
    bit-identical alone, packed at any offset, padded, in any batch order and into any stride.  ``table_in_lds``: where
    the filter table is read (default ``TABLE_IN_LDS[quality]``; same bits).  One launch.  ``ValueError`` for what
    ``check_modulation`` refuses and for a span that is not whole hops inside the row.  ``return_plan``: also the
    rows' plan, which ``modulate_labels`` takes as ``plan`` for the same rows, spans and modulations."""
    check_waves(waves, "pitch_mod.modulate")
    quality = check_res_type(quality)
    n, x_off = row_layout(waves, lengths, whole_by_default=True)
    if out is None:
        y = torch.zeros(tuple(waves.shape), dtype=torch.float32, device=waves.device)
    else:
        check_waves(out, "pitch_mod.modulate")
        y = out
        if y.device != waves.device or y.data_ptr() == waves.data_ptr():
            raise ValueError("pitch_mod.modulate: out is another tensor on waves' device (the kernel is out of place)")
    _, y_off = row_layout(y, n)
    pl = _plan(n, x_off, y_off, spans, mods, sr, hop, "pitch_mod.modulate")
    if pl["rows"] and pl["tiles"]:
        in_lds = TABLE_IN_LDS[quality] if table_in_lds is None else bool(table_in_lds)
        dev = waves.device
        meta_d, params_d = _device_copies(pl, dev)
        with torch.cuda.device(dev):
            ops._call("pe_pitch_mod_wave", waves.data_ptr(), meta_d.data_ptr(), pl["meta"].ctypes.data,
                      params_d.data_ptr(), pl["params"].ctypes.data, pl["rows"], filter_table(quality, dev).data_ptr(),
                      list(RES_TYPES).index(quality), int(in_lds), y.data_ptr(), _lib.stream_ptr())
    return (y, pl) if return_plan else y


def _device_copies(pl, dev):
    if "meta_d" not in pl or pl["meta_d"].device != dev:
        pl["meta_d"], pl["params_d"] = torch.from_numpy(pl["meta"]).to(dev), torch.from_numpy(pl["params"]).to(dev)
    return pl["meta_d"], pl["params_d"]


def modulate_labels(f0s: torch.Tensor, sils: torch.Tensor, counts, spans, hop, mods, *, sr, plan=None):
    """``pe_pitch_mod_labels``: ``(f0s, sils)`` (``(R, W)`` float32 device tensors, row r's ``counts[r]`` kept frames
    first) moved with the warp: frame ``j < counts[r]`` of a row with a modulation reads position ``tau(j hop) / hop``
    by ``world.time_warp_curve``'s rule over the row's own frames (a frame is voiced iff ``f0 > 0`` and its silence
    flag is 0); a voiced result becomes ``float32(s * value)`` with flag 0, an unvoiced one copies the nearer frame's
    ``f0`` and flag.  Everything else is copied.  ``spans[r] = (t0, t1)`` with ``t1 - t0 = (counts[r] - 1) hop`` for a
    row with a modulation.  ``plan``: what ``modulate(..., return_plan=True)`` returned for these rows, spans and
    modulations at this ``hop`` (saves making it again).  Returns new tensors.  One launch."""
    check_device_tensor(f0s, "pitch_mod.modulate_labels")
    check_device_tensor(sils, "pitch_mod.modulate_labels")
    if f0s.dim() != 2 or tuple(sils.shape) != tuple(f0s.shape) or sils.device != f0s.device:
        raise ValueError("pitch_mod.modulate_labels: f0s and sils are (rows, frames) tensors of one shape")
    R, W = int(f0s.shape[0]), int(f0s.shape[1])
    counts = i64(counts)
    spans = np.ascontiguousarray(spans, dtype=np.int64).reshape(-1, 2)
    mods = list(mods)
    if counts.size != R or spans.shape[0] != R or len(mods) != R:
        raise ValueError("pitch_mod.modulate_labels: one count, one span and one modulation (or None) per row")
    hop = int(hop)
    for r, mod in enumerate(mods):
        if mod is not None and not mod.identity and \
                (counts[r] > W or counts[r] < 2 or spans[r, 1] - spans[r, 0] != (counts[r] - 1) * hop):
            raise ValueError(f"pitch_mod.modulate_labels: row {r}'s span is not its {int(counts[r])} frames "
                             f"(at most {W}) at hop {hop}")
    if plan is not None:
        pl = plan
        if pl["rows"] != R:
            raise ValueError("pitch_mod.modulate_labels: the plan is of other rows")
    else:
        # the label pass reads no samples: the rows' lengths are only what makes the spans valid
        pl = _plan(np.maximum(spans[:, 1], 0) if R else [], np.zeros(R, np.int64), np.zeros(R, np.int64), spans, mods,
                   sr, hop, "pitch_mod.modulate_labels")
    f0_out, sil_out = torch.empty_like(f0s), torch.empty_like(sils)
    if R == 0 or W == 0:
        return f0_out, sil_out
    dev = f0s.device
    meta_d, params_d = _device_copies(pl, dev)
    with torch.cuda.device(dev):
        ops._call("pe_pitch_mod_labels", f0s.data_ptr(), sils.data_ptr(), meta_d.data_ptr(), pl["meta"].ctypes.data,
                  params_d.data_ptr(), pl["params"].ctypes.data, R, hop, W, f0_out.data_ptr(), sil_out.data_ptr(),
                  _lib.stream_ptr())
    return f0_out, sil_out


# ----------------------------------------------------------------------------------------------------------- the config
SINUSOIDS = ("vibrato", "flutter", "drift")                   # the 1st, 2nd and 3rd sinusoid of a row's Modulation
CONFIG_KEYS = ("enabled", "seed", "p", "apply_to_validation", "apply_to_synthetic", "quality") + SINUSOIDS + ("glide",)
DEFAULTS = {
    "vibrato": {"p": 0.0, "depth_cents": (10.0, 60.0), "rate_hz": (4.0, 7.5)},
    "flutter": {"p": 0.0, "depth_cents": (2.0, 10.0), "rate_hz": (8.0, 16.0)},
    "drift": {"p": 0.0, "depth_cents": (5.0, 30.0), "rate_hz": (0.2, 1.5)},
    "glide": {"p": 0.0, "cents": (-150.0, 150.0)},
}
DRAWS = 16                                                     # uniforms per row and call, whatever the config holds


def cents_to_depth(cents):
    """``d = 2^(c / 1200) - 1``: the relative frequency excursion of ``c`` cents."""
    return 2.0 ** (np.asarray(cents, dtype=np.float64) / 1200.0) - 1.0


def _range(value, what, lowest=None):
    try:
        lo, hi = (value, value) if np.ndim(value) == 0 else value
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError(f"pitch_modulation: {what} must be a number or [lo, hi]") from None
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi or (lowest is not None and lo < lowest):
        raise ValueError(f"pitch_modulation: {what} must be a finite range lo <= hi"
                         f"{'' if lowest is None else f' with lo >= {lowest}'}, got {value!r}")
    return lo, hi


def _probability(value, what):
    try:
        p = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"pitch_modulation: {what} must be a probability") from None
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"pitch_modulation: {what} must lie in [0, 1], got {value!r}")
    return p


def check_config(config) -> dict:
    """The ``pitch_modulation`` block with its defaults filled in.  ``ValueError``: an unknown key or option, a
    probability outside [0, 1], a range that is not finite ``lo <= hi`` (depths and rates: ``lo >= 0`` / ``>= 0.05``
    Hz), an unknown quality, or ranges whose largest draw could exceed the cap ``2 sum|d| + |a| <= 0.5``."""
    if config is None:
        config = {}
    if not isinstance(config, dict):
        raise ValueError("pitch_modulation: the config must be a mapping")
    for k in config:
        if k not in CONFIG_KEYS:
            raise ValueError(f"pitch_modulation: {k!r} is not an option (known: {CONFIG_KEYS})")
    out = {"enabled": bool(config.get("enabled", True)), "seed": int(config.get("seed", 0)),
           "p": _probability(config.get("p", 1.0), "p"),
           "apply_to_validation": bool(config.get("apply_to_validation", False)),
           "apply_to_synthetic": bool(config.get("apply_to_synthetic", False))}
    try:
        out["quality"] = check_res_type(config.get("quality", "kaiser_fast"))
    except (ValueError, TypeError):
        raise ValueError(f"pitch_modulation: quality must be one of {sorted(RES_TYPES)}") from None
    worst = 0.0
    for name in SINUSOIDS + ("glide",):
        given = config.get(name)
        given = {} if given is None else given
        if not isinstance(given, dict):
            raise ValueError(f"pitch_modulation: {name} must be a mapping")
        for k in given:
            if k not in DEFAULTS[name]:
                raise ValueError(f"pitch_modulation: {name} has no option {k!r} (it has {sorted(DEFAULTS[name])})")
        blk = {**DEFAULTS[name], **given}
        blk["p"] = _probability(blk["p"], f"{name}.p")
        if name == "glide":
            blk["cents"] = _range(blk["cents"], "glide.cents")
            reach = float(np.max(np.abs(cents_to_depth(blk["cents"])))) / 2.0
        else:
            blk["depth_cents"] = _range(blk["depth_cents"], f"{name}.depth_cents", lowest=0.0)
            blk["rate_hz"] = _range(blk["rate_hz"], f"{name}.rate_hz", lowest=MIN_RATE_HZ)
            reach = 2.0 * float(cents_to_depth(blk["depth_cents"][1]))
        if blk["p"] > 0:
            worst += reach
        out[name] = blk
    if worst > CAP:
        raise ValueError(f"pitch_modulation: the ranges allow 2 sum|d| + |a| = {worst:.4f}, above the cap {CAP}")
    return out


@dataclass(frozen=True)
class PitchModPlan:
    """What ``PitchModulator.draw`` drew for R rows, on the host: ``on`` (the rows selected) and one ``Modulation`` per
    row, drawn for every row, selected or not."""
    rows: int
    on: np.ndarray
    mods: tuple

    def without(self, rows) -> "PitchModPlan":
        """The plan with ``rows`` not selected."""
        keep = np.ones(self.rows, bool)
        keep[np.asarray(list(rows), dtype=np.int64)] = False
        return replace(self, on=self.on & keep)


class PitchModulator:
    """``PitchModulator(config, sr, hop, seed=0, rank=0)``: the checked ``pitch_modulation`` block of a loader at
    sample rate ``sr`` and label hop ``hop``; its generator is seeded with ``(seed, rank)``.  See the module's head."""

    def __init__(self, config, sr, hop, seed=0, rank=0):
        self.sr, self.hop = int(sr), int(hop)
        if self.sr <= 0 or self.hop <= 0:
            raise ValueError("pitch_modulation: sr and hop are positive")
        self.config = check_config(config)
        self.rng = np.random.Generator(np.random.PCG64([int(seed) & (2 ** 63 - 1), int(rank)]))

    @property
    def active(self) -> bool:
        cfg = self.config
        return cfg["enabled"] and cfg["p"] > 0 and any(cfg[k]["p"] > 0 for k in SINUSOIDS + ("glide",))

    def draw(self, n_rows: int) -> PitchModPlan:
        """The plan of ``n_rows`` rows: per call one ``(n_rows, 16)`` block of uniforms from the modulator's generator,
        whatever the config holds.  Column 0 selects the row, 1-4 its vibrato, flutter, drift and glide, 5-7 the depths
        (uniform in cents), 8-10 the rates (log-uniform), 11-13 the phases, 14 the glide's cents."""
        R, cfg = int(n_rows), self.config
        u = self.rng.random((R, DRAWS))
        on = (u[:, 0] < cfg["p"]) & cfg["enabled"]
        mods = []
        for r in range(R):
            comps = []
            for k, name in enumerate(SINUSOIDS):
                blk = cfg[name]
                if u[r, 1 + k] < blk["p"]:
                    lo, hi = blk["depth_cents"]
                    d = float(cents_to_depth(lo + (hi - lo) * u[r, 5 + k]))
                    lo, hi = blk["rate_hz"]
                    rate = math.exp(math.log(lo) + (math.log(hi) - math.log(lo)) * u[r, 8 + k])
                    comps.append((d, rate, 2.0 * math.pi * u[r, 11 + k]))
                else:
                    comps.append((0.0, 0.0, 0.0))
            a = 0.0
            if u[r, 4] < cfg["glide"]["p"]:
                lo, hi = cfg["glide"]["cents"]
                a = float(cents_to_depth(lo + (hi - lo) * u[r, 14])) / 2.0
            mods.append(Modulation(tuple(comps), a))
        return PitchModPlan(rows=R, on=on, mods=tuple(mods))

    def apply(self, waves: torch.Tensor, lengths, crops, f0s: torch.Tensor, sils: torch.Tensor, plan: PitchModPlan):
        """The stage over a ragged batch and its labels: row r, if the plan selected it and it keeps at least two label
        frames, is warped over the span of its ``L = min(f0s.shape[1], 1 + n // hop - crop)`` kept frames and its
        labels move with it.  Returns ``(waves, f0s, sils)``: new tensors of the same shapes, the inputs themselves
        when no row is warped.  Rows not selected are bit copies."""
        check_waves(waves, "PitchModulator.apply")
        n, _ = row_layout(waves, lengths, whole_by_default=True)
        if len(n) != plan.rows or f0s.shape[0] != plan.rows:
            raise ValueError(f"PitchModulator.apply: a plan of {plan.rows} rows for {len(n)}")
        spans, counts = frame_spans(n, crops, self.hop, int(f0s.shape[1]))
        mods = [m if plan.on[r] and counts[r] >= 2 and not m.identity else None for r, m in enumerate(plan.mods)]
        if all(m is None for m in mods):
            return waves, f0s, sils
        y, pl = modulate(waves, lengths, spans, mods, sr=self.sr, hop=self.hop, quality=self.config["quality"],
                         return_plan=True)
        f0_out, sil_out = modulate_labels(f0s.contiguous(), sils.contiguous(), counts, spans, self.hop, mods,
                                          sr=self.sr, plan=pl)
        return y, f0_out, sil_out
