"""Room impulse responses made on the device (``csrc/rir_synth.hip``): the image-source response of shoebox rooms
(Allen & Berkley 1979 with a windowed-sinc fractional delay), their decay time by Schroeder backward integration, the
calibration of a uniform wall coefficient to a decay time, and the nine-entry library that the reference's
Utils/room_and_microphone_stress.ipynb reads from ``ImpulseResponses/{small_room,office,hall}_t60_*.wav``, files that
neither project ships.  There is no CPU path.  ``tests/rir_ref.py`` is the float64 restatement that pins every stage.

A room is a dict ``{"dims": (Lx, Ly, Lz), "source": (x, y, z), "mic": (x, y, z), "beta": b, "n_samples": N}`` in
metres; ``beta`` is one reflection coefficient for every wall or six, ``[x0, x1, y0, y1, z0, z1]`` (the wall at
coordinate 0, the wall at ``L``).  A batch of rooms is ragged the way every audio batch here is: responses packed back
to back, or at ``offsets`` of an output (a padded one: ``r * width``).  A response is bit-identical whether it is made
alone, in a batch in any order, at an odd offset or padded: its samples are sums of integers.  One launch per call,
whatever the rooms."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, ops, stress
from .ragged import (check_device_tensor, check_waves, gpu_device, host_ptrs, i64, packed_offsets, plan_extent,
                     plan_meta, plan_output, row_layout)

DECAY_KEYS = ("t60", "slope", "intercept", "k_lo", "k_hi", "db_last")
# Build-defined: the notebook only names its rooms.  Dimensions, an off-centre source and a microphone, in metres.
ROOMS = {
    "small_room": {"dims": (4.0, 3.2, 2.6), "source": (1.3, 1.1, 1.5), "mic": (2.9, 2.2, 1.2)},
    "office": {"dims": (6.0, 4.5, 2.8), "source": (1.7, 1.4, 1.5), "mic": (4.1, 3.0, 1.2)},
    "hall": {"dims": (20.0, 15.0, 8.0), "source": (6.3, 4.1, 1.7), "mic": (13.2, 9.4, 1.4)},
}
# Utils/room_and_microphone_stress.ipynb, CONFIG["rir_library"] and CONFIG["t60_sweep"]
LIBRARY_T60S = {"small_room": (0.30, 0.60, 0.90), "office": (0.45, 0.80, 1.20), "hall": (0.80, 1.10, 1.50)}
T60_SWEEP = tuple(round(float(x), 2) for x in np.linspace(0.2, 1.5, 14))
BETA_RANGE = (0.0, 0.9999)


def _consts() -> dict:
    consts, totals = np.zeros(4, np.int64), np.zeros(2, np.int64)
    _lib.check(_lib.load().pe_rir_plan(0, None, None, *host_ptrs(consts), None, None, 0, *host_ptrs(totals)),
               "pe_rir_plan")
    return dict(tile=int(consts[0]), param_fields=int(consts[1]), tile_fields=int(consts[2]),
                decay_fields=int(consts[3]))


def room_params(rooms, fs, c=343.0, max_order=None) -> np.ndarray:
    """The ``(rows, 19)`` float64 table of ``pe_rir_plan``: dims, source, mic, six betas, fs, c, N, max_order (-1:
    none).  ``ValueError`` for a room that lacks a key or has the wrong number of values."""
    rows = []
    for room in rooms:
        try:
            dims, source, mic = (np.asarray(room[k], dtype=np.float64).reshape(-1) for k in ("dims", "source", "mic"))
            beta = np.asarray(room["beta"], dtype=np.float64).reshape(-1)
            n = room["n_samples"]
        except KeyError as e:
            raise ValueError(f"rir: a room needs dims, source, mic, beta and n_samples; {e} is missing") from None
        if beta.size == 1:
            beta = np.full(6, beta[0])
        if dims.size != 3 or source.size != 3 or mic.size != 3 or beta.size != 6:
            raise ValueError("rir: dims, source and mic have three values, beta one or six")
        rows.append([*dims, *source, *mic, *beta, float(fs), float(c), float(n), -1.0 if max_order is None else
                     float(max_order)])
    return np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(len(rows), 19))


def plan_rooms(rooms, fs, c=343.0, max_order=None, offsets=None) -> dict:
    """``pe_rir_plan`` (host only): the checked rooms, the row plan and the tile table.  ``ValueError`` for a room the
    plan refuses (PE_E_ARG); a size the kernel cannot serve raises ``HipLibraryError`` (PE_E_UNSUPPORTED)."""
    lib = _lib.load()
    params = room_params(rooms, fs, c, max_order)
    R = int(params.shape[0])
    off = None if offsets is None else i64(offsets)
    if off is None:
        n = np.asarray([int(p[17]) if math.isfinite(p[17]) else 0 for p in params], dtype=np.int64)
        off = packed_offsets(np.maximum(n, 0))
    if off.size != R:
        raise ValueError("rir plan: one offset per room")
    meta = plan_meta("pe_rir_plan_fields", R)
    consts, totals = np.zeros(4, np.int64), np.zeros(2, np.int64)

    def call(tiles):
        status = lib.pe_rir_plan(R, *host_ptrs(params, off, consts, meta, tiles), 0 if tiles is None else
                                 tiles.shape[0], *host_ptrs(totals))
        if status == -1:
            raise ValueError("rir plan: pe_rir_plan refused a room (PE_E_ARG): dimensions, fs and c positive and "
                             "finite, source and microphone strictly inside and at least 1 cm apart, beta in [0, 1], "
                             "n_samples >= 1, max_order >= 0 or None")
        _lib.check(status, "pe_rir_plan")

    call(None)
    tiles = np.zeros((max(int(totals[1]), 1), int(consts[2])), np.int64)
    call(tiles)
    lengths = meta[:R, 1].copy() if R else np.zeros(0, np.int64)
    return dict(rows=R, params=params, offsets=off, lengths=lengths, meta=meta, tiles=tiles, tile=int(consts[0]),
                n_samples=int(totals[0]), n_tiles=int(totals[1]))


def synthesize(rooms, fs, c=343.0, max_order=None, device="cuda", out=None, offsets=None):
    """``pe_rir_synth``: ``(h, lengths)``, the image-source responses of ``rooms`` as float32 on the device, packed
    back to back (or written at ``offsets`` of ``out``, a contiguous float32 device tensor of any shape, whose other
    elements are left alone) and their lengths.  ``max_order``: the largest reflection count of an image (default: all
    that arrive before the response ends).  One launch."""
    rooms = list(rooms)
    if out is not None:
        check_device_tensor(out, "rir.synthesize")
    device = gpu_device(out.device if out is not None else device, "rir")
    pl = plan_rooms(rooms, fs, c, max_order, offsets)
    R = pl["rows"]
    lengths = [int(n) for n in pl["lengths"]]
    y = plan_output(pl, out, device, "rir.synthesize", "the output is shorter than the rooms' responses")
    if R:
        meta_d = torch.from_numpy(pl["meta"]).to(device)
        params_d = torch.from_numpy(pl["params"]).to(device)
        tiles_d = torch.from_numpy(pl["tiles"]).to(device)
        with torch.cuda.device(device):
            ops._call("pe_rir_synth", meta_d.data_ptr(), pl["meta"].ctypes.data, params_d.data_ptr(),
                      pl["params"].ctypes.data, tiles_d.data_ptr(), pl["tiles"].ctypes.data, R, y.data_ptr(),
                      y.numel(), _lib.stream_ptr())
    return (y if out is not None else y[:plan_extent(pl)]), lengths


def measure_t60(h, lengths=None, fs=24000, lo_db=-5.0, hi_db=-25.0, return_curve: bool = False):
    """``pe_rir_decay``: Schroeder's backward integration of every row of ``h`` (packed with ``lengths``, padded, or
    one response) and the least-squares line of the decay curve between its first samples below ``lo_db`` and below
    ``hi_db``.  Returns a dict of float64 arrays, one value per row, under ``DECAY_KEYS``: ``t60 = -60 / slope``,
    ``slope`` (dB / s), ``intercept`` (dB), ``k_lo``, ``k_hi`` (the row's length when the threshold is never reached)
    and ``db_last``, the curve's last value.  ``t60`` is NaN when the response never reaches ``hi_db`` or the line has
    fewer than two points.  ``return_curve``: also the decay curve in dB, float32, of ``h``'s shape.  One launch."""
    check_waves(h, "measure_t60")
    h = h.contiguous()
    row_lengths, offsets = row_layout(h, lengths, whole_by_default=True)
    R = len(row_lengths)
    meta = np.zeros((max(R, 1), 2), np.int64)
    meta[:R, 0], meta[:R, 1] = offsets, row_lengths
    fields = _consts()["decay_fields"]
    out = torch.full((max(R, 1), fields), float("nan"), dtype=torch.float64, device=h.device)
    curve = torch.zeros(tuple(h.shape), dtype=torch.float32, device=h.device) if return_curve else None
    if R:
        meta_d = torch.from_numpy(meta).to(h.device)
        with torch.cuda.device(h.device):
            ops._call("pe_rir_decay", h.data_ptr(), h.numel(), meta_d.data_ptr(), meta.ctypes.data, 2, R, float(fs),
                      float(lo_db), float(hi_db), out.data_ptr(), _lib.ptr(curve), _lib.stream_ptr())
    table = out[:R].cpu().numpy()
    result = {key: table[:, j].copy() for j, key in enumerate(DECAY_KEYS)}
    return (result, curve) if return_curve else result


def eyring_beta(dims, t60) -> float:
    """The uniform reflection coefficient that Eyring's formula gives a room of ``dims`` a decay time of ``t60``
    with: ``sqrt(exp(-0.161 V / (S t60)))``.  A starting value: the shoebox model decays more slowly."""
    Lx, Ly, Lz = (float(v) for v in dims)
    t60 = float(t60)
    if not (min(Lx, Ly, Lz) > 0.0 and t60 > 0.0 and math.isfinite(t60)):
        raise ValueError("eyring_beta: dimensions and t60 must be positive")
    V, S = Lx * Ly * Lz, 2.0 * (Lx * Ly + Ly * Lz + Lx * Lz)
    return math.sqrt(math.exp(-0.161 * V / (S * t60)))


def calibrate(room, t60, fs, rtol=0.02, max_iter=20, tail=1.5, c=343.0, device="cuda", return_path: bool = False):
    """The uniform ``beta`` in ``[0, 0.9999]`` at which ``room`` (its own ``beta`` and ``n_samples`` are ignored)
    measures a decay time within ``rtol`` of ``t60``: bisection from Eyring's value with the length ``N = ceil(tail t60
    fs)`` held fixed, one ``synthesize`` and one ``measure_t60`` per step.  A response that never reaches -25 dB counts
    as too long, any other NaN as too short.  Returns ``(beta, measured t60, h)`` with ``h`` the response on the device
    (``return_path``: also the ``(beta, measured)`` of every step).  ``ValueError`` when ``max_iter`` steps do not reach
    the target."""
    t60 = float(t60)
    if not (t60 > 0.0 and math.isfinite(t60)):
        raise ValueError("calibrate: t60 must be positive")
    N = int(math.ceil(float(tail) * t60 * float(fs)))
    lo, hi = BETA_RANGE
    beta = min(max(eyring_beta(room["dims"], t60), lo), hi)
    path = []
    for _ in range(int(max_iter)):
        h, _lengths = synthesize([dict(room, beta=beta, n_samples=N)], fs, c, device=device)
        m = measure_t60(h, [N], fs)
        got, k_hi = float(m["t60"][0]), int(m["k_hi"][0])
        path.append((beta, got))
        if abs(got - t60) <= rtol * t60:
            return (beta, got, h, path) if return_path else (beta, got, h)
        too_long = k_hi >= N if math.isnan(got) else got > t60
        if too_long:
            hi = beta
        else:
            lo = beta
        beta = 0.5 * (lo + hi)
    raise ValueError(f"calibrate: {max_iter} steps did not bring the room within {rtol} of a T60 of {t60} s "
                     f"(last: beta {path[-1][0]!r}, {path[-1][1]!r} s)" if path else "calibrate: max_iter < 1")


class RirLibrary:
    """Calibrated responses of named rooms: ``entries`` (dicts ``room``, ``target_t60``, ``t60`` as measured, ``beta``,
    ``index``), the responses packed on the device (``h``, ``lengths``) and the sample rate ``fs``."""

    def __init__(self, fs, entries, h, lengths):
        self.fs, self.entries, self.h, self.lengths = fs, list(entries), h, [int(n) for n in lengths]
        self._rir_set = None

    def __len__(self):
        return len(self.entries)

    def responses(self) -> list:
        """The responses as float32 arrays on the host (one copy)."""
        packed = self.h.detach().cpu().numpy()
        offsets = packed_offsets(self.lengths)
        return [packed[o:o + n].copy() for o, n in zip(offsets.tolist(), self.lengths)]

    def rir_set(self) -> "stress.RirSet":
        """The ``stress.RirSet`` of the responses after ``stress.prepare_rir``, the notebook's load-time
        normalisation; entry ``index`` is its response ``index``.  Made once."""
        if self._rir_set is None:
            self._rir_set = stress.RirSet([stress.prepare_rir(h) for h in self.responses()])
        return self._rir_set

    def select(self, room, target_t60):
        """The notebook's ``_select_rir``: the entry of ``room`` whose measured T60 is nearest ``target_t60``, the
        first on a tie; ``None`` when the room has none."""
        valid = [e for e in self.entries if e["room"] == room and e.get("t60") is not None]
        if not valid:
            return None
        return min(valid, key=lambda e: abs(float(e["t60"]) - float(target_t60)))

    def conditions(self, t60_sweep=None) -> list:
        """The ``stress.Condition("rir", ...)`` list of the notebook's sweep: per room in order of first appearance
        and per target of ``t60_sweep`` (default ``T60_SWEEP``) the selected response.  Every condition's parameters
        also carry ``room``, ``target_t60`` and ``rir_t60``, and its label names the three."""
        sweep = T60_SWEEP if t60_sweep is None else [float(t) for t in t60_sweep]
        rooms = list(dict.fromkeys(e["room"] for e in self.entries))
        rirs = self.rir_set()
        out = []
        for room in rooms:
            for target in sweep:
                e = self.select(room, target)
                out.append(stress.Condition("rir", f"{room} target_t60={float(target):.2f} rir_t60={e['t60']:.3f}",
                                            rirs=rirs, rir_index=int(e["index"]), room=room,
                                            target_t60=float(target), rir_t60=float(e["t60"])))
        return out


def room_library(fs, rooms=None, t60s=None, rtol=0.02, max_iter=20, tail=1.5, c=343.0, device="cuda") -> RirLibrary:
    """The notebook's impulse-response library: every room of ``rooms`` (name -> ``{"dims", "source", "mic"}``,
    default ``ROOMS``) calibrated to each decay time of ``t60s[name]`` (default ``LIBRARY_T60S``: 0.30 / 0.60 / 0.90,
    0.45 / 0.80 / 1.20 and 0.80 / 1.10 / 1.50 s), then all of them measured again as one batch."""
    rooms = ROOMS if rooms is None else rooms
    t60s = LIBRARY_T60S if t60s is None else t60s
    device = gpu_device(device, "rir")
    entries, parts = [], []
    for name, room in rooms.items():
        for target in t60s[name]:
            beta, _got, h = calibrate(room, target, fs, rtol, max_iter, tail, c, device)
            entries.append(dict(room=name, target_t60=float(target), beta=beta, index=len(entries)))
            parts.append(h)
    if not entries:
        raise ValueError("room_library: no room")
    lengths = [int(h.numel()) for h in parts]
    packed = torch.cat(parts)
    measured = measure_t60(packed, lengths, fs)["t60"]
    for e, t in zip(entries, measured.tolist()):
        e["t60"] = float(t)
    return RirLibrary(fs, entries, packed, lengths)
