"""The mix at an SNR through its two entry points on fixed inputs, reduced to digests of the output bits.

Shared by tests/golden/make_snr_mix_parent_golden.py, which recorded the digests with the build BEFORE ``pe_noise_mix``
and ``pe_stim_finish`` took their rms, mix, peak and normalise steps from one place, and tests/test_snr_mix_parity_gpu.py,
which holds today's build to them: the calls below use only what both builds have (``noise.mix_at_snr``,
``noise.plan_rows`` / ``to_device`` with ``pe_noise_mix`` as tools/bench_noise.py calls it, ``stimuli.timbre_row`` /
``plan_rows`` / ``finish``).  Inputs are integer arithmetic alone (a multiplicative hash of the sample index mapped to
[-1, 1) in float64, then float32), so they do not depend on a library's generator.

Rows of 0 (``mix_at_snr`` only), 1, 7, 2047, 2048, 2049 and 6149 samples, each alone, packed at an odd offset and
padded; among them quiet rows (peak <= 0.99) and loud ones (> 0.99), a silent signal, an all-zero noise, a stimuli row
without noise next to rows with one, one SNR per row, ``peak_normalize=False``, a noise plan with a warm-up (its piece
counts are of warm-up + n samples, the mix's of n), and one row of 526 337 samples (258 pieces: more piece sums than
one 256-wide walk of the row rms takes).
"""
import hashlib

import numpy as np
import torch

from pitchextractor_amd import _lib, noise as N, ops, stimuli as S

f32 = np.float32
LONG = 526337
# (samples, amplitude, snr_db, what): what is "" or the part that is all zeros
MIX_ROWS = ([(n, 0.25, (20.0, 10.0, 0.0, -5.0)[k % 4], "") for k, n in enumerate((0, 1, 7, 2047, 2048, 2049, 6149))]
            + [(2049, 0.9, 0.0, ""), (6149, 0.9, -5.0, ""), (2049, 0.25, 20.0, "signal"), (2049, 0.25, 60.0, "noise")])
LOUD = (7, 8)
# (samples, amplitude, snr_db or None: no noise, what) at a sample rate whose fade is 1 sample, and at one of 6
STIM_SETS = {
    60: [(1, 0.25, 20.0, ""), (7, 0.25, None, ""), (7, 0.25, 10.0, ""), (2047, 0.25, 0.0, ""), (2048, 1.0, None, ""),
         (2048, 0.25, -5.0, ""), (2049, 0.9, 0.0, ""), (6149, 0.25, None, ""), (6149, 0.9, -5.0, ""),
         (2049, 0.25, 20.0, "signal"), (2049, 0.25, 60.0, "noise")],
    300: [(7, 0.25, 10.0, ""), (2047, 0.9, 0.0, ""), (2048, 0.25, None, ""), (2049, 0.25, 20.0, ""),
          (6149, 1.0, None, ""), (6149, 0.25, -5.0, "")],
}


def values(n, salt, amplitude=1.0):
    """``n`` float32 values in [-amplitude, amplitude): a 32-bit multiplicative hash of the index, two rounds."""
    h = ((np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503))
    h &= np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    return ((h.astype(np.float64) / 2147483648.0 - 1.0) * float(amplitude)).astype(f32)


def row_inputs(r, n, amplitude, what):
    x = np.zeros(n, f32) if what == "signal" else values(n, 2 * r + 1, amplitude)
    z = np.zeros(n, f32) if what == "noise" else values(n, 2 * r + 2)
    return x, z


def digest(t: torch.Tensor) -> str:
    """sha256 of the tensor's bytes."""
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _layouts(lengths):
    """Per layout ``(offsets, extent)``: packed behind one sample of slack, so that rows start at odd offsets."""
    lengths = np.asarray(lengths, np.int64)
    packed = 1 + np.cumsum(lengths) - lengths
    width = int(lengths.max()) + 3
    return {"packed": (packed.tolist(), int(1 + lengths.sum() + 3)),
            "padded": ([r * width for r in range(lengths.size)], width * int(lengths.size))}


# ------------------------------------------------------------------------------------------------------- pe_noise_mix
def _raw_noise_mix(x, z, lengths, offsets, snr, warmup, peak_normalize, dev):
    """``pe_noise_mix`` on a plan of any offsets and warm-ups, as tools/bench_noise.py calls it."""
    pl = N.to_device(N.plan_rows(lengths, offsets, warmup=warmup), dev)
    snr = np.ascontiguousarray(snr, np.float64)
    snr_d = torch.from_numpy(snr).to(dev)
    y = torch.zeros_like(x)
    stats = torch.zeros((pl["rows"], pl["stat_fields"]), dtype=torch.float64, device=dev)
    n_bytes = _lib.load().pe_noise_workspace_bytes(pl["n_pieces"])
    ws = torch.empty((max(n_bytes, 1),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        ops._call("pe_noise_mix", x.data_ptr(), z.data_ptr(), pl["meta_d"].data_ptr(), pl["meta"].ctypes.data,
                  snr_d.data_ptr(), snr.ctypes.data, int(peak_normalize), pl["rows"], y.data_ptr(), stats.data_ptr(),
                  ws.data_ptr(), n_bytes, _lib.stream_ptr())
    return y, stats


def run_mix_cases(dev):
    """{case: (y, stats)} of ``noise.mix_at_snr`` / ``pe_noise_mix``."""
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    rows = [row_inputs(r, n, amp, what) for r, (n, amp, _, what) in enumerate(MIX_ROWS)]
    lengths = [n for n, _, _, _ in MIX_ROWS]
    snr = [s for _, _, s, _ in MIX_ROWS]
    out = {}
    for r, (x, z) in enumerate(rows):
        out[f"mix/alone/{r}"] = N.mix_at_snr(up(x), up(z), snr[r], return_stats=True)

    def laid(k, offsets, extent, pick=range(len(rows))):
        a = np.full(extent, 3.0, f32)                                  # what lies between the rows is not silence
        for r, o in zip(pick, offsets):
            a[o:o + lengths[r]] = rows[r][k]
        return a

    lay = _layouts(lengths)
    offsets, extent = lay["padded"]
    width = extent // len(rows)
    out["mix/padded"] = N.mix_at_snr(up(laid(0, offsets, extent).reshape(len(rows), width)),
                                     up(laid(1, offsets, extent).reshape(len(rows), width)), snr, lengths,
                                     return_stats=True)
    # packed at odd offsets, and the same with a warm-up in the plan: through the entry point, which takes offsets
    offsets, extent = lay["packed"]
    assert offsets[3] % 2 == 1 and offsets[6] % 2 == 1
    warm = [(0, 5000, 3, 2048, 1, 4096, 7)[r % 7] for r in range(len(rows))]
    for name, warmup, peak in (("mix/packed", 0, 1), ("mix/packed_warmup_plan", warm, 1), ("mix/packed_no_peak", 0, 0)):
        out[name] = _raw_noise_mix(up(laid(0, offsets, extent)), up(laid(1, offsets, extent)), lengths, offsets, snr,
                                   warmup, peak, dev)
    # without the peak rule through the public call: the loud rows, packed from 0
    out["mix/loud_no_peak"] = N.mix_at_snr(up(np.concatenate([rows[r][0] for r in LOUD])),
                                           up(np.concatenate([rows[r][1] for r in LOUD])), [snr[r] for r in LOUD],
                                           [lengths[r] for r in LOUD], peak_normalize=False, return_stats=True)
    x, z = row_inputs(100, LONG, 0.5, "")
    out["mix/long"] = N.mix_at_snr(up(x), up(z), 3.0, return_stats=True)
    return out


# ----------------------------------------------------------------------------------------------------- pe_stim_finish
def stim_spec(n, sr, snr_db):
    """A one-partial tone row of exactly ``n`` samples; ``finish`` reads its length, fade and ``snr_db`` alone."""
    profile = {"partials": {1: 1.0}} if snr_db is None else {"partials": {1: 1.0}, "snr_db": snr_db}
    row = S.timbre_row(1.0, profile, (n + 0.5) / sr, sr)
    assert row["n"] == n
    return row


def _finish(rows, inputs, sr, offsets, extent, dev):
    """``stimuli.finish`` of ``rows`` (indices into ``inputs``) laid out at ``offsets`` of a ``y`` of ``extent``."""
    specs = [stim_spec(inputs[r][2], sr, inputs[r][3]) for r in rows]
    pl = S.plan_rows(specs, sr, offsets)
    y = np.full(extent, 3.0, f32)
    for r, o in zip(rows, pl["offsets"].tolist()):
        y[o:o + inputs[r][2]] = inputs[r][0]
    noise = [inputs[r][1] for r in rows if inputs[r][3] is not None]
    noise_d = torch.from_numpy(np.concatenate(noise)).to(dev) if noise else None
    return S.finish(pl, torch.from_numpy(y).to(dev), noise_d, return_stats=True)


def run_stim_cases(dev):
    """{case: (y, stats)} of ``stimuli.finish``."""
    out = {}
    for sr, table in STIM_SETS.items():
        inputs = [row_inputs(50 + r, n, amp, what) + (n, s) for r, (n, amp, s, what) in enumerate(table)]
        every = list(range(len(table)))
        for r in every:
            out[f"stim{sr}/alone/{r}"] = _finish([r], inputs, sr, None, max(table[r][0], 1), dev)
        for name, (offsets, extent) in _layouts([n for n, _, _, _ in table]).items():
            out[f"stim{sr}/{name}"] = _finish(every, inputs, sr, offsets, extent, dev)
    inputs = [row_inputs(101, LONG, 0.5, "") + (LONG, 3.0)]
    out["stim24000/long"] = _finish([0], inputs, 24000, None, LONG, dev)
    return out


def run_cases(dev):
    out = run_mix_cases(dev)
    out.update(run_stim_cases(dev))
    return out


def digests(cases):
    return {name: {"y": digest(y), "stats": digest(st)} for name, (y, st) in cases.items()}
