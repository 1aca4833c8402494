"""CheapTrick, D4C and the resynthesis on top of both on fixed rows, reduced to digests of the output bits.

Shared by tests/golden/make_world_frames_parent_golden.py, which recorded the digests with the build BEFORE the two
analyses took their frame plan, DC correction and interval mean from csrc/world_frames.h, and
tests/test_world_frames_parity_gpu.py, which holds today's build to them: the calls below use only what both builds have
(``world.cheaptrick_ragged``, ``world.d4c_ragged``, ``world.resynthesize``).

The rows are those of ``tests/d4c_cases.rows``: a vowel over noise, a glide through 47 and 40 Hz, unvoiced stretches
with a NaN frame, one frame, zeros, a quiet passage after a loud one, a row shorter than a window and F0 = 1000 Hz
(interval sums of 85 terms).  CheapTrick at one configuration per transform size (512, 1024, 2048), D4C at one band, at
three bands with every voiced frame through the band analysis, at N_d = 4096 and at N_l = N_d / 2.  Each configuration
runs as one ragged launch, and once more with ``frames=`` sub-ranges on two rows.
"""
import hashlib

import numpy as np
import torch

from pitchextractor_amd import world
from tests import d4c_cases as dc

Q1 = -0.15
CHEAPTRICK_CONFIGS = [(8000, 5.0), (24000, 5.0), (48000, 5.0)]                  # fft_size 512, 1024, 2048
D4C_CONFIGS = [(16000, 5.0, 0.85), (24000, 12.5, 0.0), (48000, 5.0, 0.85), (25000, 10.0, 0.85)]
ROWS = ("vowel_noise", "glide_47_40", "unvoiced_stretches", "one_frame", "zeros", "quiet_after_loud",
        "shorter_than_a_window", "f0_1000")
RESYNTHESIS = (24000, 5.0, 3.0, 20240)                                          # fs, frame period, semitones up, seed
CASES = sorted([f"cheaptrick/fs{fs}-fp{fp}/{tag}" for fs, fp in CHEAPTRICK_CONFIGS for tag in ("batch", "frames")] +
               [f"d4c/fs{fs}-fp{fp}-thr{thr}/{tag}" for fs, fp, thr in D4C_CONFIGS for tag in ("batch", "frames")] +
               [f"resynthesize/fs{RESYNTHESIS[0]}-fp{RESYNTHESIS[1]}-d4c"])


def digest(t) -> str:
    """sha256 of the float32 bytes."""
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    assert a.dtype == np.float32
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def sub_ranges(rows):
    """Per row ``(first_frame, n_frames)``: a stretch inside ``vowel_noise``, one of ``unvoiced_stretches`` that spans
    its unvoiced frames and ends on the NaN frame, every frame of the others."""
    out = []
    for name in ROWS:
        L = rows[name][1].size
        out.append({"vowel_noise": (3, min(7, L - 3)), "unvoiced_stretches": (L // 3 - 1, L - 2 - (L // 3 - 1))}
                   .get(name, (0, L)))
    return out


def _batch(rows, dev):
    xs = [rows[n][0] for n in ROWS]
    x = torch.from_numpy(np.concatenate(xs)).to(dev)
    return x, [len(a) for a in xs], [rows[n][1].copy() for n in ROWS]


def run_cheaptrick(dev, cfg):
    """{case: {row: {"sp": digest}}} of one configuration."""
    fs, fp = cfg
    rows = dc.rows(fs, fp)
    x, lengths, f0s = _batch(rows, dev)
    out = {}
    for tag, frames in (("batch", None), ("frames", sub_ranges(rows))):
        env = world.cheaptrick_ragged(x, lengths, f0s, fs, fp, q1=Q1, frames=frames)
        assert env.fft_size == {8000: 512, 24000: 1024, 48000: 2048}[fs]
        out[f"cheaptrick/fs{fs}-fp{fp}/{tag}"] = {n: {"sp": digest(env.row(r))} for r, n in enumerate(ROWS)}
    return out


def run_d4c(dev, cfg):
    """{case: {row: {"ap": digest, "bands": digest}}} of one configuration."""
    fs, fp, thr = cfg
    rows = dc.rows(fs, fp)
    x, lengths, f0s = _batch(rows, dev)
    out = {}
    for tag, frames in (("batch", None), ("frames", sub_ranges(rows))):
        env, bands = world.d4c_ragged(x, lengths, f0s, fs, fp, threshold=thr, frames=frames, return_bands=True)
        ends = np.cumsum(env.counts)
        out[f"d4c/fs{fs}-fp{fp}-thr{thr}/{tag}"] = {
            n: {"ap": digest(env.row(r)), "bands": digest(bands[ends[r] - env.counts[r]:ends[r]])}
            for r, n in enumerate(ROWS)}
    return out


def run_resynthesis(dev):
    fs, fp, semitones, seed = RESYNTHESIS
    x, f0 = dc.rows(fs, fp)["vowel_noise"]
    new = f0.astype(np.float64) * 2.0 ** (semitones / 12.0)
    y, label = world.resynthesize(torch.from_numpy(x.copy()).to(dev), f0.copy(), new, fs, fp, ap="d4c", seed=seed)
    return {f"resynthesize/fs{fs}-fp{fp}-d4c": {"vowel_noise": {"audio": digest(y),
                                                                 "label": digest(label.astype(np.float32))}}}


def run_cases(dev):
    """{case: {row: {what: digest}}} of every case."""
    out = {}
    for cfg in CHEAPTRICK_CONFIGS:
        out.update(run_cheaptrick(dev, cfg))
    for cfg in D4C_CONFIGS:
        out.update(run_d4c(dev, cfg))
    out.update(run_resynthesis(dev))
    return out
