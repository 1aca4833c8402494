"""Device cost of the pitch-shift augmentation (synthetic_data.pitch_shift) per training batch.

B = 256 rows of 2 s at 24 kHz, 64 of them synthetic (the shipped config's ratio 0.25 -> one item in five): times
(a) the four pitch-shift stages for the 64 rows alone, (b) one DeviceMelLoader device step -- the ragged mel launch --
without synthetic rows, and (c) the same step with the 64 rows shifted into the batch first.  Prints one JSON line.
Estimate for (a), not measured: about 1 GFLOP and 0.2 GB of traffic; budget 1 ms."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pitchextractor_amd import pitch_shift as ps  # noqa: E402
from pitchextractor_amd import synthetic  # noqa: E402
from pitchextractor_amd.mel import MelSpectrogram  # noqa: E402

B, K, N, SR, reps = 256, 64, 48000, 24000, 50
dev = torch.device("cuda:0")
waves_np, _, _ = synthetic.batch(0, 8)
waves = torch.from_numpy(np.tile(waves_np, (B // 8, 1))).to(dev)
lengths = torch.full((B,), N, dtype=torch.int32, device=dev)
crops = torch.zeros((B,), dtype=torch.int32, device=dev)
rows = np.arange(0, B, B // K)[:K]
steps = np.array([-4, -2, -1, 1, 2, 4] * 11)[:K]
src = waves[torch.from_numpy(rows).to(dev)].reshape(-1).contiguous()
gains = torch.rand(K, device=dev) + 0.5
tf = MelSpectrogram(sample_rate=SR, n_fft=1024, win_length=1024, hop_length=300, n_mels=80)
offs = np.arange(K) * N
lens = np.full(K, N)


def shift(out):
    ps.pitch_shift_ragged(src, offs, lens, steps, gains, out, rows, None, None, sr=SR)


def mel_only(out):
    tf.log_mel_ragged(out, lengths, crops)


def both(out):
    shift(out)
    tf.log_mel_ragged(out, lengths, crops)


def timed(fn):
    out = waves.clone()
    for _ in range(5):
        fn(out)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(out)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


plan = ps.Plan(lens, steps, offs, None, None, rows, N, sr=SR)
res = {"B": B, "synthetic_rows": K, "seconds_per_row": N / SR}
res["pitch_shift_ms_median"], res["pitch_shift_ms_min"] = timed(shift)
res["loader_step_plain_ms_median"], _ = timed(mel_only)
res["loader_step_synthetic_ms_median"], _ = timed(both)
res["work"] = {"stft_frames": plan.n_frames, "columns": plan.n_cols, "stretched_samples": plan.n_stretched,
               "output_samples": plan.n_out}
res["budget_ms"] = 1.0
print(json.dumps(res))
