"""Wall time of one pass over the loader with all three synthetic kinds on: 8 batches of 16 from ``build_dataloader``,
``num_workers=0``, host work (reads, draws, labels, pulse tables, collation) and device stages included.

Four short files (1.0 s and 2.6 s at 24 kHz, 3.2 s at 44.1 kHz, 1.4 s at 16 kHz) and 124 synthetic items from fixed
seeds: pitch shift with noise, vocoder utterances of 0.6-3.0 s, resynthesis with semitone 0, noise, aperiodicity and
vibrato.  One warm-up pass (code load, resampler filters), then the timed pass over the same draws.  Prints one JSON
line; the checksum (sum of every mel) tells two trees apart that do not compute the same batches.  Needs a GPU.
Not a gate: profiles/ab_synthetic_kinds.txt holds a parent-against-new run of it."""
import json
import random
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from pitchextractor_amd import meldataset as md  # noqa: E402
from pitchextractor_amd import synthetic  # noqa: E402
from tests.test_data_layer import write_wav  # noqa: E402

SR, HOP, BATCH, BATCHES = 24000, 300, 16, 8


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_synthetic_loader: no GPU visible; this benchmark does not run without one")
    tmp = Path(tempfile.mkdtemp())
    lines = []
    for i, (dur, sr) in enumerate([(1.0, SR), (2.6, SR), (3.2, 44100), (1.4, 16000)]):
        wave, f0, _ = synthetic.utterance(i, duration=dur, sr=sr, hop=sr // 80)
        path = tmp / f"u{i}.wav"
        write_wav(path, wave, sr, "float32")
        n = int(np.ceil(len(wave) * SR / sr))
        np.save(str(path) + "_f0.npy", md.align_length(f0, 1 + n // HOP))
        lines.append(f"{path}|0\n")
    syn = {"enabled": True, "absolute_count": BATCH * BATCHES - len(lines), "apply_to_validation": True,
           "pitch_shift": {"enabled": True, "semitones": [-4, -2, -1, 1, 2, 4], "gain_db_range": [-6.0, 3.0],
                           "noise_db": -50.0},
           "world_vocoder": {"enabled": True, "backend": "hip", "duration": {"min": 0.6, "max": 3.0}},
           "world_resynthesis": {"enabled": True, "backend": "hip", "semitones": [-3, 0, 2, 5], "noise_db": -55.0,
                                 "aperiodicity": 0.1, "modulation": {"vibrato_probability": 0.5}}}
    cfg = {"mel_params": {"sample_rate": SR, "win_len": 1024, "n_fft": 1024, "n_mels": 80, "hop_length": HOP},
           "dataloader": {"start_method": None}, "verbose": False, "synthetic_data": syn}
    loader = md.build_dataloader(lines, validation=True, batch_size=BATCH, num_workers=0, device="cuda:0",
                                 dataset_config=cfg)
    assert len(loader) == BATCHES
    ms = []
    for _ in range(2):
        random.seed(3)
        np.random.seed(3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        checksum = 0.0
        for mels, _, _ in loader:
            checksum += float(mels.sum())                        # waits for the batch
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"batches": BATCHES, "batch": BATCH, "warmup_pass_ms": ms[0], "pass_ms": ms[1],
                      "checksum": checksum}))


if __name__ == "__main__":
    main()
