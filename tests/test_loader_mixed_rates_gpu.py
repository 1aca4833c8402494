"""A file list that mixes five sample rates through build_dataloader: every batch row equals its item resampled and
transformed alone, bit for bit; pitch-shifted rows whose base files come at different rates equal the rows made one
at a time; and Trainer.run trains on the mixed loader."""
import logging
import random

import numpy as np
import pytest
import torch

from oracle import mel_ref, resample_ref as rr
from pitchextractor_amd import meldataset as md
from pitchextractor_amd import ops
from pitchextractor_amd.mel import MelSpectrogram
from pitchextractor_amd.resample import Resampler
from tests.test_data_layer import write_wav

pytestmark = pytest.mark.gpu

RATES = (16000, 22050, 24000, 44100, 48000)
MEL = {"sample_rate": 24000, "win_len": 1024, "n_fft": 1024, "n_mels": 80, "hop_length": 300}


def _file_list(tmp_path, n_files=12, long=False):
    """Whole files (< 2.4 s: no pre-crop, no random crop) so that every item is the same whichever worker and batch
    draw it; each file's constant F0 names it."""
    lines = []
    for i in range(n_files):
        sr = RATES[i % len(RATES)]
        dur = (3.0 + 0.4 * i) if long else (0.6 + 0.15 * i)
        n, f = int(dur * sr), 100.0 + 10.0 * i
        t = np.arange(n) / sr
        wave = sum(0.3 / h * np.sin(2 * np.pi * h * f * t + h) for h in (1, 2, 3)).astype(np.float32)
        p = tmp_path / f"r{i}.wav"
        write_wav(p, wave, sr, "float32")
        np.save(str(p) + "_f0.npy", np.full(1 + int(dur * 24000) // 300, f, np.float32))
        lines.append(f"{p}|0\n")
    return lines


@pytest.mark.parametrize("num_workers", [0, 2])
def test_mixed_rate_batches_equal_items_alone(tmp_path, hip_device, num_workers):
    lines = _file_list(tmp_path)
    cfg = {"mel_params": MEL, "dataloader": {"start_method": None}, "verbose": False}
    loader = md.build_dataloader(lines, validation=False, batch_size=4, num_workers=num_workers, device="cuda:0",
                                 dataset_config=cfg)
    torch.manual_seed(11); np.random.seed(11); random.seed(11)
    ds = loader.dataset
    tf = MelSpectrogram(**ds.mel_params)
    alone = {}
    for path in ds.data_list:
        wave, f0, sil, crop = ds.path_to_wave_and_label(path)
        assert crop == 0
        w = torch.from_numpy(wave).to(hip_device)
        if ds._last_sr != ds.sr:
            w = Resampler(ds._last_sr, ds.sr)(w)
        mel = tf.log_mel_ragged(w[None].contiguous(), torch.tensor([w.numel()], dtype=torch.int32, device=hip_device),
                                torch.zeros(1, dtype=torch.int32, device=hip_device))
        ref = mel_ref.log_mel(rr.resample(wave, ds._last_sr, ds.sr).astype(np.float32))
        L = ref.shape[1]
        assert np.abs(mel[0, 0, :, :L].cpu().numpy() - ref).max() <= 2e-3, path
        alone[float(f0[0])] = (mel[0], f0, sil)
    seen, mixed = set(), 0
    for mels, f0s, sils in loader:
        assert mels.shape == (4, 1, 80, 192)
        mixed += 1
        for r in range(4):
            key = float(f0s[r, 0])
            mel, f0, sil = alone[key]
            assert torch.equal(mels[r], mel), key
            L = f0.shape[0]
            assert np.array_equal(f0s[r, :L].cpu().numpy(), f0) and (f0s[r, L:] == 0).all()
            assert np.array_equal(sils[r, :L].cpu().numpy(), sil)
            seen.add(key)
    assert mixed == 3 and len(seen) == 12


def test_pitch_shift_rows_from_mixed_rate_base_files(tmp_path, hip_device):
    lines = _file_list(tmp_path, n_files=8, long=True)
    syn = {"enabled": True, "ratio": 0.5, "apply_to_validation": True,
           "pitch_shift": {"enabled": True, "semitones": [-4, -2, 2, 4], "gain_db_range": [-6.0, 3.0],
                           "noise_db": -50.0, "min_voiced_fraction": 0.05, "resample_type": "kaiser_best"}}
    cfg = {"mel_params": MEL, "dataloader": {"start_method": None}, "verbose": False, "synthetic_data": syn}

    def run(batch_size):
        loader = md.build_dataloader(lines, validation=True, batch_size=batch_size, num_workers=0, device="cuda:0",
                                     dataset_config=cfg)
        torch.manual_seed(5); np.random.seed(5); random.seed(5)
        return [tuple(t.clone() for t in b) for b in loader], loader.dataset

    batched, ds = run(6)
    assert len(ds) == 12 and len(batched) == 2
    single, _ = run(1)                              # the same draws, one row per batch
    torch.manual_seed(5); np.random.seed(5); random.seed(5)
    syn_rates = {int(item[4]) for item in [ds[i] for i in range(12)][8:]}      # the loaders' own draws, replayed
    assert len(syn_rates) > 1, "the synthetic rows should draw base files at different rates"
    for bi, (mels, f0s, sils) in enumerate(batched):
        for r in range(6):
            m1, f1, s1 = single[6 * bi + r]
            assert torch.equal(mels[r], m1[0]), (bi, r)
            assert torch.equal(f0s[r], f1[0]) and torch.equal(sils[r], s1[0])


def test_trainer_runs_on_the_mixed_loader(tmp_path, hip_device):
    from pitchextractor_amd.model import JDCNet
    from pitchextractor_amd.optimizers import build_optimizer
    from pitchextractor_amd.trainer import Trainer
    from tests.golden.make_golden import SEQ_CFG
    lines = _file_list(tmp_path)
    cfg = {"mel_params": MEL, "dataloader": {"start_method": None}, "verbose": False}
    loader = md.build_dataloader(lines, validation=False, batch_size=4, num_workers=0, device="cuda:0",
                                 dataset_config=cfg)
    torch.manual_seed(1)
    net = JDCNet(num_class=1, sequence_model_config=dict(SEQ_CFG)).to(hip_device).train()
    opt, sched = build_optimizer({"params": net.parameters(), "optimizer_params": {},
                                  "scheduler_params": {"max_lr": 3e-4, "pct_start": 0.0, "epochs": 10,
                                                       "steps_per_epoch": 3}})
    tr = Trainer(model=net, criterion={"l1": torch.nn.SmoothL1Loss(), "ce": torch.nn.BCEWithLogitsLoss()},
                 optimizer=opt, scheduler=sched, device="cuda:0", loss_config={"lambda_f0": 0.1},
                 logger=logging.getLogger("t"))
    steps = 0
    for batch in loader:
        out = tr.run(batch)
        assert all(np.isfinite(float(out[k])) for k in ("loss", "f0", "sil")), out
        steps += 1
    assert steps == 3
    assert not ops.persistent_lstm_error(hip_device)
