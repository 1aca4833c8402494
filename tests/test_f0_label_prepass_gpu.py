"""From a folder of wav files to labelled batches: ``build_dataloader`` labels every file that has no F0 cache with
the on-device tracker, writes the reference's cache files, and the loader then reads them like any other cache."""
import json
import math
import os
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from pitchextractor_amd.f0_tracker import PraatACTracker
from pitchextractor_amd.meldataset import align_length, build_dataloader, segment_plan
from pitchextractor_amd.resample import RaggedResampler
from tests import f0_track_ref as R
from tests.test_data_layer import write_wav

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SR, HOP = 24000, 300
F0_PARAMS = {"bad_f0_threshold": 5, "zero_fill_value": 0.0, "backend_order": ["swiftf0", "praat"],
             "backends": {"swiftf0": {"type": "swiftf0", "enabled": True},
                          "praat": {"type": "praat", "enabled": True,
                                    "config": {"method": "ac", "min_pitch": 40.0, "max_pitch": 1100.0}}}}
SUFFIX = "_f0-swiftf0_praat"
DATASET = {"mel_params": {"sample_rate": SR, "win_len": 1024, "n_fft": 1024, "n_mels": 80, "hop_length": HOP},
           "f0_params": F0_PARAMS}


def _folder(tmp_path):
    """A 3-s file (pre-cropped and cropped by the loader) and 2-s files at 24 / 16 / 48 kHz; one too short to track."""
    specs = [(3.0, 90.0, 300.0, 24000), (2.0, 80.0, 380.0, 24000), (2.0, 300.0, 120.0, 16000),
             (2.0, 200.0, 600.0, 48000), (1.6, 150.0, 250.0, 24000)]
    files = []
    for k, (seconds, a, b, sr) in enumerate(specs):
        y = R.glide_signal(seconds, a, b, sr, seed=20 + k)[0]
        p = str(tmp_path / f"utt{k}.wav")
        write_wav(p, y, sr, "float32")
        files.append((p, y, sr))
    p = str(tmp_path / "short.wav")
    write_wav(p, 0.1 * np.ones(1000, np.float32), SR, "float32")
    return files, p


def _expected_contour(y, sr):
    """float64 and float32 restatement on the file resampled to the dataset rate by the loader's own resampler."""
    if sr != SR:
        out, n = RaggedResampler(SR)(torch.from_numpy(y).cuda(), [sr], [len(y)])
        y = out[0, :int(n[0])].cpu().numpy()
    return (R.track(y, SR, HOP, min_pitch=40.0, max_pitch=1100.0),
            R.track(y, SR, HOP, dtype=np.float32, min_pitch=40.0, max_pitch=1100.0), len(y))


@pytest.fixture
def track_calls(monkeypatch):
    """Counts the calls of PraatACTracker.track."""
    calls = []
    real = PraatACTracker.track

    def counting(self, waves, lengths=None, **kw):
        calls.append(len(lengths) if lengths is not None else 1)
        return real(self, waves, lengths, **kw)

    monkeypatch.setattr(PraatACTracker, "track", counting)
    return calls


def test_wav_folder_to_labelled_batches(tmp_path, hip_device, track_calls):
    files, short = _folder(tmp_path)
    lines = [f"{p}|0\n" for p, _, _ in files] + [f"{short}|0\n"]
    loader = build_dataloader(lines, validation=True, batch_size=len(files), num_workers=0, device=hip_device,
                              dataset_config=dict(DATASET))
    assert len(track_calls) >= 1
    # yardstick: the float32 restatement against the float64 one on these very files (contour cents); the kernel gets 4x
    expected = [_expected_contour(y, sr) for _, y, sr in files]
    yard = max(R.deviation(a, b)["contour_cents"] for a, b, _ in expected)
    tol_cents = 4 * yard
    refs = []
    for (p, y, sr), (ref, ref32, n) in zip(files, expected):
        assert np.array_equal(ref["f0"] > 0, ref32["f0"] > 0)
        got = np.load(p + SUFFIX + ".npy")
        with open(p + SUFFIX + ".json") as fh:
            meta = json.load(fh)
        assert meta == {"cache_identifier": "-swiftf0_praat", "backend": "praat", "sample_rate": SR, "hop_length": HOP}
        assert got.dtype == np.float32 and got.shape == ref["f0"].shape
        assert np.array_equal(got > 0, ref["f0"] > 0), p
        v = got > 0
        worst = R.cents(got[v], ref["f0"][v]).max()
        print(f"[f0 prepass] {os.path.basename(p)}: contour {worst:.3e} cents (yardstick {yard:.3e}, tolerance 4x)")
        assert v.sum() > 50 and worst <= tol_cents
        refs.append((got, ref["f0"], n))
    assert np.load(short + SUFFIX + ".npy").shape == (0,)               # shorter than one window: every backend failed
    with open(short + SUFFIX + ".json") as fh:
        assert json.load(fh)["backend"] == ""
    assert not [f for f in os.listdir(tmp_path) if ".tmp" in f]

    # one batch under the loader's own pre-crop and crop (draws reproduced with the same seeds, in item order)
    random.seed(11)
    np.random.seed(11)
    batches = list(loader)
    mels, f0s, sils = batches[0]
    assert mels.shape == (len(files), 1, 80, 192) and torch.isfinite(mels).all()
    random.seed(11)
    np.random.seed(11)
    for row, (p, y, sr) in enumerate(files):
        cache, ref64, n_target = refs[row]
        exp = []
        start, seg, full = segment_plan(len(y), sr, SR, HOP, 1024, 192)
        assert (row == 0) == (not full)
        for contour in (cache, ref64.astype(np.float32)):
            if full:
                part, n_t = contour, n_target
            else:
                n_t = seg
                lo = int(math.floor(int(round(start / float(sr) * SR)) / float(HOP)))
                part = contour[lo:min(len(contour), lo + int(np.ceil(n_t / HOP)) + 2 + 4)]
            exp.append(align_length(part, 1 + n_t // HOP))
        mel_len = exp[0].shape[0]
        crop = int(np.random.randint(0, mel_len - 192)) if mel_len > 192 else 0
        exp = [e[crop:crop + 192] for e in exp]
        L = exp[0].shape[0]
        got_f0, got_sil = f0s[row].cpu().numpy(), sils[row].cpu().numpy()
        assert np.array_equal(got_f0[:L], exp[0]) and not got_f0[L:].any()          # exactly what the cache holds
        assert np.array_equal(got_sil[:L], (exp[0] == 0).astype(np.float32)) and not got_sil[L:].any()
        assert np.array_equal(exp[0] > 0, exp[1] > 0)                                # and the restatement's contour
        v = exp[0] > 0
        assert R.cents(exp[0][v], exp[1][v]).max() <= tol_cents

    # the file no backend could label arrives as an all-silent item: empty contour -> zeros, is_silence 1 on its frames
    assert len(batches) == 2
    mels, f0s, sils = batches[1]
    L = 1 + 1000 // HOP
    assert mels.shape == (1, 1, 80, 192) and torch.isfinite(mels).all() and not f0s.any()
    assert sils[0, :L].cpu().tolist() == [1.0] * L and not sils[0, L:].any()

    # a second loader on the same folder finds every cache and never calls the tracker
    before = len(track_calls)
    mtimes = {f: os.stat(tmp_path / f).st_mtime_ns for f in os.listdir(tmp_path)}
    build_dataloader(lines, validation=False, batch_size=2, num_workers=0, device=hip_device,
                     dataset_config=dict(DATASET))
    assert len(track_calls) == before
    assert mtimes == {f: os.stat(tmp_path / f).st_mtime_ns for f in os.listdir(tmp_path)}


def test_train_py_from_wavs_alone(tmp_path, hip_device):
    lines = []
    for i in range(6):
        y = R.glide_signal(2.0, 90.0 + 20 * i, 200.0 + 30 * i, 24000 if i % 2 == 0 else 16000, seed=40 + i)[0]
        p = tmp_path / f"u{i}.wav"
        write_wav(p, y, 24000 if i % 2 == 0 else 16000, "float32")
        lines.append(f"{p}|0\n")
    (tmp_path / "train_list.txt").write_text("".join(lines[:4]))
    (tmp_path / "val_list.txt").write_text("".join(lines[4:]))
    cfg = yaml.safe_load((ROOT / "Configs" / "config.yml").read_text())
    cfg.update(log_dir=str(tmp_path / "ckpt"), save_freq=1, epochs=1, batch_size=2, num_workers=0,
               train_data=str(tmp_path / "train_list.txt"), val_data=str(tmp_path / "val_list.txt"))
    cfg["model_params"]["sequence_model"].update(hidden_size=64, num_layers=1)
    cfg["dataset_params"]["f0_params"] = F0_PARAMS
    cfg_path = tmp_path / "config.yml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    res = subprocess.run([sys.executable, str(ROOT / "train.py"), "-p", str(cfg_path)], cwd=str(ROOT),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert all(os.path.isfile(f"{tmp_path}/u{i}.wav{SUFFIX}.npy") for i in range(6))
    assert all(np.count_nonzero(np.load(f"{tmp_path}/u{i}.wav{SUFFIX}.npy")) > 50 for i in range(6))
    log = (tmp_path / "ckpt" / "train.log").read_text()
    assert "train/loss" in log and "eval/loss" in log                   # 4 files / batch 2: two training steps
    ck = torch.load(tmp_path / "ckpt" / "epoch_00001.pth", map_location="cpu", weights_only=True)
    assert all(torch.isfinite(v).all() for v in ck["model"].values() if v.dtype.is_floating_point)
    losses = [float(line.split(":")[-1]) for line in log.splitlines() if "train/loss" in line or "eval/loss" in line]
    assert len(losses) >= 2 and all(math.isfinite(v) and v > 0 for v in losses)
