"""Pitch shifting on the GPU: each HIP stage against the float64 restatement (fed the GPU's own input to that stage),
end to end against float64 with the float32 librosa-like restatement as the yardstick, ragged batching, and the
data loader with synthetic items on."""
import random

import numpy as np
import pytest
import torch

from oracle import mel_ref, train_ref
from pitchextractor_amd import meldataset as md
from pitchextractor_amd import pitch_shift as ps
from pitchextractor_amd import synthetic
from tests import pitch_shift_ref as ref
from tests.test_data_layer import write_wav

pytestmark = pytest.mark.gpu
SR = 24000
STEPS = [-4, -2, -1, 1, 2, 4]


def _run(waves, steps, dev, res_type="kaiser_best", spec=None, gains=None):
    lens = [w.size for w in waves]
    plan = ps.Plan(lens, steps, sr=SR, res_type=res_type)
    flat = torch.from_numpy(np.concatenate(waves).astype(np.float32)).to(dev)
    out = torch.zeros((len(waves), max(lens)), dtype=torch.float32, device=dev)
    g = torch.ones(len(waves), dtype=torch.float32, device=dev) if gains is None else gains
    keep = ps.PitchShifter().run(plan, flat, g, out, keep=True, spec=spec)
    torch.cuda.synchronize()
    return plan, keep, out.cpu().numpy()


def _rows(plan, buf, start_field, count):
    """Split a flat workspace into per-row numpy arrays by the plan's prefix offsets."""
    buf = buf.cpu().numpy()
    return [buf[plan.meta[r, start_field]:plan.meta[r, start_field] + count(plan.meta[r])] for r in range(plan.n_rows)]


def test_stft_stage(hip_device):
    rng = np.random.default_rng(0)
    waves = [rng.standard_normal(n).astype(np.float32) for n in (1, 700, 24000, 50001)]
    plan, keep, _ = _run(waves, [1, -1, 2, -4], hip_device)
    specs = _rows(plan, keep["spec"], 3, lambda m: m[2])
    assert [g.shape[0] for g in specs][0] == 0                  # 1 sample: int(M r) = 0, nothing to compute
    for w, got in zip(waves[1:], specs[1:]):
        want = ref.stft(w)[:got.shape[0]]
        assert got.shape[0] >= 1
        assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


def test_phase_vocoder_stage(hip_device):
    """Well-conditioned random spectra (|D| in [0.5, 2]), >= 300 output columns, vs float64 on the same input."""
    rng = np.random.default_rng(1)
    n = 512 * 400
    for s in (-4, 4, 1):
        plan = ps.Plan([n], [s], sr=SR)
        F = plan.n_frames
        D = rng.uniform(0.5, 2.0, (F, 1025)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (F, 1025)))
        D = D.astype(np.complex64)
        spec = torch.view_as_real(torch.from_numpy(D)).contiguous().to(hip_device)
        _, keep, _ = _run([np.zeros(n, np.float32)], [s], hip_device, spec=spec)
        got = keep["cols"].cpu().numpy()
        c_hi = int(plan.meta[0, 5])
        assert got.shape[0] == c_hi >= 300
        full = np.concatenate([D.astype(np.complex128), np.zeros((1 + n // 512 - F, 1025))])
        want = ref.phase_vocoder(full, ps.stretch_rate(s))[:c_hi]
        assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max(), s


def test_istft_stage(hip_device):
    rng = np.random.default_rng(2)
    waves = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in (3000, 48000)]
    plan, keep, _ = _run(waves, [-2, 2], hip_device)
    cols = _rows(plan, keep["cols"], 6, lambda m: m[5] - m[4])
    st = _rows(plan, keep["stretched"], 11, lambda m: m[10] - m[9])
    for r, (c, got) in enumerate(zip(cols, st)):
        M = int(plan.meta[r, 7])
        assert plan.meta[r, 9] == 0 and got.size == plan.meta[r, 10]
        want = ref.istft(c.astype(np.complex128), M)[:got.size]
        assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("res_type", ["kaiser_best", "kaiser_fast"])
def test_resample_stage_all_semitones(hip_device, res_type):
    rng = np.random.default_rng(3)
    waves = [(0.3 * rng.standard_normal(20000 + 997 * i)).astype(np.float32) for i in range(len(STEPS))]
    plan, keep, out = _run(waves, STEPS, hip_device, res_type=res_type)
    st = _rows(plan, keep["stretched"], 11, lambda m: m[10] - m[9])
    for r, s in enumerate(STEPS):
        N = waves[r].size
        want = np.zeros(N)
        y = ref.resample(st[r].astype(np.float64), ps.resample_ratio(s, SR), res_type)
        want[:min(N, y.size)] = y[:N]
        assert np.abs(out[r, :N] - want).max() <= 1e-5 * np.abs(want).max(), s


def _signals():
    rng = np.random.default_rng(4)
    t = lambda n: np.arange(n) / SR  # noqa: E731
    sig = [synthetic.utterance(0, duration=1.5)[0], synthetic.utterance(3, duration=6.0)[0],
           (0.2 * rng.standard_normal(1024)).astype(np.float32), (0.2 * rng.standard_normal(30011)).astype(np.float32)]
    n = 77777
    multi = sum(a * np.sin(2 * np.pi * f * t(n) + p) for a, f, p in ((0.3, 180.0, 0.1), (0.2, 523.0, 1.0),
                                                                    (0.1, 1710.0, 2.0)))
    sig.append(multi.astype(np.float32))
    return sig


def _within_twice_float32(sig, steps, dev):
    """Every row is measured before the first miss is raised, so a failure names all of them."""
    _, _, out = _run(sig, steps, dev)
    misses = []
    for r, (w, s) in enumerate(zip(sig, steps)):
        N = w.size
        got = out[r, :N]
        f64 = ref.pitch_shift(w, SR, s)
        f32 = ref.pitch_shift(w, SR, s, fp32=True)
        e_gpu, e_32 = np.abs(got - f64).max(), np.abs(f32 - f64).max()
        print(f"row {r} n={N} s={s}: gpu {e_gpu:.3e}, float32 {e_32:.3e}")
        if not e_gpu <= 2 * e_32 + 1e-5:
            misses.append((r, "wave", e_gpu, e_32))
        if N > 1024:
            m64, m32, mg = (mel_ref.log_mel(np.asarray(x, np.float64)) for x in (f64, f32, got))
            e_gpu, e_32 = np.abs(mg - m64).max(), np.abs(m32 - m64).max()
            print(f"row {r} log-mel: gpu {e_gpu:.3e}, float32 {e_32:.3e}")
            if not e_gpu <= 2 * e_32 + 1e-3:
                misses.append((r, "log-mel", e_gpu, e_32))
    assert not misses, misses


def test_end_to_end_within_twice_float32_librosa(hip_device):
    _within_twice_float32(_signals(), [4, -2, 1, -4, 2], hip_device)


@pytest.mark.parametrize("s", [12, -12, 7.3])
def test_end_to_end_within_twice_float32_librosa_wide_steps(hip_device, s):
    """An octave either way and a step float32 does not represent, on speech-like and stationary signals (white noise
    bounds nothing here: its float32 yardstick is itself 1e-3).

    With a float32 forward transform the utterance missed this bound at an octave (2.30 times the yardstick at
    s = 12, 2.05 times at -12); the STFT stage runs in fp64 since, and the GPU's error against float64 is 8e-7 on
    every row here where the float32 restatement's is 2e-3 .. 4e-2."""
    _within_twice_float32([synthetic.utterance(0, duration=1.5)[0], ref.three_sines(77777)], [s, s], hip_device)


def test_row_alone_equals_row_in_ragged_batch(hip_device):
    sig = _signals()
    steps = [4, -2, 1, -4, 2]
    _, _, batch = _run(sig, steps, hip_device)
    for r in (0, 3, 4):
        _, _, alone = _run([sig[r]], [steps[r]], hip_device)
        np.testing.assert_array_equal(alone[0, :sig[r].size], batch[r, :sig[r].size])
        got = ps.pitch_shift(torch.from_numpy(sig[r]).to(hip_device), sr=SR, n_steps=steps[r]).cpu().numpy()
        np.testing.assert_array_equal(got, batch[r, :sig[r].size])


def test_window_write_matches_full_shift(hip_device):
    """The loader's form: output windows of long rows, gains and noise, written into given batch rows."""
    w = synthetic.utterance(5, duration=8.0)[0]
    full = ps.pitch_shift(torch.from_numpy(w).to(hip_device), sr=SR, n_steps=-4)
    out = torch.zeros((3, 60000), dtype=torch.float32, device=hip_device)
    noise = torch.randn(2 * 58412, device=hip_device) * 1e-3
    flat = torch.from_numpy(np.concatenate([w, w])).to(hip_device)
    ps.pitch_shift_ragged(flat, [0, w.size], [w.size, w.size], [-4, -4], torch.tensor([0.5, 2.0]), out,
                          out_rows=[2, 0], out_start=[100000, 0], out_len=[58412, 58412], sr=SR, noise=noise)
    torch.cuda.synchronize()
    f = full.cpu().numpy()
    n = noise.cpu().numpy()
    o = out.cpu().numpy()
    # bit for bit: the window only skips reads outside ranges the plan proves sufficient (test_pitch_shift_edges_cpu.py),
    # and with power-of-two gains the epilogue rounds once whether or not gain and noise are fused
    np.testing.assert_array_equal(o[2, :58412], np.float32(0.5) * f[100000:158412] + n[:58412])
    np.testing.assert_array_equal(o[0, :58412], np.float32(2.0) * f[:58412] + n[58412:])
    assert (o[1] == 0).all() and (o[0, 58412:] == 0).all()


def test_dataloader_with_synthetic_items(tmp_path, hip_device):
    """Synthetic rows of a build_dataloader batch: the reference's draws, the device shift written through the crop
    window, gains, lengths and frame offsets, against the float64 mel oracle at the loader's own tolerance."""
    lines = []
    for i, dur in enumerate((2.0, 3.0, 0.9, 2.6, 2.0, 4.0, 1.4, 2.2)):
        n, f = int(dur * SR), 110.0 + 37.0 * i
        t = np.arange(n) / SR
        wave = sum(0.3 / h * np.sin(2 * np.pi * h * f * t + h) for h in (1, 2, 3)).astype(np.float32)
        f0 = np.full(1 + n // 300, f, np.float32)
        p = tmp_path / f"u{i}.wav"
        write_wav(p, wave, SR, "float32")
        np.save(str(p) + "_f0.npy", f0)
        lines.append(f"{p}|0\n")
    syn = {"enabled": True, "ratio": 0.5, "apply_to_validation": True,
           "pitch_shift": {"enabled": True, "semitones": STEPS, "gain_db_range": [-6.0, 3.0],
                           "min_voiced_fraction": 0.05, "resample_type": "kaiser_best"}}
    cfg = {"mel_params": {"sample_rate": SR, "win_len": 1024, "n_fft": 1024, "n_mels": 80, "hop_length": 300},
           "dataloader": {"start_method": None}, "verbose": False, "synthetic_data": syn}
    loader = md.build_dataloader(lines, validation=True, batch_size=6, num_workers=0, device="cuda:0",
                                 dataset_config=cfg)
    assert len(loader.dataset) == 12 and len(loader) == 2
    np.random.seed(5); random.seed(5)
    got = [(m.cpu().numpy(), f.cpu().numpy(), s.cpu().numpy()) for m, f, s in loader]
    np.random.seed(5); random.seed(5)
    ds = loader.dataset
    n_syn = 0
    for bi in range(2):
        items = []
        for i in range(6 * bi, 6 * bi + 6):
            if i < 8:
                wave, f0, sil, crop = ds.path_to_wave_and_label(ds.data_list[i])
            else:
                # the batch row must be the GPU's own single-row shift (bit for bit the ragged batch's), cropped by
                # the item's draws; its distance to float64 is bounded like the end-to-end test's
                wave, f0, sil, _, _, req = ds[i]
                w64 = ref.pitch_shift(wave.numpy(), SR, req.n_steps)
                w32 = ref.pitch_shift(wave.numpy(), SR, req.n_steps, fp32=True)
                gpu = ps.pitch_shift(wave.to(hip_device), sr=SR, n_steps=req.n_steps).cpu().numpy()
                assert np.abs(gpu - w64).max() <= 2 * np.abs(w32 - w64).max() + 1e-5, i
                wave = gpu * np.float32(req.gain)
                crop = req.crop
                n_syn += 1
            mel = mel_ref.log_mel(wave)[:, crop:crop + 192].astype(np.float32)
            items.append((mel, f0.numpy() if torch.is_tensor(f0) else f0, sil.numpy() if torch.is_tensor(sil) else sil))
        rm, rf, rs = train_ref.collate(items)
        m, f, s = got[bi]
        assert np.abs(m - rm).max() <= 1e-3, bi
        np.testing.assert_array_equal(f, rf)
        np.testing.assert_array_equal(s, rs)
    assert n_syn == 4
