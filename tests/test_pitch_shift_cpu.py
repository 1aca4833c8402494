"""Pitch-shift augmentation without a GPU: the float64 restatement pinned by construction, the host-side layout, the
dataset's synthetic items (draw order of the reference's generator, meldataset.py:324-517) and the Collater."""
import random

import numpy as np
import pytest

from pitchextractor_amd import _lib, build
from pitchextractor_amd import meldataset as md
from pitchextractor_amd import pitch_shift as ps
from pitchextractor_amd import synthetic
from tests import pitch_shift_ref as ref
from tests.test_data_layer import write_wav

SR = 24000


# --------------------------------------------------------------------------- restatement, pinned by construction
def test_istft_inverts_stft():
    y = np.random.default_rng(0).standard_normal(30001)
    D = ref.stft(y)
    assert D.shape == (1 + 30001 // 512, 1025)
    assert np.abs(ref.istft(D, y.size) - y).max() < 1e-12


def test_phase_vocoder_at_rate_one_is_identity():
    D = ref.stft(np.random.default_rng(1).standard_normal(20000))
    assert np.abs(ref.phase_vocoder(D, 1.0) - D).max() < 1e-9 * np.abs(D).max()


def test_kaiser_best_table():
    W = ps.resample_filter("kaiser_best")
    assert W.size == 32769
    assert abs(W[0] + 2 * W[512::512].sum() - 1.0) < 1e-8            # integer-spaced taps: unit DC gain
    assert ps.resample_filter("kaiser_fast").size == 8193


@pytest.mark.parametrize("s,bound", [(-4, 1e-6), (-1, 1e-6), (2, 1e-3), (4, 1e-3)])
def test_resampler_reproduces_a_sine(s, bound):
    r = ps.resample_ratio(s, SR)
    n = 24000
    x = np.sin(2 * np.pi * 440.0 * np.arange(n) / SR)
    y = ref.resample(x, r)
    assert y.size == int(n * r)
    t = np.arange(y.size)
    want = np.sin(2 * np.pi * 440.0 * t / (SR * r))
    edge = 2000
    assert np.abs(y - want)[edge:-edge].max() < bound


def _peak_hz(y, sr):
    w = np.hanning(y.size)
    spec = np.abs(np.fft.rfft(y * w, n=8 * y.size))
    k = int(np.argmax(spec))
    a, b, c = np.log(spec[k - 1:k + 2])
    return (k + 0.5 * (a - c) / (a - 2 * b + c)) * sr / (8 * y.size)


@pytest.mark.parametrize("s,want", [(4, 277.18), (-2, 196.00)])
def test_shifted_sine_peaks_at_the_new_pitch(s, want):
    y = np.sin(2 * np.pi * 220.0 * np.arange(2 * SR) / SR)
    out = ref.pitch_shift(y, SR, s)
    assert out.shape == y.shape
    got = _peak_hz(out[6000:-6000], SR)
    assert abs(1200 * np.log2(got / (220.0 * 2 ** (s / 12)))) < 1.0


def test_host_lengths():
    for n in (1, 511, 512, 48000, 144001):
        for s in (-4, -2, -1, 1, 2, 4):
            rate = 2.0 ** (-s / 12)
            assert ps.stft_frames(n) == 1 + n // 512
            assert ps.stretched_columns(n, s) == len(np.arange(0, 1 + n // 512, rate))
            assert ps.stretched_len(n, s) == int(round(n / rate))
            assert ps.resampled_len(n, s, SR) == int(ps.stretched_len(n, s) * (SR / (SR / rate)))


# --------------------------------------------------------------------------- C ABI, host side only
@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _lib.load()


def test_plan_matches_host_lengths(lib):
    lens = [1, 700, 48000, 144000]
    steps = [-4, 1, 4, -2]
    plan = ps.Plan(lens, steps, sr=SR)
    K = lib.pe_pitch_shift_plan_fields()
    assert plan.meta.shape == (4, K)
    for r, (n, s) in enumerate(zip(lens, steps)):
        m = plan.meta[r]
        assert m[0] == n and m[7] == ps.stretched_len(n, s) and m[12] == ps.resampled_len(n, s, SR)
        assert m[17] == ps.stretched_columns(n, s)
        assert plan.ratios[r, 0] == ps.stretch_rate(s) and plan.ratios[r, 1] == ps.resample_ratio(s, SR)
    assert plan.n_out == sum(lens)
    # a window at the start of a long row computes only a prefix of its frames
    short = ps.Plan([144000], [2], out_start=[0], out_len=[24000], sr=SR)
    assert short.n_frames < ps.stft_frames(144000) // 2 and short.n_out == 24000


def test_plan_argument_checks(lib):
    import ctypes
    L = lambda *v: (ctypes.c_long * len(v))(*v)  # noqa: E731
    F = lambda *v: (ctypes.c_float * len(v))(*v)  # noqa: E731
    meta = (ctypes.c_long * 64)()
    rat = (ctypes.c_double * 8)()
    tot = (ctypes.c_long * 4)()

    def plan(n=1000, s=2.0, j_lo=0, j_cnt=1000, stride=1000, n_fft=2048, hop=512, rt=0):
        return lib.pe_pitch_shift_plan(1, L(n), F(s), L(0), L(j_lo), L(j_cnt), L(0), stride, SR, n_fft, hop, rt,
                                       meta, rat, tot)
    assert plan() == 0
    assert plan(n_fft=1024) == -2 and plan(hop=256) == -2
    assert plan(n=0, j_cnt=0) == -1                           # bad length
    assert plan(j_lo=10) == -1                                # window past the row's end
    assert plan(s=float("nan")) == -1 and plan(s=30.0) == -1  # bad semitone
    assert plan(stride=999) == -1                             # output stride shorter than the window
    assert plan(rt=2) == -1
    p = ctypes.c_void_p(1)
    assert lib.pe_pitch_shift_stft(p, p, -1, 1, p, None) == -1
    assert lib.pe_pitch_shift_resample(p, p, p, p, 3, p, None, 1, 1, p, None) == -1
    assert lib.pe_pitch_shift_istft(None, p, 1, 0, 5, None, None, None) == -1


# --------------------------------------------------------------------------- dataset
CFG = {"enabled": True, "ratio": 0.25, "apply_to_validation": False,
       "pitch_shift": {"enabled": True, "semitones": [-4, -2, -1, 1, 2, 4], "gain_db_range": [-6.0, 3.0],
                       "min_voiced_fraction": 0.05, "resample_type": "kaiser_best"},
       "world_vocoder": {"enabled": True}}
MEL = {"sample_rate": SR, "win_len": 1024, "n_fft": 1024, "n_mels": 80, "hop_length": 300}


def _files(tmp_path, durations, unvoiced=()):
    lines = []
    for i, dur in enumerate(durations):
        wave, f0, _ = synthetic.utterance(i, duration=dur)
        if i in unvoiced:
            f0 = np.zeros_like(f0)
        p = tmp_path / f"u{i}.wav"
        write_wav(p, wave, SR, "float32")
        np.save(str(p) + "_f0.npy", f0)
        lines.append(f"{p}|0\n")
    return lines


def _ds(lines, cfg=CFG, validation=False):
    return md.MelDataset(lines, mel_params=dict(MEL), validation=validation, verbose=False, synthetic_data=cfg)


def test_length_and_validation_split(tmp_path):
    lines = _files(tmp_path, [2.0, 1.0, 3.0, 2.5, 1.5, 2.0, 1.2, 0.8])
    assert len(_ds(lines)) == 8 + round(8 * 0.25)
    assert len(_ds(lines, validation=True)) == 8
    assert len(_ds(lines, {**CFG, "apply_to_validation": True}, validation=True)) == 10
    assert len(_ds(lines, {**CFG, "absolute_count": 7, "max_items": 5})) == 13
    assert len(_ds(lines, {**CFG, "ratio": 0.01})) == 9                    # at least one when ratio > 0
    assert len(_ds(lines, {**CFG, "pitch_shift": {"enabled": False}})) == 8      # no generator: disabled
    assert len(_ds(lines, None)) == 8


def test_unsupported_resample_type_is_refused(tmp_path):
    lines = _files(tmp_path, [1.0])
    with pytest.raises(ValueError, match="resample_type"):
        _ds(lines, {**CFG, "pitch_shift": {**CFG["pitch_shift"], "resample_type": "soxr_hq"}})


def _restated_draws(ds_lines, f0s, lens, n_items, cfg):
    """The reference's draw order for n_items synthetic items (all files valid, voiced)."""
    pcfg = cfg["pitch_shift"]
    out = []
    for _ in range(n_items):
        random.choice(["pitch_shift"])
        while True:
            path = random.choice(ds_lines)
            f0 = f0s[path]
            if np.count_nonzero(f0 > 0) / max(1, f0.size) < pcfg["min_voiced_fraction"]:
                continue
            s = random.choice(pcfg["semitones"])
            if s == 0:
                continue
            break
        lo, hi = pcfg["gain_db_range"]
        gain = 10.0 ** (random.uniform(lo, hi) / 20.0)
        shifted = f0.astype(np.float32) * float(2 ** (s / 12.0))
        shifted[f0 == 0] = 0.0
        L = 1 + lens[path] // 300
        lab = md.align_length(shifted, L)
        crop = int(np.random.randint(0, L - 192)) if L > 192 else 0
        out.append((path, s, gain, crop, lab[crop:crop + 192]))
    return out


def test_synthetic_items_follow_the_reference_draw_order(tmp_path):
    lines = _files(tmp_path, [2.0, 1.0, 3.0, 2.5, 1.5, 2.0, 4.0, 0.8], unvoiced=(1,))
    ds = _ds(lines)
    paths = [ln[:-1].split("|")[0] for ln in lines]
    f0s = {p: np.load(p + "_f0.npy") for p in paths}
    lens = {p: md.wav_info(p)[0] for p in paths}
    n_syn = len(ds) - 8
    random.seed(11); np.random.seed(11)
    got = [ds[8 + i] for i in range(n_syn)]
    random.seed(11); np.random.seed(11)
    want = _restated_draws(paths, f0s, lens, n_syn, CFG)
    for item, (path, s, gain, crop, lab) in zip(got, want):
        wave, f0, sil, frame_start, src_sr, req = item
        assert isinstance(req, md.PitchShiftRequest)
        assert req.path == path and req.n_steps == s and req.gain == pytest.approx(gain, rel=1e-7)
        assert req.crop == crop and src_sr == SR
        np.testing.assert_array_equal(f0.numpy(), lab)
        np.testing.assert_array_equal(sil.numpy(), (lab == 0).astype(np.float32))
        assert wave.shape[0] == lens[path]                           # the whole file goes to the device
        assert req.n == lens[path]


def test_low_voiced_files_are_rejected(tmp_path):
    lines = _files(tmp_path, [1.0, 1.0, 1.0, 1.0], unvoiced=(0, 1, 2))
    ds = _ds(lines)
    random.seed(3); np.random.seed(3)
    for i in range(4, len(ds)):
        assert ds[i][5].path.endswith("u3.wav")


def test_collater_packs_synthetic_rows(tmp_path):
    """A synthetic row on a 60-s base file ships the whole file packed, but its batch row holds only the window the
    cropped 192 frames read: the padded width does not depend on the base file."""
    lines = _files(tmp_path, [2.0, 60.0, 1.0])
    ds = _ds(lines, {**CFG, "absolute_count": 4})
    random.seed(0); np.random.seed(0)
    big = next(it for it in (ds[3] for _ in range(200)) if it[5].n == 60 * SR)
    out = md.Collater()([ds[0], ds[2], big])
    waves, lengths, crops = out[0], out[1], out[2]
    assert waves.shape == (3, max(48000, big[5].out_len)) and waves.shape[1] <= 58412
    pack = out[-1]
    assert isinstance(pack, md.PitchShiftBatch) and len(out) == 7
    assert pack.rows.tolist() == [2] and pack.src.numel() == 60 * SR and pack.src_len.tolist() == [60 * SR]
    req = big[5]
    assert int(lengths[2]) == req.out_len and int(crops[2]) == req.frame_start
    assert pack.out_start.tolist() == [req.out_start] and pack.noise is None
    # the window covers exactly what mel frames crop .. crop + 191 read (n_fft 1024, hop 300, centre padding)
    assert req.out_start <= 300 * req.crop - 512 or req.out_start == 0
    assert req.out_start + req.out_len >= min(req.n, 300 * (req.crop + 191) + 512)
    assert (waves[2] == 0).all()


def test_noise_is_drawn_over_the_whole_file(tmp_path):
    lines = _files(tmp_path, [3.0])
    cfg = {**CFG, "pitch_shift": {**CFG["pitch_shift"], "noise_db": -40.0}}
    ds = _ds(lines, cfg)
    random.seed(2); np.random.seed(2)
    req = ds[1][5]
    random.seed(2); np.random.seed(2)
    full = np.random.normal(scale=10 ** (-40 / 20), size=(3 * SR,)).astype(np.float32)
    crop = np.random.randint(0, 1 + 3 * SR // 300 - 192)
    assert req.crop == crop
    np.testing.assert_array_equal(req.noise, full[req.out_start:req.out_start + req.out_len])


def test_window_frames_equal_the_whole_waves_frames():
    """Mel frames frame_start .. frame_start + 191 of the written window equal frames crop .. crop + 191 of the whole
    shifted wave (float64 mel oracle, reflect padding included)."""
    from oracle import mel_ref
    rng = np.random.default_rng(0)
    for n in (96000, 58000, 57901, 70011, 30000):
        w = rng.standard_normal(n)
        full = mel_ref.log_mel(w)
        L = full.shape[1]
        for c in ({min(c, L - 193) for c in (0, 1, 2, 3, (L - 193) // 2, L - 193)} if L > 192 else {0}):
            start, count, first = md.synthetic_window(n, c, 300, 1024)
            keep = min(192, L)
            win = mel_ref.log_mel(w[start:start + count])
            assert count <= 58412 and win.shape[1] >= first + keep
            np.testing.assert_array_equal(win[:, first:first + keep], full[:, c:c + keep])
