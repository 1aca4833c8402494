"""CPU checks of the mel oracle: the two independent restatements must agree."""
import numpy as np
import pytest

from oracle import mel_ref
from pitchextractor_amd import synthetic
from tests import mel_plan_ref


def test_frame_count_and_reflect():
    assert mel_ref.num_frames(48000) == 161
    assert mel_ref.num_frames(58624) == 196
    idx = mel_ref.reflect_index(np.array([-3, -1, 0, 9, 10, 12]), 10)
    assert idx.tolist() == [3, 1, 0, 9, 8, 6]
    fr = mel_ref.frame_signal(np.arange(2000.0), 1024, 300)
    assert fr.shape == (7, 1024)
    assert fr[0, 0] == 512 and fr[0, 512] == 0 and fr[0, 511] == 1
    assert fr[6, -1] == 2 * 1999 - (6 * 300 + 1023 - 512)


def test_filterbank_shape_and_sparsity():
    fb = mel_ref.mel_filterbank()
    assert fb.shape == (513, 80)
    assert (fb >= 0).all() and fb.max() <= 1.0
    # HTK triangles overlap by half: at most two filters are non-zero per bin
    assert ((fb > 0).sum(axis=1) <= 2).all()


def test_direct_dft_matches_rfft():
    wave, _, _ = synthetic.utterance(0, duration=0.2)
    a = mel_ref.mel_spectrogram(wave, direct_dft=True)
    b = mel_ref.mel_spectrogram(wave, direct_dft=False)
    assert a.shape == (80, 17)
    assert np.allclose(a, b, rtol=1e-9, atol=1e-12)


def test_float64_oracle_matches_torch_stft():
    wave, _, _ = synthetic.utterance(3, duration=1.0)
    ref64 = mel_ref.mel_spectrogram(wave)
    ref32 = mel_ref.mel_spectrogram_torch_stft(wave)
    assert ref32.shape == ref64.shape == (80, 81)
    assert np.abs(ref32 - ref64).max() <= 1e-4 * ref64.max()
    # bins near the 1e-5 log floor sit on the fp32 FFT rounding floor (|dX| ~ 1e-8 |X|max):
    # two float32-vs-float64 implementations differ by a few 1e-4 there after the log
    strong = ref64 >= 1e-2
    assert np.abs(ref32 - ref64)[strong].max() <= 1e-4 * ref64[strong].min() or \
        (np.abs(ref32 - ref64)[strong] <= 1e-4 * ref64[strong]).all()
    a, b = mel_ref.log_normalise(ref64), mel_ref.log_normalise(ref32.astype(np.float64))
    assert np.abs(a - b).max() < 1e-3


def test_log_normalise_constants():
    # meldataset.py:650 with mean, std = -4, 4
    assert np.isclose(mel_ref.log_normalise(np.array([0.0]))[0], (np.log(1e-5) + 4) / 4)


# ---- off the defaults: the parameter sets of tests/test_mel_params_gpu.py ---------------------------------------

def _wave(params, seed, duration):
    """A glide with a little noise on top (synthetic.utterance silences 10-30 frames, which at these lengths and
    hops can be all of them)."""
    rng = np.random.default_rng(seed)
    audio = synthetic.glide(duration, 90.0 + 20.0 * seed, 700.0, params["sample_rate"])[0]
    return (audio + 0.01 * rng.standard_normal(audio.shape[0])).astype(np.float32)


def test_default_keywords_change_nothing():
    """f_min / f_max default to 0 .. sr // 2: the same filterbank, bit for bit, as before they were keywords."""
    wave, _, _ = synthetic.utterance(0, duration=0.2)
    assert np.abs(wave).max() > 0.5
    a = mel_ref.mel_spectrogram(wave)
    b = mel_ref.mel_spectrogram(wave, f_min=0.0, f_max=12000.0, win_length=1024)
    assert np.array_equal(a, b)
    assert np.array_equal(mel_ref.mel_spectrogram_torch_stft(wave),
                          mel_ref.mel_spectrogram_torch_stft(wave, f_min=0.0, f_max=None))
    assert np.array_equal(mel_ref.log_mel(wave), mel_ref.log_mel(wave, f_max=12000.0))
    # and a band limit does change it
    assert not np.array_equal(a, mel_ref.mel_spectrogram(wave, f_max=4000.0))


def test_filterbank_honours_band_limits():
    fb = mel_plan_ref.filterbank32(sample_rate=24000, n_mels=80, f_min=50.0, f_max=7600.0)
    freqs = np.linspace(0.0, 12000.0, 513)
    assert (fb[freqs <= 50.0] == 0).all() and (fb[freqs >= 7600.0] == 0).all()
    assert (fb.sum(axis=1)[(freqs > 100.0) & (freqs < 7000.0)] > 0).all()


@pytest.mark.parametrize("name,params,_table", mel_plan_ref.PARAM_SETS, ids=mel_plan_ref.PARAM_IDS)
def test_restatements_agree_per_parameter_set(name, params, _table):
    kw = mel_plan_ref.mel_kwargs(params)
    wave = _wave(params, 3, 1.0)
    ref64 = mel_ref.mel_spectrogram(wave, **kw)
    ref32 = mel_ref.mel_spectrogram_torch_stft(wave, **kw)
    assert ref32.shape == ref64.shape == (params["n_mels"], 1 + wave.shape[0] // params["hop_length"])
    assert np.abs(ref32 - ref64).max() <= 1e-4 * ref64.max()
    strong = ref64 >= 1e-2
    assert (np.abs(ref32 - ref64)[strong] <= 1e-4 * ref64[strong]).all()
    a, b = mel_ref.log_normalise(ref64), mel_ref.log_normalise(ref32.astype(np.float64))
    assert np.abs(a - b).max() < 1e-3


@pytest.mark.parametrize("name,params,_table", mel_plan_ref.PARAM_SETS, ids=mel_plan_ref.PARAM_IDS)
def test_direct_dft_matches_rfft_per_parameter_set(name, params, _table):
    kw = mel_plan_ref.mel_kwargs(params)
    wave = _wave(params, 0, 0.1)
    a = mel_ref.mel_spectrogram(wave, direct_dft=True, **kw)
    b = mel_ref.mel_spectrogram(wave, direct_dft=False, **kw)
    assert a.shape == (params["n_mels"], 1 + wave.shape[0] // params["hop_length"])
    assert np.allclose(a, b, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("name,params,table", mel_plan_ref.PARAM_SETS + mel_plan_ref.REJECTED_SETS,
                         ids=mel_plan_ref.PARAM_IDS + [r[0] for r in mel_plan_ref.REJECTED_SETS])
def test_chunk_table_is_pinned(name, params, table):
    """(n_pairs, most chunks of one filter, empty filters) of every parameter set the GPU tests run: they reach
    exactly kMaxParts chunks, n_mels > 64, an empty filter next to the 256-pair cap, and -- for the two sets the
    plan must refuse -- 9 chunks and 280 pairs."""
    got = mel_plan_ref.chunk_table(**params)
    assert got == table
    accepted = name in mel_plan_ref.PARAM_IDS
    assert (got[0] <= mel_plan_ref.MAX_PAIRS and got[1] <= mel_plan_ref.MAX_CHUNKS) == accepted


def test_chunk_table_edges():
    assert mel_plan_ref.empty_filters(sample_rate=24000, n_mels=200) != []
    assert max(t[1] for _, _, t in mel_plan_ref.PARAM_SETS) == mel_plan_ref.MAX_CHUNKS
    assert max(p["n_mels"] for _, p, _ in mel_plan_ref.PARAM_SETS) > 64 * 3
