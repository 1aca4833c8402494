"""WORLD CheapTrick without a GPU: the float64 restatement against itself (the interval-sum smoothing against WORLD's
literal cumulative-sum formulation; comparative checks against the unsmoothed periodogram; basic properties), the C
ABI's host-side argument checks, and the dataset's ``world_resynthesis`` items (gating, draw order, request fields,
labels, the fallback from a failing pitch shift).  pyworld is not available: parity with its binary is unpinned."""
import ctypes
import logging
import random

import numpy as np
import pytest

from pitchextractor_amd import _lib, build
from pitchextractor_amd import meldataset as md
from pitchextractor_amd import synthetic, world
from tests import cheaptrick_ref as ct
from tests import world_ref as wr
from tests.test_data_layer import write_wav

FS, HOP, N = 24000, 300, 1024
FP = 1000.0 * HOP / FS


@pytest.fixture(scope="module")
def vowel():
    """Constant 150.3 Hz "ah" from the synthesis restatement, no aperiodicity: (wave, f0, template)."""
    f0, L = 150.3, 60
    sp = wr.envelope("ah", FS, N)
    y = wr.synthesize(np.full(L, f0), sp, None, FS, 5.0, np.zeros(wr.output_length(L, FS, 5.0)))
    return y, f0, sp


# --------------------------------------------------------------------------- the restatement against itself
def test_default_fft_size_and_floor():
    assert [ct.default_fft_size(fs) for fs in (8000, 16000, 24000, 44100, 48000)] == [512, 1024, 1024, 2048, 2048]
    assert [world.cheaptrick_fft_size(fs) for fs in (8000, 16000, 24000, 44100, 48000)] == [512, 1024, 1024, 2048, 2048]
    assert world.cheaptrick_floor(FS, N) == ct.f0_floor_of(FS, N) == 3.0 * FS / (N - 3.0)
    assert ct.f0_floor_of(FS, N) <= 71.0 < ct.f0_floor_of(FS, 512)


def test_interval_sum_equals_the_cumulative_formulation():
    """Bin by bin, float64.  The bound is the cumulative sum's rounding: each of its ``bins`` entries carries up to
    2^-53 of the running total, the difference of two of them 2^-52 bins total, divided by the width; relative to the
    bin's value that is bins 2^-52 total / (w value).  The interval sum's own rounding (at most that many terms, each
    2^-53 of a partial sum no larger than w value) stays below it."""
    f0, L = 150.3, 24
    tilt = 10.0 ** (-9.0 * np.arange(N // 2 + 1) / (N // 2))
    y = wr.synthesize(np.full(L, f0), wr.envelope("ah", FS, N) * tilt, None, FS, 5.0,
                      np.zeros(wr.output_length(L, FS, 5.0)))
    P = ct.dc_correction(ct.power_spectrum(ct.frame_window(y, FS, f0, 0.06), N), FS, f0, N)
    assert P.max() / P.min() >= 1e8
    a, b = ct.smooth_interval(P, FS, f0, N), ct.smooth_cumulative(P, FS, f0, N)
    width, delta = 2.0 * f0 / 3.0, FS / N
    boundary = int(width * N / FS) + 1
    bins = N // 2 + 2 * boundary + 1
    total = P[ct._mirror(np.arange(bins) - boundary, N)].sum() * delta
    bound = bins * 2.0 ** -52 * total / (width * a)
    assert (a > 0).all() and (np.abs(b - a) / a <= bound).all(), (np.abs(b - a) / a / bound).max()
    assert a.max() / a.min() >= 1e7                              # the check spans the quiet bins


def test_envelope_is_closer_to_the_template_than_the_periodogram(vowel):
    """Comparative, no tuned number: over interior frames and the formant band, the CheapTrick envelope is closer in
    dB to the template the signal was synthesized from than the unsmoothed windowed periodogram of the same frames,
    and varies less across analysis positions within one pitch period."""
    y, f0, sp = vowel
    frames = range(10, 50)
    K = int(4000.0 / (FS / N))
    db = lambda a: 10.0 * np.log10(a)  # noqa: E731
    env = np.stack([ct.frame(y, FS, f0, f * 0.005, N) for f in frames])
    per = np.stack([ct.frame(y, FS, f0, f * 0.005, N, smooth=False) for f in frames])
    assert (per[:, 1:K] > 0).all()                               # bin 0 is out: the window removes the DC exactly
    rms = lambda a: float(np.sqrt(np.mean((db(a[:, 1:K]) - db(sp[1:K])) ** 2)))  # noqa: E731
    print(f"rms dB to the template: envelope {rms(env):.2f}, periodogram {rms(per):.2f}")
    assert rms(env) < rms(per)
    pos = 0.15 + np.arange(16) / 16.0 / f0
    E = np.stack([ct.frame(y, FS, f0, p, N) for p in pos])
    P = np.stack([ct.frame(y, FS, f0, p, N, smooth=False) for p in pos])
    spread = lambda a: float(db(a[:, 1:K]).std(axis=0).mean())  # noqa: E731
    print(f"spread in dB within one period: envelope {spread(E):.3f}, periodogram {spread(P):.3f}")
    assert spread(E) < spread(P)


def test_output_is_positive_and_finite(vowel):
    y, f0, _ = vowel
    for x, curve in ((y, np.full(12, f0)), (np.zeros(2000), np.full(12, f0)), (np.zeros(2000), np.zeros(12)),
                     (y, np.concatenate([np.zeros(6), np.full(6, 900.0)]))):
        for fp32 in (False, True):
            env = ct.cheaptrick(x, curve, FS, 5.0, fft_size=N, fp32=fp32)
            assert env.shape == (12, N // 2 + 1) and np.isfinite(env).all() and (env > 0).all()
            assert env.dtype == (np.float32 if fp32 else np.float64)
    zero = ct.cheaptrick(np.zeros(2000), np.full(3, f0), FS, 5.0, fft_size=N)
    np.testing.assert_allclose(zero, ct.EPS, rtol=1e-9)          # the stand-in for WORLD's |randn| eps, lifted flat


def test_frames_at_or_below_the_floor_are_analysed_at_500_hz(vowel):
    y, _, _ = vowel
    floor32 = float(np.float32(ct.f0_floor_of(FS, N)))
    low = np.array([0.0, 30.0, np.nextafter(np.float32(floor32), np.float32(0)), 71.0], np.float32)
    got = ct.cheaptrick(y, low, FS, 5.0, fft_size=N)
    want = ct.cheaptrick(y, np.array([500.0, 500.0, 500.0, 71.0], np.float32), FS, 5.0, fft_size=N)
    np.testing.assert_array_equal(got, want)
    assert not np.array_equal(got[3], ct.frame(y, FS, 500.0, 0.015, N))
    assert ct.used_f0(ct.f0_floor_of(FS, N), FS, N) == 500.0 and ct.used_f0(float("nan"), FS, N) == 500.0


def test_fp32_variant_stays_near_float64(vowel):
    y, f0, _ = vowel
    curve = np.full(20, f0)
    a, b = ct.cheaptrick(y, curve, FS, 5.0, fft_size=N), ct.cheaptrick(y, curve, FS, 5.0, fft_size=N, fp32=True)
    assert 0 < np.abs(np.log(b) - np.log(a)).max() < 1e-4
    sub = ct.cheaptrick(y, curve, FS, 5.0, fft_size=N, first_frame=7, n_frames=5)
    np.testing.assert_array_equal(sub, a[7:12])


def test_label_curve_and_host_refusals():
    import torch
    lowest = world.lowest_f0(FS, N)
    curve = np.array([0.0, 10.0, lowest, np.nextafter(lowest, 1e9), 220.0])
    np.testing.assert_array_equal(world.label_curve(curve, FS, N), [0.0, 0.0, 0.0, curve[3], 220.0])
    np.testing.assert_array_equal(world.label_curve(world.label_curve(curve, FS, N), FS, N),
                                  world.label_curve(curve, FS, N))
    # every labelled frame is one the synthesizer voices, every other one it does not
    table_f0 = np.where(world.label_curve(curve, FS, N) >= lowest, 1, 0)
    np.testing.assert_array_equal(table_f0, world.label_curve(curve, FS, N) > 0)
    x = torch.zeros(2400)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        world.cheaptrick(x, np.full(4, 100.0), FS, FP)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        world.cheaptrick_ragged(x, [2400], [np.full(4, 100.0)], FS, FP)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        world.resynthesize(x, np.full(4, 100.0), np.full(4, 120.0), FS, FP)


# --------------------------------------------------------------------------- C ABI, host side only
@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _lib.load()


def test_plan_and_entry_point_argument_checks(lib):
    Lg = lambda *v: (ctypes.c_long * len(v))(*v)  # noqa: E731
    K = lib.pe_cheaptrick_plan_fields()
    meta, tot = (ctypes.c_long * (4 * K))(), Lg(0)

    def plan(x_off=0, x_len=2400, f0_off=0, f0_len=8, first=0, frames=8, out_off=0, stride=513, fs=24000.0, fpm=FP,
             floor=71.0, fft=1024, rows=1, meta=meta, tot=tot):
        return lib.pe_cheaptrick_plan(rows, Lg(x_off), Lg(x_len), Lg(f0_off), Lg(f0_len), Lg(first), Lg(frames),
                                      Lg(out_off), Lg(stride), fs, fpm, floor, fft, meta, tot)
    assert plan() == 0 and tot[0] == 8
    assert [meta[i] for i in range(K)] == [0, 2400, 0, 0, 8, 0, 0, 513]
    assert plan(first=3, frames=5) == 0 and tot[0] == 5 and plan(frames=0, x_len=0) == 0 and tot[0] == 0
    assert plan(fft=4096) == -2 and plan(fft=256) == -2 and plan(fft=1000) == -2 and plan(fft=0) == -1
    assert plan(fft=512) == -2 and plan(fft=512, floor=150.0) == 0        # 3 fs / (fft_size - 3) against f0_floor
    assert plan(fs=48000.0) == -2 and plan(fs=48000.0, fft=2048, stride=1025) == 0 and plan(fs=48000.0, fft=2048) == -1
    assert plan(fs=0.0) == -1 and plan(fpm=float("nan")) == -1 and plan(floor=0.0) == -1 and plan(fpm=-5.0) == -1
    assert plan(first=1, frames=8) == -1 and plan(frames=-1) == -1 and plan(first=-1) == -1
    assert plan(x_len=0) == -1 and plan(x_len=-1) == -1 and plan(x_off=-1) == -1 and plan(f0_off=-1) == -1
    assert plan(stride=512) == -1 and plan(out_off=-1) == -1
    assert plan(meta=None) == -1 and plan(tot=None) == -1
    assert plan(rows=0, meta=None) == 0 and plan(rows=-1) == -1 and plan(rows=65536) == -1
    assert lib.pe_cheaptrick_plan(1, None, None, None, None, None, None, None, None, 24000.0, FP, 71.0, 1024, meta,
                                  tot) == -1
    assert plan() == 0
    p = ctypes.c_void_p(8)
    run = lambda x=p, f0=p, dm=p, hm=meta, tb=p, rows=1, fs=24000.0, fpm=FP, q1=-0.15, floor=71.0, fft=1024, sp=p: \
        lib.pe_cheaptrick(x, f0, dm, hm, tb, rows, fs, fpm, q1, floor, fft, sp, None)  # noqa: E731
    assert run(x=None) == -1 and run(f0=None) == -1 and run(dm=None) == -1 and run(tb=None) == -1 and run(sp=None) == -1
    assert run(hm=None) == -1 and run(q1=float("nan")) == -1
    assert run(fft=4096) == -2 and run(fft=512) == -2 and run(fft=0) == -1 and run(fs=-1.0) == -1
    assert run(rows=-1) == -1 and run(rows=65536) == -1
    assert run(rows=0, x=None, f0=None, dm=None, hm=None, tb=None, sp=None) == 0          # nothing to do
    assert run(rows=0, fft=4096) == -2                                                   # a bad configuration still is
    bad = (ctypes.c_long * K)(*[0, 2400, 0, 0, 8, 3, 0, 513])                            # not the plan's frame offsets
    assert run(hm=bad) == -1
    narrow = (ctypes.c_long * K)(*[0, 2400, 0, 0, 8, 0, 0, 512])
    assert run(hm=narrow) == -1
    assert plan(frames=0, x_len=0) == 0                                                  # no frames: no launch
    assert run(x=None, f0=None, dm=None, tb=None, sp=None) == 0


# --------------------------------------------------------------------------- dataset
MEL = {"sample_rate": FS, "win_len": 1024, "n_fft": 1024, "n_mels": 80, "hop_length": HOP}
PS_CFG = {"enabled": True, "semitones": [-4, -2, -1, 1, 2, 4], "gain_db_range": [-6.0, 3.0],
          "min_voiced_fraction": 0.05, "resample_type": "kaiser_best"}
WORLD_CFG = {"enabled": True, "backend": "hip", "duration": {"min": 0.6, "max": 1.5}}
RS_CFG = {"enabled": True, "backend": "hip", "semitones": [-4, -1, 0, 3], "gain_db_range": [-9.0, 0.0],
          "noise_db": -50.0, "min_voiced_fraction": 0.05, "max_attempts": 3, "aperiodicity": 0.2, "q1": -0.1,
          "modulation": {"vibrato_probability": 0.5, "vibrato_semitones": 0.4, "vibrato_rate_range": [4.0, 6.0]}}


def _files(tmp_path, durations):
    lines = []
    for i, dur in enumerate(durations):
        wave, f0, _ = synthetic.utterance(i, duration=dur)
        p = tmp_path / f"u{i}.wav"
        write_wav(p, wave, FS, "float32")
        np.save(str(p) + "_f0.npy", f0)
        lines.append(f"{p}|0\n")
    return lines


def _ds(lines, syn):
    return md.MelDataset(lines, mel_params=dict(MEL), verbose=False, synthetic_data=syn)


def _same_item(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        if isinstance(u, tuple) and hasattr(u, "_fields"):
            assert type(u) is type(v)
            for s, t in zip(u, v):
                np.testing.assert_array_equal(np.asarray(s), np.asarray(t))
        else:
            np.testing.assert_array_equal(np.asarray(u), np.asarray(v))


def test_absent_disabled_or_not_hip_changes_nothing(tmp_path, caplog):
    lines = _files(tmp_path, [1.0, 3.0])
    base = {"enabled": True, "absolute_count": 8, "pitch_shift": PS_CFG, "world_vocoder": WORLD_CFG}
    plain = _ds(lines, base)
    assert plain._synthetic_generators == ["pitch_shift", "world_vocoder"]
    random.seed(5); np.random.seed(5)
    want = [plain[2 + i] for i in range(8)]
    with caplog.at_level(logging.WARNING):
        variants = [{**base, "world_resynthesis": {}}, {**base, "world_resynthesis": {**RS_CFG, "enabled": False}},
                    {**base, "world_resynthesis": {"backend": "hip"}}]
        assert not [r for r in caplog.records if "resynthesis" in r.getMessage()]
        variants.append({**base, "world_resynthesis": {**RS_CFG, "backend": "pyworld"}})
        variants.append({**base, "world_resynthesis": {"enabled": True}})
        for syn in variants:
            ds = _ds(lines, syn)
            assert ds._synthetic_generators == ["pitch_shift", "world_vocoder"] and len(ds) == len(plain)
            assert ds.synthetic_resynthesis_config is None
            random.seed(5); np.random.seed(5)
            for i in range(8):
                _same_item(ds[2 + i], want[i])
    warned = [r.getMessage() for r in caplog.records if "resynthesis disabled" in r.getMessage()]
    assert len(warned) == 2 and all("backend: hip" in m for m in warned)


def test_gating_and_configuration(tmp_path, caplog):
    lines = _files(tmp_path, [1.0])
    base = {"enabled": True, "absolute_count": 2, "pitch_shift": PS_CFG}
    assert _ds(lines, {**base, "world_resynthesis": RS_CFG})._synthetic_generators == ["pitch_shift",
                                                                                       "world_resynthesis"]
    all3 = _ds(lines, {**base, "world_vocoder": WORLD_CFG, "world_resynthesis": RS_CFG})
    assert all3._synthetic_generators == ["pitch_shift", "world_vocoder", "world_resynthesis"]
    alone = _ds(lines, {**base, "pitch_shift": {"enabled": False}, "world_resynthesis": {"enabled": True,
                                                                                         "backend": "HIP"}})
    assert alone._synthetic_generators == ["world_resynthesis"] and len(alone) == 3
    cfg = alone.synthetic_resynthesis_config
    assert cfg["semitones"] == [-4, -2, -1, 1, 2, 4] and cfg["aperiodicity"] == 0.0 and cfg["q1"] == -0.15
    assert cfg["fft_size"] == 1024 and cfg["frame_period"] == FP and cfg["max_attempts"] == 5
    val = md.MelDataset(lines, mel_params=dict(MEL), verbose=False, validation=True,
                        synthetic_data={**base, "world_resynthesis": RS_CFG})
    assert val._synthetic_generators == [] and len(val) == 1
    with caplog.at_level(logging.WARNING):
        _ds(lines, {**base, "world_resynthesis": {**RS_CFG, "speed": 2, "modulation": {"max_segments": 3}}})
    said = [r.getMessage() for r in caplog.records]
    assert any("'speed'" in m and "not read" in m for m in said) and any("'max_segments'" in m for m in said)
    with pytest.raises(ValueError, match="aperiodicity"):
        _ds(lines, {**base, "world_resynthesis": {**RS_CFG, "aperiodicity": 1.0}})
    with pytest.raises(ValueError, match="gain_db_range"):
        _ds(lines, {**base, "world_resynthesis": {**RS_CFG, "gain_db_range": [1.0, 2.0, 3.0]}})
    with pytest.raises(ValueError, match="fft_size"):             # 96 kHz would need a 4096-point transform
        md.MelDataset(lines, sr=96000, mel_params={**MEL, "sample_rate": 96000}, verbose=False,
                      synthetic_data={**base, "world_resynthesis": RS_CFG})


def _restated_item(cfg, paths):
    """The documented draw order: file, semitone, gain, vibrato, noise, crop.  -> the request's expected fields."""
    path = random.choice(paths)
    wave, sr = md.read_wav(path)
    n = len(wave)
    mel_len = 1 + n // HOP
    base = md.align_length(np.load(path + "_f0.npy").astype(np.float32), mel_len).astype(np.float64)
    semitone = random.choice(cfg["semitones"])
    gain = 10.0 ** (random.uniform(*cfg["gain_db_range"]) / 20.0)
    new = base * float(2 ** (semitone / 12.0))
    mod = cfg["modulation"]
    if random.random() < mod["vibrato_probability"]:
        rate = random.uniform(*mod["vibrato_rate_range"])
        t = np.arange(mel_len, dtype=np.float64) * (FP / 1000.0)
        new = new * 2.0 ** (np.sin(2.0 * np.pi * rate * t) * (mod["vibrato_semitones"] / 12.0))
    curve = np.where(new > world.lowest_f0(FS, N), new, 0.0)
    noise = np.random.normal(scale=10.0 ** (cfg["noise_db"] / 20.0), size=(n,)).astype(np.float32)
    crop = int(np.random.randint(0, mel_len - 192)) if mel_len > 192 else 0
    return path, semitone, gain, n, base, curve, noise, crop


def _check_item(item, want):
    path, _, gain, n, base, curve, noise, crop = want
    wave, f0, sil, frame_start, sr, req = item
    assert isinstance(req, md.ResynthesisRequest) and sr == FS and wave.shape[0] == n
    assert (req.path, req.n, req.crop) == (path, n, crop) and req.gain == pytest.approx(gain, rel=1e-12)
    np.testing.assert_array_equal(req.base_curve, base)
    np.testing.assert_array_equal(req.curve, curve)
    assert req.curve.dtype == np.float64 and req.curve.size == 1 + n // HOP
    label = md.align_length(req.curve.astype(np.float32), 1 + n // HOP)[crop:crop + 192]
    np.testing.assert_array_equal(f0.numpy(), label)
    np.testing.assert_array_equal(sil.numpy(), (label == 0).astype(np.float32))
    assert (f0.numpy()[req.curve[crop:crop + 192] <= world.lowest_f0(FS, N)] == 0).all()
    start, count, first = md.synthetic_window(n, crop, HOP, 1024)
    assert (req.out_start, req.out_len, req.frame_start, frame_start) == (start, count, first, first)
    np.testing.assert_array_equal(req.noise, noise[start:start + count])
    table = world.time_base(req.curve, FS, FP, N)
    np.testing.assert_array_equal(req.index, table.index)
    np.testing.assert_array_equal(req.shift, table.shift)
    np.testing.assert_array_equal(req.vuv, table.vuv)
    assert req.seed == world.noise_seed(req.curve)


def test_items_follow_the_documented_draw_order(tmp_path):
    lines = _files(tmp_path, [1.0, 3.0, 1.6])
    paths = [ln[:-1].split("|")[0] for ln in lines]
    # frames the synthesizer will not voice: 26 Hz, four semitones down, is below lowest_f0 = 24.4 Hz
    f0 = np.load(paths[2] + "_f0.npy")
    f0[10:20] = 26.0
    np.save(paths[2] + "_f0.npy", f0)
    ds = _ds(lines, {"enabled": True, "absolute_count": 12, "pitch_shift": {"enabled": False},
                     "world_resynthesis": RS_CFG})
    random.seed(3); np.random.seed(3)
    got = [ds[3 + i] for i in range(12)]
    random.seed(3); np.random.seed(3)
    seen, cropped, unvoiced = set(), 0, 0
    for item in got:
        assert random.choice(["world_resynthesis"]) == "world_resynthesis"
        want = _restated_item(RS_CFG, paths)
        _check_item(item, want)
        seen.add(want[1])
        cropped += want[7] > 0
        unvoiced += bool(want[0] == paths[2] and want[1] == -4 and (item[-1].curve[10:20] == 0).all())
    assert len(seen) >= 3 and 0 in seen and cropped >= 1 and unvoiced >= 1


def test_failed_pitch_shift_falls_back_to_resynthesis(tmp_path):
    lines = _files(tmp_path, [1.0])
    paths = [ln[:-1].split("|")[0] for ln in lines]
    ps = {**PS_CFG, "semitones": [0], "max_attempts": 2}           # a zero shift is never accepted: it gives up
    ds = _ds(lines, {"enabled": True, "absolute_count": 4, "pitch_shift": ps, "world_resynthesis": RS_CFG})
    random.seed(2); np.random.seed(2)
    got = [ds[1 + i] for i in range(4)]
    random.seed(2); np.random.seed(2)
    fell = 0
    for item in got:
        if random.choice(["pitch_shift", "world_resynthesis"]) == "pitch_shift":
            for _ in range(2):
                random.choice(paths)
                random.choice([0])
            assert random.choice(["world_resynthesis"]) == "world_resynthesis"
            fell += 1
        _check_item(item, _restated_item(RS_CFG, paths))
    assert fell >= 1


def test_unusable_files_end_in_an_error_or_the_vowel_generator(tmp_path):
    lines = _files(tmp_path, [1.0])
    path = lines[0][:-1].split("|")[0]
    np.save(path + "_f0.npy", np.zeros(81, np.float32))               # unvoiced: nothing to resynthesize
    base = {"enabled": True, "absolute_count": 2, "pitch_shift": {"enabled": False}}
    alone = _ds(lines, {**base, "world_resynthesis": RS_CFG})
    with pytest.raises(RuntimeError, match="resynthesis"):
        alone[1]
    both = _ds(lines, {**base, "world_vocoder": WORLD_CFG, "world_resynthesis": RS_CFG})
    random.seed(0); np.random.seed(0)
    kinds = {type(both[1 + i][-1]) for i in range(2)}
    assert kinds == {md.WorldRequest}


def test_collater_packs_resynthesis_rows(tmp_path):
    lines = _files(tmp_path, [2.0, 1.0])
    ds = _ds(lines, {"enabled": True, "absolute_count": 6, "pitch_shift": PS_CFG, "world_vocoder": WORLD_CFG,
                     "world_resynthesis": RS_CFG})
    random.seed(11); np.random.seed(11)
    items = [ds[2 + i] for i in range(6)]
    batch = [ds[0]] + items
    rows = [i for i, it in enumerate(batch) if isinstance(it[-1], md.ResynthesisRequest)]
    assert rows and len(rows) < 6
    out = md.Collater()(batch)
    waves, lengths, crops = out[0], out[1], out[2]
    pack = out[-1]
    assert isinstance(pack, md.ResynthesisBatch) and pack.rows.tolist() == rows
    assert sum(isinstance(t, md._SYNTHETIC_BATCHES) for t in out) == len({type(it[-1]) for it in items})
    src_off = np.concatenate([[0], np.cumsum(pack.src_len.numpy())])
    base_off = np.concatenate([[0], np.cumsum([len(c) for c in pack.curves])])
    for k, r in enumerate(rows):
        req = batch[r][-1]
        assert int(lengths[r]) == req.out_len and int(crops[r]) == req.frame_start and (waves[r] == 0).all()
        np.testing.assert_array_equal(pack.src[src_off[k]:src_off[k + 1]].numpy(), batch[r][0].numpy())
        np.testing.assert_array_equal(pack.base[base_off[k]:base_off[k + 1]].numpy(),
                                      req.base_curve.astype(np.float32))
        assert int(pack.n[k]) == req.n and pack.out_start[k] == req.out_start and int(pack.out_len[k]) == req.out_len
        assert float(pack.gains[k]) == np.float32(req.gain) and pack.seeds[k] == req.seed
        assert int(pack.src_sr[k]) == FS
        np.testing.assert_array_equal(pack.curves[k], req.curve)
        np.testing.assert_array_equal(pack.tables[k][0], req.index)
    assert pack.noise.numel() == sum(batch[r][-1].out_len for r in rows)
    plain = md.Collater()([ds[0], ds[1]])
    assert len(plain) == 6 and not any(isinstance(t, md._SYNTHETIC_BATCHES) for t in plain)
