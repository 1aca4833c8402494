"""WORLD-vocoder synthesis without a GPU: the host time base against the restatement's sequential loop, the
restatement's own sanity (length, amplitude law), the dataset's WORLD items against the reference's draw order
(Utils/synthetic.py:150-220, meldataset.py:382-418), gating by ``backend: hip``, the Collater, and the C ABI's host-side
checks."""
import ctypes
import random

import numpy as np
import pytest

from pitchextractor_amd import _lib, build
from pitchextractor_amd import meldataset as md
from pitchextractor_amd import synthetic, world
from tests import world_ref as ref
from tests.test_data_layer import write_wav

FS, HOP, N, FP = ref.FS, ref.HOP, ref.FFT, ref.FRAME_PERIOD


# --------------------------------------------------------------------------- time base
@pytest.mark.parametrize("name", list(ref.rows()))
def test_time_base_equals_the_sequential_restatement(name):
    f0 = ref.rows()[name][0]
    index, shift, vuv, noise_size, margin = ref.time_base(f0, FS, FP, N, check_margin=True)
    got = world.time_base(f0, FS, FP, N)
    np.testing.assert_array_equal(got.index, index)
    np.testing.assert_array_equal(got.noise_size, noise_size)
    np.testing.assert_array_equal(got.vuv, vuv)
    assert np.abs(got.shift - shift).max() <= 1e-15
    assert got.noise_size[-1] == 0 and (got.shift >= 0).all() and (got.shift * FS <= 1).all()
    assert {"two": 2, "glide_vib": 109, "hi": 409}.get(name, index.size) == index.size


def test_time_base_on_an_exact_period():
    """200 Hz at 24 kHz: every period is 120 samples exactly and the wraps hang on the phase sum's last bits, so only
    what rounding cannot move is asserted."""
    L = 120
    got = world.time_base(np.full(L, 200.0), FS, FP, N)
    assert abs(got.index.size - L * FP / 1000.0 * 200.0) <= 1
    assert (got.shift >= 0).all() and (got.shift <= 1.0 / FS).all()
    assert (np.diff(got.index) > 0).all()


def test_time_base_refuses_bad_curves():
    with pytest.raises(ValueError):
        world.time_base([100.0], FS, FP, N)
    with pytest.raises(ValueError):
        world.time_base([100.0, float("nan")], FS, FP, N)
    assert world.lowest_f0(FS, N) == FS / N + 1.0
    # frames below the floor are unvoiced: 500 Hz pulses
    low = world.time_base(np.full(8, 20.0), FS, FP, N)
    assert not low.vuv.any() and abs(low.index.size - 8 * FP / 1000.0 * 500.0) <= 1


# --------------------------------------------------------------------------- restatement: length and amplitude law
def test_output_length():
    for L, fs, fp in ((2, 24000, 12.5), (120, 24000, 12.5), (77, 16000, 5.0), (33, 22050, 1000.0 * 256 / 22050)):
        assert world.output_length(L, fs, fp) == ref.output_length(L, fs, fp) == int(L * fp * fs / 1000)
    assert world.output_length(120, FS, FP) == 120 * HOP
    y = ref.synthesize(np.full(7, 150.0), ref.envelope("ih", FS, N), None, FS, FP, np.zeros(7 * HOP))
    assert y.shape == (7 * HOP,)


def test_harmonic_amplitudes_follow_the_envelope():
    """Constant 200 Hz, "ah": harmonic h has amplitude 2 sqrt(sp(h f0)) / sqrt(period in samples)."""
    L = 120
    sp = ref.envelope("ah", FS, N)
    noise = np.random.default_rng(0).standard_normal(L * HOP)
    y = ref.synthesize(np.full(L, 200.0), sp, None, FS, FP, noise)
    spec = np.abs(np.fft.rfft(y[6000:6000 + FS])) * 2 / FS
    freq = np.linspace(0, FS / 2, N // 2 + 1)
    for h in (4, 5, 6, 12):
        want = 2 * np.sqrt(np.interp(200.0 * h, freq, sp)) / np.sqrt(120)
        assert abs(spec[200 * h] / want - 1) <= 0.05, (h, spec[200 * h] / want)
    quiet = ref.synthesize(np.full(L, 200.0), sp, None, FS, FP, np.zeros(L * HOP))
    assert np.sqrt(np.mean((y - quiet) ** 2)) < 1e-2 * np.sqrt(np.mean(y ** 2))       # ap = 0 is a ratio of 1e-6


def test_two_frames_give_two_pulses():
    f0, sp, _ = ref.rows()["two"]
    noise = np.random.default_rng(1).standard_normal(2 * HOP)
    y = ref.synthesize(f0, sp, None, FS, FP, noise)
    assert ref.time_base(f0, FS, FP, N)[0].size == 2 and y.shape == (2 * HOP,) and np.isfinite(y).all()
    assert np.abs(y).max() > 0.1
    y32 = ref.synthesize(f0, sp, None, FS, FP, noise, fp32=True)
    assert y32.dtype == np.float32 and np.abs(y32 - y).max() < 1e-6


def test_formant_templates_and_dc_remover():
    got = world.formant_templates(world.DEFAULT_VOWELS, FS, N)
    assert len(got) == 3
    for t, label in zip(got, ("ah", "ih", "uh")):
        np.testing.assert_array_equal(t, ref.envelope(label, FS, N))
    np.testing.assert_array_equal(world.dc_remover(N), ref.dc_remover(N))
    assert abs(world.dc_remover(N).sum() - 1.0) < 1e-12
    with pytest.raises(ValueError, match="No valid vowel templates"):
        world.formant_templates([{"label": "x", "formants": []}], FS, N)


# --------------------------------------------------------------------------- dataset
WORLD_CFG = {"enabled": True, "backend": "hip", "duration": {"min": 0.6, "max": 1.5}, "pitch_range": [110.0, 320.0],
             "gain_db_range": [-18.0, -6.0], "noise_db": -60.0,
             "modulation": {"vibrato_probability": 0.5, "vibrato_semitones": 0.4, "vibrato_rate_range": [4.0, 6.0]}}
PS_CFG = {"enabled": True, "semitones": [-4, -2, -1, 1, 2, 4], "gain_db_range": [-6.0, 3.0],
          "min_voiced_fraction": 0.05, "resample_type": "kaiser_best"}
MEL = {"sample_rate": FS, "win_len": 1024, "n_fft": 1024, "n_mels": 80, "hop_length": HOP}


def _files(tmp_path, durations):
    lines = []
    for i, dur in enumerate(durations):
        wave, f0, _ = synthetic.utterance(i, duration=dur)
        p = tmp_path / f"u{i}.wav"
        write_wav(p, wave, FS, "float32")
        np.save(str(p) + "_f0.npy", f0)
        lines.append(f"{p}|0\n")
    return lines


def _ds(lines, syn, validation=False):
    return md.MelDataset(lines, mel_params=dict(MEL), validation=validation, verbose=False, synthetic_data=syn)


def _restated_world_item(cfg):
    """``WorldSynthesizer.generate`` + ``_build_training_example`` as the reference draws them; -> (curve, template,
    gain, noise, crop, label)."""
    dur = cfg.get("duration", {})
    lo, hi = float(dur.get("min", 0.5)), float(dur.get("max", 1.8))
    duration = max(hi, 0.1) if hi <= lo else random.uniform(lo, hi)
    frames = max(2, int(np.ceil(duration * 1000.0 / FP)))
    template = random.choice([0, 1, 2])
    p_lo, p_hi = cfg.get("pitch_range", [110.0, 320.0])
    mod = {"vibrato_probability": 0.6, "vibrato_semitones": 0.35, "vibrato_rate_range": (4.0, 7.0), "max_segments": 4,
           **cfg.get("modulation", {})}
    curve = np.full(frames, random.uniform(p_lo, p_hi), dtype=np.float64)
    segments = random.randint(1, max(1, int(mod["max_segments"])))
    if segments > 1 and frames > 2:
        available = max(1, frames - 1)
        pos = [0] + sorted(random.sample(range(1, available), min(segments - 1, available - 1))) + [frames - 1]
        vals = [random.uniform(p_lo, p_hi) for _ in range(len(pos))]
        for i in range(len(pos) - 1):
            if pos[i + 1] > pos[i]:
                curve[pos[i]:pos[i + 1] + 1] = np.linspace(vals[i], vals[i + 1], pos[i + 1] - pos[i] + 1)
    if random.random() < mod["vibrato_probability"]:
        depth = max(float(mod["vibrato_semitones"]), 0.0)
        if depth > 0:
            rate = random.uniform(*mod["vibrato_rate_range"])
            t = np.arange(frames, dtype=np.float64) * (FP / 1000.0)
            curve *= 2.0 ** (np.sin(2.0 * np.pi * rate * t) * (depth / 12.0))
    g_lo, g_hi = cfg.get("gain_db_range", [-18.0, -6.0])
    gain = float(10.0 ** (random.uniform(g_lo, g_hi) / 20.0))
    n = frames * HOP
    noise = None
    if cfg.get("noise_db", -60.0) is not None:
        noise = np.random.normal(scale=float(10.0 ** (cfg.get("noise_db", -60.0) / 20.0)), size=(n,))
    mel_len = 1 + n // HOP
    label = md.align_length(curve.astype(np.float32), mel_len)
    crop = int(np.random.randint(0, mel_len - 192)) if mel_len > 192 else 0
    return curve, template, gain, noise, crop, label[crop:crop + 192]


def _check_world_item(item, want):
    curve, template, gain, noise, crop, label = want
    wave, f0, sil, frame_start, sr, req = item
    assert isinstance(req, md.WorldRequest) and wave.numel() == 0 and sr == FS
    np.testing.assert_array_equal(req.curve, curve)
    assert req.template == template and req.gain == gain and req.crop == crop and req.n == curve.size * HOP
    np.testing.assert_array_equal(f0.numpy(), label)
    np.testing.assert_array_equal(sil.numpy(), (label == 0).astype(np.float32))
    start, count, first = md.synthetic_window(req.n, crop, HOP, 1024)
    assert (req.out_start, req.out_len, req.frame_start, frame_start) == (start, count, first, first)
    np.testing.assert_array_equal(req.noise, noise[start:start + count].astype(np.float32))
    table = world.time_base(curve, FS, FP, N)
    np.testing.assert_array_equal(req.index, table.index)
    np.testing.assert_array_equal(req.shift, table.shift)
    assert req.seed == world.noise_seed(curve) and 0 <= req.seed < 2 ** 64


def test_world_only_items_follow_the_reference_draw_order(tmp_path):
    lines = _files(tmp_path, [1.0, 1.2])
    syn = {"enabled": True, "absolute_count": 6, "pitch_shift": {"enabled": False}, "world_vocoder": WORLD_CFG}
    ds = _ds(lines, syn)
    assert ds._synthetic_generators == ["world_vocoder"] and len(ds) == 8
    random.seed(21); np.random.seed(21)
    got = [ds[2 + i] for i in range(6)]
    random.seed(21); np.random.seed(21)
    for item in got:
        assert random.choice(["world_vocoder"]) == "world_vocoder"
        want = _restated_world_item(WORLD_CFG)
        _check_world_item(item, want)
        assert want[4] == 0 and item[-1].out_len == item[-1].n          # the default durations never crop
    assert len({it[-1].seed for it in got}) == 6


def test_long_world_items_are_cropped(tmp_path):
    lines = _files(tmp_path, [1.0])
    cfg = {**WORLD_CFG, "duration": {"min": 3, "max": 3}}
    ds = _ds(lines, {"enabled": True, "absolute_count": 4, "pitch_shift": {"enabled": False}, "world_vocoder": cfg})
    random.seed(4); np.random.seed(4)
    got = [ds[1 + i] for i in range(4)]
    random.seed(4); np.random.seed(4)
    crops = []
    for item in got:
        random.choice(["world_vocoder"])
        want = _restated_world_item(cfg)
        _check_world_item(item, want)
        assert item[1].shape[0] == 192 and item[-1].n == 240 * HOP and item[-1].out_len < item[-1].n
        crops.append(want[4])
    assert max(crops) > 0


def test_both_generators_follow_the_reference_draw_order(tmp_path):
    lines = _files(tmp_path, [1.0, 1.5, 2.0])
    paths = [ln[:-1].split("|")[0] for ln in lines]
    syn = {"enabled": True, "absolute_count": 12, "pitch_shift": PS_CFG, "world_vocoder": WORLD_CFG}
    ds = _ds(lines, syn)
    assert ds._synthetic_generators == ["pitch_shift", "world_vocoder"]
    random.seed(8); np.random.seed(8)
    got = [ds[3 + i] for i in range(12)]
    random.seed(8); np.random.seed(8)
    kinds = []
    for item in got:
        name = random.choice(["pitch_shift", "world_vocoder"])
        kinds.append(name)
        if name == "world_vocoder":
            _check_world_item(item, _restated_world_item(WORLD_CFG))
            continue
        path = random.choice(paths)                                   # every file is voiced, no semitone is 0
        s = random.choice(PS_CFG["semitones"])
        gain = 10.0 ** (random.uniform(*PS_CFG["gain_db_range"]) / 20.0)
        req = item[-1]
        assert isinstance(req, md.PitchShiftRequest)
        assert (req.path, req.n_steps, req.crop) == (path, s, 0) and req.gain == pytest.approx(gain, rel=1e-12)
    assert kinds.count("world_vocoder") >= 3 and kinds.count("pitch_shift") >= 3


def test_failed_pitch_shift_falls_back_to_world(tmp_path):
    """meldataset.py:391-394: when the pitch shift gives up, the reference draws again among the remaining
    generators."""
    lines = _files(tmp_path, [1.0])
    np.save(lines[0][:-1].split("|")[0] + "_f0.npy", np.zeros(81, np.float32))      # unvoiced: pitch shift returns None
    ds = _ds(lines, {"enabled": True, "absolute_count": 3, "pitch_shift": {**PS_CFG, "max_attempts": 2},
                     "world_vocoder": WORLD_CFG})
    random.seed(1); np.random.seed(1)
    got = [ds[1 + i] for i in range(3)]
    random.seed(1); np.random.seed(1)
    for item in got:
        if random.choice(["pitch_shift", "world_vocoder"]) == "pitch_shift":
            for _ in range(2):
                random.choice([lines[0]])
            assert random.choice(["world_vocoder"]) == "world_vocoder"
        _check_world_item(item, _restated_world_item(WORLD_CFG))


def test_gating(tmp_path):
    lines = _files(tmp_path, [1.0, 1.0, 1.0, 1.0])
    base = {"enabled": True, "ratio": 0.5, "pitch_shift": PS_CFG}
    plain = _ds(lines, {**base, "world_vocoder": {"enabled": True}})              # as today: warned about, not registered
    assert plain._synthetic_generators == ["pitch_shift"] and len(plain) == 6
    hip = _ds(lines, {**base, "world_vocoder": {"enabled": True, "backend": "hip"}})
    assert hip._synthetic_generators == ["pitch_shift", "world_vocoder"] and len(hip) == 6
    off = _ds(lines, {**base, "world_vocoder": {"enabled": False, "backend": "hip"}})
    assert off._synthetic_generators == ["pitch_shift"]
    alone = _ds(lines, {**base, "pitch_shift": {"enabled": False}, "world_vocoder": WORLD_CFG})
    assert alone._synthetic_generators == ["world_vocoder"] and len(alone) == 6
    none = _ds(lines, {**base, "pitch_shift": {"enabled": False}, "world_vocoder": {"enabled": True}})
    assert none._synthetic_generators == [] and len(none) == 4
    assert len(_ds(lines, {**base, "world_vocoder": WORLD_CFG}, validation=True)) == 4
    val = _ds(lines, {**base, "apply_to_validation": True, "world_vocoder": WORLD_CFG}, validation=True)
    assert len(val) == 6 and val._synthetic_generators == ["pitch_shift", "world_vocoder"]


def test_constructor_validation(tmp_path):
    lines = _files(tmp_path, [1.0])
    mk = lambda **kw: _ds(lines, {"enabled": True, "ratio": 1.0, "world_vocoder": {**WORLD_CFG, **kw}})  # noqa: E731
    with pytest.raises(ValueError, match="duration must be positive"):
        mk(duration={"min": 0, "max": 0})
    with pytest.raises(ValueError, match="pitch_range"):
        mk(pitch_range=[100.0])
    with pytest.raises(ValueError, match="gain_db_range"):
        mk(gain_db_range=[-1.0, -2.0, -3.0])
    with pytest.raises(ValueError, match="vowel templates"):
        mk(vowel_profiles=[{"label": "x", "formants": []}])
    with pytest.raises(ValueError, match="fft_size"):
        md.MelDataset(lines, mel_params={**MEL, "n_fft": 4096, "win_len": 4096}, verbose=False,
                      synthetic_data={"enabled": True, "ratio": 1.0, "world_vocoder": WORLD_CFG})
    gen = world.WorldGenerator(FS, HOP, None, {"gain_db_range": -3.0, "noise_db": None, "duration": {"min": 2, "max": 1}})
    assert gen.fft_size == 1024 and gen.gain_db_range == (-3.0, -3.0)
    random.seed(0); np.random.seed(0)
    state = np.random.get_state()[1].copy()
    d = gen.draw()
    assert d.noise is None and d.curve.size == 80 and d.gain == pytest.approx(10 ** (-3 / 20))
    np.testing.assert_array_equal(np.random.get_state()[1], state)        # no noise: np.random untouched


def test_collater_packs_world_rows(tmp_path):
    lines = _files(tmp_path, [2.0, 1.0])
    ds = _ds(lines, {"enabled": True, "absolute_count": 4, "pitch_shift": PS_CFG, "world_vocoder": WORLD_CFG})
    random.seed(8); np.random.seed(8)
    items = [ds[2 + i] for i in range(4)]
    kinds = [type(it[-1]) for it in items]
    assert md.WorldRequest in kinds and md.PitchShiftRequest in kinds
    batch = [ds[0]] + items
    out = md.Collater()(batch)
    waves, lengths, crops = out[0], out[1], out[2]
    assert isinstance(out[-1], md.WorldBatch) and isinstance(out[-2], md.PitchShiftBatch) and len(out) == 8
    pack = out[-1]
    rows = [i for i, it in enumerate(batch) if isinstance(it[-1], md.WorldRequest)]
    assert pack.rows.tolist() == rows
    for k, r in enumerate(rows):
        req = batch[r][-1]
        assert int(lengths[r]) == req.out_len and int(crops[r]) == req.frame_start and (waves[r] == 0).all()
        assert pack.templates[k] == req.template and pack.out_start[k] == req.out_start
        assert float(pack.gains[k]) == np.float32(req.gain) and pack.seeds[k] == req.seed
        np.testing.assert_array_equal(pack.tables[k][0], req.index)
    assert pack.noise.numel() == sum(batch[r][-1].out_len for r in rows)
    # a batch without WORLD rows is the tuple it was
    plain = md.Collater()([ds[0], ds[1]])
    assert len(plain) == 6 and not any(isinstance(t, (md.WorldBatch, md.PitchShiftBatch)) for t in plain)
    only_ps = md.Collater()([ds[0]] + [it for it in items if isinstance(it[-1], md.PitchShiftRequest)])
    assert isinstance(only_ps[-1], md.PitchShiftBatch) and len(only_ps) == 7


# --------------------------------------------------------------------------- C ABI, host side only
@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _lib.load()


def test_plan_keeps_only_the_pulses_a_window_needs(lib):
    f0 = ref.rows()["glide_vib"][0]
    table = world.time_base(f0, FS, FP, N)
    full = world.Plan([f0.size], [table], [0], [0], fs=FS, frame_period_ms=FP, fft_size=N, f0s=[f0])
    assert full.meta.shape == (1, lib.pe_world_plan_fields())
    assert full.n_pulses == table.index.size == 109 and full.n_out == f0.size * HOP
    np.testing.assert_array_equal(full.pulses[:, 0], table.index)
    np.testing.assert_array_equal(full.pulses[:, 3], table.noise_size)
    pos = (table.index / FS) / (FP / 1000.0)
    np.testing.assert_array_equal(full.pulses[:, 1], np.minimum(f0.size - 1, np.floor(pos)))
    np.testing.assert_array_equal(full.pulses[:, 2], np.minimum(f0.size - 1, np.ceil(pos)))
    np.testing.assert_array_equal(full.pulse_f[:, 0], pos - np.floor(pos))
    np.testing.assert_array_equal(full.pulse_f[:, 1], table.shift * FS)
    win = world.Plan([f0.size, f0.size], [table, table], [0, 513], [0, 513], out_start=[6000, 0], out_len=[1000, 0],
                     out_rows=[3, 1], out_stride=2000, fs=FS, frame_period_ms=FP, fft_size=N)
    keep = (table.index >= 6000 - 512) & (table.index <= 6999 + 511)
    assert win.n_pulses == keep.sum() < 109 and win.n_out == 1000
    np.testing.assert_array_equal(win.pulses[:win.n_pulses, 0], table.index[keep])
    np.testing.assert_array_equal(win.pulses[:win.n_pulses, 3], table.noise_size[keep])   # from the whole row's table


def test_plan_and_entry_point_argument_checks(lib):
    Lg = lambda *v: (ctypes.c_long * len(v))(*v)  # noqa: E731
    D = lambda *v: (ctypes.c_double * len(v))(*v)  # noqa: E731
    meta, pulses, pf, tot = (ctypes.c_long * 64)(), (ctypes.c_long * 64)(), (ctypes.c_double * 16)(), Lg(0, 0)

    def plan(frames=4, f0=(100.0,) * 4, index=(100, 400), shift=(0.0, 1.0 / FS), j_lo=0, j_cnt=1200, stride=1200,
             fft=1024, sp_stride=0, fs=float(FS), fpm=FP):
        voiced = (ctypes.c_ubyte * len(index))(*([1] * len(index)))
        return lib.pe_world_plan(1, Lg(frames), D(*f0), Lg(len(index)), Lg(*index), D(*shift), voiced, Lg(0),
                                 Lg(sp_stride), None, None, None, None, Lg(j_lo), Lg(j_cnt), Lg(0), stride, fs, fpm,
                                 fft, meta, pulses, pf, tot)
    assert plan() == 0 and tot[0] == 2 and tot[1] == 1200
    assert plan(fft=4096) == -2 and plan(fft=256) == -2 and plan(fft=1000) == -1 and plan(fft=0) == -1
    assert plan(frames=0) == -1                                     # no frames
    assert plan(j_lo=1, j_cnt=1200) == -1 and plan(j_lo=-1) == -1  # window outside the row
    assert plan(stride=1199) == -1                                  # output stride shorter than the window
    assert plan(f0=(100.0, float("inf"), 100.0, 100.0)) == -1 and plan(f0=(100.0, float("nan"), 1.0, 1.0)) == -1
    assert plan(index=(400, 400)) == -1 and plan(index=(400, 100)) == -1     # not strictly increasing
    assert plan(index=(100, 1200)) == -1 and plan(index=(-1, 100)) == -1     # outside the row
    assert plan(index=(10, 1100)) == -1                              # a noise segment longer than the transform
    assert plan(shift=(0.0, 1.01 / FS)) == -1 and plan(shift=(-1e-9, 0.0)) == -1 and plan(shift=(float("nan"), 0.0)) == -1
    assert plan(sp_stride=512) == -1 and plan(sp_stride=-1) == -1
    assert plan(fs=0.0) == -1 and plan(fpm=float("nan")) == -1
    assert lib.pe_world_plan(1, None, None, None, None, None, None, None, None, None, None, None, None, None, None,
                             None, 0, float(FS), FP, 1024, None, None, None, tot) == -1
    assert lib.pe_world_plan(0, None, None, None, None, None, None, None, None, None, None, None, None, None, None,
                             None, 0, float(FS), FP, 1024, None, None, None, None) == -1
    p = ctypes.c_void_p(1)
    assert lib.pe_world_responses(p, None, None, p, p, p, p, -1, 1, 1024, p, None) == -1
    assert lib.pe_world_responses(p, None, None, p, p, p, p, 1, -1, 1024, p, None) == -1
    assert lib.pe_world_responses(p, None, None, p, p, p, p, 1, 1, 4096, p, None) == -2
    assert lib.pe_world_responses(None, None, None, p, p, p, p, 1, 1, 1024, p, None) == -1
    assert lib.pe_world_responses(p, None, None, p, p, p, None, 1, 1, 1024, p, None) == -1
    assert lib.pe_world_responses(p, None, None, p, p, p, p, 1, 0, 1024, p, None) == 0      # nothing to do
    assert lib.pe_world_overlap_add(p, p, p, p, None, 1, -1, 1024, p, None) == -1
    assert lib.pe_world_overlap_add(p, p, p, p, None, -1, 1, 1024, p, None) == -1
    assert lib.pe_world_overlap_add(p, p, p, p, None, 1, 1, 100, p, None) == -2
    assert lib.pe_world_overlap_add(p, None, p, p, None, 1, 1, 1024, p, None) == -1
    assert lib.pe_world_overlap_add(p, p, p, None, None, 1, 1, 1024, None, None) == -1


def test_host_tensors_are_refused():
    import torch
    sp = torch.ones(513)
    with pytest.raises(RuntimeError, match="no CPU path"):
        world.world_synthesize(np.full(4, 100.0), sp, None, FS, FP)
    with pytest.raises(ValueError, match="fft_size"):
        world.check_fft_size(4096)
