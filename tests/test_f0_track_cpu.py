"""The F0 tracker without a device: the float64 restatement (tests/f0_track_ref.py) against the analytic F0 of synthetic
signals, its transition costs on hand-built candidate tables, the float32 yardstick the GPU test uses, every refusal of
the C ABI and of the Python layer, and the dataset's label pre-pass with a stub tracker.

Accuracy of the restatement against the analytic curve at the frame centre (24 kHz, hop 300, reference defaults;
records of the run that wrote this file, not gates -- the gate is 50 cents on every frame whose window lies inside a
voiced stretch):
    steady sines 50..1000 Hz          rms 0.27   max 3.51 cents
    three-partial tones 60..700 Hz    rms 0.01   max 0.03 cents
    linear glides                     rms 0.20   max 2.95 cents
    vibrato (5.5 Hz, +-60 cents)      rms 2.77   max 3.95 cents
    weak fundamental (150 Hz)         rms 0.00   max 0.00 cents
    voiced - gap - voiced             rms 2.77   max 3.94 cents
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from pitchextractor_amd import _lib, build, synthetic
from pitchextractor_amd.meldataset import MelDataset, f0_cache_identifier
from tests import f0_track_ref as R

SR, HOP = 24000, 300


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _lib.load()


# --------------------------------------------------------------------------- accuracy of the restatement
def _score(tag, y, curve, sr=SR, hop=HOP, **config):
    """Frames whose window lies inside a voiced stretch: voiced and within 50 cents of the curve at the centre;
    frames whose window lies inside an unvoiced stretch: unvoiced; frames across an edge: free (the contour's edge
    therefore falls within one window length of the true edge).  Returns (rms, max) cents."""
    res = R.track(y, sr, hop, **config)
    c = res["consts"]
    left, _ = R.frame_left_samples(len(res["f0"]), res["times"][0] if len(res["f0"]) else 0.0, c)
    voiced = np.asarray(curve) > 0
    cum = np.concatenate([[0], np.cumsum(voiced)])
    start = left + 1 - c.hw
    inside = cum[start + c.nw] - cum[start]
    all_v, all_u = inside == c.nw, inside == 0
    f0 = res["f0"].astype(np.float64)
    assert np.all(f0[all_v] > 0), f"{tag}: unvoiced frame inside a voiced stretch"
    assert not np.any(f0[all_u] > 0), f"{tag}: voiced frame inside an unvoiced stretch"
    if not all_v.any():
        return 0.0, 0.0
    truth = 0.5 * (np.asarray(curve, np.float64)[left[all_v]] + np.asarray(curve, np.float64)[left[all_v] + 1])
    ce = R.cents(f0[all_v], truth)
    assert ce.max() <= 50.0, f"{tag}: {ce.max():.1f} cents"
    return float(np.sqrt(np.mean(ce ** 2))), float(ce.max())


def _report(name, scores):
    rms = np.sqrt(np.mean([s[0] ** 2 for s in scores]))
    print(f"[f0_track accuracy] {name}: rms {rms:.2f} max {max(s[1] for s in scores):.2f} cents")


def test_steady_sines_and_tones():
    n = SR
    scores = []
    for hz in (50.0, 110.0, 220.0, 440.0, 880.0, 1000.0):
        curve = np.full(n, hz)
        scores.append(_score(f"sine {hz}", synthetic.sine_from_f0(curve, SR), curve))
    _report("steady sines", scores)
    scores = []
    for hz in (60.0, 150.0, 333.0, 700.0):
        curve = np.full(n, hz)
        scores.append(_score(f"tone {hz}", R.harmonic(curve, SR), curve))
    _report("three-partial tones", scores)


def test_glides_and_vibrato():
    scores = []
    for a, b in ((80.0, 380.0), (300.0, 120.0), (200.0, 800.0)):
        y, _, curve = synthetic.glide(2.0, a, b, SR)
        scores.append(_score(f"sine glide {a}-{b}", y, curve))
        y, curve = R.glide_signal(2.0, a, b, SR)
        scores.append(_score(f"harmonic glide {a}-{b}", y, curve))
    _report("linear glides", scores)
    y, curve = R.vibrato_signal(3.0, 180.0, SR, gaps=())
    _report("vibrato", [_score("vibrato", y, curve)])


def test_weak_fundamental_is_still_chosen():
    curve = np.full(SR, 150.0)
    y = R.harmonic(curve, SR, partials=(0.3, 1.0, 0.2))
    _report("weak fundamental", [_score("weak fundamental", y, curve)])


def test_silence_noise_and_gaps():
    res = R.track(np.zeros(SR, np.float32), SR, HOP)
    assert res["f0"].shape == (R.frame_layout(SR, res["consts"])[0],) and not np.any(res["f0"] > 0)
    assert np.all(res["cand_n"] == 1)
    # loud tone, then white noise 60 dB down: unvoiced through the silence threshold
    rng = np.random.default_rng(3)
    curve = np.concatenate([np.full(SR, 200.0), np.zeros(SR)])
    y = np.concatenate([R.harmonic(curve[:SR], SR), (5e-4 * rng.standard_normal(SR)).astype(np.float32)])
    _score("tone then noise", y, curve)
    y, curve = R.vibrato_signal(3.0, 140.0, SR, seed=7, gaps=((0.35, 0.5),))
    _report("voiced - gap - voiced", [_score("gap", y, curve)])
    # the zeroed gap of the benchmark utterances is digital silence inside a voiced file
    for i in range(3):
        audio, f0, _ = synthetic.utterance(i)
        res = R.track(audio, SR, HOP)
        assert np.isfinite(res["cand_s"]).all() and res["silent"].any()
        assert not np.any(res["f0"][res["silent"]] > 0)


# --------------------------------------------------------------------------- frame layout
def test_frame_counts_and_times(lib):
    from pitchextractor_amd.f0_tracker import PraatACTracker
    for sr, hop, mp in ((24000, 300, 40.0), (16000, 160, 75.0), (48000, 480, 40.0), (22050, 256, 60.0)):
        tr = PraatACTracker(sr, hop, min_pitch=mp)
        c = R.Consts(sr, hop, min_pitch=mp)
        assert (tr.nsamp_window, tr.nsamp_period, tr.n_fft, tr.max_lag, tr.half_window, tr.half_period) == \
               (c.nw, c.nper, c.nfft, c.maxlag, c.hw, c.hper)
        assert tr.ceiling == c.ceiling and tr.time_step == c.dt
        win = int(np.ceil(3.0 * sr / mp))
        lengths = [0, 1, win - hop, win - 2, win - 1, win, win + 1, win + hop - 1, win + hop, win + hop + 1,
                   2 * sr, 4 * sr, 30 * sr + 7]
        for n in lengths:
            nf, t1 = R.frame_layout(n, c)
            assert tr.frame_count(n) == nf, (sr, n)
            if nf:
                times = tr.frame_times(n)
                assert times[0] == t1 and times.shape == (nf,)
                left, _ = R.frame_left_samples(nf, t1, c)
                assert left[0] + 1 - c.hw >= 0 and left[-1] + 1 - c.hw + c.nw <= n   # every window inside the file
        assert tr.frame_count(win - 2) == 0                          # shorter than one window: no frame
    c = R.Consts(24000, 300)
    # 4 s at hop 300 / 24 kHz: 314 frames in float64 in the stated order (315 in exact arithmetic)
    assert R.frame_layout(96000, c)[0] == 314 and PraatACTracker(24000, 300).frame_count(96000) == 314
    assert R.frame_layout(1800, c) == (1, 0.0375)
    assert (c.nw, c.nper, c.nfft, c.maxlag) == (1798, 600, 4096, 601)
    plan = PraatACTracker(24000, 300).plan([96000, 100, 48000, 0, 1800])
    assert plan["frames"].tolist() == [314, 0, 155, 0, 1] and plan["frame_offsets"].tolist() == [0, 314, 314, 469, 469]
    assert plan["n_frames"] == 470 and plan["workspace_bytes"] == 0


# --------------------------------------------------------------------------- transition costs
def _table(frames):
    T = len(frames)
    f, s, n = np.zeros((T, R.N_CAND)), np.zeros((T, R.N_CAND)), np.zeros(T, np.int32)
    for t, cands in enumerate(frames):
        n[t] = len(cands)
        for j, (hz, strength) in enumerate(cands):
            f[t, j], s[t, j] = hz, strength
    return f, s, n


def test_octave_jump_cost_decides_the_path():
    # frame 1 prefers the octave (strength 0.95 against 0.90); the neighbours know only 100 Hz
    frames = [[(0, 0.45), (100.0, 0.9)], [(0, 0.45), (100.0, 0.90), (200.0, 0.95)], [(0, 0.45), (100.0, 0.9)]]
    f, s, n = _table(frames)
    kw = dict(octave_cost=0.0, voiced_unvoiced_cost=0.3)
    _, f0 = R.viterbi(f, s, n, R.Consts(SR, HOP, octave_jump_cost=1.0, **kw))
    assert f0.tolist() == [100.0, 100.0, 100.0]                     # the jump is refused at cost 1.0
    _, f0 = R.viterbi(f, s, n, R.Consts(SR, HOP, octave_jump_cost=0.0, **kw))
    assert f0.tolist() == [100.0, 200.0, 100.0]                     # and taken at 0


def test_voicing_change_is_delayed_by_its_cost():
    c0 = 0.01 / (HOP / SR)                                           # 0.8 at the shipped hop
    # one frame whose voiced candidate beats the unvoiced one by 0.5 inside an unvoiced stretch: two voicing changes
    # cost 2 * 0.3 * c = 0.48 < 0.5 -> taken; with cost 0.4 (0.64) it is not
    frames = [[(0, 0.6)], [(0, 0.6)], [(0, 0.45), (150.0, 0.95)], [(0, 0.6)], [(0, 0.6)]]
    f, s, n = _table(frames)
    _, f0 = R.viterbi(f, s, n, R.Consts(SR, HOP, octave_cost=0.0, voiced_unvoiced_cost=0.3))
    assert f0.tolist() == [0, 0, 150.0, 0, 0] and 2 * 0.3 * c0 < 0.5
    _, f0 = R.viterbi(f, s, n, R.Consts(SR, HOP, octave_cost=0.0, voiced_unvoiced_cost=0.4))
    assert not np.any(f0 > 0)
    # an onset: the first voiced frame is weak (gain 0.1 < one change 0.24), so the path stays unvoiced one frame longer
    frames = [[(0, 0.6)], [(0, 0.5), (150.0, 0.6)], [(0, 0.45), (150.0, 0.95)], [(0, 0.45), (150.0, 0.95)]]
    f, s, n = _table(frames)
    path, f0, margin = R.viterbi(f, s, n, R.Consts(SR, HOP, octave_cost=0.0), return_margin=True)
    assert f0.tolist() == [0, 150.0, 150.0, 150.0] and margin > 0    # the change costs the same wherever it happens
    _, f0 = R.viterbi(f, s, n, R.Consts(SR, HOP, octave_cost=0.0, voiced_unvoiced_cost=0.0))
    assert f0.tolist() == [0, 150.0, 150.0, 150.0]
    # candidates at or above the ceiling count as unvoiced and ties go to the lowest index
    frames = [[(0, 0.5), (5000.0, 0.5)], [(0, 0.5), (5000.0, 0.5)]]
    path, f0 = R.viterbi(*_table(frames), R.Consts(SR, HOP))
    assert path.tolist() == [0, 0] and not np.any(f0 > 0)


# --------------------------------------------------------------------------- the float32 yardstick
def test_float32_restatement_keeps_every_margin_path():
    """Per configuration of the GPU tests: the yardstick (printed; the kernel gets 4x), every margin input qualifies
    under (a)-(c), and the float32 run keeps every path on them and stays inside 1 % on the natural inputs."""
    for cfg in R.GPU_CONFIGS + [R.SPILL_CONFIG]:
        yard = R.config_yardstick(*cfg)
        print(f"[f0_track yardstick] {cfg}: float32 vs float64 restatement {yard['cents']:.3e} cents, strength "
              f"{yard['strength']:.3e} on the margin inputs, contour {yard['natural_cents']:.3e} cents on the natural ones")
        assert 0 < yard["strength"] < 1e-5 and 0 < yard["cents"] < 0.5 and 0 < yard["natural_cents"] < 0.5
        for a, b in R.reference_pairs(*cfg):
            bound = 1000.0 * yard["strength"]
            assert R.is_margin_input(a, yard["strength"]), (cfg, a["margin"], a["thr_gap"], a["gap15"])
            assert a["margin"] >= 10 * bound, (cfg, a["margin"])         # room: no input sits at the edge of (a)
            d = R.deviation(a, b)
            assert d["voicing_flips"] == 0 and d["set_mismatches"] == 0, (cfg, d)
            assert np.array_equal(a["f0"] > 0, b["f0"] > 0)
        sr, hop, mp, _ = cfg
        for a, b in R.natural_pairs(sr, hop, mp):
            d = R.deviation(a, b)
            assert d["voicing_flips"] <= 0.01 * d["frames"] and d["set_mismatches"] <= 0.01 * d["frames"], (cfg, d)


# --------------------------------------------------------------------------- ABI refusals, no device present
def test_track_argument_checks_run_before_any_device_call(lib):
    ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
    K = lib.pe_f0_track_plan_fields()
    good = np.array([40.0, 1100.0, 0.03, 0.45, 0.01, 1.0, 0.3])
    n, off = np.array([96000, 0], np.int64), np.array([0, 96000], np.int64)
    consts, dconsts, totals = np.zeros(8, np.int64), np.zeros(2), np.zeros(2, np.int64)
    meta, t1 = np.zeros((2, K), np.int64), np.zeros(2)
    p = lambda a: a.ctypes.data  # noqa: E731

    def plan(sr=24000, hop=300, cfg=good, rows=2, **null):
        cfg = np.ascontiguousarray(cfg, dtype=np.float64)             # stays alive across the call
        a = dict(n=p(n), off=p(off), config=p(cfg), consts=p(consts), dconsts=p(dconsts), meta=p(meta), t1=p(t1),
                 totals=p(totals))
        a.update({k: None for k in null})
        return lib.pe_f0_track_plan(rows, a["n"], a["off"], sr, hop, a["config"], a["consts"], a["dconsts"], a["meta"],
                                    a["t1"], a["totals"])

    assert plan() == 0 and meta[0, 2] == 314 and meta[1, 2] == 0
    for name in ("n", "off", "cfg", "consts", "dconsts", "meta", "t1", "totals"):
        assert plan(**{name: True}) == ARG, name
    assert plan(hop=0) == ARG and plan(hop=-3) == ARG and plan(sr=0) == ARG and plan(rows=-1) == ARG

    def cfg(**kw):
        keys = ["min_pitch", "max_pitch", "silence", "voicing", "octave", "jump", "vuv"]
        out = good.copy()
        for k, v in kw.items():
            out[keys.index(k)] = v
        return out

    assert plan(cfg=cfg(min_pitch=1100.0)) == ARG and plan(cfg=cfg(min_pitch=2000.0)) == ARG
    assert plan(cfg=cfg(min_pitch=0.0)) == ARG and plan(cfg=cfg(max_pitch=float("nan"))) == ARG
    assert plan(cfg=cfg(silence=0.0)) == ARG and plan(cfg=cfg(voicing=-0.1)) == ARG and plan(cfg=cfg(jump=-1.0)) == ARG
    assert plan(sr=16000, cfg=cfg(min_pitch=8000.0, max_pitch=9000.0)) == ARG      # above sr / 2 after the cut
    # FFT lengths 1024 .. 8192 only
    assert plan(sr=48000, cfg=cfg(min_pitch=30.0)) == 0 and consts[2] == 8192
    assert plan(sr=48000, cfg=cfg(min_pitch=20.0)) == UNSUPPORTED     # 7198-sample window: 16384 points
    assert plan(sr=8000, cfg=cfg(min_pitch=75.0)) == UNSUPPORTED
    assert plan(sr=16000, cfg=cfg(min_pitch=75.0)) == 0 and consts[2] == 1024
    assert plan(sr=16000, cfg=cfg(min_pitch=20.0)) == 0 and consts[2] == 4096

    # launch entry points: a real plan, fake (never dereferenced) device pointers
    assert plan() == 0
    buf = (ctypes.c_float * 64)()
    d = ctypes.cast(buf, ctypes.c_void_p)
    ntab = int(consts[6])
    gc = p(good)
    sws, K = lib.pe_row_stats_workspace_bytes(2), lib.pe_f0_track_plan_fields()
    assert sws == 2 * 64 * 12 and lib.pe_row_stats_workspace_bytes(0) == 0
    assert lib.pe_row_stats(None, d, K, 2, d, d, sws, None) == ARG
    assert lib.pe_row_stats(d, None, K, 2, d, d, sws, None) == ARG
    assert lib.pe_row_stats(d, d, K, 2, None, d, sws, None) == ARG
    assert lib.pe_row_stats(d, d, K, -1, d, d, sws, None) == ARG
    assert lib.pe_row_stats(d, d, 1, 2, d, d, sws, None) == ARG            # a plan row holds at least offset and length
    assert lib.pe_row_stats(d, d, K, 2, d, None, sws, None) == WORKSPACE
    assert lib.pe_row_stats(d, d, K, 2, d, d, sws - 1, None) == WORKSPACE
    assert lib.pe_row_stats(None, None, K, 0, None, None, 0, None) == 0

    def frames(x=d, m=d, hm=p(meta), t=d, st=d, tab=d, nt=ntab, rows=2, sr=24000, hop=300, c=gc, cf=d, cs=d, cn=d):
        return lib.pe_f0_track_frames(x, m, hm, t, st, tab, nt, rows, sr, hop, c, cf, cs, cn, None)

    for name in ("x", "m", "hm", "t", "st", "tab", "c", "cf", "cs", "cn"):
        assert frames(**{name: None}) == ARG, name
    assert frames(nt=ntab - 1) == ARG and frames(rows=-1) == ARG and frames(hop=0) == ARG
    low = cfg(min_pitch=75.0)
    assert frames(sr=8000, c=p(low)) == UNSUPPORTED
    bad = meta.copy()
    bad[1, 3] = 7                                                    # frame offsets that are not the prefix sums
    assert frames(hm=p(bad)) == ARG
    assert frames(rows=0, x=None, m=None, hm=None) == 0

    def path(cf=d, cs=d, cn=d, m=d, hm=p(meta), rows=2, sr=24000, hop=300, c=gc, f0=d, ws=None, nb=0):
        return lib.pe_f0_track_path(cf, cs, cn, m, hm, rows, sr, hop, c, f0, ws, nb, None)

    for name in ("cf", "cs", "cn", "m", "hm", "c", "f0"):
        assert path(**{name: None}) == ARG, name
    zero = cfg(min_pitch=0.0)
    assert path(rows=-1) == ARG and path(hop=0) == ARG and path(c=p(zero)) == ARG
    n[0] = 24000 * 60                                                # 4794 frames: back-pointers leave LDS
    assert plan() == 0 and totals[1] == 16 * meta[0, 2] and meta[0, 2] > consts[7] and meta[0, 4] == 0
    assert path(ws=None, nb=0) == WORKSPACE and path(ws=d, nb=int(totals[1]) - 1) == WORKSPACE


def test_python_layer_refusals(lib, caplog):
    from pitchextractor_amd.f0_tracker import PraatACTracker, check_config
    tr = PraatACTracker(SR, HOP, method="autocorrelation", max_pitch=800)
    assert tr.config["max_pitch"] == 800.0 and tr.cache_key == "praat"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.track(torch.zeros(SR))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.track(np.zeros(SR, np.float32))
    for bad in (dict(method="cc"), dict(method="cross-correlation"), dict(method="shs"), dict(very_accurate=True),
                dict(very_accurate="yes"), dict(unit="semitones")):
        with pytest.raises(NotImplementedError):
            PraatACTracker(SR, HOP, **bad)
    # a key the reference's backend does not read either is ignored with a warning, as there
    with caplog.at_level("WARNING"):
        assert PraatACTracker(SR, HOP, comment="tuned for speech").config == PraatACTracker(SR, HOP).config
    assert any("comment" in r.getMessage() for r in caplog.records)
    with pytest.raises(NotImplementedError):
        check_config({}, require_method=True)                        # a dataset entry must name its method
    with pytest.raises(_lib.HipLibraryError):
        PraatACTracker(8000, 100, min_pitch=75.0)                     # FFT length below 1024
    with pytest.raises(_lib.HipLibraryError):
        PraatACTracker(SR, HOP, min_pitch=500.0, max_pitch=400.0)


# --------------------------------------------------------------------------- dataset pre-pass with a stub tracker
def _write_wav(path, y, sr):
    import struct
    data = (np.clip(y, -1, 1) * 32767).astype("<i2").tobytes()
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " +
                 struct.pack("<IHHIIHH", 16, 1, 1, sr, 2 * sr, 2, 16) + b"data" + struct.pack("<I", len(data)) + data)


class StubTracker:
    calls = []

    def __init__(self, sr, hop, **config):
        self.sr, self.hop, self.config = sr, hop, config

    def track(self, waves, lengths=None):
        StubTracker.calls.append(list(lengths))
        return [np.full(max(n // self.hop - 5, 0), 100.0 + i, np.float32) if n >= self.sr // 2
                else np.zeros(3, np.float32) for i, n in enumerate(lengths)]


PRAAT = {"backend_order": ["swiftf0", "praat"],
         "backends": {"swiftf0": {"type": "swiftf0", "enabled": True},
                      "praat": {"type": "praat", "enabled": True, "config": {"method": "ac", "min_pitch": 40.0}}}}


def _folder(tmp_path, count=5, seconds=1.0):
    paths = []
    for i in range(count):
        p = str(tmp_path / f"utt{i}.wav")
        _write_wav(p, 0.3 * np.sin(2 * np.pi * 120 * np.arange(int(seconds * SR)) / SR), SR)
        paths.append(p)
    return paths


def _dataset(paths, f0_params=PRAAT, **kw):
    return MelDataset([p + "|0\n" for p in paths], f0_params=f0_params, verbose=False, **kw)


def test_prepass_writes_the_reference_cache_format(tmp_path, caplog):
    paths = _folder(tmp_path)
    _write_wav(paths[4], np.zeros(SR // 4), SR)                      # too short to be voiced: every backend fails
    ds = _dataset(paths)
    assert ds.has_native_f0 and ds.f0_cache_identifier == "-swiftf0_praat" == f0_cache_identifier(PRAAT)
    # an existing valid cache and a legacy cache are used as they are
    keep = np.arange(7, dtype=np.float32)
    np.save(paths[0] + "_f0-swiftf0_praat.npy", keep)
    meta_text = json.dumps({"cache_identifier": "-swiftf0_praat", "backend": "swiftf0", "sample_rate": SR,
                            "hop_length": HOP}, sort_keys=True)
    with open(paths[0] + "_f0-swiftf0_praat.json", "w") as fh:
        fh.write(meta_text)
    np.save(paths[1] + "_f0.npy", keep)
    before = {p: os.stat(p).st_mtime_ns for p in (paths[0] + "_f0-swiftf0_praat.npy", paths[1] + "_f0.npy")}
    StubTracker.calls = []
    with caplog.at_level("WARNING"):
        done = ds.prepare_f0_caches("cpu", files_per_batch=2, tracker_factory=StubTracker)
    assert done == paths[2:] and StubTracker.calls == [[SR, SR], [SR // 4]]
    assert sum("swiftf0" in r.getMessage() and "not part of this build" in r.getMessage()
               for r in caplog.records) == 1
    assert {p: os.stat(p).st_mtime_ns for p in before} == before
    assert np.array_equal(np.load(paths[0] + "_f0-swiftf0_praat.npy"), keep)
    for k, p in enumerate(paths[2:4]):
        arr = np.load(p + "_f0-swiftf0_praat.npy")
        assert arr.dtype == np.float32 and np.array_equal(arr, np.full(SR // HOP - 5, 100.0 + k, np.float32))
        with open(p + "_f0-swiftf0_praat.json") as fh:
            text = fh.read()
        # meldataset.py:606-619: json.dump of these four keys with sort_keys=True
        assert text == ('{"backend": "praat", "cache_identifier": "-swiftf0_praat", "hop_length": 300, '
                        '"sample_rate": 24000}')
        assert np.array_equal(ds._load_cached_f0(p), arr)            # accepted by the existing loader
    # all native entries failed: the empty array, backend ""
    assert np.load(paths[4] + "_f0-swiftf0_praat.npy").shape == (0,)
    with open(paths[4] + "_f0-swiftf0_praat.json") as fh:
        assert json.load(fh)["backend"] == ""
    assert not [f for f in os.listdir(tmp_path) if ".tmp" in f]
    # second pass: nothing left to do, no tracker is even built
    StubTracker.calls = []
    assert ds.prepare_f0_caches("cpu", tracker_factory=StubTracker) == [] and StubTracker.calls == []
    # items now load through the ordinary path
    wave, f0, sil, crop = ds.path_to_wave_and_label(paths[2])
    assert f0.shape == (1 + SR // HOP,) and np.all(f0 == 100.0)


def test_prepass_never_overwrites_and_is_atomic(tmp_path, monkeypatch, caplog):
    paths = _folder(tmp_path, 3)
    ds = _dataset(paths)
    # a cache computed for another hop sits under the expected name: skipped with the existing warning, not replaced
    np.save(paths[0] + "_f0-swiftf0_praat.npy", np.ones(4, np.float32))
    with open(paths[0] + "_f0-swiftf0_praat.json", "w") as fh:
        json.dump({"cache_identifier": "-swiftf0_praat", "sample_rate": SR, "hop_length": 256}, fh)
    with caplog.at_level("WARNING"):
        assert ds.files_to_label() == paths[1:]
    assert sum("is in the way" in r.getMessage() for r in caplog.records) == 1
    # a failure between the two files leaves neither under its final name
    real = os.replace
    state = {"n": 0}

    def failing(src, dst):
        state["n"] += 1
        if state["n"] == 2:
            raise KeyboardInterrupt("interrupted between the two files")
        return real(src, dst)

    monkeypatch.setattr(os, "replace", failing)
    with pytest.raises(KeyboardInterrupt):
        ds.prepare_f0_caches("cpu", tracker_factory=StubTracker)
    monkeypatch.setattr(os, "replace", real)
    left = sorted(f for f in os.listdir(tmp_path) if "_f0" in f)
    assert left == ["utt0.wav_f0-swiftf0_praat.json", "utt0.wav_f0-swiftf0_praat.npy"]
    assert np.array_equal(np.load(paths[0] + "_f0-swiftf0_praat.npy"), np.ones(4, np.float32))
    assert ds.prepare_f0_caches("cpu", tracker_factory=StubTracker) == paths[1:]


def test_prepass_rank_sharding_and_refusals(tmp_path):
    paths = _folder(tmp_path, 5)
    ds = _dataset(paths + paths[:2])                                 # duplicates in the list are labelled once
    assert ds.files_to_label(0, 2) == paths[0::2] and ds.files_to_label(1, 2) == paths[1::2]
    assert ds.prepare_f0_caches("cpu", rank=1, world=2, tracker_factory=StubTracker) == paths[1::2]
    assert ds.files_to_label(0, 1) == paths[0::2]
    # no native entry: as before -- no pre-pass, and an item without labels fails loudly
    plain = _dataset(paths[:1], f0_params={"backends": {"swiftf0": {"type": "swiftf0"}}})
    assert not plain.has_native_f0
    with pytest.raises(RuntimeError, match="enables no praat"):
        plain.prepare_f0_caches("cpu", tracker_factory=StubTracker)
    with pytest.raises(RuntimeError, match="no F0 labels"):
        plain.path_to_wave_and_label(paths[0])
    assert not _dataset(paths[:1], f0_params={}).has_native_f0
    disabled = {"backends": {"praat": {"type": "praat", "enabled": False, "config": {"method": "cc"}}}}
    assert not _dataset(paths[:1], f0_params=disabled).has_native_f0
    # what is not built is refused when the dataset is built
    for config in ({"method": "cc"}, {}, {"method": "ac", "very_accurate": True}, {"method": "ac", "unit": "mel"}):
        with pytest.raises(NotImplementedError):
            _dataset(paths[:1], f0_params={"backends": {"parselmouth": {"type": "parselmouth", "config": config}}})
