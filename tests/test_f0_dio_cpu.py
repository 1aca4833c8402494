"""The DIO + StoneMask restatement (tests/dio_ref.py) and the host side of the HIP tracker (no GPU needed).

The restatement is held to the analytic F0 of synthetic signals (50 cents, the project's bar for its trackers and the
raw-pitch-accuracy threshold); its float32 run defines the yardstick of every GPU test configuration, and the margin
inputs of each configuration are shown to be margin inputs.  Every figure is printed before it is asserted."""
import ctypes
import logging

import numpy as np
import pytest

from tests import dio_ref as D
from tests import f0_track_ref as S

SR, HOP = 24000, 300


def _interior(truth_voiced, vrm):
    """Frames further than ``vrm`` frames from a voicing boundary of the analytic curve (the ends count as one)."""
    v = np.asarray(truth_voiced, bool)
    change = np.nonzero(v[1:] != v[:-1])[0]
    edges = np.concatenate([[-1], change, change + 1, [v.size]])
    dist = np.min(np.abs(np.arange(v.size)[:, None] - edges[None, :]), axis=1)
    return dist > vrm


@pytest.mark.parametrize("name,signal", [("glide 80-380", lambda: S.glide_signal(2.0, 80.0, 380.0, SR)),
                                         ("glide 300-120", lambda: S.glide_signal(2.0, 300.0, 120.0, SR, seed=1)),
                                         ("vibrato 140", lambda: S.vibrato_signal(3.0, 140.0, SR))])
def test_restatement_tracks_the_analytic_curve(name, signal):
    y, curve = signal()
    res = D.track(y, SR, HOP)
    c = res["consts"]
    at = np.minimum(np.arange(res["f0"].size) * HOP, len(curve) - 1)
    truth = curve[at]
    inner = _interior(truth > 0, c.vrm)
    voiced, unvoiced = inner & (truth > 0), inner & (truth == 0)
    for key in ("dio", "f0"):
        f0 = res[key].astype(np.float64)
        missed = int(np.count_nonzero(f0[voiced] == 0))
        worst = float(np.max(D.cents(f0[voiced & (f0 > 0)], truth[voiced & (f0 > 0)])))
        false_voiced = int(np.count_nonzero(f0[unvoiced] > 0))
        print(f"[f0_dio] {name} {key}: frames {f0.size} interior voiced {int(voiced.sum())} missed {missed} worst "
              f"{worst:.3f} cents; interior unvoiced {int(unvoiced.sum())} voiced there {false_voiced}")
        assert missed == 0 and worst <= 50.0
        assert false_voiced == 0                                  # the lead-in and the gaps come out unvoiced


@pytest.mark.parametrize("sr,hop", D.GPU_CONFIGS)
def test_yardstick_and_margin_inputs(sr, hop):
    yard = D.config_yardstick(sr, hop)
    print(f"[f0_dio] sr {sr} hop {hop}: " + " ".join(f"{k} {v:.3e}" for k, v in yard.items() if isinstance(v, float)))
    n_margin = len(D.margin_inputs(sr))
    pairs = D.reference_pairs(sr, hop)
    assert len(pairs) == n_margin
    tol = 4 * yard["cand_cents"]
    for r, ((a, b), st) in enumerate(zip(pairs, yard["stage_dev"][:n_margin])):
        print(f"[f0_dio]   margin row {r}: margins {a['margin']} stage {st}")
        assert D.is_margin_input(a, yard)
        assert st["same_counts"] and st["cand_flips"] == 0
        assert st["best_band_differs"] == 0 or st["best_band_gap"] <= tol
        assert st["stonemask_flips"] == 0
        assert np.array_equal(a["f0"] > 0, b["f0"] > 0) and np.array_equal(a["dio"] > 0, b["dio"] > 0)
        assert int(np.count_nonzero(a["f0"] > 0)) >= a["f0"].size - 1          # voiced up to both ends
    if sr == 48000:                                               # the long row: see dio_ref.long_input
        a, b = pairs[-1]
        own = D.contour_deviation(a["dio"], b["dio"])[0]
        bound = 1000.0 * (2.0 ** (own / 1200.0) - 1.0)
        print(f"[f0_dio]   long row: {a['f0'].size} frames, own DIO yardstick {own:.3e} cents, StoneMask's discrete "
              f"choices at least {a['margin']['discrete']:.3e} (relative) from a step, bound {bound:.3e}")
        assert a["f0"].size == 2001 and a["margin"]["discrete"] >= bound
    for (a, b), flips in zip(D.natural_pairs(sr, hop), yard["natural_flips"]):
        print(f"[f0_dio]   natural row: frames {a['f0'].size} voicing flips (dio, refined) {flips}")
        assert max(flips) <= 0.01 * a["f0"].size
    # the batch covers at least three overlap-save blocks and every StoneMask transform of the rate
    c = pairs[0][0]["consts"]
    assert min(len(y) for y in D.margin_inputs(sr)) >= 3 * c.step
    sizes = set()
    for a, _ in pairs:
        sizes |= {2 ** (2 + int(np.floor(np.log2(2 * int(1.5 * sr / float(f) + 1.0) + 1)))) for f in a["dio"] if f > 0}
    lo = 2 ** (2 + int(np.floor(np.log2(2 * int(1.5 * sr / c.f0_ceil + 1.0) + 1))))
    hi = 2 ** (2 + int(np.floor(np.log2(2 * int(1.5 * sr / 75.0 + 1.0) + 1))))
    print(f"[f0_dio]   StoneMask transforms hit: {sorted(sizes)}; of the rate: {lo} .. {hi}")
    assert {s for s in (128, 256, 512, 1024, 2048, 4096) if lo <= s <= hi} <= sizes


def test_float32_events_keep_integer_and_fraction():
    """At 10^6 samples a float32 absolute position resolves 0.06 samples; index + fraction keeps the interval."""
    sr = 48000
    n = 1_000_000
    y = np.sin(2 * np.pi * 790.0 * np.arange(n - 2000, n) / sr)
    sig = np.zeros((1, n))
    sig[0, n - 2000:] = y
    e64 = D.events(sig, np.float64)[0][0]
    e32 = D.events(sig.astype(np.float32), np.float32)[0][0]
    xs2 = 2.0 * np.array([n - 1000.0])
    v64 = D.interval_track(e64[0], e64[1], xs2, sr, np.float64)[0]
    v32 = D.interval_track(e32[0], e32[1], xs2, sr, np.float32)[0]
    print(f"[f0_dio] interval at sample 10^6: float64 {v64:.6f} Hz float32 {v32:.6f} Hz "
          f"({float(D.cents(v64, v32)):.2e} cents)")
    assert float(D.cents(v64, 790.0)) < 0.1 and float(D.cents(v64, v32)) < 0.01


# --------------------------------------------------------------------------- host plan
def _tracker(sr, hop, **config):
    from pitchextractor_amd.f0_tracker import WorldDioTracker
    return WorldDioTracker(sr, hop, **config)


PLAN_CONFIGS = [(16000, 160, ()), (24000, 300, ()), (48000, 480, ())] + [c[1:4] for c in D.CONFIG_CASES]


@pytest.mark.parametrize("sr,hop,config", PLAN_CONFIGS,
                         ids=["16000-160", "24000-300", "48000-480"] + D.CASE_IDS)
def test_plan_matches_the_restatement(sr, hop, config):
    tr = _tracker(sr, hop, **dict(config))
    c = D.Consts(sr, hop, **dict(config))
    assert (tr.bands, tr.half_average_length, tr.cut, tr.voice_range_minimum) == (c.bands, c.half, c.cut, c.vrm)
    default = (sr, hop, config) in PLAN_CONFIGS[:3]                   # the literal figures below are theirs
    if default:
        assert tr.bands == 7
    assert len(tr.boundary) == c.bands and np.allclose(tr.boundary, c.boundary, rtol=1e-15, atol=0)
    assert (tr.n_fft, tr.taps, tr.block_step, tr.lead) == (c.nfft, c.taps, c.step, c.lead)
    assert tr.frame_period == c.frame_period
    for n in (0, 1, hop - 1, hop, 10 ** 7):
        assert tr.frame_count(n) == D.frame_count(n, c)
        assert np.array_equal(tr.frame_times(n), D.frame_times(n, c))
    assert tr.frame_count(0) == 1 and tr.frame_count(hop - 1) == 1
    if default:
        assert tr.frame_count(hop) == 2
    pl = tr.plan([0, 100, 5 * tr.block_step + 1])
    assert list(pl["frames"]) == [1, 1 if default else D.frame_count(100, c), D.frame_count(5 * tr.block_step + 1, c)]
    assert pl["n_blocks"] == 0 + 1 + 6 and pl["n_samples"] == 101 + 5 * tr.block_step
    # the tables' band filters are the restatement's combined filters
    tab = tr.host_tables()
    C = tr.n_fft // 2
    G = tab[2 * C + 2 * (C + 1):].reshape(tr.bands, C + 1, 2)
    for b in (0, tr.bands - 1):
        g, delay = D.combined_filter(c, b)
        gd = np.zeros(tr.n_fft)
        shift = (2 * c.half[0] + c.cut) - delay
        gd[shift:shift + g.size] = g
        ref = np.fft.rfft(gd) / C
        assert np.allclose(G[b, :, 0] + 1j * G[b, :, 1], ref, atol=1e-9)


def test_configurations_reach_their_plans():
    """What each configuration of ``dio_ref.CONFIG_CASES`` is there for, on the plan."""
    plans = {name: _tracker(sr, hop, **dict(config)) for name, sr, hop, config, _ in D.CONFIG_CASES}
    assert plans["sr8000"].n_fft == 1024 and plans["sr8000"].taps == 480
    assert (plans["sr22050"].cut, plans["sr44100"].cut) == (441, 882)
    for name in ("sr22050", "sr44100"):
        assert plans[name].frame_period != round(plans[name].frame_period * 2) / 2       # no whole or half millisecond
    assert plans["one_band"].bands == 1 and plans["sixteen_bands"].bands == 16
    assert plans["wide"].bands == 13 and plans["wide"].voice_range_minimum == 5
    assert plans["narrow"].frame_period == 8.0 and plans["narrow"].bands == 4
    assert plans["narrow"].voice_range_minimum != _tracker(16000, 128).voice_range_minimum


@pytest.mark.parametrize("sr,hop", [(22050, 256), (44100, 512), (16000, 128)])
def test_frame_counts_on_the_integer_boundary(sr, hop):
    """n = k hop: 1000 n / sr / frame_period is k in exact arithmetic, and k or k - 1 after the truncation of its
    float64 value.  The plan and the restatement divide in the same order, so they agree whichever it is."""
    tr, c = _tracker(sr, hop), D.Consts(sr, hop)
    k = np.arange(1, 2001, dtype=np.int64)
    lengths = np.stack([k * hop - 1, k * hop, k * hop + 1], axis=1).reshape(-1)
    got = tr.plan(lengths.tolist())["frames"]
    want = np.array([D.frame_count(int(n), c) for n in lengths], np.int64)
    below = int(np.count_nonzero(want.reshape(-1, 3)[:, 1] == k))
    print(f"[f0_dio] sr {sr} hop {hop}: frame counts at n = k hop - 1, k hop, k hop + 1 for k = 1 .. 2000; the quotient "
          f"at n = k hop truncates to k - 1 in {below} cases")
    assert np.array_equal(got, want)
    assert np.all(want.reshape(-1, 3)[:, 0] == k) and np.all(want.reshape(-1, 3)[:, 2] == k + 1)


def test_configurations_refused_by_the_plan():
    from pitchextractor_amd import _lib
    _tracker(16000, 160, channels_in_octave=4.5)                       # log2(800 / 71) 4.5 = 15.7: sixteen bands
    for sr, hop, bad in ((16000, 160, dict(channels_in_octave=4.6)),   # 16.07: a seventeenth band
                         (48000, 480, dict(f0_floor=30.0)),            # band filter of 2 * 960 + 4 * 566 taps: 16384 points
                         (48000, 480, dict(f0_floor=70.3))):           # StoneMask window of 2 * 1025 + 1 samples: 8192 points
        with pytest.raises(_lib.HipLibraryError, match="unsupported"):
            _tracker(sr, hop, **bad)
    _tracker(48000, 480, f0_floor=70.5)
    c = D.Consts(48000, 480, f0_floor=30.0)
    assert 2 * c.taps > 8192 and D.Consts(48000, 480, f0_floor=70.3).nfft == 8192


@pytest.mark.parametrize("case", D.CONFIG_CASES, ids=D.CASE_IDS)
def test_configuration_yardstick_and_margin_inputs(case):
    name, sr, hop, config, inputs = case
    yard = D.config_yardstick(sr, hop, config, inputs)
    print(f"[f0_dio] {name} sr {sr} hop {hop} {dict(config)}: " +
          " ".join(f"{k} {v:.3e}" for k, v in yard.items() if isinstance(v, float)))
    pairs = D.reference_pairs(sr, hop, True, config, inputs)
    assert len(pairs) == 2 and all(seconds <= 1.5 for seconds, _, _, _ in inputs)
    tol = 4 * yard["cand_cents"]
    changed = np.zeros(4, np.int64)
    for r, ((a, b), st) in enumerate(zip(pairs, yard["stage_dev"])):
        print(f"[f0_dio]   margin row {r}: frames {a['f0'].size} voiced {int((a['f0'] > 0).sum())} margins {a['margin']} "
              f"stage {st}")
        assert D.is_margin_input(a, yard)
        assert st["same_counts"] and st["cand_flips"] == 0
        assert st["best_band_differs"] == 0 or st["best_band_gap"] <= tol
        assert st["stonemask_flips"] == 0
        assert np.array_equal(a["f0"] > 0, b["f0"] > 0) and np.array_equal(a["dio"] > 0, b["dio"] > 0)
        assert int(np.count_nonzero(a["f0"] > 0)) >= 40
        before = [a["best"]] + list(a["steps"][:3])
        changed += [int(np.count_nonzero(a["steps"][s] != before[s])) for s in range(4)]
    c = pairs[0][0]["consts"]
    assert min(len(y) for y in D.config_margin_inputs(sr, inputs)) >= 3 * c.step or c.nfft == 8192
    print(f"[f0_dio]   frames changed by steps 1 .. 4 of the contour fix: {changed.tolist()}")
    if name == "allowed_0.02":
        assert changed.max() > 20                                  # far more than the ends any configuration trims
    if name == "allowed_0.5":                                      # a change the default allowed_range would refuse
        for a, _ in pairs:
            at_default = D.fix_contour(a["best"], a["cand"], D.Consts(sr, hop), np.float64)
            assert any(not np.array_equal(x, y) for x, y in zip(at_default, a["steps"]))
    if name == "sr8000":
        above = [(a["dio"] > sr / 12.0, a, b) for a, b in pairs]
        total = sum(int(m.sum()) for m, _, _ in above)
        print(f"[f0_dio]   frames with a DIO value above fs / 12 = {sr / 12.0:.1f} Hz: {total}")
        assert total >= 10
        for m, a, b in above:
            assert not np.any(a["f0"][m] > 0) and not np.any(b["f0"][m] > 0)
            assert np.array_equal(b["dio"] > sr / 12.0, m)


def test_argument_checks_run_before_any_device_call():
    from pitchextractor_amd import _lib
    lib = _lib.load()
    cfg = (ctypes.c_double * 4)(71.0, 800.0, 2.0, 0.1)
    consts, half, dc = (ctypes.c_long * 10)(), (ctypes.c_long * 16)(), (ctypes.c_double * 17)()
    tot, meta = (ctypes.c_long * 6)(), (ctypes.c_long * 16)()
    n, off = (ctypes.c_long * 1)(1000), (ctypes.c_long * 1)(0)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    plan = lambda sr, hop, c=cfg, nn=n: lib.pe_f0_dio_plan(1, p(nn), p(off), sr, hop, p(c), p(consts), p(half),  # noqa: E731
                                                            p(dc), p(meta), p(tot))
    assert plan(24000, 300) == 0
    assert plan(4000, 50) == _lib.PE_E_UNSUPPORTED if hasattr(_lib, "PE_E_UNSUPPORTED") else plan(4000, 50) == -2
    assert plan(4000, 50) == -2 and plan(96000, 960) == -2
    assert plan(24000, 0) == -1 and plan(0, 300) == -1
    assert plan(24000, 300, (ctypes.c_double * 4)(800.0, 71.0, 2.0, 0.1)) == -1
    assert plan(24000, 300, (ctypes.c_double * 4)(71.0, 800.0, 2.0, float("nan"))) == -1
    assert plan(24000, 300, cfg, (ctypes.c_long * 1)(-1)) == -1
    assert lib.pe_f0_dio_plan(1, None, None, 24000, 300, p(cfg), p(consts), p(half), p(dc), p(meta), p(tot)) == -1
    # the device entry points check (sr, hop, config) and the plan on the host, before any launch
    buf = p((ctypes.c_float * 64)())
    for sr, hop in ((4000, 50), (96000, 960)):
        assert lib.pe_f0_dio_bands(buf, buf, p(meta), buf, buf, 0, 1, sr, hop, p(cfg), buf, None) == -2
        assert lib.pe_f0_dio_events(buf, buf, p(meta), 1, sr, hop, p(cfg), buf, buf, buf, buf, 0, None) == -2
        assert lib.pe_f0_dio_candidates(buf, buf, buf, buf, p(meta), 1, sr, hop, p(cfg), buf, buf, buf, buf, None) == -2
        assert lib.pe_f0_dio_fix(buf, buf, buf, p(meta), 1, sr, hop, p(cfg), buf, None) == -2
        assert lib.pe_f0_stonemask(buf, buf, p(meta), buf, buf, 0, 1, sr, hop, 71.0, buf, None) == -2
    assert plan(24000, 300) == 0
    assert lib.pe_f0_dio_events(buf, buf, p(meta), 1, 24000, 300, p(cfg), buf, buf, buf, None, 0, None) == -3
    bad = (ctypes.c_long * 16)(*meta)
    bad[3] = 7                                                     # a frame prefix that is not the plan's
    assert lib.pe_f0_dio_fix(buf, buf, buf, p(bad), 1, 24000, 300, p(cfg), buf, None) == -1
    assert lib.pe_f0_stonemask(buf, buf, p(meta), buf, buf, 0, 1, 48000, 480, 41.0, buf, None) == -2
    assert lib.pe_f0_stonemask(buf, buf, p(meta), buf, buf, 5, 1, 24000, 300, 71.0, buf, None) == -1


# --------------------------------------------------------------------------- Python layer
def test_refusals_at_construction():
    for bad in (dict(algorithm="harvest"), dict(fallback="harvest"), dict(speed=2), dict(frame_period_ms=5.0)):
        with pytest.raises(NotImplementedError):
            _tracker(24000, 300, **bad)
    from pitchextractor_amd.f0_tracker import check_dio_config
    with pytest.raises(NotImplementedError, match="harvest"):
        check_dio_config({}, 24000, 300, require_algorithm=True)
    for ok in (dict(algorithm="dio", fallback="dio"), dict(fallback=None), dict(fallback=""),
               dict(frame_period_ms=12.5, stonemask=False, min_voiced_frames=3), dict(f0_floor=80.0, f0_ceil=600.0)):
        _tracker(24000, 300, **ok)
    assert _tracker(24000, 300, stonemask="false").stonemask is False
    from pitchextractor_amd import _lib
    with pytest.raises(_lib.HipLibraryError):
        _tracker(4000, 50)


def test_host_tensors_are_refused():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _tracker(24000, 300).track(torch.zeros(24000))


def _dataset(tmp_path, backends, order=None):
    from pitchextractor_amd.meldataset import MelDataset
    f0_params = {"backends": backends}
    if order:
        f0_params["backend_order"] = order
    return MelDataset([], sr=24000, f0_params=f0_params, verbose=False)


def test_chain_selection(tmp_path, caplog):
    from pitchextractor_amd import f0_tracker
    praat = {"type": "praat", "method": "ac"}
    ds = _dataset(tmp_path, {"pyworld_harvest": {"type": "pyworld", "algorithm": "harvest"},
                             "pyworld_dio": {"type": "pyworld", "algorithm": "dio", "fallback": "dio",
                                             "stonemask": True},
                             "praat": praat})
    assert [(n, cls) for n, cls, _ in ds._native_f0] == [("pyworld_dio", "WorldDioTracker"),
                                                                  ("praat", "PraatACTracker")]
    with caplog.at_level(logging.WARNING):
        assert ds.prepare_f0_caches(device="cpu") == []               # nothing listed: only the warnings run
    skipped = [r.getMessage() for r in caplog.records if "is not part of this build: skipped" in r.getMessage()]
    assert skipped == ["[MelDataset] F0 backend 'pyworld_harvest' (pyworld) is not part of this build: skipped"]
    # order against a praat entry is the chain's
    ds = _dataset(tmp_path, {"praat": praat, "pyworld_dio": {"type": "pyworld", "algorithm": "dio"}})
    assert [n for n, _, _ in ds._native_f0] == ["praat", "pyworld_dio"]
    # a pyworld entry without algorithm is harvest; one with another fallback is not native either
    ds = _dataset(tmp_path, {"a": {"type": "pyworld"}, "b": {"type": "pyworld", "algorithm": "dio",
                                                              "fallback": "harvest"}})
    assert ds._native_f0 == []
    with pytest.raises(RuntimeError, match="enables no praat"):
        ds.prepare_f0_caches(device="cpu")
    assert f0_tracker.NATIVE_TYPES == ("praat", "parselmouth")
