"""The stress-condition restatements (tests/stress_ref.py) against numpy and scipy, and the host side of
``pitchextractor_amd.stress`` (no GPU needed).  Every figure is printed before it is asserted."""
import ctypes
import math

import numpy as np
import pytest

from tests import stress_ref as R

f32 = np.float32


# --------------------------------------------------------------------------------------------------------------- rir
@pytest.mark.parametrize("n,taps", [(1, 1), (2047, 2048), (2049, 5000), (3 * 2048 + 5, 2049), (700, 5000)])
def test_partitioned_overlap_save_is_the_convolution(n, taps):
    rng = np.random.default_rng(n + taps)
    x, h = rng.standard_normal(n), R.decaying_rir(taps, 3).astype(np.float64)
    direct = np.convolve(x, h)[:n]
    scale = float(np.max(np.abs(direct)))
    y, peak, scaled = R.rir(x, h)
    assert peak == scale and scaled == (peak > 0.99) and np.array_equal(y, direct / (peak + 1e-6) if scaled else direct)
    y64, dt64 = R.rir_partitioned(x, h, np.float64)
    y32, dt32 = R.rir_partitioned(x, h, np.float32)
    e64, e32 = float(np.max(np.abs(y64 - direct))) / scale, float(np.max(np.abs(y32 - direct))) / scale
    print(f"[stress] overlap-save n {n} taps {taps}: float64 {e64:.2e} float32 {e32:.2e} of the peak")
    assert dt64 == np.complex128 and dt32 == np.complex64          # numpy keeps the float32 transform in float32
    assert e64 <= 1e-12 and e32 <= 1e-4


def test_rir_normalisation_branch():
    x = np.zeros(100)
    x[3] = 1.0
    for gain, scaled in ((0.5, False), (3.0, True)):
        y, peak, did = R.rir(x * gain, [1.0, 0.5])
        assert did is scaled and peak == gain
        assert float(np.max(np.abs(y))) == (gain / (gain + 1e-6) if scaled else gain)
    assert R.rir(np.zeros(0), [1.0])[0].size == 0


def test_prepare_rir_is_the_load_time_normalisation():
    from pitchextractor_amd import stress
    h = R.decaying_rir(300, 1) * f32(7.0)
    want = (h / (np.max(np.abs(h)) + 1e-6)).astype(np.float32)     # the notebook's line on a float32 array
    assert np.array_equal(stress.prepare_rir(h), want)
    with pytest.raises(ValueError):
        stress.prepare_rir([])


# ----------------------------------------------------------------------------------------------------------- clipping
def test_quantile_restatement_is_numpys():
    rng = np.random.default_rng(0)
    cases = [np.array([0.25], f32), np.array([0.1, 0.7], f32), np.array([0.1, 0.7, 0.3, 0.9, 0.45], f32),
             (np.round(rng.standard_normal(500) * 4) / 8).astype(f32),                  # ties
             rng.standard_normal(4097).astype(f32), (rng.standard_normal(1023) * 1e-3).astype(f32),
             np.zeros(16, f32)]
    seen = set()
    for x in cases:
        for percent in (0.3, 2.0, 10.0, 37.5, 50.0, 100.0):
            q = max(0.0, 1.0 - percent / 100.0)
            want = np.quantile(np.abs(x), q)
            got = R.quantile_f32(np.abs(x), q)
            v = f32(f32(x.size - 1) * f32(q))
            g = float(v - np.floor(v))
            seen.add("g0" if g == 0 else ("hi" if g >= 0.5 else "lo"))
            assert want.dtype == np.float32 and got == want, (x.size, percent, got, want)
            y, thr = R.sample_clipping(x, percent)
            ref = np.clip(x, -want, want).astype(np.float32) if want > 0 else x
            assert np.array_equal(y, ref)
    assert seen == {"g0", "hi", "lo"}
    assert np.array_equal(R.sample_clipping(cases[2], 0.0)[0], cases[2])


# ---------------------------------------------------------------------------------------------------------------- agc
@pytest.mark.parametrize("s", [1, 2, 25, 64, 239, 240])
def test_moving_average_is_numpys_same_mode(s):
    rng = np.random.default_rng(s)
    g = rng.uniform(0.2, 7.0, 1000).astype(f32)
    want = np.convolve(g.astype(np.float64), np.ones(s) / s, mode="same")
    got = R.smooth_same(g, s)
    err = float(np.max(np.abs(got - want)))
    print(f"[stress] same-mode average s {s}: {err:.2e}")
    assert got.size == g.size and err <= 1e-13
    assert np.allclose(R.smooth_same(g[:s], s), np.convolve(g[:s].astype(np.float64), np.ones(s) / s, "same"), atol=1e-13)


def _notebook_agc(audio, level_db, sr, target_rms):
    """Utils/amplitude_pathologies.ipynb ``apply_agc_pumping``, line by line."""
    attack = 0.01
    release = np.interp(level_db, [0.0, 10.0], [0.05, 0.4])
    depth_db = np.interp(level_db, [0.0, 10.0], [3.0, 18.0])
    attack_coeff, release_coeff = np.exp(-1.0 / (attack * sr)), np.exp(-1.0 / (release * sr))
    env, gains = 0.0, np.zeros_like(audio, dtype=np.float32)
    for i, sample in enumerate(audio):
        rectified = abs(float(sample))
        if rectified > env:
            env = attack_coeff * env + (1.0 - attack_coeff) * rectified
        else:
            env = release_coeff * env + (1.0 - release_coeff) * rectified
        max_gain = 10 ** (depth_db / 20.0)
        gains[i] = np.clip(target_rms / (env + 1e-6), 1.0 / max_gain, max_gain)
    smoothing = int(sr * np.interp(level_db, [0.0, 10.0], [0.01, 0.12]))
    raw = gains
    if smoothing > 1:
        gains = np.convolve(gains, np.ones(smoothing, dtype=np.float32) / smoothing, mode="same")
    return np.clip(audio * gains, -1.0, 1.0).astype(np.float32), raw, smoothing


@pytest.mark.parametrize("level", [2.0, 10.0])
def test_agc_restatement_follows_the_notebook(level):
    x = R.agc_input(5000, 5)
    want, raw_want, s = _notebook_agc(x, level, 2000, 0.15)
    got, raw, smooth, p = R.agc_pumping(x, level, 2000, 0.15, return_stages=True)
    assert p["smoothing"] == s and np.array_equal(raw, raw_want)               # the follower is the notebook's exactly
    # the notebook sums the window in float32 (s terms): s float32 roundings of the gain, the restatement makes one
    err = float(np.max(np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 2.0 ** -20)))
    print(f"[stress] agc level {level}: smoothing {s}, restatement vs notebook {err:.2e} relative")
    assert err <= (s + 2) * 2.0 ** -24
    assert raw.min() == f32(1.0 / p["max_gain"]) and raw.max() == f32(p["max_gain"])   # both bounds are hit
    assert np.abs(got).max() == 1.0                                                    # and the final clip
    assert np.array_equal(R.agc_pumping(x, 0.0, 2000), x)
    with pytest.raises(ValueError):
        R.agc_pumping(x[:s - 1], level, 2000)


# ------------------------------------------------------------------------------------------------------------ biquads
def test_biquad_restatement_is_lfilter():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(1)
    x = (0.3 * rng.standard_normal(6000)).astype(f32)
    for stage in ({"freq": 80.0, "gain_db": 2.0, "Q": 0.9}, {"freq": 3500.0, "gain_db": 5.0, "Q": 1.2},
                  {"freq": 9000.0, "gain_db": -6.0, "Q": 0.7}):
        b, a = R.peaking_biquad(24000, stage["freq"], stage["gain_db"], stage["Q"])
        want = signal.lfilter(b, a, x.astype(np.float64))
        err = float(np.max(np.abs(R.biquad_stage(x, b, a) - want)))
        print(f"[stress] biquad {stage}: restatement vs lfilter {err:.2e}")
        assert err <= 1e-11
        got = R.microphone_eq(x, 24000, [stage])
        assert np.array_equal(got, np.clip(want, -1, 1).astype(f32)) or \
            float(np.max(np.abs(got - np.clip(want, -1, 1)))) <= 2.0 ** -24
    loud = (3.0 * rng.standard_normal(500)).astype(f32)
    out = R.microphone_eq(loud, 24000, R_profiles()["smartphone"])
    assert out.max() == 1.0 and out.min() == -1.0                                   # the clamp is driven


def R_profiles():
    from pitchextractor_amd import stress
    return stress.MICROPHONE_PROFILES


def test_coefficients_and_the_nyquist_rule():
    from pitchextractor_amd import stress
    for name, curve in stress.MICROPHONE_PROFILES.items():
        c = stress.cascade_coefficients(24000, name)
        assert c.shape == (3, 5)
        for row, stage in zip(c, curve):
            b, a = R.peaking_biquad(24000, stage["freq"], stage["gain_db"], stage["Q"])
            if np.array_equal(b, a):
                assert name == "studio_ldc" and stage["freq"] == 12000.0 and list(row) == [1, 0, 0, 0, 0]
            else:
                assert np.allclose(row, [b[0], b[1], b[2], a[1], a[2]], rtol=1e-14, atol=1e-16)
    assert list(stress.cascade_coefficients(24000, [{"freq": 1000.0, "gain_db": 0.0, "Q": 1.0}])[0]) == [1, 0, 0, 0, 0]
    # 11 990 Hz at 24 kHz: decided by the pole radius alone
    b, a = stress.peaking_biquad(24000, 11990.0, 1.5, 0.9)
    radius = stress.pole_radius(a)
    print(f"[stress] 11 990 Hz stage: pole radius {radius!r}")
    if radius < stress.POLE_RADIUS_LIMIT:
        assert stress.cascade_coefficients(24000, [{"freq": 11990.0, "gain_db": 1.5, "Q": 0.9}]).shape == (1, 5)
    else:
        with pytest.raises(ValueError):
            stress.cascade_coefficients(24000, [{"freq": 11990.0, "gain_db": 1.5, "Q": 0.9}])
    with pytest.raises(ValueError, match="pole radius"):          # a narrow stage a hair below the band edge
        stress.cascade_coefficients(24000, [{"freq": 11999.9999, "gain_db": 1.5, "Q": 1e6}])
    with pytest.raises(ValueError):
        stress.cascade_coefficients(24000, [{"freq": 100.0}] * 9)
    with pytest.raises(ValueError):
        stress.cascade_coefficients(24000, "no such microphone")


# ------------------------------------------------------------------------------------------------------------ metrics
def _notebook_metrics(reference, prediction, thr=10.0):
    """``compute_metrics`` of the notebooks, in float64."""
    length = min(reference.shape[0], prediction.shape[0])
    reference, prediction = reference[:length].astype(np.float64), prediction[:length].astype(np.float64)
    ref_voiced, pred_voiced = reference > 0, prediction > thr
    voiced = int(np.count_nonzero(ref_voiced))
    vuv = float(np.count_nonzero(ref_voiced == pred_voiced) / max(length, 1))
    if voiced == 0:
        return dict(RPA=math.nan, RCA=math.nan, VUV=vuv, OctaveError=math.nan)
    cents = lambda f: 1200.0 * np.log2(f / 55.0)  # noqa: E731
    d = cents(np.clip(prediction[ref_voiced], a_min=float(f32(1e-5)), a_max=None)) - cents(reference[ref_voiced])
    circ = np.mod(d + 600.0, 1200.0) - 600.0
    numbers = np.round(d / 1200.0)
    octave = (np.abs(d) > 50.0) & (numbers != 0) & (np.abs(d - numbers * 1200.0) <= 50.0)
    return dict(RPA=float(np.count_nonzero(np.abs(d) <= 50.0) / voiced),
                RCA=float(np.count_nonzero(np.abs(circ) <= 50.0) / voiced), VUV=vuv,
                OctaveError=float(np.count_nonzero(octave) / voiced))


def test_metrics_restatement_on_hand_built_tracks():
    ref = np.array([0, 220, 220, 220, 220, 220, 220, 0, 220, 220], f32)
    cents = np.array([0, 10, -40, 1210, -1190, 600 + 300, 2400 - 20, 0, 70, 0], np.float64)
    pred = (220.0 * 2.0 ** (cents / 1200.0)).astype(f32)
    pred[0], pred[7], pred[9] = 0.0, 150.0, 0.0            # unvoiced agree, a false voiced frame, a missed one
    got = R.melody_metrics(ref, pred)
    want = _notebook_metrics(ref, pred)
    print(f"[stress] metrics on the hand-built track: {got}")
    for k, v in want.items():
        assert got[k] == v
    # voiced: 8 frames; within 50 cents: +10, -40; chroma adds the two octave slips and the two-octave one
    assert got["n_voiced"] == 8 and got["n_frames"] == 10
    assert got["RPA"] == 2 / 8 and got["RCA"] == 5 / 8 and got["OctaveError"] == 3 / 8 and got["VUV"] == 8 / 10
    assert math.isnan(got["VUV_flips"])
    base = pred.copy()
    base[1] = 0.0
    base = base[:6]
    assert R.melody_metrics(ref, pred, baseline=base)["VUV_flips"] == 1 / 6
    none = R.melody_metrics(np.zeros(4, f32), np.array([0, 50, 0, 5], f32))
    assert math.isnan(none["RPA"]) and math.isnan(none["RCA"]) and math.isnan(none["OctaveError"])
    assert none["VUV"] == 3 / 4 and none["n_voiced"] == 0
    short = R.melody_metrics(ref, pred[:4])
    assert short["n_frames"] == 4 and short == {**R.melody_metrics(ref[:4], pred[:4])}
    assert np.round(0.5) == 0 and np.round(1.5) == 2                     # the octave number rounds half to even
    assert R.boundary_margin_cents(np.array([10.0, 1210.0, -1190.0])) == 40.0


# ----------------------------------------------------------------------------------------------------- plan and checks
def test_plan_arithmetic():
    from pitchextractor_amd import stress
    pl = stress.plan_rows([0, 1, 2048, 2049, 3 * 2048 + 5], [0, 0, 1, 2049, 4098], [7, 7, 8, 2056, 4105])
    assert (pl["block_step"], pl["piece"], pl["clip_chunk"]) == (R.BLOCK, 512, 1024)
    assert pl["table_floats"] == 2 * 2048 + 2 * 2049 == stress.host_tables().size
    assert pl["meta"].tolist() == [[0, 0, 7, 0, 0, 0], [0, 1, 7, 0, 1, 0], [1, 2048, 8, 1, 1, 1],
                                   [2049, 2049, 2056, 2049, 2, 2], [4098, 6149, 4105, 4098, 4, 4]]
    assert pl["n_samples"] == 1 + 2048 + 2049 + 6149 and pl["n_blocks"] == 8
    assert stress.plan_rows([], [], [])["rows"] == 0
    tw = stress.host_tables()[:4096].reshape(2048, 2)
    assert np.allclose(tw[:, 0] + 1j * tw[:, 1], np.exp(-2j * np.pi * np.arange(2048) / 2048), atol=1e-7)
    with pytest.raises(Exception):
        stress.plan_rows([-1], [0], [0])
    # an impulse-response set is a ragged batch whose blocks are the partitions
    rirs = stress.RirSet([np.ones(1), np.ones(2048), np.ones(2049), np.ones(5000)])
    assert rirs.plan["meta"][:, 4].tolist() == [1, 1, 2, 3] and len(rirs) == 4
    with pytest.raises(ValueError):
        stress.RirSet([np.ones(3), np.ones(0)])


def test_argument_checks_run_before_any_device_call():
    from pitchextractor_amd import _lib, stress
    lib = _lib.load()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    buf = p((ctypes.c_float * 64)())
    K = lib.pe_stress_plan_fields()
    assert K == 6 and lib.pe_melody_metrics_fields() == 5
    pl = stress.plan_rows([1000], [0], [0])
    meta = pl["meta"].ctypes.data
    bad = pl["meta"].copy()
    bad[0, 4] = 7                                                  # a block count that is not the plan's
    nt = pl["table_floats"]
    rir = stress.plan_rows([10], [0], [0])["meta"]
    idx = (ctypes.c_int * 1)(0)
    ARG, UNSUP, WS = -1, -2, -3
    # the plan
    assert lib.pe_stress_plan(1, None, None, None, buf, buf, buf) == ARG
    assert lib.pe_stress_plan(-1, buf, buf, buf, buf, buf, buf) == ARG
    # spectra
    assert lib.pe_stress_spectra(buf, buf, bad.ctypes.data, 1, 0, buf, nt, buf, None) == ARG
    assert lib.pe_stress_spectra(buf, buf, meta, 1, 2, buf, nt, buf, None) == ARG
    assert lib.pe_stress_spectra(buf, buf, meta, 1, 0, buf, nt - 1, buf, None) == ARG
    assert lib.pe_stress_spectra(None, buf, meta, 1, 0, buf, nt, buf, None) == ARG
    # rir: plan, index range, an empty impulse response, workspace
    rir_args = lambda m=meta, r=rir.ctypes.data, i=p(idx), ws=None, nb=0: lib.pe_stress_rir(  # noqa: E731
        buf, buf, m, 1, buf, buf, r, 1, buf, i, buf, nt, buf, ws, nb, None)
    assert rir_args(m=bad.ctypes.data) == ARG
    assert rir_args(i=p((ctypes.c_int * 1)(1))) == ARG and rir_args(i=p((ctypes.c_int * 1)(-1))) == ARG
    assert rir_args(r=stress.plan_rows([0], [0], [0])["meta"].ctypes.data) == ARG
    assert rir_args() == WS and rir_args(ws=buf, nb=16) == WS
    assert lib.pe_stress_rir_workspace_bytes(3) == 3 * (2048 * 8 + 4) and lib.pe_stress_rir_workspace_bytes(0) == 0
    # biquads: stage count, finiteness, stability
    ok = (ctypes.c_double * 5)(1.0, 0.0, 0.0, -1.9, 0.95)
    assert lib.pe_stress_biquad(buf, buf, bad.ctypes.data, 1, p(ok), 1, buf, None) == ARG
    assert lib.pe_stress_biquad(buf, buf, meta, 1, p(ok), 0, buf, None) == ARG
    assert lib.pe_stress_biquad(buf, buf, meta, 1, p(ok), 9, buf, None) == ARG
    assert lib.pe_stress_biquad(buf, buf, meta, 1, p((ctypes.c_double * 5)(1, 0, 0, math.nan, 0)), 1, buf, None) == ARG
    assert lib.pe_stress_biquad(buf, buf, meta, 1, p((ctypes.c_double * 5)(1, 0, 0, -2.0, 1.0)), 1, buf, None) == UNSUP
    assert lib.pe_stress_biquad(None, buf, meta, 1, p(ok), 1, buf, None) == ARG
    # clip
    assert lib.pe_stress_clip(buf, buf, meta, 1, 1.5, 0, buf, None, None) == ARG
    assert lib.pe_stress_clip(buf, buf, bad.ctypes.data, 1, 0.9, 0, buf, None, None) == ARG
    assert lib.pe_stress_clip(None, buf, meta, 1, 0.9, 0, buf, None, None) == ARG
    # agc: parameters, a row shorter than the smoothing length, workspace
    prm = (ctypes.c_double * 4)(0.95, 0.99, 0.15, 7.9)
    assert lib.pe_stress_agc(buf, buf, meta, 1, p(prm), 1001, buf, buf, 1 << 20, None) == ARG
    assert lib.pe_stress_agc(buf, buf, meta, 1, p((ctypes.c_double * 4)(1.5, 0.99, 0.15, 7.9)), 10, buf, buf, 1 << 20,
                             None) == ARG
    assert lib.pe_stress_agc(buf, buf, meta, 1, p((ctypes.c_double * 4)(0.95, 0.99, 0.15, 300.0)), 10, buf, buf,
                             1 << 20, None) == ARG
    assert lib.pe_stress_agc(buf, buf, meta, 1, p(prm), 1000, buf, None, 0, None) == WS
    assert lib.pe_stress_agc(buf, buf, meta, 1, p(prm), 1000, buf, buf, 3999, None) == WS
    assert lib.pe_stress_agc_workspace_bytes(1000) == 4000
    # metrics
    tracks = (ctypes.c_long * 5)(0, 10, 0, 0, 0)
    assert lib.pe_melody_metrics(buf, buf, None, buf, None, 1, 10.0, buf, None) == ARG
    assert lib.pe_melody_metrics(buf, buf, None, buf, p((ctypes.c_long * 5)(0, -1, 0, 0, 0)), 1, 10.0, buf, None) == ARG
    assert lib.pe_melody_metrics(None, buf, None, buf, p(tracks), 1, 10.0, buf, None) == ARG
    assert lib.pe_melody_metrics(buf, buf, None, buf, p(tracks), 1, math.nan, buf, None) == ARG
    # nothing to do is not an error, and needs no pointer
    empty = stress.plan_rows([0, 0], [0, 0], [0, 0])["meta"].ctypes.data
    assert lib.pe_stress_clip(None, None, empty, 2, 0.9, 0, None, None, None) == 0
    assert lib.pe_stress_biquad(None, None, empty, 2, p(ok), 1, None, None) == 0
    assert lib.pe_stress_agc(None, None, empty, 2, p(prm), 1, None, None, 0, None) == 0
    assert lib.pe_stress_rir(None, None, empty, 2, None, None, rir.ctypes.data, 1, None, p((ctypes.c_int * 2)(0, 0)),
                             None, nt, None, None, 0, None) == 0
    assert lib.pe_melody_metrics(None, None, None, None, None, 0, 10.0, None, None) == 0


def test_host_tensors_are_refused():
    import torch
    from pitchextractor_amd import inference, stress
    x = torch.zeros(24000)
    rirs = stress.RirSet([np.ones(4)])
    for call in (lambda: stress.apply_rir(x, rirs), lambda: stress.apply_microphone_eq(x, 24000, "headset"),
                 lambda: stress.apply_sample_clipping(x, 10.0), lambda: stress.apply_sample_clipping(x, 0.0),
                 lambda: stress.apply_agc_pumping(x, 10.0, 24000), lambda: stress.apply_agc_pumping(x, 0.0, 24000),
                 lambda: stress.apply_resample_condition(x, 24000, 8000),
                 lambda: stress.apply_resample_condition(x, 24000, 24000)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stress.apply_sample_clipping(np.zeros(10, f32), 10.0)
    assert callable(inference.melody_metrics) and callable(inference.stress_sweep)


def test_python_layer_refusals():
    import torch
    from pitchextractor_amd import stress
    s = stress.agc_parameters(10.0, 24000, 0.15)["smoothing"]
    assert s == 2880 and stress.agc_parameters(2.0, 2000, 0.15)["smoothing"] == 64
    ref = R.agc_parameters(10.0, 24000, 0.15)
    got = stress.agc_parameters(10.0, 24000, 0.15)
    assert all(float(ref[k]) == got[k] for k in ref)
    with pytest.raises(ValueError, match="shorter than the smoothing length"):
        stress.apply_agc_pumping(torch.zeros(s - 1), 10.0, 24000)
    with pytest.raises(ValueError, match="shorter than the smoothing length"):
        stress.apply_agc_pumping(torch.zeros(2, s), 10.0, 24000, lengths=[s, s - 1])
    with pytest.raises(ValueError):
        stress.Condition("noise", "snr 10")
    c = stress.Condition("clipping", "clip 10 %", percent=10.0)
    assert (c.kind, c.label, c.params) == ("clipping", "clip 10 %", {"percent": 10.0})
