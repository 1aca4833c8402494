"""Pitch modulation without a GPU: the time map, the float64 restatement against analytic sinusoids, the label rule
against ``world.time_warp_curve``, the config, the draws, the cap, and the entry points' host checks."""
import ctypes
import random

import numpy as np
import pytest
import torch

from pitchextractor_amd import _lib, build, pitch_mod as PM, world
from tests import f0_track_ref as F, pitch_mod_ref as R

SR = 24000
MIXED = PM.Modulation(((0.03, 6.0, 0.7), (0.005, 13.0, 2.0)), 0.06)


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _lib.load()


# --------------------------------------------------------------------------------------------------------- the time map
@pytest.mark.parametrize("mod", [MIXED, PM.Modulation((), 0.5), PM.Modulation(((0.0625,) * 1 + (5.0, 0.1),) * 4, 0.0),
                                 PM.Modulation(((0.1, 0.05, 1.0),), -0.3)])
def test_time_map_ends_monotone_and_speed(mod):
    T = 11400
    u = np.arange(0, T + 1, dtype=np.float64)
    tau, s = PM.time_map(mod, T, u, SR)
    assert tau[0] == 0.0 and tau[-1] == float(T)                # pinned
    free = PM.time_map(mod, T, np.array([T - 1e-9]), SR)[0][0]   # the unpinned form lands there too
    assert abs(free - T) < 1e-6
    assert np.all(np.diff(tau) > 0)
    assert s.min() >= 0.5 - 1e-12 and s.max() <= 1.5 + 1e-12
    h = 1e-3
    mid = u[1:-1]
    numeric = (PM.time_map(mod, T, mid + h, SR)[0] - PM.time_map(mod, T, mid - h, SR)[0]) / (2 * h)
    assert np.max(np.abs(numeric - s[1:-1])) < 1e-7


def test_the_ramp_is_a_glide_between_its_ends():
    _, s = PM.time_map(PM.Modulation((), 0.2), 1000, np.array([0.0, 500.0, 1000.0]), SR)
    assert np.allclose(s, [0.8, 1.0, 1.2], atol=1e-15)


# ------------------------------------------------------------------------------------------------------ the restatement
# measured deviation of the float64 restatement from sin(2 pi f (t0 + tau) / sr) on 12 000 samples, span 300 .. 11 700,
# 200 samples inside the span's ends: kaiser_fast 3.03e-5 (220 Hz), 2.81e-5 (1000 Hz); kaiser_best 1.55e-6, 1.53e-6
ANALYTIC = {("kaiser_fast", 220.0): 3.03e-5, ("kaiser_fast", 1000.0): 2.81e-5,
            ("kaiser_best", 220.0): 1.55e-6, ("kaiser_best", 1000.0): 1.53e-6}


@pytest.mark.parametrize("quality,f", sorted(ANALYTIC))
def test_restatement_against_the_analytic_sinusoid(quality, f):
    """A sinusoid read at tau is sin(2 pi f (t0 + tau) / sr): the interpolator's own error is what remains.  The bound
    is the value the restatement measures (``ANALYTIC``: 3.03e-5 / 2.81e-5 for kaiser_fast at 220 / 1000 Hz, 1.55e-6 /
    1.53e-6 for kaiser_best) times 1.5."""
    n, t0, t1 = 12000, 300, 11700
    x = np.sin(2 * np.pi * f * np.arange(n) / SR)
    y = R.warp(x, t0, t1, MIXED, SR, quality)
    i = np.arange(t0 + 200, t1 - 200)
    tau, _ = PM.time_map(MIXED, t1 - t0, (i - t0).astype(np.float64), SR)
    dev = float(np.abs(y[i] - np.sin(2 * np.pi * f * (t0 + tau) / SR)).max())
    print(f"{quality} {f} Hz: deviation {dev:.3e}, bound {1.5 * ANALYTIC[quality, f]:.3e}")
    assert dev <= 1.5 * ANALYTIC[quality, f]
    assert np.array_equal(y[:t0 + 1], x[:t0 + 1]) and np.array_equal(y[t1:], x[t1:])
    y32 = R.warp_f32(x.astype(np.float32), t0, t1, MIXED, SR, quality)
    assert np.abs(y32 - R.warp(x.astype(np.float32), t0, t1, MIXED, SR, quality)).max() < 4e-6


# ----------------------------------------------------------------------------------------------------------- the labels
def test_label_rule_is_time_warp_curves():
    rng = np.random.default_rng(3)
    L, hop = 61, 32
    f0 = (150.0 + 60.0 * rng.random(L)).astype(np.float32)
    f0[:3] = 0
    f0[20:27] = 0
    f0[40] = 0
    f0[-2:] = 0
    sil = np.zeros(L, np.float32)
    got, flags = R.labels(f0, sil, L, MIXED, hop, SR)
    tau, s = PM.time_map(MIXED, (L - 1) * hop, np.arange(L) * float(hop), SR)
    want = world.time_warp_curve(f0, tau / hop)
    assert np.allclose(got, np.where(want > 0, s * want, 0.0), rtol=1e-14, atol=0)
    assert np.count_nonzero(got == 0) >= 8 and not flags.any()


def test_label_rule_keeps_unvoiced_fill_and_flags():
    L, hop = 12, 32
    f0 = np.full(L, 200.0, np.float32)
    sil = np.zeros(L, np.float32)
    f0[4:7], sil[4:7] = 55.0, 1.0                                # a non-zero fill under the silence flag
    got, flags = R.labels(f0, sil, L, PM.Modulation((), 0.3), hop, SR)
    assert set(np.unique(flags)) == {0.0, 1.0}
    assert np.all(got[flags == 1] == 55.0)                      # copied, neither scaled nor averaged
    _, s = PM.time_map(PM.Modulation((), 0.3), (L - 1) * hop, np.arange(L) * float(hop), SR)
    assert np.allclose(got[flags == 0], (s * 200.0)[flags == 0], rtol=1e-15)


# ----------------------------------------------------------------------------------------------------------- the config
@pytest.mark.parametrize("config", [
    {"pitch": 1}, {"p": 1.5}, {"vibrato": {"depth": 3}}, {"vibrato": {"p": 2}}, {"vibrato": {"depth_cents": [40, 10]}},
    {"vibrato": {"depth_cents": [-5, 10]}}, {"vibrato": {"rate_hz": [0.01, 5]}},
    {"glide": {"cents": [1, float("nan")]}},
    {"quality": "sinc_best"}, {"vibrato": 3}, [1, 2],
    {"vibrato": {"p": 1, "depth_cents": [10, 400]}},                                              # 2 d alone passes 0.5
    {"vibrato": {"p": 1, "depth_cents": [0, 150]}, "flutter": {"p": 0.1, "depth_cents": [0, 150]},
     "glide": {"p": 0.5, "cents": [-600, 600]}},                                                  # only together
])
def test_config_refusals(config):
    with pytest.raises(ValueError):
        PM.PitchModulator(config, SR, 300)


def test_config_defaults_and_activity():
    assert not PM.PitchModulator({}, SR, 300).active
    assert not PM.PitchModulator({"enabled": False, "vibrato": {"p": 1}}, SR, 300).active
    assert not PM.PitchModulator({"p": 0, "vibrato": {"p": 1}}, SR, 300).active
    pm = PM.PitchModulator({"vibrato": {"p": 1}}, SR, 300)
    assert pm.active and pm.config["quality"] == "kaiser_fast" and not pm.config["apply_to_synthetic"]
    # a block that is off does not count towards the cap
    PM.PitchModulator({"vibrato": {"p": 0, "depth_cents": [10, 900]}, "glide": {"p": 1}}, SR, 300)
    with pytest.raises(ValueError):
        PM.PitchModulator({}, SR, 0)


FULL = {"p": 0.7, "vibrato": {"p": 0.8}, "flutter": {"p": 0.5}, "drift": {"p": 0.5}, "glide": {"p": 0.6}}


def test_draws_are_deterministic_and_leave_the_global_generators_alone():
    random.seed(11)
    np.random.seed(11)
    before = (random.getstate(), np.random.get_state()[1].copy(), np.random.get_state()[2])
    a = PM.PitchModulator(FULL, SR, 300, seed=4, rank=1)
    plans = [a.draw(5), a.draw(3)]
    after = (random.getstate(), np.random.get_state()[1], np.random.get_state()[2])
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2] == after[2]
    b = PM.PitchModulator(FULL, SR, 300, seed=4, rank=1)
    again = [b.draw(5), b.draw(3)]
    assert all(np.array_equal(p.on, q.on) and p.mods == q.mods for p, q in zip(plans, again))
    other = PM.PitchModulator(FULL, SR, 300, seed=4, rank=2).draw(5)
    assert other.mods != plans[0].mods
    # one fixed-size block per call whatever the config holds: a sparser config leaves the generator in the same place
    c = PM.PitchModulator({"vibrato": {"p": 1}}, SR, 300, seed=4, rank=1)
    c.draw(5)
    c.draw(3)
    assert c.rng.random() == a.rng.random()
    for plan in plans:
        for mod in plan.mods:
            PM.check_modulation(mod)
    assert any(p.on.any() for p in plans) and not plans[0].without(range(5)).on.any()


def test_draws_follow_the_config():
    pm = PM.PitchModulator({"vibrato": {"p": 1, "depth_cents": [20, 20], "rate_hz": [5, 5]},
                            "glide": {"p": 1, "cents": [120, 120]}}, SR, 300)
    plan = pm.draw(4)
    assert plan.on.all()
    for mod in plan.mods:
        g = mod.row()
        assert g[0] == pytest.approx(2.0 ** (20 / 1200) - 1) and g[4] == pytest.approx(5.0) and 0 <= g[8] < 2 * np.pi
        assert np.all(g[1:4] == 0) and g[12] == pytest.approx((2.0 ** (120 / 1200) - 1) / 2)


# ------------------------------------------------------------------------------------------------------------ the cap
def _c_plan(lib, n, t0, t1, row, on=1, hop=32):
    arrs = [np.array([v], np.int64) for v in (n, 0, 0, t0, t1)]
    on = np.array([on], np.int32)
    row = np.ascontiguousarray(row, np.float64)
    meta = np.zeros((1, lib.pe_pitch_mod_plan_fields()), np.int64)
    params, totals = np.zeros((1, PM.PARAMS), np.float64), np.zeros(2, np.int64)
    ptrs = [a.ctypes.data for a in arrs + [on, row]]
    status = lib.pe_pitch_mod_plan(1, *ptrs, SR, hop, meta.ctypes.data, params.ctypes.data, totals.ctypes.data)
    return status, meta, params, totals


def test_the_cap_and_the_other_refusals(lib):
    at_cap = PM.Modulation(((0.125, 5.0, 0.0),), 0.25)
    PM.check_modulation(at_cap)
    assert _c_plan(lib, 4096, 0, 4096, at_cap.row())[0] == 0
    for bad in (PM.Modulation(((0.126, 5.0, 0.0),), 0.25), PM.Modulation((), -0.51),
                PM.Modulation(((0.1, 0.04, 0.0),), 0.0), PM.Modulation(((0.1, 5.0, float("inf")),), 0.0)):
        with pytest.raises(ValueError):
            PM.check_modulation(bad)
        assert _c_plan(lib, 4096, 0, 4096, bad.row())[0] == -1
        assert _c_plan(lib, 4096, 0, 4096, bad.row(), on=0)[0] == 0          # not selected: not read
    with pytest.raises(ValueError):
        PM.Modulation(((0.01, 5.0, 0.0),) * 5).row()
    with pytest.raises(ValueError):
        PM.check_modulation(at_cap, T=31, hop=32)
    ok = at_cap.row()
    assert _c_plan(lib, 4096, 0, 0, ok)[0] == -1                              # T < hop
    assert _c_plan(lib, 4096, 0, 48, ok)[0] == -1                             # not whole hops
    assert _c_plan(lib, 4096, 64, 4128, ok)[0] == -1                          # past the row
    for spans in ([[0, 16]], [[0, 48]], [[64, 4128]], [[-32, 32]]):
        with pytest.raises(ValueError):
            PM._plan([4096], [0], [0], spans, [at_cap], SR, 32, "test")
    with pytest.raises(ValueError):
        PM._plan([4096], [0], [0], [[0, 64]], [at_cap, at_cap], SR, 32, "test")


def test_the_plan_lays_out_tiles_and_parameters(lib):
    tile = PM.kernel_consts()["tile"]
    assert PM.kernel_consts() == dict(tile=tile, block=256, span=tile * 3 // 2 + 200, max_sinusoids=4)
    pl = PM._plan([0, 1, tile, tile + 1, 5000], [0, 0, 1, 9000, 20000], [0, 0, 1, 9000, 20000],
                  [[0, 0], [0, 0], [32, 1024], [0, 64], [0, 4992]],
                  [None, None, MIXED, PM.Modulation(), PM.Modulation((), 0.1)], SR, 32, "test")
    assert pl["tiles"] == 0 + 1 + 1 + 2 + 3 and pl["warped"] == 2 and pl["on"].tolist() == [0, 0, 1, 0, 1]
    T = 1024 - 32
    P = pl["params"][2]
    w = 2 * np.pi * 6.0 / SR
    assert P[0] == 0.03 and P[4] == pytest.approx(w, rel=1e-15) and P[8] == 0.7 and P[16] == 0.06 and P[18] == T
    assert P[12] == pytest.approx(np.cos(0.7), rel=1e-15)
    mbar = (0.03 * (np.cos(0.7) - np.cos(w * T + 0.7)) / w +
            0.005 * (np.cos(2.0) - np.cos(2 * np.pi * 13.0 / SR * T + 2.0)) / (2 * np.pi * 13.0 / SR)) / T
    assert P[17] == pytest.approx(mbar, rel=1e-13)
    assert not pl["params"][3].any() and pl["params"][4][18] == 4992


def test_entry_points_check_their_arguments_before_any_device_call(lib):
    """No GPU here: every refusal below is answered from the host copies alone."""
    buf = (ctypes.c_float * 8)()
    p, q = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast((ctypes.c_float * 8)(), ctypes.c_void_p)
    status, meta, params, _ = _c_plan(lib, 4096, 0, 4096, MIXED.row())
    assert status == 0
    m, P = meta.ctypes.data, params.ctypes.data
    assert lib.pe_pitch_mod_wave(p, p, m, p, P, 1, p, 2, 0, q, None) == -1          # not a quality
    assert lib.pe_pitch_mod_wave(p, p, m, p, P, 1, p, 0, 1, q, None) == -2          # kaiser_best does not fit in LDS
    assert lib.pe_pitch_mod_wave(p, p, None, p, P, 1, p, 1, 0, q, None) == -1
    assert lib.pe_pitch_mod_wave(p, p, m, p, None, 1, p, 1, 0, q, None) == -1       # a warped row needs its parameters
    assert lib.pe_pitch_mod_wave(p, p, m, p, P, 1, p, 1, 0, p, None) == -1          # in place
    assert lib.pe_pitch_mod_wave(None, p, m, p, P, 1, p, 1, 0, q, None) == -1
    assert lib.pe_pitch_mod_wave(p, p, m, p, P, 0, p, 1, 0, q, None) == 0           # no rows: nothing to do
    over = params.copy()
    over[0, 16] = 0.6                                                           # past the cap behind the plan's back
    assert lib.pe_pitch_mod_wave(p, p, m, p, over.ctypes.data, 1, p, 1, 0, q, None) == -1
    moved = meta.copy()
    moved[0, 4] = 5000                                                              # t1 past the row
    assert lib.pe_pitch_mod_wave(p, p, moved.ctypes.data, p, P, 1, p, 1, 0, q, None) == -1
    assert lib.pe_pitch_mod_labels(p, p, p, m, p, P, 1, 32, 64, q, q, None) == -1   # 129 frames do not fit 64
    assert lib.pe_pitch_mod_labels(p, p, p, m, p, P, 1, 64, 192, q, q, None) == -1  # another hop than the plan's
    assert lib.pe_pitch_mod_labels(p, p, p, m, p, P, 1, 32, 192, p, q, None) == -1  # in place
    assert lib.pe_pitch_mod_labels(None, p, p, m, p, P, 1, 32, 192, q, q, None) == -1
    assert lib.pe_pitch_mod_consts(None) == -1


def test_there_is_no_cpu_path():
    x = torch.zeros(4096)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PM.modulate(x, None, [[0, 4096]], [MIXED], sr=SR, hop=32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PM.modulate_labels(torch.zeros(1, 192), torch.zeros(1, 192), [129], [[0, 4096]], 32, [MIXED], sr=SR)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pm = PM.PitchModulator({"vibrato": {"p": 1}}, SR, 32)
        pm.apply(x.view(1, -1), [4096], [0], torch.zeros(1, 192), torch.zeros(1, 192), pm.draw(1))


def test_frame_spans():
    spans, counts = PM.frame_spans([0, 1, 31, 32, 6400, 9600, 100], [0, 0, 0, 0, 7, 0, 9], 32)
    assert counts.tolist() == [1, 1, 1, 2, 192, 192, 0]
    assert spans.tolist() == [[0, 0], [0, 0], [0, 0], [0, 32], [224, 224 + 191 * 32], [0, 191 * 32], [288, 288]]
    assert PM.frame_spans([6400], [9], 32)[0].tolist() == [[288, 6400]]          # t1 = n


# ------------------------------------------------------------------------------------------------------ audio and label
def test_audio_and_label_agree_on_the_restatement():
    """The consistency condition of the GPU test (tracked contour within a quarter of the distance between old and new
    labels), here on the restatement's output with the float64 tracker of tests/f0_track_ref.py: measured 0.55 cents
    against 65.8 cents."""
    c = R.CONSISTENCY
    x = R.complex_tone(c["f0"], c["sr"], c["n"])
    y = R.warp(x, 0, c["n"], c["mod"], c["sr"]).astype(np.float32)
    res = F.track(y, c["sr"], c["hop"], min_pitch=c["min_pitch"])
    L = 1 + c["n"] // c["hop"]
    new, flags = R.labels(np.full(L, c["f0"], np.float32), np.zeros(L, np.float32), L, c["mod"], c["hop"], c["sr"])
    to_new, old_to_new = R.consistency_scores(res["f0"], res["times"], new)
    print(f"rms cents: tracked vs new labels {to_new:.3f}, old vs new labels {old_to_new:.3f}")
    assert not flags.any() and to_new <= 0.25 * old_to_new
    plain = F.track(x, c["sr"], c["hop"], min_pitch=c["min_pitch"])
    assert R.rms_cents(plain["f0"], np.full(plain["f0"].size, c["f0"])) < 1.0      # the input does carry the old label
