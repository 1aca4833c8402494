"""The stimulus restatement (tests/stimuli_ref.py) against arrays captured from the reference's own functions
(tests/golden/stimuli_*.npz, written by tests/golden/make_stimuli_golden.py), and the host side of
``pitchextractor_amd.stimuli`` (no GPU needed).  Every figure is printed before it is asserted."""
import ctypes
import math

import numpy as np
import pytest

from tests import stimuli_ref as R

GOLDEN = __import__("pathlib").Path(__file__).resolve().parent / "golden"
f32 = np.float32


@pytest.fixture(scope="module")
def dyn():
    return np.load(GOLDEN / "stimuli_dynamic.npz")


def _frame_counts(g, prefix):
    return sorted(int(k.rsplit("_", 1)[1]) for k in g.files if k.startswith(prefix + "_ref_"))


# ----------------------------------------------------------------------------------------- synthesis, bit for bit
def test_glides_are_the_references_bit_for_bit(dyn):
    frames = 0
    for k, (duration, start, end, sr) in enumerate(dyn["glides"]):
        sr = int(sr)
        t, curve = R.glide_curve(duration, start, end, sr)
        assert np.array_equal(t.astype(f32), dyn[f"glide_{k}_t"]) and np.array_equal(curve.astype(f32), dyn[f"glide_{k}_curve"])
        assert curve[-1] == end and curve[0] == start
        assert np.array_equal(R.synthesize_from_f0_curve(curve, sr), dyn[f"glide_{k}_audio"])
        n, tstep = t.size, duration / t.size
        assert np.array_equal((np.arange(n) * tstep).astype(f32), dyn[f"glide_{k}_t"])      # the kernels' time axis
        c32 = curve.astype(f32)
        for nf in _frame_counts(dyn, f"glide_{k}"):
            want = dyn[f"glide_{k}_ref_{nf}"]
            assert np.array_equal(R.sample_reference_arrays(t.astype(f32), c32, nf), want)
            assert np.array_equal(R.sample_reference(n, tstep, lambda j: c32[j], nf), want)
            frames += nf
    print(f"[stimuli] glides: {frames} reference frames bit for bit")


def test_vibrato_is_the_references_bit_for_bit(dyn):
    for k, (rate, depth, base, duration, sr) in enumerate(dyn["vibratos"]):
        sr = int(sr)
        t, curve = R.vibrato_curve(rate, depth, base, duration, sr)
        assert np.array_equal(t.astype(f32), dyn[f"vibrato_{k}_t"])
        assert np.array_equal(curve.astype(f32), dyn[f"vibrato_{k}_curve"])
        assert np.array_equal(R.synthesize_from_f0_curve(curve, sr), dyn[f"vibrato_{k}_audio"])
        c32 = curve.astype(f32)
        for nf in _frame_counts(dyn, f"vibrato_{k}"):
            assert np.array_equal(R.sample_reference(t.size, duration / t.size, lambda j: c32[j], nf),
                                  dyn[f"vibrato_{k}_ref_{nf}"])


def test_constant_tones_and_the_normalisation_branch(dyn):
    taken = []
    for k, (freq, duration, sr, amplitude) in enumerate(dyn["tones"]):
        sr = int(sr)
        curve = np.full(int(duration * sr), freq, dtype=f32)
        y, stats = R.finish(R.prefade(curve, sr, amplitude), sr)
        assert np.array_equal(y, dyn[f"tone_{k}_audio"])
        taken.append(stats["peak"] > 0.99)
    assert taken == [False, True]


def test_fade_overlap_and_short_rows():
    w = R.fade_window(480, 480)
    ramp = 0.5 - 0.5 * np.cos(np.linspace(0.0, np.pi, 480))
    assert np.array_equal(w, ramp[::-1])                          # n == fade: the tail ramp overwrites all of it
    w = R.fade_window(700, 480)
    assert np.array_equal(w[:220], ramp[:220]) and np.array_equal(w[220:], ramp[::-1])
    assert np.array_equal(R.fade_window(5, 0), np.ones(5))
    with pytest.raises(ValueError):
        R.fade_window(479, 480)
    assert R.fade_samples(24000) == 480 and R.fade_samples(16000) == 320


def test_blocked_scan_differs_from_the_sequential_sum_by_rounding_only():
    t, curve = R.glide_curve(3.2, 60.0, 500.0, 24000)
    seq, blk = R.phase_of(curve, 24000), R.phase_of(curve, 24000, blocked=R.PIECE)
    d = float(np.max(np.abs(seq - blk)))
    n = curve.size
    bound = 2 * n * 2.0 ** -53 * float(seq[-1])
    flips = int(np.count_nonzero(R.prefade(curve, 24000) != R.prefade(curve, 24000, blocked=R.PIECE)))
    print(f"[stimuli] 3.2 s glide: blocked vs sequential phase {d:.2e} rad (bound {bound:.2e}), {flips} of {n} samples differ")
    assert d <= bound and flips <= n // 100


# ------------------------------------------------------------------------------------------------------------- timbre
def test_timbre_tones_against_the_notebooks_function():
    from pitchextractor_amd.stimuli import TIMBRE_PROFILES
    g = np.load(GOLDEN / "stimuli_timbre.npz")
    branch = set()
    for k, (freq, duration, sr) in enumerate(g["rows"]):
        sr = int(sr)
        for j, (name, profile) in enumerate(TIMBRE_PROFILES.items()):
            want = g[f"audio_{k}_{j}"]
            noise = g[f"noise_{k}_{j}"] if f"noise_{k}_{j}" in g.files else None
            y, stats = R.timbre_waveform(freq, sr, duration, profile, noise)
            branch.add(stats["peak"] > 0.99)
            # the reference takes the rms by float32 pairwise sums, so `scale` may differ by one float32 step:
            # 2^-23 |noise scale| <= 2^-22 |noise| on top of one rounding of the sum
            tol = np.spacing(np.abs(want)) + (2.0 ** -22 * np.abs(noise) if noise is not None else 0.0)
            diff = np.abs(y.astype(np.float64) - want)
            share = float(np.mean(y != want))
            print(f"[stimuli] timbre {freq} Hz {sr} Hz {name}: peak {stats['peak']:.4f} scale {stats['scale']:.6g} "
                  f"differing samples {share:.4f} worst {float(diff.max()):.2e}")
            assert y.shape == want.shape and np.all(diff <= tol)
            if noise is None:
                assert share == 0.0
    assert branch == {True}                      # a fundamental of amplitude 1 always takes the normalisation


# ------------------------------------------------------------------------------------------------------------- metrics
def test_dynamic_metrics_against_the_references():
    g = np.load(GOLDEN / "stimuli_metrics.npz")
    period = float(g["period_ms"])
    lags = []
    for k in range(int(g["n_cases"])):
        ref, pred, want = g[f"ref_{k}"], g[f"pred_{k}"], g[f"out_{k}"]
        got = R.dynamic_metrics(ref, pred)
        print(f"[stimuli] metrics case {k}: {got} reference {want.tolist()}")
        # RMSE: the reference keeps cents in float32 (spacing 2.4e-4 at 4000 cents) and averages in float32
        if math.isnan(want[0]):
            assert math.isnan(got["RMSE_cents"])
        else:
            assert abs(got["RMSE_cents"] - want[0]) <= 1e-3 + 1e-5 * abs(want[0])
        if math.isnan(want[1]):
            assert math.isnan(got["Lag_frames"])
        else:
            margin = R.lag_margin(ref, pred)
            print(f"[stimuli]   lag margin {margin:.3f}")
            if k < 4:
                assert margin >= 1e-3
            if margin >= 1e-3:
                assert got["Lag_frames"] * period == want[1]
                lags.append(want[1])
        for key, w in (("Overshoot_cents", want[2]), ("Final_error_cents", want[3])):
            if math.isnan(w):
                assert math.isnan(got[key])
            else:
                # the reference evaluates the ratio and the logarithm in float32
                assert abs(got[key] - w) <= 1200.0 * 2.0 ** -23 / math.log(2.0) + 2 * float(np.spacing(f32(abs(w))))
    assert lags[:4] == [0.0, 37.5, -25.0, 0.0]                    # the delayed linear glide gives lag 0


def test_correlation_index_convention():
    rng = np.random.default_rng(0)
    ref, pred = rng.standard_normal(9), rng.standard_normal(9)
    c = np.correlate(pred, ref, mode="full")
    L = 9
    for k in range(2 * L - 1):
        s = sum(pred[n + k - (L - 1)] * ref[n] for n in range(L) if 0 <= n + k - (L - 1) < L)
        assert abs(s - c[k]) <= 1e-12


# ----------------------------------------------------------------------------------------------------- plan and checks
def test_plan_parameters_and_layout(dyn):
    from pitchextractor_amd import stimuli as S
    rows = [S.glide_row(0.3, 60.0, 500.0, 24000), S.vibrato_row(6.0, 60.0, 220.0, 0.3, 24000),
            S.curve_row(2049, 24000, 0.5, 3, 1), S.curve_row(480, 24000, 0.8, 10, 480),
            S.timbre_row(220.0, S.TIMBRE_PROFILES["Breathy Head"], 0.1, 24000, timbre="Breathy Head")]
    pl = S.plan_rows(rows, 24000)
    assert (pl["piece"], pl["fade"], pl["rows"]) == (R.PIECE, 480, 5)
    n = [7200, 7200, 2049, 480, 2400]
    assert pl["lengths"].tolist() == n and pl["n_samples"] == sum(n) and pl["n_noise"] == 2400
    m = pl["meta"]
    assert m[:, 0].tolist() == np.cumsum([0] + n[:-1]).tolist() and m[:, 1].tolist() == n
    assert m[:, 2].tolist() == [1, 2, 0, 0, 3] and m[:, 4].tolist() == [4, 4, 2, 1, 2]
    assert m[:, 5].tolist() == [0, 4, 8, 10, 11] and pl["n_pieces"] == 13
    assert m[:, 8].tolist() == [0, 0, 0, 0, 3] and m[:, 10].tolist() == [-1, -1, -1, -1, 0]
    p = pl["params"]
    assert p[0, :4].tolist() == [0.8, 60.0, (500.0 - 60.0) / 7199, 500.0] and p[0, 6] == 0.3 / 7200
    assert p[1, :4].tolist() == [0.8, 220.0, 60.0 / 1200.0, 2.0 * np.pi * 6.0]
    assert p[4, 8:14].tolist() == [1.0, 2.0 * math.pi * 220.0 * 1.0, 0.5, 2.0 * math.pi * 220.0 * 2.0, 0.35,
                                   2.0 * math.pi * 220.0 * 3.0] and p[4, 4] == 25.0
    # an odd layout keeps the pieces relative to the rows
    odd = S.plan_rows(rows, 24000, offsets=[1, 7300, 15001, 17051, 17600])
    assert np.array_equal(odd["meta"][:, 1:], m[:, 1:]) and odd["meta"][:, 0].tolist() == [1, 7300, 15001, 17051, 17600]
    assert S.plan_rows([], 24000)["rows"] == 0
    assert np.array_equal(S.frame_times(7200, 0.3 / 7200, 25), R.frame_times(7200, 0.3 / 7200, 25))


def test_plan_refusals():
    from pitchextractor_amd import stimuli as S
    with pytest.raises(ValueError, match="shorter than the fade"):
        S.plan_rows([S.glide_row(0.019, 60.0, 500.0, 24000)], 24000)
    S.plan_rows([S.glide_row(0.02, 60.0, 500.0, 24000)], 24000)                     # n == fade is the shortest row
    with pytest.raises(ValueError, match="at least one sample"):
        S.plan_rows([S.glide_row(1e-6, 60.0, 500.0, 24000)], 24000)
    with pytest.raises(ValueError, match="partials"):
        S.timbre_row(100.0, {"partials": {h: 1.0 for h in range(1, 18)}}, 0.1, 24000)
    assert len(S.timbre_row(100.0, {"partials": {**{h: 1.0 for h in range(1, 17)}, 17: 0.0}}, 0.1, 24000)["partials"]) == 16
    with pytest.raises(ValueError, match="envelope"):
        S.timbre_row(100.0, {"partials": {1: 1.0}, "envelope": lambda t: t}, 0.1, 24000)
    for bad in (0.0, -5.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            S.glide_row(0.1, bad, 500.0, 24000)
        with pytest.raises(ValueError):
            S.timbre_row(bad, S.TIMBRE_PROFILES["Pure Sine"], 0.1, 24000)
        with pytest.raises(ValueError):
            S.vibrato_row(6.0, 60.0, bad, 0.1, 24000)
    for sr in (0, -24000):
        with pytest.raises(ValueError):
            S.plan_rows([S.glide_row(0.1, 60.0, 500.0, 24000)], sr)
    with pytest.raises(ValueError):
        S.timbre_tones([220.0], noise="host")


def test_argument_checks_run_before_any_device_call():
    from pitchextractor_amd import _lib, stimuli as S
    lib = _lib.load()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    buf = p((ctypes.c_double * 64)())
    ARG, WS = -1, -3
    assert lib.pe_stim_plan_fields() == 11 and lib.pe_stim_param_fields() == 40 and lib.pe_dynamic_metrics_fields() == 3
    rows = [S.glide_row(0.1, 60.0, 500.0, 24000), S.curve_row(600, 24000, 0.8, 0, 1),
            S.timbre_row(220.0, S.TIMBRE_PROFILES["Breathy Head"], 0.1, 24000)]
    pl = S.plan_rows(rows, 24000)
    meta = pl["meta"].ctypes.data
    ws_bytes = lib.pe_stim_workspace_bytes(pl["n_pieces"])
    assert ws_bytes == pl["n_pieces"] * 24 and lib.pe_stim_workspace_bytes(0) == 0

    def broken(field, value, row=0):
        bad = pl["meta"].copy()
        bad[row, field] = value
        return bad

    # the C plan refuses what the Python layer refuses
    one = lambda t, v: p((t * 1)(v))  # noqa: E731
    raw = lambda *v: p((ctypes.c_double * 6)(*v))  # noqa: E731
    parts = p((ctypes.c_double * 32)(1.0, 1.0))
    L, I = ctypes.c_long, ctypes.c_int
    plan = lambda n=2400, kind=1, r=raw(0.8, 60.0, 500.0, 0.0, 0.1, 0.0), np_=0, sr=24000.0, clen=0: lib.pe_stim_plan(  # noqa: E731
        1, one(L, n), one(L, 0), one(I, kind), r, parts, one(I, np_), one(L, 0), one(L, clen), one(L, -1), sr, buf, buf,
        buf, buf)
    assert plan() == 0
    assert plan(n=0) == ARG and plan(n=479) == ARG and plan(n=480) == 0
    assert plan(sr=0.0) == ARG and plan(sr=math.nan) == ARG and plan(kind=4) == ARG
    assert plan(r=raw(0.8, 0.0, 500.0, 0.0, 0.1, 0.0)) == ARG and plan(r=raw(0.8, 60.0, math.inf, 0.0, 0.1, 0.0)) == ARG
    assert plan(r=raw(math.nan, 60.0, 500.0, 0.0, 0.1, 0.0)) == ARG
    assert plan(kind=3, np_=17) == ARG and plan(kind=3, np_=0) == ARG and plan(kind=3, np_=1) == 0
    assert plan(kind=0, clen=7) == ARG and plan(kind=0, clen=1) == 0 and plan(kind=0, clen=2400) == 0
    assert lib.pe_stim_plan(1, None, None, None, None, None, None, None, None, None, 24000.0, buf, buf, buf, buf) == ARG
    # every stage: a plan that is not pe_stim_plan's, null pointers, the workspace
    for bad in (broken(4, 9), broken(1, 0), broken(1, 100), broken(2, 7), broken(3, 5, row=1), broken(8, 17, row=2),
                broken(7, 5, row=1)):
        b = bad.ctypes.data
        assert lib.pe_stim_phase(buf, b, buf, buf, 3, buf, buf, ws_bytes, None) == ARG
        assert lib.pe_stim_synth(buf, b, buf, buf, 3, buf, None) == ARG
        assert lib.pe_stim_tone(buf, b, buf, 3, buf, None) == ARG
        assert lib.pe_stim_finish(buf, b, buf, buf, 3, buf, buf, buf, ws_bytes, None) == ARG
        assert lib.pe_stim_reference(buf, b, buf, buf, buf, buf, buf, 3, buf, None) == ARG
    assert lib.pe_stim_phase(buf, meta, buf, None, 3, buf, buf, ws_bytes, None) == ARG          # a curve row, no curves
    assert lib.pe_stim_phase(None, meta, buf, buf, 3, buf, buf, ws_bytes, None) == ARG
    assert lib.pe_stim_phase(buf, meta, buf, buf, 3, buf, None, 0, None) == WS
    assert lib.pe_stim_phase(buf, meta, buf, buf, 3, buf, buf, ws_bytes - 1, None) == WS
    assert lib.pe_stim_phase(buf, None, buf, buf, 3, buf, buf, ws_bytes, None) == ARG
    assert lib.pe_stim_phase(buf, meta, buf, buf, -1, buf, buf, ws_bytes, None) == ARG
    assert lib.pe_stim_synth(buf, meta, buf, None, 3, buf, None) == ARG
    assert lib.pe_stim_tone(buf, meta, buf, 3, None, None) == ARG
    assert lib.pe_stim_finish(buf, meta, buf, None, 3, buf, buf, buf, ws_bytes, None) == ARG    # a noise row, no noise
    assert lib.pe_stim_finish(buf, meta, buf, buf, 3, buf, None, buf, ws_bytes, None) == ARG
    assert lib.pe_stim_finish(buf, meta, buf, buf, 3, buf, buf, buf, 8, None) == WS
    table = (ctypes.c_long * 6)(0, 5, 5, 0, 5, 9)
    assert lib.pe_stim_reference(buf, meta, buf, buf, buf, None, buf, 3, buf, None) == ARG
    assert lib.pe_stim_reference(buf, meta, buf, buf, buf, p((ctypes.c_long * 6)(0, 5, 4, 0, 5, 9)), buf, 3, buf,
                                 None) == ARG
    assert lib.pe_stim_reference(buf, meta, buf, buf, buf, p((ctypes.c_long * 6)(0, -1, 0, 0, 0, 0)), buf, 3, buf,
                                 None) == ARG
    assert lib.pe_stim_reference(buf, meta, buf, buf, buf, p(table), None, 3, buf, None) == ARG
    # metrics
    tracks = (ctypes.c_long * 3)(0, 10, 0)
    assert lib.pe_dynamic_metrics(buf, buf, buf, None, 1, buf, None) == ARG
    assert lib.pe_dynamic_metrics(buf, buf, buf, p((ctypes.c_long * 3)(0, -1, 0)), 1, buf, None) == ARG
    assert lib.pe_dynamic_metrics(None, buf, buf, p(tracks), 1, buf, None) == ARG
    assert lib.pe_dynamic_metrics(buf, buf, buf, p(tracks), 1, None, None) == ARG
    # nothing to do is not an error, and needs no pointer
    assert lib.pe_stim_phase(None, None, None, None, 0, None, None, 0, None) == 0
    assert lib.pe_stim_finish(None, None, None, None, 0, None, None, None, 0, None) == 0
    assert lib.pe_stim_reference(buf, meta, buf, buf, None, p((ctypes.c_long * 6)(0, 0, 0, 0, 0, 0)), None, 3, None,
                                 None) == 0
    assert lib.pe_dynamic_metrics(None, None, None, None, 0, None, None) == 0


def test_host_tensors_are_refused():
    import torch
    from pitchextractor_amd import inference, stimuli as S
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.from_f0_curves(torch.full((4800,), 220.0), sr=24000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.from_f0_curves(np.full(4800, 220.0, f32), sr=24000)
    pl = S.plan_rows([S.glide_row(0.1, 60.0, 500.0, 24000)], 24000)
    pl["meta_d"] = pl["params_d"] = torch.zeros(1)                 # never reached
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.synth(pl, torch.zeros(2400, dtype=torch.float64), torch.zeros(2400))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.finish(pl, torch.zeros(2400))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.tone(pl, np.zeros(2400, f32))
    assert callable(inference.dynamic_pitch_sweep) and callable(inference.timbre_coverage_sweep)
    assert list(S.TIMBRE_PROFILES) == ["Pure Sine", "Warm Vocal", "Bright Belt", "Breathy Head"]
    assert [r["name"] for r in S.VOCAL_RANGES] == ["Bass", "Baritone/Tenor", "Alto", "Child/Falsetto"]
    assert [S.edge_region(f, 70.0, 120.0, 0.15) for f in (70.0, 77.5, 77.6, 112.4, 112.5, 120.0)] == \
        ["low", "low", "mid", "mid", "high", "high"]
