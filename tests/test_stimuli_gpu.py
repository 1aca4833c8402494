"""The stimulus kernels (``csrc/stimuli.hip`` through ``pitchextractor_amd.stimuli``) on the device against the float64
restatement in tests/stimuli_ref.py, and the two sweeps of ``pitchextractor_amd.inference``.

Shapes: with S = 2048 the scan piece and fade = 480 at 24 kHz / 320 at 16 kHz, rows of n in {fade, 2 fade - 1, 2 fade,
S - 1, S, S + 1, 3 S + 5}; kinds rotate over them so that a glide, a vibrato, a constant tone, a given curve and a
5-partial tone with noise share every batch.  Each batch is made alone (one row per call), packed so that every row
starts at an odd offset, and padded; a row must come out bit-identical in the three.  Every figure is printed before it
is asserted."""
import math

import numpy as np
import pytest
import torch

from oracle import model_ref
from pitchextractor_amd import inference, stimuli as S, stress
from tests import stimuli_ref as R

pytestmark = pytest.mark.gpu

f32 = np.float32
GOLDEN = __import__("pathlib").Path(__file__).resolve().parent / "golden"
BELT = S.TIMBRE_PROFILES["Bright Belt"]["partials"]


def step32(a):
    """The float32 spacing at |a|."""
    return np.spacing(np.abs(np.asarray(a)).astype(f32)).astype(np.float64)


def host(t):
    return t.detach().cpu().numpy()


class Batch:
    """Row specs of one rate, their curve and noise tensors, and the restatement of every row."""

    def __init__(self, sr, device):
        fade = R.fade_samples(sr)
        self.sr, self.fade, self.device = sr, fade, device
        self.n = [fade, 2 * fade - 1, 2 * fade, R.PIECE - 1, R.PIECE, R.PIECE + 1, 3 * R.PIECE + 5]
        rng = np.random.default_rng(sr)
        self.specs, self.curve64, self.pre, self.noise, curves, noises = [], [], [], [], [], []
        for r, n in enumerate(self.n):
            duration = n / sr
            kind = ("glide", "vibrato", "constant", "curve", "tone")[r % 5]
            noise = None
            if kind == "glide":
                spec = dict(S.glide_row(duration, 60.0, 500.0, sr), n=n)
                curve = R.glide_curve(duration, 60.0, 500.0, sr, n)[1]
            elif kind == "vibrato":
                spec = dict(S.vibrato_row(6.0, 120.0, 220.0, duration, sr), n=n)
                curve = R.vibrato_curve(6.0, 120.0, 220.0, duration, sr, n)[1]
            elif kind == "constant":
                spec = S.curve_row(n, sr, 1.3, sum(c.size for c in curves), 1)           # the normalisation is taken
                curves.append(np.array([311.13], f32))
                curve = np.full(n, curves[-1][0], np.float64)
            elif kind == "curve":
                given = (200.0 + 150.0 * rng.random(n)).astype(f32)
                spec = S.curve_row(n, sr, 0.8, sum(c.size for c in curves), n)
                curves.append(given)
                curve = given.astype(np.float64)
            else:
                spec = dict(S.timbre_row(220.0, {"partials": BELT, "snr_db": 25.0}, duration, sr), n=n)
                curve = np.full(n, float(f32(220.0)))
                noise = rng.standard_normal(n).astype(f32)
                noises.append(noise)
            self.specs.append(spec)
            self.curve64.append(curve)
            self.noise.append(noise)
            self.pre.append(R.tone_prefade(220.0, sr, duration, BELT, n) if kind == "tone"
                            else R.prefade(curve, sr, spec["amplitude"]))
        self.kinds = [("glide", "vibrato", "constant", "curve", "tone")[r % 5] for r in range(len(self.n))]
        self.curves = torch.from_numpy(np.concatenate(curves + [np.zeros(1, f32)])).to(device)
        self.noise_d = torch.from_numpy(np.concatenate(noises)).to(device)
        self.final = [R.finish(p, sr, z, 25.0 if z is not None else None, return_stages=True)
                      for p, z in zip(self.pre, self.noise)]

    def layouts(self):
        """name -> list of (row indices, offsets, output size)."""
        odd, at = [], 1
        for n in self.n:
            odd.append(at)
            at += n + n % 2 + 2                            # keeps every start odd
        assert all(o % 2 == 1 for o in odd)
        width = max(self.n) + 3
        rows = list(range(len(self.n)))
        return {"alone": [([r], [0], self.n[r]) for r in rows], "packed": [(rows, odd, at)],
                "padded": [(rows, [r * width for r in rows], width * len(rows))]}

    def noise_for(self, rows):
        parts = [self.noise[r] for r in rows if self.noise[r] is not None]
        return torch.from_numpy(np.concatenate(parts)).to(self.device) if parts else None

    def frames(self, r, which):
        return 1 + self.n[r] // 300 if which == 0 else (97, 7)[r % 2]

    def run(self, groups, given_pre=False):
        """Every stage over the groups of one layout: per row ``dict(phase, pre, y, stats, ref0, ref1)`` as arrays."""
        out = {}
        for rows, offsets, size in groups:
            pl = S.plan_rows([self.specs[r] for r in rows], self.sr, offsets)
            y = torch.zeros(size, dtype=torch.float32, device=self.device)
            ph = S.phase(pl, self.curves, self.device)
            if given_pre:
                for r, o in zip(rows, offsets):
                    y[o:o + self.n[r]] = torch.from_numpy(self.pre[r]).to(self.device)
            else:
                S.synth(pl, ph, y)
                S.tone(pl, y)
            pre = host(y).copy()
            y, stats = S.finish(pl, y, self.noise_for(rows), return_stats=True)
            refs = [S.reference(pl, [self.frames(r, w) for r in rows], self.curves) for w in (0, 1)]
            yh, sh, phh, at = host(y), host(stats), host(ph), 0
            covered = np.zeros(size, bool)
            for i, (r, o) in enumerate(zip(rows, offsets)):
                n = self.n[r]
                covered[o:o + n] = True
                rec = dict(phase=phh[at:at + n], pre=pre[o:o + n], y=yh[o:o + n], stats=sh[i])
                for w, (ref, foff) in enumerate(refs):
                    rec[f"ref{w}"] = host(ref)[foff[i]:foff[i] + self.frames(r, w)]
                out[r] = rec
                at += n
            assert not yh[~covered].any()                  # nothing is written outside the rows
        return out


@pytest.fixture(scope="module", params=[24000, 16000])
def batch(request, hip_device):
    b = Batch(request.param, hip_device)
    b.results = {name: b.run(groups) for name, groups in b.layouts().items()}
    return b


def test_a_row_is_bit_identical_alone_packed_and_padded(batch):
    alone = batch.results["alone"]
    for name in ("packed", "padded"):
        for r, rec in batch.results[name].items():
            for key, a in rec.items():
                b = alone[r][key]
                if batch.kinds[r] == "tone" and key == "phase":
                    continue                                # a tone row has no phase
                same = np.array_equal(a.view(np.int64 if a.dtype == np.float64 else np.int32),
                                      b.view(np.int64 if b.dtype == np.float64 else np.int32))
                assert same, (batch.sr, name, r, batch.kinds[r], key)


def test_synthesis_against_the_restatement(batch):
    for r, rec in batch.results["packed"].items():
        kind, n, y = batch.kinds[r], batch.n[r], rec["y"].astype(np.float64)
        want = batch.final[r][0].astype(np.float64)
        if kind == "tone":
            # the partial sum: one float32 rounding flip, and a few double ulps of the device's sines
            pre_tol = step32(batch.pre[r]) + 2.0 ** -50 * sum(abs(a) for a in BELT.values())
            d = np.abs(rec["pre"].astype(np.float64) - batch.pre[r])
            share = float(np.mean(rec["pre"] != batch.pre[r]))
            print(f"[stimuli] sr {batch.sr} row {r} tone n {n}: pre-fade worst {d.max():.2e}, {share:.4f} differ")
            assert np.all(d <= pre_tol) and share <= 0.01
            continue
        amp = batch.specs[r]["amplitude"]
        phi = R.phase_of(batch.curve64[r], batch.sr)
        dphi = float(np.max(np.abs(rec["phase"] - phi)))
        scale = 1.0 / (batch.final[r][1]["peak"] + 1e-6) if batch.final[r][1]["peak"] > 0.99 else 1.0
        tol = 2 * step32(want) + scale * amp * 2 * n * 2.0 ** -53 * float(phi[-1])
        d = np.abs(y - want)
        share = float(np.mean(rec["y"] != batch.final[r][0]))
        print(f"[stimuli] sr {batch.sr} row {r} {kind} n {n}: phase vs cumsum {dphi:.2e} rad, audio worst {d.max():.2e} "
              f"(bound at the peak {tol.max():.2e}), {share:.4f} of samples differ")
        assert dphi <= 2 * n * 2.0 ** -53 * float(phi[-1])
        assert np.all(d <= tol) and share <= 0.01


def test_finish_on_the_restatements_samples(batch):
    given = batch.run(batch.layouts()["packed"], given_pre=True)
    for r, rec in given.items():
        want, stats, faded, mixed = batch.final[r]
        got = dict(zip(S.STAT_KEYS, (float(v) for v in rec["stats"])))
        print(f"[stimuli] sr {batch.sr} row {r} {batch.kinds[r]}: device {got} restatement {stats}")
        for key in S.STAT_KEYS:
            assert f32(got[key]) == f32(stats[key]), key
        n, fade = batch.n[r], batch.fade
        inner = np.zeros(n, bool)
        inner[fade:n - fade] = True
        y = rec["y"]
        assert np.array_equal(y[inner], want[inner])                 # the mix and the division, bit for bit
        d = np.abs(y.astype(np.float64) - want)
        if stats["scale"] == 0.0 and stats["peak"] <= 0.99:
            tol = step32(want)                                        # the fade product alone: one float32 step
        else:                                                         # that step carried through the mix and the division
            div = stats["peak"] + 1e-6 if stats["peak"] > 0.99 else 1.0
            tol = step32(np.maximum(np.abs(faded), np.abs(mixed))) / div + step32(want)
        share = float(np.mean(y[~inner] != want[~inner])) if n > 0 else 0.0
        print(f"[stimuli]   fade region: worst {d[~inner].max():.2e}, {share:.4f} of its samples differ")
        assert np.all(d[~inner] <= tol[~inner])
        if stats["scale"] == 0.0:                                     # the ramps start at 0; below 2 fade the tail
            assert y[n - 1] == 0.0 and (y[0] == 0.0 or n < 2 * fade)   # ramp overwrites the head's
    assert any(batch.final[r][1]["peak"] > 0.99 for r in given) and any(batch.final[r][1]["scale"] for r in given)


def test_reference_at_frame_rate(batch):
    frames = 0
    for r, rec in batch.results["padded"].items():
        n, kind = batch.n[r], batch.kinds[r]
        c32 = batch.curve64[r].astype(f32)
        for w in (0, 1):
            nf = batch.frames(r, w)
            want = R.sample_reference(n, batch.specs[r]["duration"] / n, lambda j: c32[j], nf)
            t32 = (np.arange(n) * (batch.specs[r]["duration"] / n)).astype(f32)
            assert np.array_equal(want, R.sample_reference_arrays(t32, c32, nf))
            got = rec[f"ref{w}"]
            frames += nf
            if kind == "vibrato":                                   # the device's sin / exp2 against NumPy's last bit
                assert np.all(np.abs(got.astype(np.float64) - want) <= step32(want)), (batch.sr, r, nf)
            else:
                assert np.array_equal(got, want), (batch.sr, r, kind, nf)
    print(f"[stimuli] sr {batch.sr}: {frames} reference frames")


def test_dynamic_metrics_on_the_device(hip_device):
    g = np.load(GOLDEN / "stimuli_metrics.npz")
    refs = [g[f"ref_{k}"] for k in range(int(g["n_cases"]))]
    preds = [g[f"pred_{k}"] for k in range(int(g["n_cases"]))]
    rng = np.random.default_rng(12)
    long_ref = R.shifted_vibrato_track(0, frames=700)               # more lags than one pass of the workgroup
    refs += [long_ref, np.zeros(0, f32), np.full(40, 220.0, f32)]
    preds += [(R.shifted_vibrato_track(5, frames=700) * (1 + 1e-3 * rng.standard_normal(700))).astype(f32),
              np.zeros(0, f32), np.full(40, 220.0, f32)]
    got = S.dynamic_metrics_rows(preds, refs, hip_device)
    alone = [S.dynamic_metrics_rows([p], [r], hip_device)[0] for p, r in zip(preds, refs)]
    for k, (ref, pred, rec) in enumerate(zip(refs, preds, got)):
        want = R.dynamic_metrics(ref, pred)
        print(f"[stimuli] metrics row {k}: device {rec} restatement {want}")
        assert all(rec[key] == alone[k][key] or (math.isnan(rec[key]) and math.isnan(alone[k][key])) for key in rec)
        for key, rel in (("RMSE_cents", 1e-6), ("Overshoot_cents", 1e-9), ("Final_error_cents", 1e-9)):
            if math.isnan(want[key]):
                assert math.isnan(rec[key]), (k, key)
            else:
                assert abs(rec[key] - want[key]) <= rel * abs(want[key]), (k, key)
        if math.isnan(want["Lag_frames"]):
            assert math.isnan(rec["Lag_frames"])
        else:
            margin = R.lag_margin(ref, pred)
            assert margin >= 1e-3 and rec["Lag_frames"] == want["Lag_frames"], (k, margin)
    assert [rec["Lag_frames"] for rec in got[:4]] == [0.0, 3.0, -2.0, 0.0] and got[7]["Lag_frames"] == 5.0
    assert all(math.isnan(v) for v in got[8].values()) and math.isnan(got[9]["Lag_frames"])


def test_builders_return_one_ragged_device_batch(hip_device):
    sr = 24000
    st = S.glides([0.05, 0.1], 60.0, 500.0, sr, device=hip_device)
    assert st.audio.is_cuda and st.audio.dtype == torch.float32 and st.lengths == [1200, 2400] and len(st) == 2
    for k, wave in enumerate(st.rows()):
        t, curve = R.glide_curve((0.05, 0.1)[k], 60.0, 500.0, sr)
        want = R.synthesize_from_f0_curve(curve, sr)
        assert np.all(np.abs(host(wave).astype(np.float64) - want) <= 2 * step32(want) + 1e-9)
    vib = S.vibratos([4.0, 6.0], [20.0, 60.0], 220.0, 0.1, sr, device=hip_device)
    assert [(v["rate_hz"], v["depth_cents"]) for v in vib.labels] == [(4.0, 20.0), (4.0, 60.0), (6.0, 20.0), (6.0, 60.0)]
    tn = S.tones([110.0, 440.0], 0.1, sr, amplitude=0.5, device=hip_device)
    for f, wave in zip((110.0, 440.0), tn.rows()):
        want = R.finish(R.prefade(np.full(2400, f32(f)), sr, 0.5), sr)[0]
        assert np.all(np.abs(host(wave).astype(np.float64) - want) <= 2 * step32(want) + 1e-9)
    given = torch.from_numpy(np.linspace(100.0, 300.0, 3000).astype(f32)).to(hip_device)
    fc = S.from_f0_curves(given, [1000, 2000], sr)
    assert fc.lengths == [1000, 2000]
    refs = fc.reference_f0([5, 9])
    assert [int(r.numel()) for r in refs] == [5, 9] and float(refs[1][0]) == float(given[1000])
    # the timbre set: the notebook's order and its noise, drawn on the host and uploaded once
    tt = S.timbre_tones([220.0, 330.0], duration=0.1, sr=sr, seed=7, device=hip_device)
    assert [v["timbre"] for v in tt.labels] == list(S.TIMBRE_PROFILES) * 2 and len(tt) == 8
    rng = np.random.default_rng(7)
    stats = host(tt.stats)
    for k, (label, wave) in enumerate(zip(tt.labels, tt.rows())):
        profile = S.TIMBRE_PROFILES[label["timbre"]]
        noise = rng.standard_normal(2400).astype(f32) if "snr_db" in profile else None
        want, ws = R.timbre_waveform(label["frequency_hz"], sr, 0.1, profile, noise)
        assert f32(stats[k][0]) == f32(ws["peak"]) and f32(stats[k][3]) == f32(ws["scale"]), (k, stats[k], ws)
        d = np.abs(host(wave).astype(np.float64) - want)
        print(f"[stimuli] timbre row {k} {label['timbre']}: peak {stats[k][0]:.4f} scale {stats[k][3]:.6g} worst {d.max():.2e}")
        assert np.all(d <= 3 * step32(want) + 1e-9)
    dev = S.timbre_tones([220.0], duration=0.1, sr=sr, seed=7, noise="device", device=hip_device)
    again = S.timbre_tones([220.0], duration=0.1, sr=sr, seed=7, noise="device", device=hip_device)
    assert torch.equal(dev.audio, again.audio) and not torch.equal(dev.rows()[3], tt.rows()[3])
    items = list(st.items())
    assert items[0]["audio"].data_ptr() == st.audio.data_ptr() and int(items[1]["reference_f0"].numel()) == 9


# ------------------------------------------------------------------------------------------------------------ sweeps
@pytest.fixture(scope="module")
def net(tmp_path_factory, hip_device):
    path = tmp_path_factory.mktemp("stimuli") / "r.pth"
    torch.save({"model": model_ref.seeded_state(31, hidden_size=64, num_layers=2)}, path)
    return inference.load_model(path, device=hip_device)


def _same(a, b):
    return a == b or (isinstance(a, float) and math.isnan(a) and math.isnan(b))


def _spy(monkeypatch):
    """Records every set a builder returns and every batch handed to ``predict_f0_batch``."""
    built, fed = [], []
    for name in ("glides", "vibratos", "timbre_tones"):
        def wrapped(*a, _f=getattr(S, name), **k):
            built.append(_f(*a, **k))
            return built[-1]
        monkeypatch.setattr(S, name, wrapped)
    real = inference.predict_f0_batch

    def predict(model, waves, lengths=None, **k):
        fed.append((waves, list(lengths), k))
        return real(model, waves, lengths, **k)
    monkeypatch.setattr(inference, "predict_f0_batch", predict)
    return built, fed, real


def test_dynamic_pitch_sweep(net, hip_device, monkeypatch):
    built, fed, predict = _spy(monkeypatch)
    vib = {"duration_seconds": 0.3, "rates_hz": [4.0, 6.0], "depth_cents": [60]}
    gl = {"durations_seconds": [0.25, 0.4]}
    out = inference.dynamic_pitch_sweep(net, vibrato=vib, glide=gl)
    assert [list(r) for r in out["vibrato"]] == [["rate_hz", "depth_cents", "RPA", "RCA", "VUV", "OctaveError",
                                                  "RMSE_cents"]] * 2
    assert [list(r) for r in out["glide"]] == [["duration_s", "RPA", "RCA", "VUV", "OctaveError", "RMSE_cents", "Lag_ms",
                                                "Overshoot_cents", "Final_error_cents"]] * 2
    assert [(r["rate_hz"], r["depth_cents"]) for r in out["vibrato"]] == [(4.0, 60.0), (6.0, 60.0)]
    assert [r["duration_s"] for r in out["glide"]] == [0.25, 0.4]
    # one call per set, on the builder's own device tensor, stitched the notebooks' way
    assert len(built) == 2 and len(fed) == 2
    for st, (waves, lengths, kw) in zip(built, fed):
        assert waves is st.audio and waves.is_cuda and lengths == st.lengths and kw["stitch"] == "concat"
    for st, records, dynamic in zip(built, (out["vibrato"], out["glide"]), (False, True)):
        preds = predict(net, st.audio, st.lengths, stitch="concat")
        refs = st.reference_f0([int(p.numel()) for p in preds])
        for k, rec in enumerate(records):
            p, f = host(preds[k]), host(refs[k])
            want = inference.melody_metrics(preds[k], refs[k])
            assert all(_same(rec[key], want[key]) for key in ("RPA", "RCA", "VUV", "OctaveError"))
            dm = R.dynamic_metrics(f, p)
            assert abs(rec["RMSE_cents"] - dm["RMSE_cents"]) <= 1e-6 * abs(dm["RMSE_cents"])
            if dynamic:
                for key in ("Overshoot_cents", "Final_error_cents"):
                    assert _same(rec[key], dm[key]) or abs(rec[key] - dm[key]) <= 1e-9 * abs(dm[key])
                margin = R.lag_margin(f, p) if not math.isnan(dm["Lag_frames"]) else 0.0
                print(f"[stimuli] glide {rec['duration_s']} s: {rec}; lag margin {margin:.3g}")
                if math.isnan(dm["Lag_frames"]):
                    assert math.isnan(rec["Lag_ms"])
                elif margin >= 1e-3:
                    assert rec["Lag_ms"] == dm["Lag_frames"] * 300 * 1000.0 / 24000
    centre = inference.dynamic_pitch_sweep(net, vibrato=vib, glide=gl, stitch="center")
    assert fed[-1][2]["stitch"] == "center" and len(centre["glide"]) == 2


def test_timbre_coverage_sweep(net, hip_device, monkeypatch):
    built, fed, predict = _spy(monkeypatch)
    ranges = [{"name": "Bass", "min_hz": 70.0, "max_hz": 120.0}, {"name": "Alto", "min_hz": 220.0, "max_hz": 350.0}]
    profiles = {k: S.TIMBRE_PROFILES[k] for k in ("Warm Vocal", "Breathy Head")}
    out = inference.timbre_coverage_sweep(net, ranges=ranges, profiles=profiles, duration=0.25,
                                          frequencies_per_range=2)
    records = out["records"]
    assert [list(r) for r in records] == [["range", "frequency_hz", "timbre", "edge_region", "RPA", "RCA", "VUV",
                                           "OctaveError"]] * 8
    assert [(r["range"], r["frequency_hz"], r["timbre"], r["edge_region"]) for r in records] == [
        (rg["name"], f, t, e) for rg in ranges for f, e in ((rg["min_hz"], "low"), (rg["max_hz"], "high"))
        for t in profiles]
    assert len(built) == 1 and len(fed) == 1 and fed[0][0] is built[0].audio and fed[0][2]["stitch"] == "concat"
    st = built[0]
    preds = predict(net, st.audio, st.lengths, stitch="concat")
    refs = st.reference_f0([int(p.numel()) for p in preds])
    for k, rec in enumerate(records):
        want = inference.melody_metrics(preds[k], refs[k])
        assert all(_same(rec[key], want[key]) for key in ("RPA", "RCA", "VUV", "OctaveError"))
        assert np.all(host(refs[k]) == f32(rec["frequency_hz"]))
    assert list(out["per_range"]) == ["Bass", "Alto"]
    for name, means in out["per_range"].items():
        assert list(means) == ["RPA_mean", "RCA_mean", "VUV_mean", "OctaveError_mean"]
        vuv = [r["VUV"] for r in records if r["range"] == name]
        assert means["VUV_mean"] == float(np.mean(vuv))


def test_a_stimulus_set_feeds_the_stress_sweep(net, hip_device):
    st = S.tones([110.0, 220.0], 0.5, 24000, amplitude=0.5, device=hip_device)
    conditions = [stress.Condition("clipping", "clip 0 %", percent=0.0)]
    out = inference.stress_sweep(net, st.items(), conditions, batched=True)
    assert len(out["baseline"]) == 2 and len(out["conditions"]) == 2
    for rec, clean in zip(out["conditions"], out["baseline"]):
        assert rec["n_frames"] == 41 and all(_same(rec[k], clean[k]) for k in stress.METRIC_KEYS)
