"""The codec conditions without a GPU: the properties of the restatement in tests/codec_ref.py
and the host side of ``pitchextractor_amd/codec.py`` (band tables, the row plan, every refusal, ``CodecCondition``),
none of which reaches the device."""
import numpy as np
import pytest

from pitchextractor_amd import _lib, codec, stress
from tests import codec_ref as R

f32 = np.float32


# ------------------------------------------------------------------------------------------------- restatement properties
@pytest.mark.parametrize("M", R.FRAMES)
def test_perfect_reconstruction_without_the_quantiser(M):
    """Rows that end inside the first frame, on a frame edge and inside a later frame; float64 rounding only."""
    rng = np.random.default_rng(M)
    worst = 0.0
    for n in (1, M - 1, M, M + 1, 3 * M + 7):
        x = rng.standard_normal(n)
        y, _, _ = R.codec(x, 24000, 64, M, bypass=True)
        assert y.shape == x.shape
        worst = max(worst, float(np.max(np.abs(y - x))))
    print(f"M {M}: largest reconstruction error {worst:.3e}")
    assert worst < 1e-11                                   # 2M-term float64 sums of O(1) terms, twice


def _test_frames(M, seed=0):
    """Coefficient frames with band levels spread over 2^-40 .. 2^10, two zeroed bands and a frame of tiny values."""
    rng = np.random.default_rng(seed)
    e = R.band_edges(M)
    X = rng.standard_normal((4, M))
    for f in range(3):
        for b in range(len(e) - 1):
            X[f, e[b]:e[b + 1]] *= 2.0 ** rng.uniform(-40, 10)
    X[1, e[3]:e[4]] = 0
    X[1, e[7]:e[8]] = 0
    X[3] *= 2.0 ** -110
    return X.astype(f32)


@pytest.mark.parametrize("M, k_c", [(256, 256), (256, 85), (1024, 700)])
def test_cost_does_not_increase_with_the_gain(M, k_c):
    """What the bisection stands on, over all 256 g."""
    for X in _test_frames(M)[:3]:
        bits = [R.quantize_at(X, M, k_c, g)[2] for g in range(R.G_MAX + 1)]
        assert all(a >= b for a, b in zip(bits, bits[1:]))
        assert bits[-1] >= 8 + R.bands_below(M, k_c)


@pytest.mark.parametrize("M", [256, 1024])
def test_budget_and_cutoff_hold_in_every_frame(M):
    X = _test_frames(M, 1)
    for k_c in (17, M // 3, M):
        floor = 8 + R.bands_below(M, k_c)
        for budget in (floor, 3 * floor, 20 * floor, 100000):
            q, g, bits, deq = R.quantize_frames(X, M, k_c, budget)
            assert np.all(bits <= budget) and np.all(bits >= floor)
            assert np.all(q[:, k_c:] == 0) and np.all(deq[:, k_c:] == 0)
            assert np.all((g >= 0) & (g <= R.G_MAX))
            for f in range(len(X)):                        # g is the smallest gain that fits
                assert R.quantize_at(X[f], M, k_c, int(g[f]))[2] == bits[f] or g[f] == R.G_MAX
                if g[f] > 0:
                    assert R.quantize_at(X[f], M, k_c, int(g[f]) - 1)[2] > budget
            if budget == floor:
                assert np.all(q == 0)
            if budget == 100000:
                assert np.all(g == 0)
    assert R.quantize_frames(np.zeros((1, M), f32), M, M, 100)[1][0] == 0       # an all-zero frame costs its floor


def test_scale_index_is_the_floor_of_four_log2():
    rng = np.random.default_rng(3)
    a = (2.0 ** rng.uniform(-100, 60, 4000)).astype(f32)
    a = np.concatenate([a, (2.0 ** (np.arange(-400, 240) / 4.0)).astype(f32), f32([2.0 ** -100, 1.0, 0.5])])
    for v in a:
        s = R.scale_index(v)
        # float32(2^(s / 4)) <= v < float32(2^((s + 1) / 4)): the floor as the float32 constants define it
        assert f32(2.0 ** (s / 4.0)) <= v < f32(2.0 ** ((s + 1) / 4.0)), (v, s)


def test_snr_rises_with_the_bitrate():
    """A fixed 1 s vibrato harmonic complex at 24 kHz, M = 1024."""
    x = R.vibrato_complex()
    snr = []
    for kbps in (8, 16, 32, 64, 128):
        y, g, bits = R.codec(x, 24000, kbps, 1024)
        assert np.all(bits <= R.budget_bits(24000, 1024, kbps))
        snr.append(10 * np.log10(np.sum(x.astype(np.float64) ** 2) / np.sum((y - x) ** 2)))
    print("SNR at 8 / 16 / 32 / 64 / 128 kbps:", " / ".join(f"{s:.1f}" for s in snr), "dB")
    assert all(a < b for a, b in zip(snr, snr[1:]))


def test_mulaw_against_its_brute_force_table():
    p = np.arange(-32768, 32768)
    y = R.mulaw((p / 32768.0).astype(f32))
    assert np.array_equal(np.rint(y.astype(np.float64) * 32768).astype(np.int64), R.mulaw_table())
    assert R.mulaw(f32([1.0]))[0] == f32(32124 / 32768) and abs(float(R.mulaw(f32([1.0]))[0]) - 0.98034668) < 1e-8
    assert np.array_equal(R.mulaw(f32([3.0, -3.0, 0.0])), f32([32124, -32124, 0]) / f32(32768))
    t = np.arange(8000) / 8000.0
    s = (0.5 * np.sin(2 * np.pi * 440.0 * t)).astype(f32)
    err = R.mulaw(s).astype(np.float64) - s
    snr = 10 * np.log10(np.sum(s.astype(np.float64) ** 2) / np.sum(err ** 2))
    print(f"mu-law on a half-scale sine: {snr:.1f} dB")
    assert 35.0 < snr < 39.0                               # G.711's flat 36 to 38 dB over its upper segments


# ------------------------------------------------------------------------------------------------------------ host logic
def test_band_tables():
    for M, bands in ((256, 29), (512, 35), (1024, 41)):
        e = codec.band_edges(M)
        assert np.array_equal(e, R.band_edges(M)) and len(e) - 1 == bands
        assert e[0] == 0 and e[-1] == M and np.all(np.diff(e) > 0) and np.all(e % 4 == 0)
    with pytest.raises(ValueError):
        codec.band_edges(128)


@pytest.mark.parametrize("M", R.FRAMES)
def test_plan_and_frame_counts(M):
    lengths = [0, 1, M - 1, M, M + 1]
    c = codec.TransformCodec(24000, 64, M)
    pl = c.plan(lengths)
    assert pl["rows"] == 5 and pl["frame"] == M and pl["bands"] == len(R.band_edges(M)) - 1
    assert pl["frames"].tolist() == [0, 2, 2, 2, 3] == [R.n_frames(n, M) for n in lengths]
    assert pl["frame_offsets"].tolist() == [0, 0, 2, 4, 6] and pl["n_frames"] == 9 and pl["n_samples"] == sum(lengths)
    assert pl["meta"][:, 0].tolist() == [0, 0, 1, M, 2 * M] and pl["meta"][:, 1].tolist() == lengths
    assert pl["table_floats"] == codec.host_tables(M).size == 4 * M + 2 * 448
    assert c.plan([])["n_frames"] == 0
    with pytest.raises(ValueError):
        c.plan([3, 4], [0])
    with pytest.raises(_lib.HipLibraryError):
        c.plan([-1])


def test_tables_are_rounded_from_float64():
    t = codec.host_tables(256)
    T, Rr = R.step_tables()
    assert t.dtype == f32 and np.array_equal(t[-896:-448], T) and np.array_equal(t[-448:], Rr)
    assert np.array_equal(t[512:1024], R.window(256, f32))
    assert T[224] == 1.0 and T[228] == 2.0 and Rr[228] == 0.5


def test_codec_parameters():
    c = codec.TransformCodec(24000, 16)
    assert c.frame == 1024 and c.bandwidth_hz == 4000.0 and c.cutoff_bin == 342 and c.budget == 682
    assert c.cutoff_bin == R.cutoff_bin(24000, 1024, R.default_bandwidth(24000, 16))
    assert codec.TransformCodec(24000, 128).bandwidth_hz == 12000.0
    assert codec.TransformCodec(24000, 128).cutoff_bin == 1024
    assert codec.TransformCodec(24000, 64, 256, bandwidth_hz=3000.0).cutoff_bin == 64
    for kbps in (8, 16, 32, 64, 128):
        c = codec.TransformCodec(24000, kbps)
        assert c.budget == R.budget_bits(24000, 1024, kbps)
        assert c.bands == R.bands_below(1024, c.cutoff_bin)
    for bad in (dict(frame=128), dict(frame=1000), dict(frame=True), dict(frame="1024"), dict(sr=0), dict(sr=-8000),
                dict(sr=float("nan")), dict(sr="24000"), dict(bitrate_kbps=0), dict(bitrate_kbps=float("inf")),
                dict(bitrate_kbps=None), dict(bandwidth_hz=0.0), dict(bandwidth_hz=-1.0),
                dict(bandwidth_hz=float("nan")), dict(bandwidth_hz="wide")):
        with pytest.raises(ValueError):
            codec.TransformCodec(**{"sr": 24000, "bitrate_kbps": 64, **bad})
    # 1 kbps at 24 kHz: a frame of 256 has 10 bits, fewer than the 8 + bands of an empty frame
    with pytest.raises(ValueError, match="empty frame"):
        codec.TransformCodec(24000, 1, 256)
    floor = 8 + R.bands_below(256, 256)
    assert codec.TransformCodec(256000, floor, 256, bandwidth_hz=128000).budget == floor
    with pytest.raises(ValueError, match="empty frame"):
        codec.TransformCodec(256000, floor - 1, 256, bandwidth_hz=128000)


def test_host_tensors_are_refused():
    import torch
    x = torch.zeros(100)
    c = codec.TransformCodec(24000, 64)
    for call in (lambda: c(x), lambda: c.mdct(x), lambda: c.quantize(torch.zeros(2, 1024)),
                 lambda: c.imdct(torch.zeros(2, 1024), x), lambda: codec.apply_mulaw(x),
                 lambda: codec.apply_g711u(x, 24000), lambda: codec.apply_transform_codec(x, 24000, 64)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError):
        codec.apply_g711u(x, 24000.5)


def test_library_refusals():
    lib = _lib.load()
    meta = np.zeros((1, lib.pe_codec_plan_fields()), np.int64)
    consts, totals = np.zeros(4, np.int64), np.zeros(2, np.int64)
    one, zero = np.array([5], np.int64), np.array([0], np.int64)
    args = lambda frame, n: (1, frame, n.ctypes.data, zero.ctypes.data, zero.ctypes.data, consts.ctypes.data,  # noqa
                             meta.ctypes.data, totals.ctypes.data)
    assert lib.pe_codec_plan(*args(1024, one)) == 0 and meta[0].tolist() == [0, 5, 0, 2, 0]
    assert lib.pe_codec_plan(*args(1000, one)) == -2
    assert lib.pe_codec_plan(*args(1024, np.array([-1], np.int64))) == -1
    # checked before any device call: the frame size, the cutoff, the budget, a plan that is not pe_codec_plan's
    assert lib.pe_codec_quantize(None, 1, 100, 10, 1000, None, 0, None, None, None, None, None) == -2
    assert lib.pe_codec_quantize(None, 1, 256, 0, 1000, None, 0, None, None, None, None, None) == -1
    assert lib.pe_codec_quantize(None, 1, 256, 257, 1000, None, 0, None, None, None, None, None) == -1
    assert lib.pe_codec_quantize(None, 1, 256, 256, 8 + 28, None, 0, None, None, None, None, None) == -1
    assert lib.pe_codec_quantize(None, 0, 256, 256, 8 + 29, None, 0, None, None, None, None, None) == 0
    bad = meta.copy()
    bad[0, 3] = 3
    assert lib.pe_codec_mdct(None, None, bad.ctypes.data, 1, 1024, None, 0, None, None) == -1
    assert lib.pe_codec_mulaw(None, None, bad.ctypes.data, 1, 1024, None, None) == -1
    assert lib.pe_codec_apply(None, None, meta.ctypes.data, 1, 1024, 1024, 10, None, 0, None, None, None, None, 0,
                              None) == -1
    assert lib.pe_codec_mdct(None, None, None, 0, 1024, None, 0, None, None) == 0
    assert lib.pe_codec_workspace_bytes(1024, 3) == 3 * 2048 * 4 and lib.pe_codec_workspace_bytes(100, 3) == 0


def test_condition_kinds_are_unchanged():
    assert stress.CONDITION_KINDS == ("rir", "microphone", "clipping", "agc", "resample", "additive_noise")
    with pytest.raises(ValueError):
        stress.Condition("codec", "transform 64 kbps", bitrate_kbps=64)


def test_codec_condition():
    c = codec.CodecCondition("ptc 64", bitrate_kbps=64)
    assert isinstance(c, stress.Condition) and c.kind == "codec" and c.codec == "transform" and c.label == "ptc 64"
    assert c.bitrate_kbps == 64.0 and c.params == {"bitrate_kbps": 64} and callable(c.apply)
    g = codec.CodecCondition("phone", codec="g711u")
    assert g.kind == "codec" and g.bitrate_kbps == 64.0 and g.params == {}
    full = codec.CodecCondition("x", codec="transform", bitrate_kbps=16, frame=256, bandwidth_hz=3000.0)
    assert full.params["frame"] == 256
    for kwargs in (dict(codec="opus", bitrate_kbps=64), dict(codec="transform"), dict(bitrate_kbps=0),
                   dict(bitrate_kbps="64"), dict(bitrate_kbps=64, frame=100), dict(bitrate_kbps=64, bandwidth_hz=-1),
                   dict(bitrate_kbps=64, quality=3), dict(codec="g711u", bitrate_kbps=64)):
        with pytest.raises(ValueError):
            codec.CodecCondition("bad", **kwargs)


def test_the_restatement_keeps_a_tracker_on_pitch_at_128_kbps():
    """What tests/test_codec_gpu.py asks of the kernel, of the restatement first: a 220 Hz harmonic complex through
    the 128 kbps codec, tracked by the autocorrelation tracker's restatement, has RPA 1.0 at 50 cents against the clean
    track."""
    from tests import f0_track_ref as T
    t = np.arange(24000) / 24000.0
    x = sum(np.sin(2 * np.pi * 220.0 * h * t) / h for h in range(1, 9))
    x = (0.4 * x / np.max(np.abs(x))).astype(f32)
    y, _, _ = R.codec(x, 24000, 128, 1024)
    clean, coded = T.track(x, 24000, 300)["f0"], T.track(y.astype(f32), 24000, 300)["f0"]
    voiced = clean > 0
    cents = 1200.0 * np.abs(np.log2(np.maximum(coded[voiced], 1e-5) / clean[voiced]))
    print(f"{int(voiced.sum())} voiced frames, largest deviation {cents.max():.3f} cents")
    assert voiced.sum() >= 40 and np.all(cents <= 50.0)
