"""Voice transforms of WORLD frames without a GPU: the restatement (tests/world_warp_ref.py) against what it states (the
frequency map and its inverse, where formant peaks land, what the tilt measures), the host conventions of
``pitchextractor_amd.world`` against it (``time_warp_curve``, frame counts, positions), the C plan's refusals (host only,
null device pointers), the ``world_resynthesis.transform`` block (configuration, draw order, untouched streams when it
is off), and that the rows of tests/world_warp_cases.py make a usable yardstick for tests/test_world_warp_gpu.py."""
import ctypes
import logging
import random

import numpy as np
import pytest

from pitchextractor_amd import _lib, build
from pitchextractor_amd import meldataset as md
from pitchextractor_amd import world
from tests import world_warp_cases as wc
from tests import world_warp_ref as wwr
from tests.test_cheaptrick_cpu import FP, FS, HOP, N, RS_CFG, _ds, _files

ALPHAS = (0.8, 0.9, 1.0, 1.1, 1.25)


# --------------------------------------------------------------------------- the restatement against what it states
@pytest.mark.parametrize("fs", [16000, 24000, 48000])
def test_map_and_inverse(fs):
    f = np.linspace(0.0, fs / 2.0, 4001)
    for alpha in ALPHAS:
        up, down = wwr.w(f, alpha, 4800.0, fs), wwr.w_inv(f, alpha, 4800.0, fs)
        assert (np.diff(up) > 0).all() and (np.diff(down) > 0).all()
        assert up[0] == 0 and down[0] == 0 and up[-1] == pytest.approx(fs / 2) and down[-1] == pytest.approx(fs / 2)
        np.testing.assert_allclose(wwr.w_inv(up, alpha, 4800.0, fs), f, rtol=0, atol=1e-9 * fs)
        np.testing.assert_allclose(wwr.w(down, alpha, 4800.0, fs), f, rtol=0, atol=1e-9 * fs)
        x0, y0 = wwr.knee(alpha, 4800.0)
        assert max(x0, y0) <= 4800.0 + 1e-9 and wwr.w(x0, alpha, 4800.0, fs) == pytest.approx(y0)
        low = f <= x0
        np.testing.assert_allclose(up[low], alpha * f[low])


def _peaks(fs, fft_size, freqs, width=300.0):
    f = np.arange(fft_size // 2 + 1) * fs / fft_size
    env = np.full(f.size, 1e-4)
    for f0 in freqs:
        d = np.abs(f - f0)
        env += np.where(d < width, 0.5 + 0.5 * np.cos(np.pi * d / width), 0.0)
    return env.astype(np.float32)[None, :]


@pytest.mark.parametrize("fp32", [False, True])
def test_formant_peaks_move_by_alpha(fp32):
    fs, fft_size = 24000, 1024
    freqs = (500.0, 1500.0, 2700.0)                               # alpha f stays below the knee for every alpha
    sp = _peaks(fs, fft_size, freqs)
    for alpha in ALPHAS:
        out, _ = wwr.warp(sp, None, [0.0], alpha, tilt=1e-9 if alpha == 1.0 else 0.0, fs=fs, fp32=fp32)
        for f0 in freqs:
            k = int(round(alpha * f0 * fft_size / fs))
            lo, hi = k - 8, k + 9
            assert abs(lo + int(np.argmax(out[0, lo:hi])) - alpha * f0 * fft_size / fs) <= 1.0, (alpha, f0)
        wrong, _ = wwr.warp(sp, None, [0.0], alpha, tilt=1e-9, fs=fs, fp32=fp32, invert=False)
        if alpha != 1.0:                                          # the mistake moves them the other way
            k = 1500.0 / alpha * fft_size / fs
            assert abs(int(np.argmax(wrong[0, int(k) - 8:int(k) + 9])) + int(k) - 8 - k) <= 1.0


def test_tilt_measures_its_db_per_octave():
    fs, fft_size = 24000, 1024
    sp = np.full((1, fft_size // 2 + 1), 0.37, np.float32)
    k1, k4 = 1000.0 * fft_size / fs, 4000.0 * fft_size / fs
    for tilt in (-6.0, -3.0, 2.0):
        for fp32 in (False, True):
            out, _ = wwr.warp(sp, None, [0.0], 1.0, tilt=tilt, fs=fs, fp32=fp32)
            db = 10.0 * np.log10(out[0].astype(np.float64))
            at = lambda k: np.interp(k, np.arange(db.size), db)  # noqa: E731
            assert (at(k4) - at(k1)) / 2.0 == pytest.approx(tilt, abs=1e-3)
            assert at(k1) == pytest.approx(10.0 * np.log10(0.37), abs=1e-3)            # 1 kHz is the pivot
            np.testing.assert_allclose(db[:5], db[0], atol=1e-5)                       # flat below 125 Hz


def test_breath_scales_and_clamps_the_aperiodicity():
    sp = np.full((2, 513), 1.0, np.float32)
    ap = np.stack([np.linspace(0.01, 0.9, 513), np.linspace(0.02, 1.0, 513)]).astype(np.float32)
    out = wwr.warp(sp, ap, [0.0, 0.5, 1.0], 1.0, breath=6.0, fs=24000)[1]
    g = 10.0 ** (6.0 / 20.0)
    np.testing.assert_allclose(out[0], np.minimum(ap[0].astype(np.float64) * g, 1.0), rtol=1e-12)
    np.testing.assert_allclose(out[1], np.minimum(0.5 * (ap[0].astype(np.float64) + ap[1]) * g, 1.0), rtol=1e-12)
    assert out.max() == 1.0 and out.min() > 0
    same = wwr.warp(sp, ap, [0.0, 1.0], fs=24000)
    assert same[0].dtype == np.float64 and np.array_equal(same[0], sp) and np.array_equal(same[1], ap)


# --------------------------------------------------------------------------- host conventions
def test_time_warp_curve_never_averages_with_zero():
    rng = np.random.default_rng(0)
    base = rng.uniform(80.0, 400.0, 40)
    base[rng.random(40) < 0.4] = 0.0
    base[[0, 17, 18, 39]] = [0.0, 150.0, 0.0, 210.0]
    for rate in (0.8, 1.0, 1.25, 0.37):
        pos = world.source_positions(int(39 / rate) + 3, rate, base.size)
        got = world.time_warp_curve(base, pos)
        np.testing.assert_array_equal(got, wwr.time_warp_curve(base, pos))
        i = np.floor(pos).astype(int)
        j = np.minimum(i + 1, base.size - 1)
        a, b = base[i], base[j]
        both = (a > 0) & (b > 0)
        assert ((got[both] >= np.minimum(a, b)[both]) & (got[both] <= np.maximum(a, b)[both])).all()
        assert ((got[~both] == a[~both]) | (got[~both] == b[~both])).all()             # a neighbour's value, never a mix
        smaller = np.where(both, np.minimum(a, b), np.where(a > 0, a, b))
        assert not ((got > 0) & (got < smaller)).any()
    np.testing.assert_array_equal(world.time_warp_curve([100.0, 0.0, 300.0], [0.4, 0.5, 0.6, 1.5, 1.51]),
                                  [100.0, 100.0, 0.0, 0.0, 300.0])                     # a tie goes to the earlier frame
    np.testing.assert_array_equal(world.time_warp_curve(base, np.arange(40.0)), base)


def test_frame_counts_and_positions():
    for n, hop, rate in ((24000, 300, 1.0), (24000, 300, 0.8), (24000, 300, 1.25), (1000, 300, 0.8), (7, 300, 1.25),
                         (96000, 256, 0.93)):
        G = world.warped_frames(n, hop, rate)
        assert G == 1 + int(round(n / rate)) // hop == wwr.warped_frames(n, hop, rate)
        assert world.warped_length(n, rate) == int(round(n / rate))
        S = 1 + n // hop
        pos = world.source_positions(G, rate, S)
        np.testing.assert_array_equal(pos, wwr.source_positions(G, rate, S))
        assert pos[0] == 0 and (np.diff(pos) >= 0).all() and pos.max() <= S - 1
        assert world.output_length(G, 24000, 1000.0 * hop / 24000) == int(G * (1000.0 * hop / 24000) * 24000 / 1000)
    assert world.warped_frames(24000, 300, 1.0) == 81 and world.warped_frames(24000, 300, 0.8) == 101
    pos = world.source_positions(6, 0.8, 4)                      # n = 1000, hop 300: the last frames are clamped
    np.testing.assert_allclose(pos, [0.0, 0.8, 1.6, 2.4, 3.0, 3.0])
    assert world.VoiceTransform() == (1.0, 1.0, 0.0, 0.0, 4800.0)


# --------------------------------------------------------------------------- C ABI, host side only
@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _lib.load()


def test_plan_and_entry_point_argument_checks(lib):
    Lg = lambda *v: (ctypes.c_long * len(v))(*v)  # noqa: E731
    K = lib.pe_world_warp_plan_fields()
    assert K == lib.pe_cheaptrick_plan_fields() + 3
    meta, tot = (ctypes.c_long * (4 * K))(), Lg(0)
    default_params = (1.1, 4800.0, -3.0, 6.0)

    def plan(src=7, in_off=0, in_stride=513, ap_off=None, ap_stride=513, out=4, out_off=0, stride=513,
             frames=(0, 1, 2, 6), fracs=(0.0, 0.25, 0.5, 0.0), params=default_params, fs=24000.0, fft=1024, rows=1,
             meta=meta, tot=tot, null=()):
        args = dict(src=Lg(src), in_off=Lg(in_off), in_stride=Lg(in_stride), ap_off=None if ap_off is None else
                    Lg(ap_off), ap_stride=Lg(ap_stride), out=Lg(out), out_off=Lg(out_off), stride=Lg(stride),
                    frames=(ctypes.c_int * len(frames))(*frames), fracs=(ctypes.c_float * len(fracs))(*fracs),
                    params=(ctypes.c_float * 4)(*params))
        for k in null:
            args[k] = None
        return lib.pe_world_warp_plan(rows, args["src"], args["in_off"], args["in_stride"], args["ap_off"],
                                      args["ap_stride"], args["out"], args["out_off"], args["stride"], args["frames"],
                                      args["fracs"], args["params"], fs, fft, meta, tot)
    assert plan() == 0 and tot[0] == 4
    assert [meta[i] for i in range(K)] == [0, 7, 0, 0, 4, 0, 0, 513, 513, -1, 0]
    assert plan(ap_off=11, ap_stride=0) == 0 and [meta[i] for i in range(K)][-3:] == [513, 11, 0]
    assert plan(in_stride=0) == 0 and plan(stride=600, out_off=3) == 0
    # a null pointer; a non-finite or non-positive fs
    for k in ("src", "in_off", "in_stride", "out", "out_off", "stride", "frames", "fracs", "params"):
        assert plan(null=(k,)) == -1, k
    assert plan(ap_off=0, null=("ap_stride",)) == -1 and plan(meta=None) == -1 and plan(tot=None) == -1
    assert plan(fs=0.0) == -1 and plan(fs=-24000.0) == -1 and plan(fs=float("nan")) == -1 and plan(fs=float("inf")) == -1
    # alpha outside [0.5, 2]; any parameter that is not finite
    P = lambda **kw: tuple(kw.get(k, d) for k, d in zip(("alpha", "f_hi", "tilt", "breath"), default_params))  # noqa: E731
    assert plan(params=P(alpha=0.49)) == -1 and plan(params=P(alpha=2.01)) == -1 and plan(params=P(alpha=0.5)) == 0
    assert plan(params=P(alpha=2.0)) == 0 and plan(params=P(alpha=float("nan"))) == -1
    assert plan(params=P(tilt=float("inf"))) == -1 and plan(params=P(breath=float("nan"))) == -1
    # a frequency map that does not rise strictly on [0, fs / 2]: the knee at or beyond Nyquist, or not above 0
    assert plan(params=P(f_hi=12000.0)) == -1 and plan(params=P(f_hi=13000.0)) == -1 and plan(params=P(f_hi=0.0)) == -1
    assert plan(params=P(f_hi=-1.0)) == -1 and plan(params=P(f_hi=float("nan"))) == -1
    assert plan(params=P(f_hi=11999.0)) == 0 and plan(params=P(f_hi=4800.0), fs=8000.0, fft=512, stride=257) == -1
    # a source position outside [0, src_frames - 1]
    assert plan(frames=(0, 1, 2, 7)) == -1 and plan(frames=(-1, 1, 2, 6)) == -1
    assert plan(fracs=(0.0, 0.25, 0.5, 0.5)) == -1                # 6.5 > 6: what a missing clamp hands over
    assert plan(fracs=(0.0, 1.0, 0.5, 0.0)) == -1 and plan(fracs=(0.0, -0.1, 0.5, 0.0)) == -1
    assert plan(fracs=(0.0, float("nan"), 0.5, 0.0)) == -1
    # negative counts, offsets and strides; an output stride below the bins; output frames of an empty row
    assert plan(src=-1) == -1 and plan(out=-1) == -1 and plan(in_off=-1) == -1 and plan(out_off=-1) == -1
    assert plan(in_stride=-1) == -1 and plan(ap_off=0, ap_stride=-1) == -1 and plan(stride=512) == -1
    assert plan(src=0) == -1 and plan(src=0, out=0) == 0 and tot[0] == 0
    assert plan(rows=-1) == -1 and plan(rows=65536) == -1 and plan(rows=0, meta=None) == 0
    # an fft_size other than 512 / 1024 / 2048
    assert plan(fft=256) == -2 and plan(fft=4096) == -2 and plan(fft=1000) == -2 and plan(fft=0) == -2
    assert plan(fft=512, stride=257) == 0 and plan(fft=2048, stride=1025) == 0 and plan(fft=2048) == -1
    # the launch: every check before any device call (there is no device here)
    assert plan(ap_off=0) == 0
    p = ctypes.c_void_p(8)
    run = lambda sp=p, ap=p, dm=p, hm=meta, pf=p, pr=p, pa=p, rows=1, fs=24000.0, fft=1024, out=p, ao=p: \
        lib.pe_world_warp(sp, ap, dm, hm, pf, pr, pa, rows, fs, fft, out, ao, None)  # noqa: E731
    for k in ("sp", "ap", "dm", "hm", "pf", "pr", "pa", "out", "ao"):
        assert run(**{k: None}) == -1, k
    assert run(fft=4096) == -2 and run(fs=0.0) == -1 and run(rows=-1) == -1 and run(rows=65536) == -1
    assert run(rows=0, sp=None, ap=None, dm=None, hm=None, pf=None, pr=None, pa=None, out=None, ao=None) == 0
    assert run(rows=0, fft=4096) == -2
    bad = (ctypes.c_long * K)(*[0, 7, 0, 0, 4, 1, 0, 513, 513, -1, 0])                # not the plan's frame prefix
    assert run(hm=bad) == -1
    narrow = (ctypes.c_long * K)(*[0, 7, 0, 0, 4, 0, 0, 512, 513, -1, 0])
    assert run(hm=narrow) == -1
    assert plan() == 0                                             # no row has an ap: its pointers may be null
    assert run(ap=None, ao=None, sp=None) == -1
    assert plan(src=0, out=0) == 0                                 # nothing to launch
    assert run(sp=None, ap=None, dm=None, pf=None, pr=None, pa=None, out=None, ao=None) == 0


# --------------------------------------------------------------------------- the yardstick of the GPU test
@pytest.mark.parametrize("cfg", wc.CONFIGS, ids=wc.config_id)
def test_float32_restatement_is_a_usable_yardstick(cfg):
    """On every row the float32 restatement is finite and positive, deviates from float64 (so 4 x its deviation is a
    bound a float32 kernel can meet) and stays small; a kernel that interpolates sp linearly or warps with alpha in
    place of 1 / alpha would miss the bound the GPU test asserts on these rows by orders of magnitude."""
    fs, fp, fft_size, thr, rate, alpha, tilt, breath = cfg
    rows = wc.cases(cfg)
    assert [len(c["sp"]) for c in rows][:4] == [7, 3, 2, 0] and len(rows[4]["sp"]) > 20
    for c in rows:
        assert c["sp32"].dtype == np.float32 and c["sp64"].dtype == np.float64
        assert np.isfinite(c["sp32"]).all() and (c["sp32"] > 0).all() and (c["sp"] > 0).all()
        if c["ap"] is not None:
            assert (c["ap32"] >= 0).all() and (c["ap32"] <= 1).all() and np.isfinite(c["ap64"]).all()
        if len(c["pos"]):
            assert c["pos"][0] == 0 and c["pos"][-1] == c["pos"][-2] == len(c["sp"]) - 1   # on a frame; clamped
    e_sp, e_ap = wc.yardsticks(cfg)
    print(f"[world_warp] {wc.config_id(cfg)}: float32 restatement ln sp {e_sp:.3e} ap {e_ap:.3e}")
    assert 0 < e_sp < 1e-3 and (thr is None or 0 < e_ap < 1e-5)
    for tag, kw, shows in (("linear sp", dict(log_domain=False), True), ("alpha for 1 / alpha", dict(invert=False),
                                                                         alpha != 1.0)):
        got = [wwr.warp(c["sp"], c["ap"], c["pos"], alpha, wc.f_hi_of(cfg), tilt, breath, fs=fs, fp32=True, **kw)
               for c in rows]
        m_sp, _ = wc.deviations(rows, [g[0] for g in got], [g[1] for g in got])
        print(f"[world_warp] {wc.config_id(cfg)}: {tag}: ln sp {m_sp:.3e} = {m_sp / e_sp:.0f} x the yardstick")
        assert (m_sp > 100 * 4 * e_sp) == shows
    # the third mistake: positions that are not clamped to the last source frame are refused, not read
    loose = wwr.source_positions(len(rows[0]["pos"]), rate, 7, clamp=False)
    assert loose.max() > 6
    with pytest.raises(ValueError, match="outside"):
        wwr.warp(rows[0]["sp"], None, loose, alpha, fs=fs)


# --------------------------------------------------------------------------- the data layer
BLOCK = {"probability": 0.7, "formant_ratio_range": [0.85, 1.2], "rate_range": [0.8, 1.25],
         "tilt_db_per_octave_range": [-3.0, 3.0], "breath_db_range": [4.0, 4.0], "f_hi": 4500.0}


def _syn(block, **more):
    rs = {**RS_CFG, **more}
    if block is not None:
        rs["transform"] = block
    return {"enabled": True, "absolute_count": 12, "pitch_shift": {"enabled": False}, "world_resynthesis": rs}


def test_configuration_of_the_block(tmp_path, caplog):
    lines = _files(tmp_path, [1.0])
    assert _ds(lines, _syn(None)).synthetic_resynthesis_config["transform"] is None
    assert _ds(lines, _syn({**BLOCK, "probability": 0})).synthetic_resynthesis_config["transform"] is None
    cfg = _ds(lines, _syn(BLOCK)).synthetic_resynthesis_config["transform"]
    assert cfg == {"probability": 0.7, "ranges": ((0.85, 1.2), (0.8, 1.25), (-3.0, 3.0), (4.0, 4.0)), "f_hi": 4500.0}
    cfg = _ds(lines, _syn({"rate_range": [1.25, 0.8], "tilt_db_per_octave_range": -2})).synthetic_resynthesis_config
    assert cfg["transform"] == {"probability": 0.5, "ranges": ((1.0, 1.0), (0.8, 1.25), (-2.0, -2.0), (0.0, 0.0)),
                                "f_hi": 4800.0}
    with caplog.at_level(logging.WARNING):
        _ds(lines, _syn({**BLOCK, "pitch": 2}))
    assert any("transform" in r.getMessage() and "'pitch'" in r.getMessage() for r in caplog.records)
    for bad, what in (({"probability": 1.5}, "probability"), ({"formant_ratio_range": [0.4, 1.0]}, "formant_ratio"),
                      ({"formant_ratio_range": [1.0, 2.5]}, "formant_ratio"), ({"rate_range": [0.0, 1.0]}, "rate_range"),
                      ({"rate_range": [1.0]}, "rate_range"), ({"tilt_db_per_octave_range": [0.0, float("nan")]}, "tilt"),
                      ({"breath_db_range": [-100.0, 0.0]}, "breath"), ({"f_hi": 12000.0}, "f_hi"),
                      ({"f_hi": 0.0}, "f_hi")):
        with pytest.raises(ValueError, match=what):
            _ds(lines, _syn({**BLOCK, **bad}))


def test_streams_are_untouched_without_the_block_or_at_probability_zero(tmp_path):
    lines = _files(tmp_path, [1.0, 3.0, 1.6])
    states, items = [], []
    for block in (None, {**BLOCK, "probability": 0}, {**BLOCK, "probability": 0.0}):
        ds = _ds(lines, _syn(block))
        random.seed(4); np.random.seed(4)
        items.append([ds[3 + i] for i in range(12)])
        states.append((random.getstate(), np.random.get_state()))
    for st, its in zip(states[1:], items[1:]):
        assert st[0] == states[0][0]
        assert all(np.array_equal(a, b) for a, b in zip(st[1], states[0][1]))
        for a, b in zip(its, items[0]):
            assert a[-1].transform is None and a[-1].positions is None
            for u, v in zip(a[:-1], b[:-1]):
                np.testing.assert_array_equal(np.asarray(u), np.asarray(v))
            for u, v in zip(a[-1], b[-1]):
                np.testing.assert_array_equal(np.asarray(u, dtype=object) if u is None else np.asarray(u),
                                              np.asarray(v, dtype=object) if v is None else np.asarray(v))


def _restated_item(cfg, block, paths):
    """The documented draw order: file, semitone, gain, vibrato, transform (its gate, then formant, rate, tilt, breath
    where the range is not a single value), noise, crop."""
    path = random.choice(paths)
    wave, _ = md.read_wav(path)
    n = len(wave)
    mel_len = 1 + n // HOP
    base = md.align_length(np.load(path + "_f0.npy").astype(np.float32), mel_len).astype(np.float64)
    semitone = random.choice(cfg["semitones"])
    gain = 10.0 ** (random.uniform(*cfg["gain_db_range"]) / 20.0)
    mod = cfg["modulation"]
    vibrato = random.uniform(*mod["vibrato_rate_range"]) if random.random() < mod["vibrato_probability"] else None
    transform = None
    if random.random() < block["probability"]:
        values = [lo if lo == hi else random.uniform(lo, hi) for lo, hi in
                  (block["formant_ratio_range"], block["rate_range"], block["tilt_db_per_octave_range"],
                   block["breath_db_range"])]
        transform = tuple(values) + (block["f_hi"],)
    rate = 1.0 if transform is None else transform[1]
    n_out = n if transform is None else int(round(n / rate))
    frames = 1 + n_out // HOP
    pos = None if transform is None else wwr.source_positions(frames, rate, mel_len)
    new = (base if pos is None else wwr.time_warp_curve(base, pos)) * float(2 ** (semitone / 12.0))
    if vibrato is not None:
        t = np.arange(frames, dtype=np.float64) * (FP / 1000.0)
        new = new * 2.0 ** (np.sin(2.0 * np.pi * vibrato * t) * (mod["vibrato_semitones"] / 12.0))
    curve = np.where(new > world.lowest_f0(FS, N), new, 0.0)
    noise = np.random.normal(scale=10.0 ** (cfg["noise_db"] / 20.0), size=(n_out,)).astype(np.float32)
    crop = int(np.random.randint(0, frames - 192)) if frames > 192 else 0
    return path, gain, n, n_out, base, curve, noise, crop, transform, pos


def test_items_follow_the_documented_draw_order(tmp_path):
    lines = _files(tmp_path, [1.0, 3.0, 1.6])
    paths = [ln[:-1].split("|")[0] for ln in lines]
    f0 = np.load(paths[2] + "_f0.npy")
    f0[10:20] = 0.0                                               # an unvoiced stretch inside a voiced one
    np.save(paths[2] + "_f0.npy", f0)
    ds = _ds(lines, _syn(BLOCK))
    random.seed(3); np.random.seed(3)
    got = [ds[3 + i] for i in range(12)]
    end = (random.getstate(), np.random.get_state())
    random.seed(3); np.random.seed(3)
    with_t = without = cropped = 0
    for item in got:
        assert random.choice(["world_resynthesis"]) == "world_resynthesis"
        path, gain, n, n_out, base, curve, noise, crop, transform, pos = _restated_item(RS_CFG, BLOCK, paths)
        wave, labels, sil, frame_start, sr, req = item
        assert isinstance(req, md.ResynthesisRequest) and (req.path, req.n, req.crop) == (path, n, crop)
        assert req.gain == pytest.approx(gain, rel=1e-12) and wave.shape[0] == n
        np.testing.assert_array_equal(req.base_curve, base)
        np.testing.assert_array_equal(req.curve, curve)
        np.testing.assert_array_equal(req.curve, world.label_curve(req.curve, FS, N))
        assert req.transform == transform
        if transform is None:
            without += 1
            assert req.positions is None and req.curve.size == 1 + n // HOP
        else:
            with_t += 1
            assert 0.85 <= transform[0] <= 1.2 and 0.8 <= transform[1] <= 1.25 and -3 <= transform[2] <= 3
            assert transform[3:] == (4.0, 4500.0)
            np.testing.assert_array_equal(req.positions, pos)
            assert req.curve.size == req.positions.size == world.warped_frames(n, HOP, transform[1])
            voiced = req.curve[req.curve > 0]                     # a label is never an average with 0
            assert voiced.min() >= 0.7 * base[base > 0].min()
        # noise, crop and window are planned on the output length
        start, count, first = md.synthetic_window(n_out, crop, HOP, 1024)
        assert (req.out_start, req.out_len, req.frame_start, frame_start) == (start, count, first, first)
        np.testing.assert_array_equal(req.noise, noise[start:start + count])
        label = md.align_length(req.curve.astype(np.float32), 1 + n_out // HOP)[crop:crop + 192]
        np.testing.assert_array_equal(labels.numpy(), label)
        np.testing.assert_array_equal(sil.numpy(), (label == 0).astype(np.float32))
        table = world.time_base(req.curve, FS, FP, N)
        np.testing.assert_array_equal(req.index, table.index)
        assert req.seed == world.noise_seed(req.curve)
        cropped += crop > 0
    assert with_t >= 3 and without >= 1 and cropped >= 1
    assert random.getstate() == end[0] and all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), end[1]))


def test_collater_carries_transforms_and_positions(tmp_path):
    lines = _files(tmp_path, [1.0, 1.6])
    ds = _ds(lines, _syn(BLOCK))
    random.seed(8); np.random.seed(8)
    items = [ds[2 + i] for i in range(6)]
    assert any(it[-1].transform is not None for it in items) and any(it[-1].transform is None for it in items)
    pack = md.Collater()([ds[0]] + items)[-1]
    assert isinstance(pack, md.ResynthesisBatch) and pack.rows.tolist() == [1, 2, 3, 4, 5, 6]
    assert pack.transforms == tuple(it[-1].transform for it in items)
    assert pack.base_len == tuple(len(it[-1].base_curve) for it in items)
    for p, it in zip(pack.positions, items):
        assert (p is None) == (it[-1].positions is None) and (p is None or np.array_equal(p, it[-1].positions))
    plain = _ds(lines, _syn(None))
    random.seed(8); np.random.seed(8)
    pack = md.Collater()([plain[0]] + [plain[2 + i] for i in range(6)])[-1]
    assert pack.transforms is None and pack.positions is None and pack.base_len is None
