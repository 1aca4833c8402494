"""WORLD D4C without a GPU: the constants the restatement (tests/d4c_ref.py) derives from a sample rate, the C ABI's
host-side plan and argument checks, independent checks of the restatement in float64 (orderings only: more aperiodic
input reads as more aperiodic; values are printed as records), its sort / cumulative-sum index against a brute-force
loop, its expansion against ``np.interp``, the float32 restatement's verdicts against the float64 one's on the rows the
GPU test uses, and the ``world_resynthesis`` block's ``aperiodicity: d4c``.  pyworld is not available: parity with its
binary is unpinned."""
import ctypes
import random

import numpy as np
import pytest
import torch

from pitchextractor_amd import _lib, build, world
from tests import cheaptrick_ref as ct
from tests import d4c_cases as dc
from tests import d4c_ref as d4
from tests import world_ref as wr
from tests.test_cheaptrick_cpu import PS_CFG, RS_CFG, WORLD_CFG, _ds, _files, _same_item

FS, FP = 24000, 5.0


# --------------------------------------------------------------------------- derived constants
def test_derived_constants():
    got = {fs: d4.constants(fs) for fs in (16000, 22050, 24000, 44100, 48000)}
    assert [got[fs]["N_d"] for fs in got] == [2048, 2048, 2048, 4096, 4096]
    assert [got[fs]["N_l"] for fs in got] == [2048, 2048, 2048, 4096, 4096]
    assert [got[fs]["bands"] for fs in got] == [1, 2, 3, 5, 5]
    assert [got[fs]["L"] for fs in got] == [2 * int(3000 * got[fs]["N_d"] / fs) + 1 for fs in got] == \
        [769, 557, 513, 557, 513]
    assert d4.constants(25000) == {"N_d": 4096, "N_l": 2048, "bands": 3, "L": 983}      # the two transforms differ
    for fs in (8000, 15800, 50000):
        with pytest.raises(ValueError):
            d4.constants(fs)
    w = d4.nuttall(513)
    assert w.argmax() == 256 and abs(w[256] - 1.0) < 1e-12 and abs(w[0]) < 1e-12 and abs(w[-1]) < 1e-12


# --------------------------------------------------------------------------- C ABI, host side only
@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _lib.load()


def test_plan_and_entry_point_argument_checks(lib):
    Lg = lambda *v: (ctypes.c_long * len(v))(*v)  # noqa: E731
    K = lib.pe_d4c_plan_fields()
    assert K == 8 == lib.pe_cheaptrick_plan_fields()
    meta, tot = (ctypes.c_long * (4 * K))(), Lg(0, 0, 0, 0, 0)

    def plan(x_off=0, x_len=2400, f0_off=0, f0_len=8, first=0, frames=8, out_off=0, stride=513, fs=24000.0, fpm=FP,
             fft=1024, rows=1, meta=meta, tot=tot):
        return lib.pe_d4c_plan(rows, Lg(x_off), Lg(x_len), Lg(f0_off), Lg(f0_len), Lg(first), Lg(frames), Lg(out_off),
                               Lg(stride), fs, fpm, fft, meta, tot)
    assert plan() == 0 and list(tot) == [8, 2048, 2048, 3, 513]
    assert [meta[i] for i in range(K)] == [0, 2400, 0, 0, 8, 0, 0, 513]
    for fs in (16000, 22050, 25000, 44100, 48000):
        c = d4.constants(fs)
        assert plan(fs=float(fs), fft=2048, stride=1025) == 0
        assert list(tot) == [8, c["N_d"], c["N_l"], c["bands"], c["L"]]
    # two rows: the second row's frame prefix
    two = (ctypes.c_long * (2 * K))()
    assert lib.pe_d4c_plan(2, Lg(0, 2401), Lg(2400, 1000), Lg(0, 8), Lg(8, 6), Lg(3, 0), Lg(5, 6), Lg(7, 9000),
                           Lg(513, 600), 24000.0, FP, 1024, two, tot) == 0 and tot[0] == 11
    assert [two[K + i] for i in range(K)] == [2401, 1000, 8, 0, 6, 5, 9000, 600]
    assert plan(first=3, frames=5) == 0 and tot[0] == 5 and plan(frames=0, x_len=0) == 0 and tot[0] == 0
    assert plan(fs=8000.0) == -2 and plan(fs=15800.0) == -2 and plan(fs=15801.0) == 0       # fs / 2 <= 7900
    assert plan(fs=48200.0, fft=2048, stride=1025) == -2 and plan(fs=96000.0, fft=2048, stride=1025) == -2   # N_d 8192
    assert plan(fft=4096) == -2 and plan(fft=1000) == -2 and plan(fft=0) == -1
    assert plan(fs=0.0) == -1 and plan(fs=float("inf")) == -1 and plan(fpm=float("nan")) == -1 and plan(fpm=-5.0) == -1
    assert plan(first=1, frames=8) == -1 and plan(frames=-1) == -1 and plan(first=-1) == -1
    assert plan(x_len=0) == -1 and plan(x_len=-1) == -1 and plan(x_off=-1) == -1 and plan(f0_off=-1) == -1
    assert plan(stride=512) == -1 and plan(out_off=-1) == -1
    assert plan(meta=None) == -1 and plan(tot=None) == -1
    assert plan(rows=0, meta=None) == 0 and plan(rows=-1) == -1 and plan(rows=65536) == -1
    assert lib.pe_d4c_plan(1, None, None, None, None, None, None, None, None, 24000.0, FP, 1024, meta, tot) == -1
    assert plan() == 0
    p = ctypes.c_void_p(8)
    bands = lambda x=p, f0=p, dm=p, hm=meta, tb=p, rows=1, fs=24000.0, fpm=FP, thr=0.85, fft=1024, out=p: \
        lib.pe_d4c_bands(x, f0, dm, hm, tb, rows, fs, fpm, thr, fft, out, None)  # noqa: E731
    expand = lambda b=p, dm=p, hm=meta, rows=1, fs=24000.0, fft=1024, ap=p: \
        lib.pe_d4c_expand(b, dm, hm, rows, fs, fft, ap, None)  # noqa: E731
    assert bands(x=None) == -1 and bands(f0=None) == -1 and bands(dm=None) == -1 and bands(tb=None) == -1
    assert bands(out=None) == -1 and bands(hm=None) == -1
    assert bands(thr=float("nan")) == -1 and bands(thr=float("inf")) == -1 and bands(fs=float("nan")) == -1
    assert bands(fs=8000.0) == -2 and bands(fs=50000.0) == -2 and bands(fft=4096) == -2 and bands(fft=0) == -1
    assert bands(rows=-1) == -1 and bands(rows=65536) == -1
    assert bands(rows=0, x=None, f0=None, dm=None, hm=None, tb=None, out=None) == 0      # nothing to do
    assert bands(rows=0, fs=8000.0) == -2                                                # a bad configuration still is
    assert expand(b=None) == -1 and expand(dm=None) == -1 and expand(ap=None) == -1 and expand(hm=None) == -1
    assert expand(fs=8000.0) == -2 and expand(fft=4096) == -2 and expand(rows=65536) == -1
    assert expand(rows=0, b=None, dm=None, hm=None, ap=None) == 0
    bad = (ctypes.c_long * K)(*[0, 2400, 0, 0, 8, 3, 0, 513])                            # not the plan's frame offsets
    narrow = (ctypes.c_long * K)(*[0, 2400, 0, 0, 8, 0, 0, 512])
    assert bands(hm=bad) == -1 and bands(hm=narrow) == -1 and expand(hm=bad) == -1 and expand(hm=narrow) == -1
    assert plan(frames=0, x_len=0) == 0                                                  # no frames: no launch
    assert bands(x=None, f0=None, dm=None, tb=None, out=None) == 0 and expand(b=None, dm=None, ap=None) == 0


def test_no_cpu_path():
    x = torch.zeros(2400)
    for call in (lambda: world.d4c(x, np.full(4, 100.0), FS, FP),
                 lambda: world.d4c_ragged(x, [2400], [np.full(4, 100.0)], FS, FP),
                 lambda: world.resynthesize(x, np.full(4, 100.0), np.full(4, 120.0), FS, FP, ap="d4c")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# --------------------------------------------------------------------------- the restatement, float64
L_FRAMES = 40
INTERIOR = slice(8, 32)


def _vowel(a, seed=0):
    """A constant 150 Hz "ah" from the synthesis restatement with the constant aperiodicity template ``a``."""
    f0 = np.full(L_FRAMES, 150.0)
    n = wr.output_length(L_FRAMES, FS, FP)
    noise = np.random.default_rng(seed).standard_normal(n)
    return wr.synthesize(f0, wr.envelope("ah", FS, 1024), None if a is None else np.full(513, a), FS, FP, noise), f0


def test_more_aperiodic_input_reads_as_more_aperiodic():
    """Band 1's mean coarse dB over interior voiced frames rises strictly with the template the vowel was synthesized
    with; a pure harmonic complex lies below all three, white noise under a forced 150 Hz F0 and threshold 0 above; and
    LoveTrain rejects the noise and accepts the vowels.  Only these orderings are asserted."""
    means, a0s = {}, {}
    for a in (0.05, 0.2, 0.5):
        y, f0 = _vowel(a)
        _, band, _ = d4.d4c(y, f0, FS, FP)
        assert not np.isnan(band[INTERIOR]).any()
        means[a], a0s[a] = band[INTERIOR, 1].mean(), band[INTERIOR, 0].min()
    n = wr.output_length(L_FRAMES, FS, FP)
    t = np.arange(n) / FS
    f0 = np.full(L_FRAMES, 150.0)
    harmonic = sum(np.sin(2 * np.pi * k * 150.0 * t + k) / k for k in range(1, 60))
    _, band, _ = d4.d4c(harmonic, f0, FS, FP)
    means["harmonic"] = band[INTERIOR, 1].mean()
    white = np.random.default_rng(1).standard_normal(n)
    _, band, _ = d4.d4c(white, f0, FS, FP, threshold=0.0)
    means["white"] = band[INTERIOR, 1].mean()
    _, gated, _ = d4.d4c(white, f0, FS, FP)
    a0s["white"] = gated[INTERIOR, 0].max()
    print("[d4c] band 1 mean coarse dB:", {k: round(float(v), 3) for k, v in means.items()})
    print("[d4c] LoveTrain a0 (vowels: min, white: max):", {k: round(float(v), 4) for k, v in a0s.items()})
    assert means["harmonic"] < means[0.05] < means[0.2] < means[0.5] < means["white"] <= 0.0
    assert a0s["white"] <= 0.85 < min(a0s[a] for a in (0.05, 0.2, 0.5))
    assert np.isnan(gated[INTERIOR, 1:]).all()                   # the rejected frames have no band values ...
    ap, _, _ = d4.d4c(white, f0, FS, FP)
    assert (ap[INTERIOR] == 1.0 - 1e-12).all()                   # ... and are all aperiodic


def test_frames_with_a0_zero():
    """F0 of 0, a negative or missing F0, and a silent window all have a0 = 0 and the unvoiced verdict, at any
    threshold (a0 <= threshold holds at 0 too)."""
    y, f0 = _vowel(0.2)
    f0 = f0.copy()
    f0[[3, 4]] = 0.0
    f0[5] = np.nan
    f0[6] = -100.0
    y = y.copy()
    y[int(0.1 * FS):int(0.15 * FS)] = 0.0                        # frames 20 .. 30; a 3-period window is 20 ms
    for thr in (0.0, 0.85):
        ap, band, _ = d4.d4c(y, f0, FS, FP, threshold=thr)
        zero = np.flatnonzero(band[:, 0] == 0.0)
        assert set([3, 4, 5, 6, 24, 25, 26]) <= set(zero) and np.isnan(band[zero, 1:]).all()
        assert (ap[zero] == 1.0 - 1e-12).all()
    assert (band[10:15, 0] > 0.85).all() and not np.isnan(band[10:15]).any()


def test_sort_and_cumulative_sum_index():
    """A hand-made group delay: the restatement's coarse value of each band against a loop that adds up the smallest
    N / 2 - round(8 N / L) power values one by one."""
    c = d4.constants(FS)
    N, L = c["N_d"], c["L"]
    rng = np.random.default_rng(3)
    k = np.arange(N // 2 + 1)
    g = 1e-3 * np.sin(2 * np.pi * k / 37.0) + 1e-4 * rng.standard_normal(k.size) + 2e-3 * (k == 300)
    got = d4.coarse_aperiodicity(g, FS, N, c["bands"], L)
    bw = int(8.0 * N / L + 0.5)
    assert (N, L, bw) == (2048, 513, 32)
    for i in range(c["bands"]):
        centre = int(3000.0 * (i + 1) * N / FS)
        assert centre == 256 * (i + 1)
        seg = np.zeros(N)
        seg[:L] = g[centre - 256:centre + 257] * d4.nuttall(L)
        power = sorted(abs(v) ** 2 for v in np.fft.fft(seg)[:N // 2 + 1])
        low = 0.0
        for v in power[:N // 2 - bw]:                            # S[N / 2 - bw - 1]: N / 2 - bw values
            low += v
        total = low
        for v in power[N // 2 - bw:]:
            total += v
        assert len(power) - (N // 2 - bw) == bw + 1
        assert got[i] == pytest.approx(10.0 * np.log10(low / total), abs=1e-9)
    assert d4.coarse_aperiodicity(np.zeros(N // 2 + 1), FS, N, 3, L).tolist() == [0.0, 0.0, 0.0]


def test_expansion_is_numpy_interp():
    for fs, fft in ((16000, 1024), (24000, 1024), (48000, 2048), (44100, 2048)):
        bands = d4.constants(fs)["bands"]
        coarse = -np.linspace(3.0, 40.0, bands)
        xs = np.concatenate([[0.0], 3000.0 * (np.arange(bands) + 1), [fs / 2.0]])
        ys = np.concatenate([[-60.0], coarse, [-1e-12]])
        want = 10.0 ** (np.interp(np.arange(fft // 2 + 1) * fs / fft, xs, ys) / 20.0)
        got = d4.expand(coarse, fs, fft)
        np.testing.assert_allclose(got, want, rtol=1e-12)
        assert got[0] == 1e-3 and got[-1] == pytest.approx(1.0, abs=1e-12)
        assert (d4.expand(np.full(bands, np.nan), fs, fft) == 1.0 - 1e-12).all()


def test_smoothing_is_cheaptricks_at_a_general_width():
    P = np.random.default_rng(5).random(513) + 0.1
    for f0 in (71.0, 150.3, 480.0):
        np.testing.assert_array_equal(d4.smooth(P, f0 * 1024 / (3.0 * FS), 1024), ct.smooth_interval(P, FS, f0, 1024))
    signed = P - 0.6
    np.testing.assert_allclose(d4.smooth(signed, 7.3, 1024), d4.smooth(P, 7.3, 1024) - 0.6, atol=1e-12)


def test_verdict_margins_of_the_gpu_rows():
    """What tests/test_d4c_gpu.py relies on, with the two restatements alone: on each configuration's rows the frames
    whose float64 a0 lies within 1000 x the a0 yardstick of the threshold (or whose smallest smoothed power lies within
    the zero rule's margin) are at most 10 % of the F0-voiced frames, and every other frame has the same verdict in
    float32 and float64."""
    for cfg in dc.CONFIGS:
        cases = dc.cases(cfg)
        voiced = sum(int((c["f0"] > 0).sum()) for c in cases.values())
        out = 0
        for name, c in cases.items():
            ex = dc.excluded_frames(cases, c, cfg)
            out += int(ex.sum())
            v64, v32 = np.isnan(c["b64"][:, 1]), np.isnan(c["b32"][:, 1])
            assert (v64 == v32)[~ex].all(), (cfg, name)
        print(f"[d4c] {cfg}: {voiced} F0-voiced frames, {out} excluded from the verdict comparison")
        assert out <= 0.1 * voiced


# --------------------------------------------------------------------------- the world_resynthesis block
def test_aperiodicity_d4c_in_the_configuration(tmp_path):
    lines = _files(tmp_path, [1.0, 3.0])
    base = {"enabled": True, "absolute_count": 8, "pitch_shift": PS_CFG, "world_vocoder": WORLD_CFG}
    numeric = _ds(lines, {**base, "world_resynthesis": RS_CFG})
    assert numeric.synthetic_resynthesis_config["aperiodicity"] == 0.2
    assert numeric.synthetic_resynthesis_config["d4c_threshold"] == 0.0
    for value in ("d4c",):
        ds = _ds(lines, {**base, "world_resynthesis": {**RS_CFG, "aperiodicity": value}})
        cfg = ds.synthetic_resynthesis_config
        assert cfg["aperiodicity"] == "d4c" and cfg["d4c_threshold"] == 0.0
        assert ds._synthetic_generators == numeric._synthetic_generators == ["pitch_shift", "world_vocoder",
                                                                             "world_resynthesis"]
        # the mode draws nothing: every item is the numeric mode's, request included
        random.seed(5); np.random.seed(5)
        want = [numeric[2 + i] for i in range(8)]
        random.seed(5); np.random.seed(5)
        for i in range(8):
            _same_item(ds[2 + i], want[i])
    with_thr = _ds(lines, {**base, "world_resynthesis": {**RS_CFG, "aperiodicity": "d4c", "d4c_threshold": 0.85}})
    assert with_thr.synthetic_resynthesis_config["d4c_threshold"] == 0.85
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="d4c_threshold"):
            _ds(lines, {**base, "world_resynthesis": {**RS_CFG, "aperiodicity": "d4c", "d4c_threshold": bad}})
    for bad in ("D4C", "harvest", ""):
        with pytest.raises(ValueError, match="aperiodicity"):
            _ds(lines, {**base, "world_resynthesis": {**RS_CFG, "aperiodicity": bad}})
    # absent: the generators and every draw are what they are without the block
    plain = _ds(lines, base)
    absent = _ds(lines, {**base, "world_resynthesis": {"aperiodicity": "d4c"}})          # not enabled
    assert plain._synthetic_generators == absent._synthetic_generators == ["pitch_shift", "world_vocoder"]
    random.seed(7); np.random.seed(7)
    want = [plain[2 + i] for i in range(8)]
    random.seed(7); np.random.seed(7)
    for i in range(8):
        _same_item(absent[2 + i], want[i])
