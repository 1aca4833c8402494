"""What the ragged audio entry points share on the host: the trackers' ``f0_tracker._RaggedTracker`` and
``NATIVE_BACKENDS``, the table roots ``fft_roots`` / ``real_split_roots``, and the gate of ``csrc/dsp.h`` that every
entry point with a ``host_meta`` passes before its own checks; no GPU needed."""
import ctypes

import numpy as np
import pytest

from pitchextractor_amd import f0_tracker as F


def _roots_inline(C):
    """The FFT roots and the real-split roots as both ``host_tables`` wrote them out before ``fft_roots`` /
    ``real_split_roots`` existed."""
    m = np.arange(C, dtype=np.float64)
    k = np.arange(C + 1, dtype=np.float64)
    tw = np.stack([np.cos(2 * np.pi * m / C), -np.sin(2 * np.pi * m / C)], axis=1)
    tr = np.stack([np.cos(np.pi * k / C), -np.sin(np.pi * k / C)], axis=1)
    return [tw.reshape(-1), tr.reshape(-1)]


def _praat_tables_inline(tr):
    nw, hw = tr.nsamp_window, tr.half_window
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1, nw + 1, dtype=np.float64) / (nw + 1))
    spec = np.fft.rfft(window, tr.n_fft)
    ac = np.fft.irfft(spec.real ** 2 + spec.imag ** 2, tr.n_fft)
    return np.concatenate(_roots_inline(tr.n_fft // 2) + [window, ac[:hw + 1] / ac[0]]).astype(np.float32)


def _dio_tables_inline(tr):
    N, C = tr.n_fft, tr.n_fft // 2
    n_cut = 2 * tr.cut + 1
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1, n_cut + 1, dtype=np.float64) / (n_cut + 1))
    low_cut = -w / np.sum(w)
    low_cut[tr.cut] += 1.0
    parts = _roots_inline(C)
    a = (0.355768, 0.487396, 0.144232, 0.012604)
    for h in tr.half_average_length:
        t = np.arange(4 * h, dtype=np.float64) / (4 * h - 1.0)
        nut = a[0] - a[1] * np.cos(2 * np.pi * t) + a[2] * np.cos(4 * np.pi * t) - a[3] * np.cos(6 * np.pi * t)
        g = np.zeros(N)
        shift = 2 * (tr.half_average_length[0] - h)
        taps = np.convolve(low_cut, nut)
        g[shift:shift + taps.size] = taps
        G = np.fft.rfft(g) / C
        parts.append(np.stack([G.real, G.imag], axis=1).reshape(-1))
    return np.concatenate(parts).astype(np.float32)


def _dio_roots_inline():
    parts = []
    for lg in range(7, 13):
        m = np.arange(1 << lg, dtype=np.float64) / (1 << lg)
        parts.append(np.stack([np.cos(2 * np.pi * m), -np.sin(2 * np.pi * m)], axis=1).reshape(-1))
    return np.concatenate(parts).astype(np.float32)


def _world_table_inline(fft_size):
    from pitchextractor_amd.world import dc_remover
    ang = -2.0 * np.pi * np.arange(fft_size) / fft_size
    return np.concatenate([np.stack([np.cos(ang), np.sin(ang)], axis=1).reshape(-1),
                           dc_remover(fft_size)]).astype(np.float32)


@pytest.mark.parametrize("sr,hop", [(16000, 200), (24000, 300), (48000, 600)])
def test_table_bytes_are_unchanged(sr, hop, monkeypatch):
    from pitchextractor_amd import _lib, stress, world
    monkeypatch.setattr(_lib, "device_table",                       # the host table itself, as the device copy is made
                        lambda key, device, build: np.ascontiguousarray(build(), dtype=np.float32))
    for C in (64, 512):
        assert F.fft_roots(C).shape == (C, 2) and F.fft_roots(C).dtype == np.float64
        assert F.real_split_roots(C).shape == (C + 1, 2) and F.real_split_roots(C).dtype == np.float64
    praat, dio = F.PraatACTracker(sr, hop), F.WorldDioTracker(sr, hop)
    for name, got, want in (("praat tables", praat.host_tables(), _praat_tables_inline(praat)),
                            ("dio tables", dio.host_tables(), _dio_tables_inline(dio)),
                            ("stonemask roots", dio.host_roots(), _dio_roots_inline()),
                            ("stress tables", stress.host_tables(), np.concatenate(_roots_inline(2048)).astype(np.float32)),
                            *((f"world table {n}", world.WorldSynth().table(n, "cpu"), _world_table_inline(n))
                              for n in (512, 1024, 2048))):
        assert got.dtype == np.float32 and got.shape == want.shape, name
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name


def test_backend_table_is_the_only_resolver():
    from pitchextractor_amd import inference
    from pitchextractor_amd.meldataset import MelDataset, f0_backend_chain
    backends = {"praat": {"type": "praat", "method": "ac"},
                "parselmouth": {"type": "parselmouth", "method": "ac"},
                "pyworld_plain": {"type": "pyworld"},
                "pyworld_harvest_fb": {"type": "pyworld", "algorithm": "dio", "fallback": "harvest"},
                "pyworld_dio": {"type": "pyworld", "algorithm": "dio"}}
    f0_params = {"backends": backends}
    chain = f0_backend_chain(f0_params)
    assert [name for name, _, _ in chain] == list(backends)
    rows = [(name, F.native_backend(btype, cfg)) for name, btype, cfg in chain]
    assert [(name, None if row is None else row.key) for name, row in rows] == \
        [("praat", "praat"), ("parselmouth", "praat"), ("pyworld_plain", None), ("pyworld_harvest_fb", None),
         ("pyworld_dio", "dio")]
    ds = MelDataset([], sr=24000, f0_params=f0_params, verbose=False)
    hop = int(ds.mel_params["hop_length"])
    assert ds._native_f0 == [(name, row.tracker.__name__, row.check(cfg, 24000, hop))
                             for (name, row), (_, _, cfg) in zip(rows, chain) if row is not None]
    assert [cls for _, cls, _ in ds._native_f0] == ["PraatACTracker", "PraatACTracker", "WorldDioTracker"]
    # the table's keys are track_f0's backend names, and nothing else is one
    assert [row.key for row in F.NATIVE_BACKENDS] == ["praat", "dio"]
    assert F.native_backend("swiftf0", {}) is None and F.native_backend("pyworld", None) is None
    for bad in ("pyworld", "parselmouth", "harvest", "PraatACTracker", ""):
        with pytest.raises(ValueError, match="is not one of"):
            inference.track_f0(np.zeros(8, np.float32), sr=24000, hop_length=300, backend=bad)


# --------------------------------------------------------------------------- the gate of the entry points with a host plan
ARG, UNSUP = -1, -2
# Return codes of the build before the gate was shared (one open_rows in dsp.h), per plan:
#   rows -1 | rows 65536 | no rows, host parameters given | no rows, every pointer null | null host_meta, one row |
#   wrong prefix offset in row 1 | negative length | rows all empty | rows of 1 and 2049 samples, device pointers null |
#   rows -1, unsupported rate | no rows, unsupported rate |
#   rows all empty with a wrong prefix offset in row 1 | rows all empty, the first of length -1
# Device pointers are null throughout, so a 0 shows that the gate answered before the pointer checks; where "rows all
# empty" is not 0 the entry point has work without samples (DIO gives an empty row one frame).  The last two columns
# hold the order range check, derive(), "no rows" for the entry points that take (sr, hop, config); the stress entry
# points take no rate.  The two after them tell the gate's consistency walk from the pointer checks wherever "rows all
# empty" is 0: a plan without work that is inconsistent is still refused.
GATE_CODES = {
    "pe_f0_track_frames": (ARG, ARG, 0, ARG, ARG, ARG, ARG, 0, ARG, ARG, UNSUP, ARG, ARG),
    "pe_f0_track_path": (ARG, ARG, 0, ARG, ARG, ARG, ARG, 0, ARG, ARG, UNSUP, ARG, ARG),
    "pe_f0_dio_bands": (ARG, ARG, 0, ARG, ARG, ARG, ARG, 0, ARG, ARG, UNSUP, ARG, ARG),
    "pe_f0_dio_events": (ARG, ARG, 0, ARG, ARG, ARG, ARG, ARG, ARG, ARG, UNSUP, ARG, ARG),
    "pe_f0_dio_candidates": (ARG, ARG, 0, ARG, ARG, ARG, ARG, ARG, ARG, ARG, UNSUP, ARG, ARG),
    "pe_f0_dio_fix": (ARG, ARG, 0, ARG, ARG, ARG, ARG, ARG, ARG, ARG, UNSUP, ARG, ARG),
    "pe_f0_stonemask": (ARG, ARG, 0, 0, ARG, ARG, ARG, ARG, ARG, ARG, UNSUP, ARG, ARG),
    "pe_stress_spectra": (ARG, ARG, 0, 0, ARG, ARG, ARG, 0, ARG, ARG, 0, ARG, ARG),
    "pe_stress_rir": (ARG, ARG, 0, ARG, ARG, ARG, ARG, 0, ARG, ARG, 0, ARG, ARG),
    "pe_stress_biquad": (ARG, ARG, 0, ARG, ARG, ARG, ARG, 0, ARG, ARG, 0, ARG, ARG),
    "pe_stress_clip": (ARG, ARG, 0, 0, ARG, ARG, ARG, 0, ARG, ARG, 0, ARG, ARG),
    "pe_stress_agc": (ARG, ARG, 0, ARG, ARG, ARG, ARG, 0, ARG, ARG, 0, ARG, ARG),
}


def _gate_calls():
    """name -> (plans, call(host_meta, n_rows, host, sr)): ``plans(lengths)`` is the entry point's host plan, ``host``
    says whether the host-side parameters (config, coefficients, the impulse responses' plan) are given or null."""
    from pitchextractor_amd import _lib, stress
    lib = _lib.load()
    praat, dio = F.PraatACTracker(16000, 200), F.WorldDioTracker(16000, 200)
    track_plan = lambda n: praat.plan(n)["meta"]  # noqa: E731
    dio_plan = lambda n: dio.plan(n)["meta"]  # noqa: E731
    stress_plan = lambda n: stress.plan_rows(n, np.cumsum([0] + n[:-1]), np.cumsum([0] + n[:-1]))["meta"]  # noqa: E731
    keep = dict(cfg7=praat._cfg, cfg4=dio._cfg, rir=stress.plan_rows([10], [0], [0])["meta"],
                index=np.zeros(2, np.int32), biquad=np.array([1.0, 0.0, 0.0, -1.9, 0.95]),
                agc=np.array([0.95, 0.99, 0.15, 7.9]))
    h = lambda name, host: keep[name].ctypes.data if host else None  # noqa: E731
    n_track, n_dio, n_stress = praat.n_table, dio.n_table, stress.plan_rows([], [], [])["table_floats"]
    N = None
    return keep, {
        "pe_f0_track_frames": (track_plan, lambda m, R, host, sr: lib.pe_f0_track_frames(
            N, N, m, N, N, N, n_track, R, sr, 200, h("cfg7", host), N, N, N, N)),
        "pe_f0_track_path": (track_plan, lambda m, R, host, sr: lib.pe_f0_track_path(
            N, N, N, N, m, R, sr, 200, h("cfg7", host), N, N, 0, N)),
        "pe_f0_dio_bands": (dio_plan, lambda m, R, host, sr: lib.pe_f0_dio_bands(
            N, N, m, N, N, n_dio, R, sr, 200, h("cfg4", host), N, N)),
        "pe_f0_dio_events": (dio_plan, lambda m, R, host, sr: lib.pe_f0_dio_events(
            N, N, m, R, sr, 200, h("cfg4", host), N, N, N, N, 0, N)),
        "pe_f0_dio_candidates": (dio_plan, lambda m, R, host, sr: lib.pe_f0_dio_candidates(
            N, N, N, N, m, R, sr, 200, h("cfg4", host), N, N, N, N, N)),
        "pe_f0_dio_fix": (dio_plan, lambda m, R, host, sr: lib.pe_f0_dio_fix(
            N, N, N, m, R, sr, 200, h("cfg4", host), N, N)),
        "pe_f0_stonemask": (dio_plan, lambda m, R, host, sr: lib.pe_f0_stonemask(
            N, N, m, N, N, dio.n_roots, R, sr, 200, 71.0, N, N)),
        "pe_stress_spectra": (stress_plan, lambda m, R, host, sr: lib.pe_stress_spectra(
            N, N, m, R, 0, N, n_stress, N, N)),
        "pe_stress_rir": (stress_plan, lambda m, R, host, sr: lib.pe_stress_rir(
            N, N, m, R, N, N, h("rir", host), 1, N, h("index", host), N, n_stress, N, N, 0, N)),
        "pe_stress_biquad": (stress_plan, lambda m, R, host, sr: lib.pe_stress_biquad(
            N, N, m, R, h("biquad", host), 1, N, N)),
        "pe_stress_clip": (stress_plan, lambda m, R, host, sr: lib.pe_stress_clip(N, N, m, R, 0.9, 0, N, N, N)),
        "pe_stress_agc": (stress_plan, lambda m, R, host, sr: lib.pe_stress_agc(
            N, N, m, R, h("agc", host), 1, N, N, 0, N)),
    }


def _gate_codes(plan, call):
    valid, empty = plan([1, 2049]), plan([0, 0])
    offset, negative = valid.copy(), valid.copy()
    offset[1, 3] += 1                     # field 3 is a prefix offset in all three plans (frames, frames, samples)
    negative[0, 1] = -1                   # field 1 is the row's length (the shared row header)
    empty_offset, empty_negative = empty.copy(), empty.copy()
    empty_offset[1, 3] += 1
    empty_negative[0, 1] = -1
    at = lambda m: m.ctypes.data  # noqa: E731
    return (call(at(valid), -1, True, 16000), call(at(valid), 65536, True, 16000), call(None, 0, True, 16000),
            call(None, 0, False, 16000), call(None, 1, True, 16000), call(at(offset), 2, True, 16000),
            call(at(negative), 2, True, 16000), call(at(empty), 2, True, 16000), call(at(valid), 2, True, 16000),
            call(at(valid), -1, True, 4000), call(None, 0, True, 4000),
            call(at(empty_offset), 2, True, 16000), call(at(empty_negative), 2, True, 16000))


@pytest.mark.parametrize("name", sorted(GATE_CODES))
def test_gate_return_codes_are_the_parents(name):
    keep, calls = _gate_calls()
    got = _gate_codes(*calls[name])
    assert got == GATE_CODES[name]
