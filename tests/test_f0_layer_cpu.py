"""What the two F0 trackers share on the host (``f0_tracker._RaggedTracker``, ``fft_roots`` / ``real_split_roots``,
``NATIVE_BACKENDS``); no GPU needed."""
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


@pytest.mark.parametrize("sr,hop", [(16000, 200), (24000, 300), (48000, 600)])
def test_table_bytes_are_unchanged(sr, hop):
    for C in (64, 512):
        assert F.fft_roots(C).shape == (C, 2) and F.fft_roots(C).dtype == np.float64
        assert F.real_split_roots(C).shape == (C + 1, 2) and F.real_split_roots(C).dtype == np.float64
    praat, dio = F.PraatACTracker(sr, hop), F.WorldDioTracker(sr, hop)
    for name, got, want in (("praat tables", praat.host_tables(), _praat_tables_inline(praat)),
                            ("dio tables", dio.host_tables(), _dio_tables_inline(dio)),
                            ("stonemask roots", dio.host_roots(), _dio_roots_inline())):
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
