"""The device time base without a device: the two forms of the integer restatement against each other and against
``world.time_base``, the host plan's ABI, and the Python and data layers' opt-in (no GPU needed)."""
import ctypes
import random

import numpy as np
import pytest

from pitchextractor_amd import _lib, build
from pitchextractor_amd import meldataset as md
from pitchextractor_amd import synthetic, world
from tests import world_time_base_ref as tb
from tests.test_data_layer import write_wav

FS, N, HOP = 24000, 1024, 300
FP = 1000.0 * HOP / FS


def steep_fall(L=40):
    f0 = np.append(np.linspace(173.0, 200.0, L - 1), 60.0)        # the last frame: 60 Hz after 200 Hz
    return f0


def _cases():
    """name -> (f0, fs, frame_period_ms, fft_size): the margin curves in the five configurations, the zero-margin rows,
    the steep final fall and the shortest row."""
    cases = {}
    for c, (fs, fft, fp) in enumerate(tb.CONFIGS):
        L = (300, 420, 330, 800, 560)[c]
        for name, f0 in tb.margin_curves(L, seed=c).items():
            cases[f"{name}@{fs}"] = (f0, fs, fp, fft)
    cases["const200@24000"] = (np.full(120, 200.0), 24000, 12.5, 1024)
    cases["unvoiced@24000"] = (np.zeros(120), 24000, 12.5, 1024)
    cases["unvoiced@16000"] = (np.zeros(120), 16000, 12.5, 1024)
    cases["steep@24000"] = (steep_fall(), 24000, 12.5, 1024)
    cases["two@8000"] = (np.array([140.0, 150.0]), 8000, 10.0, 512)
    return cases


CASES = _cases()
MARGIN = [k for k in CASES if k.split("@")[0] in ("glide", "vibrato", "vuv", "trailing")]


@pytest.fixture(scope="module")
def traces():
    return {k: tb.time_base_vec(*v) for k, v in CASES.items()}


def _same_trace(a, b):
    assert a.count == b.count
    for x, y in zip(a.table, b.table):
        assert x.dtype == y.dtype
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a.f0i.view(np.uint64), b.f0i.view(np.uint64))
    np.testing.assert_array_equal(a.lo, b.lo)
    np.testing.assert_array_equal(a.hi, b.hi)
    np.testing.assert_array_equal(a.table.shift.view(np.uint64), b.table.shift.view(np.uint64))


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_int_loop_equals_the_vectorised_form(traces, name):
    a = tb.time_base_int(*CASES[name])
    _same_trace(a, traces[name])
    t = a.table
    assert a.count == t.index.size and (np.diff(t.index) > 0).all()
    fs = CASES[name][1]
    assert ((t.shift * fs > 0) & (t.shift * fs <= 1)).all()
    assert (a.f0i >= 0).all() and a.count <= tb.capacity(tb.coarse_curves(*CASES[name])[0], a.f0i.size, fs)


@pytest.mark.parametrize("name", sorted(MARGIN))
def test_margin_curves_match_the_host_time_base(traces, name):
    """Same pulses and voicing as ``world.time_base``; the shifts differ by the host's accumulated double rounding
    (measured: at most 9.4e-8 samples on rows of up to 4 s; the bound is ten times that)."""
    f0, fs, fp, fft = CASES[name]
    host = world.time_base(f0, fs, fp, fft)
    got = traces[name].table
    assert got.index.size == host.index.size and got.index.size > 50
    np.testing.assert_array_equal(got.index, host.index)
    np.testing.assert_array_equal(got.vuv, host.vuv)
    np.testing.assert_array_equal(got.noise_size, host.noise_size)
    worst = np.abs(got.shift - host.shift).max() * fs
    print(f"[time base] {name}: {host.index.size} pulses, worst |d shift fs| {worst:.3g}")
    assert worst <= 1e-6


def test_the_sample_interpolation_is_numpy_interp(traces):
    for name in MARGIN:
        f0, fs, fp, fft = CASES[name]
        cf, cv = tb.coarse_curves(f0, fs, fp, fft)
        L = len(f0)
        t = np.arange(world.output_length(L, fs, fp)) / fs
        ct = np.arange(L + 1) * (fp / 1000.0)
        vuv = np.interp(t, ct, cv) > 0.5
        want = np.where(vuv, np.interp(t, ct, cf), 500.0)
        np.testing.assert_array_equal(traces[name].f0i.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("name,spacing", [("const200@24000", 120), ("unvoiced@24000", 48)])
def test_zero_margin_rows_are_regular(traces, name, spacing):
    f0, fs, fp, fft = CASES[name]
    host = world.time_base(f0, fs, fp, fft)
    got = traces[name].table
    assert (np.diff(got.index) == spacing).all() and got.index.size > 100
    assert abs(got.index.size - host.index.size) <= 1
    step = np.diff(got.shift * fs)                                # the increment's one rounding, the same every period:
    assert (step >= 0).all() or (step <= 0).all()                 # a drift, no jitter from pulse to pulse
    assert np.abs(got.shift * fs - got.shift[0] * fs).max() < 1e-9
    print(f"[time base] {name}: {got.index.size} pulses, host {host.index.size}")


def test_final_steep_fall(traces):
    f0, fs, fp, fft = CASES["steep@24000"]
    tr = traces["steep@24000"]
    assert (tr.f0i >= 0).all()
    host = world.time_base(f0, fs, fp, fft)
    edge = (len(f0) - 1) * (fp / 1000.0) * fs - 1
    h, g = host.index < edge, tr.table.index < edge
    assert h.sum() == g.sum() > 50
    np.testing.assert_array_equal(tr.table.index[g], host.index[h])
    np.testing.assert_array_equal(tr.table.vuv[g], host.vuv[h])
    assert np.abs(tr.table.shift[g] - host.shift[h]).max() * fs <= 1e-6
    # the host's own curve does go negative there: that is what the clamp removes
    cf = np.where(f0 >= world.lowest_f0(fs, fft), f0, 0.0)
    assert 2 * cf[-1] - cf[-2] < 0 and tb.coarse_curves(f0, fs, fp, fft)[0][-1] == 0.0


# --------------------------------------------------------------------------- the plan's ABI
@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _lib.load()


def _plan(lib, rows, fs, fp, cf=None, cv=None, n_frames=None, meta=True, totals=True, n_rows=None):
    curves = [tb.coarse_curves(f, FS, FP, 1024) for f in rows]     # the values are what matters here, not their origin
    cf_a = np.ascontiguousarray(np.concatenate([c[0] for c in curves])) if cf is None and rows else cf
    cv_a = np.ascontiguousarray(np.concatenate([c[1] for c in curves])) if cv is None and rows else cv
    L = np.array([len(f) for f in rows], np.int64) if n_frames is None else np.asarray(n_frames, np.int64)
    K = lib.pe_world_time_base_plan_fields()
    m = np.zeros((max(len(rows), 1), K), np.int64)
    t = np.zeros(3, np.int64)
    ptr = lambda a: None if a is None or a is False else a.ctypes.data  # noqa: E731
    st = lib.pe_world_time_base_plan(len(rows) if n_rows is None else n_rows, ptr(L), ptr(cf_a), ptr(cv_a), float(fs),
                                     float(fp), ptr(m if meta else None), ptr(t if totals else None))
    return st, m, t


def test_plan_fields_and_totals(lib):
    rows = [np.full(7, 200.0), np.zeros(2), np.full(400, 450.0), np.linspace(100.0, 300.0, 55)]
    st, m, t = _plan(lib, rows, FS, FP)
    assert st == 0 and lib.pe_world_time_base_plan_fields() == 8
    n = np.array([world.output_length(len(f), FS, FP) for f in rows])
    pieces = (n + tb.PIECE - 1) // tb.PIECE
    cap = np.array([tb.capacity(tb.coarse_curves(f, FS, FP, 1024)[0], k, FS) for f, k in zip(rows, n)])
    L = np.array([len(f) for f in rows])
    excl = lambda a: np.cumsum(a) - a  # noqa: E731
    want = np.stack([excl(n), n, L, excl(L + 1), pieces, excl(pieces), excl(cap), cap], axis=1)
    np.testing.assert_array_equal(m, want)
    assert pieces.tolist() == [1, 1, 30, 5] and t.tolist() == [pieces.sum(), cap.sum(), n.sum()]
    assert cap[1] == 600 * 500 // FS + 1 and cap[2] == n[2] * 500 // FS + 1
    # no rows: nothing to lay out
    st, _, t = _plan(lib, [], FS, FP, cf=np.zeros(1), cv=np.zeros(1), n_frames=np.zeros(1, np.int64))
    assert st == 0 and t.tolist() == [0, 0, 0]


def test_plan_refusals(lib):
    rows = [np.full(7, 200.0), np.full(5, 150.0)]
    ok = _plan(lib, rows, FS, FP)[0]
    assert ok == 0
    bad = -1
    cf, cv = (np.concatenate(c) for c in zip(*[tb.coarse_curves(f, FS, FP, 1024) for f in rows]))
    assert _plan(lib, rows, FS, FP, meta=False)[0] == bad
    assert _plan(lib, rows, FS, FP, totals=False)[0] == bad
    for null in ("cf", "cv", "n_frames"):
        assert _plan(lib, rows, FS, FP, **{null: False})[0] == bad, null
    assert _plan(lib, rows, FS, FP, n_frames=[7, 1])[0] == bad                    # L < 2
    for value in (np.nan, np.inf, -np.inf):
        for which in ("cf", "cv"):
            a = (cf if which == "cf" else cv).copy()
            a[9] = value
            assert _plan(lib, rows, FS, FP, **{which: a})[0] == bad, (which, value)
    for value, want in ((FS / 2.0, bad), (np.nextafter(FS / 2.0, 0.0), 0), (-1.0, bad)):
        a = cf.copy()
        a[3] = value
        assert _plan(lib, rows, FS, FP, cf=a)[0] == want, value
    assert _plan(lib, rows, 1000.0, FP)[0] == bad                                  # 500 Hz is not below fs / 2
    assert _plan(lib, rows, 1000.0 + 1e-9, 100.0)[0] == 0
    for fs, fp in ((0.0, FP), (-FS, FP), (np.nan, FP), (np.inf, FP), (FS, 0.0), (FS, -1.0), (FS, np.nan)):
        assert _plan(lib, rows, fs, fp, cf=cf, cv=cv)[0] == bad, (fs, fp)
    assert _plan(lib, rows, FS, FP, n_rows=-1)[0] == bad
    assert _plan(lib, rows, FS, FP, n_rows=65536)[0] == bad
    # the launch entry refuses before any device call: a foreign meta, a missing one, rows out of range
    st, m, t = _plan(lib, rows, FS, FP)
    p = ctypes.c_void_p(8)                                            # never dereferenced: the host checks come first
    run = lambda meta, R=2, fs=FS, fp=FP, stages=7: lib.pe_world_time_base(  # noqa: E731
        p, p, p, meta, R, float(fs), float(fp), stages, p, p, p, p, p, None, None, None, p, 0, None)
    for row, field in [(0, k) for k in range(8)] + [(1, k) for k in range(7)]:
        foreign = m.copy()
        foreign[row, field] += 1
        assert run(foreign.ctypes.data) == bad, (row, field)
    foreign = m.copy()
    foreign[1, 7] = 0                                                 # a last row without a slot
    assert run(foreign.ctypes.data) == bad
    assert run(None) == bad and run(m.ctypes.data, R=-1) == bad and run(m.ctypes.data, R=70000) == bad
    assert run(m.ctypes.data, fp=FP * 2) == bad and run(m.ctypes.data, fs=np.nan) == bad
    assert run(m.ctypes.data, stages=0) == bad and run(m.ctypes.data, stages=8) == bad
    assert run(m.ctypes.data) == -3                                   # a workspace of 0 bytes is too small
    assert run(None, R=0) == 0                                        # no rows: nothing to launch
    assert lib.pe_world_time_base_workspace_bytes(int(t[0])) == 16 * int(t[0])


def test_capacity_covers_every_case(lib, traces):
    for name, (f0, fs, fp, fft) in CASES.items():
        plan = world.TimeBasePlan([f0], fs, fp, fft)
        assert plan.capacity[0] >= traces[name].count, name
        assert plan.capacity[0] == tb.capacity(tb.coarse_curves(f0, fs, fp, fft)[0], plan.samples[0], fs)
        np.testing.assert_array_equal(plan.cf, tb.coarse_curves(f0, fs, fp, fft)[0])
        np.testing.assert_array_equal(plan.cv, tb.coarse_curves(f0, fs, fp, fft)[1])
        assert plan.samples[0] == traces[name].f0i.size


# --------------------------------------------------------------------------- the Python layer
def test_modes_and_refusals(lib):
    for bad in ("gpu", "", None, "Device"):
        with pytest.raises(ValueError, match="time base"):
            world.world_synthesize(np.full(4, 200.0), None, time_base=bad)
        with pytest.raises(ValueError, match="time base"):
            world.resynthesize(None, np.full(4, 200.0), np.full(4, 200.0), FS, time_base=bad)
        with pytest.raises(ValueError, match="time base"):
            world.WorldGenerator(FS, HOP, N, {"time_base": bad})
    assert world.WorldGenerator(FS, HOP, N, {}).time_base == "host"
    assert world.WorldGenerator(FS, HOP, N, {"time_base": "device"}).time_base == "device"
    with pytest.raises(ValueError, match="tables"):
        world._tables_of("gpu", [np.full(4, 200.0)], FS, FP, N, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        world.time_base_device([np.full(4, 200.0)], FS, FP, N, "cpu")
    with pytest.raises(ValueError, match="two frames"):
        world.TimeBasePlan([[100.0]], FS, FP, N)
    with pytest.raises(ValueError, match="finite"):
        world.TimeBasePlan([[100.0, np.nan]], FS, FP, N)
    with pytest.raises(ValueError, match="half the sample rate"):
        world.TimeBasePlan([[100.0, FS / 2.0]], FS, FP, N)
    with pytest.raises(ValueError, match="half the sample rate"):
        world.TimeBasePlan([[100.0, 200.0]], 1000, 10.0, 512)


MEL = {"sample_rate": FS, "win_len": 1024, "n_fft": 1024, "n_mels": 80, "hop_length": HOP}
WORLD_CFG = {"enabled": True, "backend": "hip", "duration": {"min": 0.6, "max": 1.5}}
RS_CFG = {"enabled": True, "backend": "hip", "semitones": [-4, -1, 0, 3], "gain_db_range": [-9.0, 0.0],
          "noise_db": -50.0, "min_voiced_fraction": 0.05, "max_attempts": 3, "aperiodicity": 0.2, "q1": -0.1,
          "modulation": {"vibrato_probability": 0.5, "vibrato_semitones": 0.4, "vibrato_rate_range": [4.0, 6.0]},
          "transform": {"probability": 0.5, "rate_range": [0.8, 1.25], "formant_ratio_range": [0.9, 1.1]}}


def _files(tmp_path, durations):
    lines = []
    for i, dur in enumerate(durations):
        wave, f0, _ = synthetic.utterance(i, duration=dur)
        p = tmp_path / f"u{i}.wav"
        write_wav(p, wave, FS, "float32")
        np.save(str(p) + "_f0.npy", f0)
        lines.append(f"{p}|0\n")
    return lines


def _ds(lines, mode):
    key = {} if mode is None else {"time_base": mode}
    syn = {"enabled": True, "absolute_count": 12, "pitch_shift": {"enabled": False},
           "world_vocoder": {**WORLD_CFG, **key}, "world_resynthesis": {**RS_CFG, **key}}
    return md.MelDataset(lines, mel_params=dict(MEL), verbose=False, synthetic_data=syn)


def _items(ds, seed):
    random.seed(seed); np.random.seed(seed)
    items = [ds[3 + i] for i in range(12)]
    return items, random.getstate(), np.random.get_state()


def _same_state(a, b):
    assert a[0] == b[0]
    assert a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]


def test_dataset_keys(tmp_path, caplog):
    import logging
    lines = _files(tmp_path, [1.0])
    for block in ("world_vocoder", "world_resynthesis"):
        with pytest.raises(ValueError, match="time base"):
            md.MelDataset(lines, mel_params=dict(MEL), verbose=False, synthetic_data={
                "enabled": True, "absolute_count": 2, block: {"enabled": True, "backend": "hip", "time_base": "gpu"}})
    with caplog.at_level(logging.WARNING):
        ds = _ds(lines, "device")
    assert not [r for r in caplog.records if "time_base" in r.getMessage()]          # the key is read: no warning
    assert "time_base" in md.WORLD_RESYNTHESIS.KEYS
    assert ds.synthetic_resynthesis_config["time_base"] == "device" and ds._world_generator.time_base == "device"
    assert _ds(lines, None).synthetic_resynthesis_config["time_base"] == "host"


def test_device_mode_ships_empty_tables_and_changes_no_draw(tmp_path, monkeypatch):
    lines = _files(tmp_path, [1.0, 3.0, 1.6])
    host, host_rand, host_np = _items(_ds(lines, "host"), 11)
    absent, absent_rand, absent_np = _items(_ds(lines, None), 11)
    # without the key: the host mode's items, field for field
    _same_state((host_rand, host_np), (absent_rand, absent_np))
    for a, b in zip(host, absent):
        assert type(a[-1]) is type(b[-1])
        for u, v in zip(a[:-1], b[:-1]):
            np.testing.assert_array_equal(np.asarray(u), np.asarray(v))
        for name, u, v in zip(a[-1]._fields, a[-1], b[-1]):
            np.testing.assert_array_equal(np.asarray(u), np.asarray(v), err_msg=name)

    def refuse(*a, **k):
        raise AssertionError("the worker computed a host time base in device mode")

    monkeypatch.setattr(world, "time_base", refuse)
    dev, dev_rand, dev_np = _items(_ds(lines, "device"), 11)
    _same_state((host_rand, host_np), (dev_rand, dev_np))
    kinds = set()
    for a, b in zip(host, dev):
        assert type(a[-1]) is type(b[-1]) and isinstance(b[-1], (md.WorldRequest, md.ResynthesisRequest))
        kinds.add(type(b[-1]).__name__)
        for u, v in zip(a[:-1], b[:-1]):                              # audio, labels, silences, first frame, rate
            np.testing.assert_array_equal(np.asarray(u), np.asarray(v))
        for name, u, v in zip(a[-1]._fields, a[-1], b[-1]):
            if name in ("index", "shift", "vuv"):
                assert np.asarray(v).size == 0 and np.asarray(v).dtype == np.asarray(u).dtype, name
                assert np.asarray(u).size > 0
            else:
                np.testing.assert_array_equal(np.asarray(u), np.asarray(v), err_msg=name)
    assert kinds == {"WorldRequest", "ResynthesisRequest"}
    # the collated batches carry the empty tables as they are
    batch = md.Collater(return_wave=True)([b for b in dev if isinstance(b[-1], md.WorldRequest)][:2])
    packs = [p for p in batch if isinstance(p, md.WorldBatch)]
    assert len(packs) == 1 and all(t[0].size == 0 for t in packs[0].tables)
