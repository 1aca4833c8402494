"""The stress conditions and melody metrics on the device (``pitchextractor_amd.stress``, ``csrc/stress.hip``) against
the float64 restatement tests/stress_ref.py, at the smallest shapes at which each kernel can go wrong.  Every figure
is printed before it is asserted."""
import math

import numpy as np
import pytest
import torch

from oracle import model_ref
from pitchextractor_amd import inference, stress
from pitchextractor_amd.resample import RaggedResampler
from tests import stress_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32
S = R.BLOCK


def run_layouts(fn, rows, device):
    """``fn(x, lengths, row_ids)`` on the rows packed (with trailing slack), padded (garbage past each row) and one by
    one: the three give bit-identical rows, and everything outside the rows is zero.  Returns the rows."""
    rows = [np.ascontiguousarray(r, dtype=f32) for r in rows]
    lengths, ids = [int(r.size) for r in rows], list(range(len(rows)))
    packed = torch.from_numpy(np.concatenate(rows + [np.full(3, 7.0, f32)])).to(device)
    yp = fn(packed, lengths, ids)
    assert yp.shape == packed.shape and yp.dtype == torch.float32
    yp = yp.cpu().numpy()
    assert np.all(yp[sum(lengths):] == 0)
    out = np.split(yp[:sum(lengths)], np.cumsum(lengths)[:-1])
    pad = torch.full((len(rows), max(lengths) + 5), 7.0, dtype=torch.float32, device=device)
    for r, row in enumerate(rows):
        pad[r, :row.size] = torch.from_numpy(row).to(device)
    yd = fn(pad, lengths, ids).cpu().numpy()
    for r, n in enumerate(lengths):
        assert np.array_equal(yd[r, :n], out[r]), f"row {r}: padded differs from packed"
        assert np.all(yd[r, n:] == 0)
        alone = fn(torch.from_numpy(rows[r]).to(device), None, [r]).cpu().numpy()
        assert alone.shape == (n,) and np.array_equal(alone, out[r]), f"row {r}: alone differs from packed"
    return out


# --------------------------------------------------------------------------------------------------------------- rir
ROW_LENGTHS = (0, 1, 2047, 2048, 2049, 3 * S + 5)
RIR_LENGTHS = (1, 2048, 2049, 5000)                                # one, one, two and three partitions


@pytest.fixture(scope="module")
def rir_set():
    return [stress.prepare_rir(R.decaying_rir(n, 10 + k)) for k, n in enumerate(RIR_LENGTHS)]


@pytest.mark.parametrize("peak", [0.5, 3.0])
@pytest.mark.parametrize("index", [(0, 3, 1, 2, 3, 2), (3, 0, 3, 0, 1, 3)])
def test_rir(peak, index, rir_set, hip_device):
    rng = np.random.default_rng(int(peak * 10) + index[0])
    rows = []
    for n, k in zip(ROW_LENGTHS, index):
        x = rng.standard_normal(n)
        if n:
            x *= peak / float(np.max(np.abs(np.convolve(x, rir_set[k].astype(np.float64))[:n])))
        rows.append(x.astype(f32))
    assert any(RIR_LENGTHS[k] > n > 0 for n, k in zip(ROW_LENGTHS, index))        # an impulse response longer than its row
    rirs = stress.RirSet(rir_set)
    got = run_layouts(lambda x, lengths, ids: stress.apply_rir(x, rirs, [index[i] for i in ids], lengths), rows,
                      hip_device)
    dev = yard = 0.0
    for n, k, x, y in zip(ROW_LENGTHS, index, rows, got):
        if n == 0:
            assert y.size == 0
            continue
        ref, p, scaled = R.rir(x, rir_set[k])
        assert abs(p - peak) < 0.01 * peak and scaled == (peak > 0.99)            # rounding cannot flip the branch
        y32, dtype = R.rir_partitioned(x, rir_set[k], np.float32)
        assert dtype == np.complex64 and y32.dtype == np.float32
        p32 = np.max(np.abs(y32))
        if p32 > f32(0.99):
            y32 = y32 / (p32 + f32(1e-6))
        dev = max(dev, float(np.max(np.abs(y.astype(np.float64) - ref))))
        yard = max(yard, float(np.max(np.abs(y32.astype(np.float64) - ref))))
    print(f"[stress] rir peak {peak} index {index}: kernel {dev:.3e} yardstick {yard:.3e} ratio {dev / yard:.2f}")
    assert dev <= 4.0 * yard


def test_rir_single_index_and_cache(rir_set, hip_device):
    rirs = stress.RirSet(rir_set)
    x = torch.from_numpy((0.1 * np.random.default_rng(0).standard_normal(3000)).astype(f32)).to(hip_device)
    a = stress.apply_rir(x, rirs, 2)
    b = stress.apply_rir(x, stress.RirSet(rir_set), [2])                        # an equal set finds the kept spectra
    assert torch.equal(a, b) and len(stress._RIR_SPECTRA) >= 1
    delta = stress.apply_rir(x, stress.RirSet([np.array([1.0], f32)]))
    assert float((delta - x).abs().max()) <= 1e-6                               # h = {1}
    with pytest.raises(ValueError):
        stress.apply_rir(x, rirs, 4)


# ------------------------------------------------------------------------------------------------------------ mic eq
PIECE = 512
EQ_LENGTHS = (1, 2, 3, PIECE - 1, PIECE, PIECE + 1, 3 * PIECE + 77)
EQ_CURVES = {"80 Hz": [{"freq": 80.0, "gain_db": 2.0, "Q": 0.9}],
             "0 dB": [{"freq": 1000.0, "gain_db": 0.0, "Q": 0.7}],
             **{name: list(curve) for name, curve in stress.MICROPHONE_PROFILES.items()}}


@pytest.fixture(scope="module")
def eq_rows():
    rng = np.random.default_rng(5)
    rows = [(0.4 * rng.standard_normal(n)).astype(f32) for n in EQ_LENGTHS]
    rows.append((3.0 * rng.standard_normal(2 * PIECE + 9)).astype(f32))          # drives the clamp
    return rows


@pytest.mark.parametrize("name", sorted(EQ_CURVES))
def test_microphone_eq(name, eq_rows, hip_device):
    assert stress.plan_rows([1], [0], [0])["piece"] == PIECE
    curve = EQ_CURVES[name]
    got = run_layouts(lambda x, lengths, ids: stress.apply_microphone_eq(x, 24000, curve, lengths), eq_rows, hip_device)
    worst = 0.0
    for x, y in zip(eq_rows, got):
        ref = R.microphone_eq(x, 24000, curve)
        worst = max(worst, float(np.max(np.abs(y.astype(np.float64) - ref.astype(np.float64)))))
    print(f"[stress] microphone eq {name}: worst |kernel - ref| {worst:.3e} (bound {2.0 ** -21:.3e})")
    assert np.max(np.abs(got[-1])) == 1.0                                        # the clamp was driven
    # one float32 rounding of a value <= 1 per stage, later stages amplify by at most 10^(6/20)
    assert worst <= 2.0 ** -21
    if name == "0 dB":
        assert all(np.array_equal(y, np.clip(x, -1, 1)) for x, y in zip(eq_rows, got))


# ----------------------------------------------------------------------------------------------------------- clipping
@pytest.fixture(scope="module")
def clip_rows():
    rng = np.random.default_rng(9)
    chunk = stress.plan_rows([1], [0], [0])["clip_chunk"]
    assert chunk == 1024
    rows = [np.array([0.3], f32), np.array([-0.8, 0.2], f32),
            (np.round(rng.uniform(-1, 1, 3000) * 8) / 8).astype(f32),           # 16 levels: ties
            np.concatenate([np.zeros(5, f32), rng.standard_normal(200).astype(f32)]),   # zeros: threshold 0 at 100 %
            *[rng.standard_normal(n).astype(f32) for n in (chunk - 1, chunk, chunk + 1, 5000)],
            (1e-3 * rng.standard_normal(777)).astype(f32)]
    return rows


@pytest.mark.parametrize("percent", [0.0, 0.3, 2.0, 10.0, 100.0])
def test_sample_clipping(percent, clip_rows, hip_device):
    got = run_layouts(lambda x, lengths, ids: stress.apply_sample_clipping(x, percent, lengths), clip_rows, hip_device)
    packed = torch.from_numpy(np.concatenate(clip_rows)).to(hip_device)
    _, thr = stress.apply_sample_clipping(packed, percent, [r.size for r in clip_rows], return_threshold=True)
    thr = thr.cpu().numpy()
    for r, (x, y) in enumerate(zip(clip_rows, got)):
        ref, t = R.sample_clipping(x, percent)
        assert (math.isnan(thr[r]) if t is None else thr[r] == t), (r, thr[r], t)
        assert np.array_equal(y, ref), f"row {r} at {percent} %"
    if percent == 100.0:
        assert thr[3] == 0 and np.array_equal(got[3], clip_rows[3])            # threshold 0 is a copy
    if percent == 0.0:
        assert all(np.array_equal(x, y) for x, y in zip(clip_rows, got))


# ---------------------------------------------------------------------------------------------------------------- agc
@pytest.mark.parametrize("level", [2.0, 10.0])
def test_agc_pumping(level, hip_device):
    sr = 2000
    s = stress.agc_parameters(level, sr, 0.15)["smoothing"]
    assert 25 <= s <= 240
    long_row = R.agc_input(5000, 3)
    rows = [long_row[150:150 + s], long_row[150:150 + s + 1], long_row]
    got = run_layouts(lambda x, lengths, ids: stress.apply_agc_pumping(x, level, sr, 0.15, lengths), rows, hip_device)
    worst = 0.0
    for x, y in zip(rows, got):
        ref, raw, smooth, p = R.agc_pumping(x, level, sr, 0.15, return_stages=True)
        if x.size == 5000:
            assert raw.min() == f32(1.0 / p["max_gain"]) and raw.max() == f32(p["max_gain"]) and np.abs(ref).max() == 1.0
        err = np.abs(y.astype(np.float64) - ref) / np.maximum(np.abs(ref), 2.0 ** -20)
        worst = max(worst, float(err.max()))
    print(f"[stress] agc level {level} smoothing {s}: worst relative deviation {worst:.3e} (bound {3 * 2.0 ** -23:.3e})")
    # one float32 rounding each for the gain, the smoothed gain and the product
    assert worst <= 3 * 2.0 ** -23
    with pytest.raises(ValueError):
        stress.apply_agc_pumping(torch.zeros(s - 1, device=hip_device), level, sr)
    x = torch.from_numpy(long_row).to(hip_device)
    assert torch.equal(stress.apply_agc_pumping(x, 0.0, sr), x)


# ----------------------------------------------------------------------------------------------------------- resample
def test_resample_condition(hip_device):
    rng = np.random.default_rng(2)
    lengths = [2400, 1, 3001]
    x = torch.zeros((3, 3100), dtype=torch.float32, device=hip_device)
    for r, n in enumerate(lengths):
        x[r, :n] = torch.from_numpy((0.3 * rng.standard_normal(n)).astype(f32)).to(hip_device)
    y, out_lengths = stress.apply_resample_condition(x, 24000, 8000, lengths)
    down, _ = RaggedResampler(8000)(x, [24000] * 3, lengths)
    down_lengths = [-(-n // 3) for n in lengths]
    up, up_lengths = RaggedResampler(24000)(down, [8000] * 3, down_lengths)
    assert torch.equal(y, up) and out_lengths == up_lengths.cpu().tolist() == [3 * n for n in down_lengths]
    same, same_lengths = stress.apply_resample_condition(x, 24000, 24000, lengths)
    assert same_lengths == lengths and same.shape == x.shape
    for r, n in enumerate(lengths):
        assert torch.equal(same[r, :n], x[r, :n]) and bool((same[r, n:] == 0).all())
    packed = torch.cat([x[r, :n] for r, n in enumerate(lengths)])
    again, _ = stress.apply_resample_condition(packed, 24000, 24000, lengths)
    assert torch.equal(again[:, :3001], same[:, :3001])


# ------------------------------------------------------------------------------------------------------------ metrics
def test_melody_metrics(hip_device):
    rng = np.random.default_rng(4)
    n = 700
    ref = np.where(rng.uniform(size=n) < 0.7, rng.uniform(80.0, 600.0, n), 0.0).astype(f32)
    kinds = rng.integers(0, 6, n)
    cents = np.choose(kinds, [rng.uniform(-45, 45, n), rng.uniform(60, 540, n), 1200 + rng.uniform(-45, 45, n),
                              -1200 + rng.uniform(-45, 45, n), 2400 + rng.uniform(60, 500, n),
                              -rng.uniform(660, 1100, n)])
    pred = (np.where(ref > 0, ref, 200.0) * 2.0 ** (cents / 1200.0)).astype(f32)
    # a predicted 0 Hz (clipped to 1e-5) and a predicted 7 Hz (below the voicing threshold) on voiced frames: the
    # reference is placed a whole number of octaves plus 300 cents above them, far from every boundary
    for value, eff, octaves in ((0.0, float(f32(1e-5)), (23, 24, 25)), (7.0, 7.0, (4, 5, 6))):
        at = np.nonzero((ref > 0) & (rng.uniform(size=n) < 0.1))[0]
        ref[at] = (eff * 2.0 ** (0.25 + rng.choice(octaves, at.size))).astype(f32)
        pred[at] = value
    assert ref[ref > 0].min() > 79.0 and ref.max() < 700.0
    unvoiced = np.nonzero(ref == 0)[0]
    pred[unvoiced[::3]] = 0.0
    pred[unvoiced[1::3]] = 7.0
    base = pred.copy()
    base[rng.uniform(size=n) < 0.1] = 0.0
    rows = [(pred, ref, base), (pred[:300], ref[:450], base[:200]), (pred[:5], np.zeros(5, f32), base[:5]),
            (pred[:1], ref[:1], base[:1])]
    want = []
    for p, f, b in rows:
        m, d = R.melody_metrics(f, p, b, return_diffs=True)
        margin = R.boundary_margin_cents(d)
        print(f"[stress] metrics row of {m['n_frames']} frames: voiced {m['n_voiced']} margin {margin:.2f} cents")
        assert margin >= 1.0
        want.append(m)
    assert want[0]["n_voiced"] > 300 and 0 < want[0]["OctaveError"] < want[0]["RCA"] < 1 and want[2]["n_voiced"] == 0
    got = stress.melody_metrics_rows([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], 10.0, hip_device)
    plain = stress.melody_metrics_rows([r[0] for r in rows], [r[1] for r in rows], None, 10.0, hip_device)
    for g, pl, w in zip(got, plain, want):
        print(f"[stress]   kernel {g}")
        assert g["n_voiced"] == w["n_voiced"] and g["n_frames"] == w["n_frames"]
        for k in ("RPA", "RCA", "VUV", "OctaveError", "VUV_flips"):
            assert (math.isnan(g[k]) and math.isnan(w[k])) or abs(g[k] - w[k]) <= 1e-12, (k, g[k], w[k])
        assert math.isnan(pl["VUV_flips"]) and all(pl[k] == g[k] or math.isnan(g[k]) for k in ("RPA", "RCA", "VUV"))
    one = inference.melody_metrics(torch.from_numpy(pred).to(hip_device), ref, baseline=base, device=hip_device)
    assert one == got[0]
    assert set(one) == set(stress.METRIC_KEYS)


# -------------------------------------------------------------------------------------------------------------- sweep
def test_stress_sweep(tmp_path, hip_device):
    torch.save({"model": model_ref.seeded_state(31, hidden_size=64, num_layers=2)}, tmp_path / "r.pth")
    net = inference.load_model(tmp_path / "r.pth", device=hip_device)
    rng = np.random.default_rng(8)
    t = np.arange(24000) / 24000.0
    items = []
    for f0 in (110.0, 220.0):
        audio = (0.5 * np.sin(2 * np.pi * f0 * t) + 0.01 * rng.standard_normal(t.size)).astype(f32)
        items.append({"audio": audio, "reference_f0": np.full(81, f0, f32)})
    conditions = [stress.Condition("clipping", "clip 0 %", percent=0.0),
                  stress.Condition("clipping", "clip 10 %", percent=10.0),
                  stress.Condition("microphone", "headset", curve="headset")]
    out = inference.stress_sweep(net, items, conditions)
    assert len(out["baseline"]) == 2 and len(out["conditions"]) == 6
    keys = {"condition", "kind", "item", *stress.METRIC_KEYS}
    assert all(set(rec) == keys for rec in out["baseline"] + out["conditions"])
    assert [(rec["condition"], rec["item"]) for rec in out["conditions"]] == [(c.label, i) for c in conditions
                                                                              for i in range(2)]
    same = lambda a, b: a == b or (isinstance(a, float) and math.isnan(a) and math.isnan(b))  # noqa: E731
    for rec, clean in zip(out["conditions"][:2], out["baseline"]):
        assert rec["VUV_flips"] == 0.0 and clean["VUV_flips"] == 0.0 and clean["condition"] == "clean"
        assert all(same(rec[k], clean[k]) for k in stress.METRIC_KEYS)           # 0 % is the clean run exactly
        assert rec["n_frames"] == 81
