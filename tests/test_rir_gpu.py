"""The room-response kernels (``csrc/rir_synth.hip`` through ``pitchextractor_amd.rir``) on the device against the
float64 restatement in tests/rir_ref.py.

Shapes: 8 kHz and rooms of about 3 x 2.5 x 2.2 m keep the restatement under a second per row.  With T the plan's tile
length, the rows have N = 2 T + 77 (two full tiles and an odd remainder), a source 10 cm from the microphone (taps
before k = 0 are dropped), N = 40 with the direct path at 32.3 samples (taps straddle the last sample), ``max_order``
0 and 1, one wall at beta = 0 among walls at 1 (0^0), and the anechoic room whose one delay is an integer.

The accuracy bound is derived, not measured: per sample ``|h - ref| <= 2^-24 |ref| + K 2^-44``, one float32 rounding
plus at most one unit of the fixed-point grid for each of the K contributions to the sample (a contribution's double
value differs from the restatement's by far less than 2^-44, so its rounding to the grid moves by at most one unit).
Every figure is printed before it is asserted."""
import functools
import math

import numpy as np
import pytest
import torch

from pitchextractor_amd import rir, stress
from tests import rir_ref as R

pytestmark = pytest.mark.gpu

FS = 8000.0
ROOM = {"dims": (3.0, 2.5, 2.2), "source": (1.1, 0.9, 1.3), "mic": (2.2, 1.7, 1.0)}
ANECHOIC = {"dims": (5.0, 4.0, 3.0), "source": (1.0, 1.0, 1.0), "mic": (3.0, 1.0, 1.0), "beta": 0.0, "n_samples": 300}
SIX = [0.9, 0.7, 0.8, 0.6, 0.95, 0.5]


def host(t):
    return t.detach().cpu().numpy()


def _key(room):
    return tuple((k, tuple(np.asarray(room[k], dtype=np.float64).reshape(-1).tolist())) for k in sorted(room))


@functools.lru_cache(maxsize=None)
def _reference(key, fs, c, max_order):
    h, K, _ = R.image_source({k: (v[0] if k == "n_samples" else v) for k, v in key}, fs, c, max_order)
    h.setflags(write=False)
    K.setflags(write=False)
    return h, K


def reference(room, fs=FS, c=343.0, max_order=None):
    """``(h, K)`` of the restatement, computed once per room and shared."""
    return _reference(_key(room), fs, c, max_order)


def tile():
    return rir.plan_rooms([], FS)["tile"]


def assert_within_bound(got, room, what, **kw):
    h, K = reference(room, **kw)
    err = np.abs(got.astype(np.float64) - h.astype(np.float64))
    bound = 2.0 ** -24 * np.abs(h.astype(np.float64)) + K * 2.0 ** -44
    at = int(np.argmax(err - bound))
    print(f"{what}: N {h.size}, at most {int(K.max())} contributions, {float(np.mean(got == h)):.4%} of the samples "
          f"bit-equal, max |err| {err.max():.3e}; tightest at k {at}: err {err[at]:.3e}, bound {bound[at]:.3e}")
    assert got.dtype == np.float32 and got.shape == h.shape
    assert np.all(err <= bound), what


# ------------------------------------------------------------------------------------------------------------- accuracy
def test_accuracy_of_a_ragged_batch(hip_device):
    T = tile()
    rooms = {"six betas": dict(ROOM, beta=SIX, n_samples=2 * T + 77),
             "source 10 cm from the microphone": dict(ROOM, mic=(1.17, 0.95, 1.35), beta=0.8, n_samples=700),
             "taps straddle the last sample": dict(ROOM, beta=0.9, n_samples=40),
             "one wall at 0 among walls at 1": dict(ROOM, beta=[1.0, 1.0, 0.0, 1.0, 1.0, 1.0], n_samples=600)}
    assert math.dist(rooms["source 10 cm from the microphone"]["source"],
                     rooms["source 10 cm from the microphone"]["mic"]) < 0.1
    tau = math.dist(ROOM["source"], ROOM["mic"]) * FS / 343.0
    assert 40 - 41 < tau < 40 and tau + 41 > 40                  # the direct path's taps run past N = 40
    h, lengths = rir.synthesize(list(rooms.values()), FS, device=hip_device)
    assert lengths == [r["n_samples"] for r in rooms.values()] and h.numel() == sum(lengths)
    got, at = host(h), 0
    for (what, room), n in zip(rooms.items(), lengths):
        assert_within_bound(got[at:at + n], room, what)
        at += n
    K = reference(rooms["six betas"])[1]
    assert K.max() > 1000 and np.count_nonzero(got) > 0.8 * got.size       # a dense response, not a handful of taps


@pytest.mark.parametrize("max_order", [0, 1])
def test_accuracy_at_a_reflection_limit(hip_device, max_order):
    rooms = [dict(ROOM, beta=0.9, n_samples=tile() + 3), dict(ROOM, beta=SIX, n_samples=40)]
    h, lengths = rir.synthesize(rooms, FS, max_order=max_order, device=hip_device)
    got = host(h)
    assert_within_bound(got[:lengths[0]], rooms[0], f"max_order {max_order}", max_order=max_order)
    assert_within_bound(got[lengths[0]:], rooms[1], f"max_order {max_order}, N 40", max_order=max_order)
    K = reference(rooms[0], max_order=max_order)[1]
    assert int(K.max()) <= (1, 7)[max_order] and np.count_nonzero(K) >= 70


def test_an_integer_delay_is_exactly_one_sample(hip_device):
    """2 m at 320 m/s and 16 kHz: the delay is 100 samples, sin(pi f) is 0 and no tap divides by it."""
    h, _ = rir.synthesize([ANECHOIC], 16000.0, c=320.0, device=hip_device)
    got = host(h)
    print(f"h[100] = {got[100]!r}, 1 / (8 pi) = {np.float32(1.0 / (8.0 * math.pi))!r}, "
          f"{int(np.count_nonzero(got))} non-zero samples")
    assert got[100] == np.float32(1.0 / (8.0 * math.pi))
    assert np.count_nonzero(got) == 1 and np.all(np.delete(got, 100) == 0.0)
    assert_within_bound(got, ANECHOIC, "anechoic", fs=16000.0, c=320.0)


# --------------------------------------------------------------------------------------------------------- bit identity
def test_a_row_is_the_same_wherever_it_is_made(hip_device):
    T = tile()
    rooms = [dict(ROOM, beta=SIX, n_samples=T + 101),
             {"dims": (4.1, 3.3, 2.6), "source": (1.3, 2.1, 0.7), "mic": (3.0, 0.8, 1.9), "beta": 0.6, "n_samples": 2 * T + 1},
             {"dims": (2.4, 2.9, 3.1), "source": (0.5, 1.4, 2.2), "mic": (1.8, 2.0, 0.9),
              "beta": [0.3, 0.8, 0.9, 0.4, 0.7, 0.85], "n_samples": 333}]
    lengths = [r["n_samples"] for r in rooms]
    alone = [rir.synthesize([r], FS, device=hip_device)[0] for r in rooms]
    assert [a.numel() for a in alone] == lengths and all(torch.count_nonzero(a) > n // 2 for a, n in zip(alone, lengths))
    batch, _ = rir.synthesize(rooms, FS, device=hip_device)
    backwards, _ = rir.synthesize(rooms[::-1], FS, device=hip_device)
    assert torch.equal(batch, torch.cat(alone)) and torch.equal(backwards, torch.cat(alone[::-1]))
    odd, at = [], 1
    for n in lengths:
        odd.append(at)
        at += n + n % 2 + 2                                       # keeps every start odd
    packed = torch.zeros(at + 3, dtype=torch.float32, device=hip_device)
    assert rir.synthesize(rooms, FS, out=packed, offsets=odd)[0] is packed
    width = max(lengths) + 5
    padded = torch.zeros((len(rooms), width), dtype=torch.float32, device=hip_device)
    rir.synthesize(rooms, FS, out=padded, offsets=[r * width for r in range(len(rooms))])
    gaps = torch.ones(packed.numel(), dtype=torch.bool, device=hip_device)
    for r, (o, n) in enumerate(zip(odd, lengths)):
        assert torch.equal(packed[o:o + n], alone[r]), r
        assert torch.equal(padded[r, :n], alone[r]) and torch.count_nonzero(padded[r, n:]) == 0, r
        gaps[o:o + n] = False
    assert torch.count_nonzero(packed[gaps]) == 0
    with pytest.raises(ValueError):
        rir.synthesize(rooms, FS, out=packed[:100], offsets=odd)


# ---------------------------------------------------------------------------------------------------------------- decay
def test_decay_time_against_the_restatement(hip_device):
    a = 3.0 * math.log(10.0) / (0.2 * FS)
    k = np.arange(1200)
    rows = {"six betas": np.array(reference(dict(ROOM, beta=SIX, n_samples=2 * tile() + 77))[0]),
            "uniform 0.71": np.array(reference(dict(ROOM, beta=0.71, n_samples=1800))[0]),
            "exponential": (np.exp(-a * k) * np.where(k % 2, -1.0, 1.0)).astype(np.float32),
            "never reaches -25 dB": np.ones(257, np.float32),
            "one sample": np.array([0.5], np.float32)}
    lengths = [int(v.size) for v in rows.values()]
    packed = torch.from_numpy(np.concatenate(list(rows.values()))).to(hip_device)
    got, curve = rir.measure_t60(packed, lengths, FS, return_curve=True)
    width = max(lengths) + 3
    padded = torch.zeros((len(rows), width), dtype=torch.float32, device=hip_device)
    for r, v in enumerate(rows.values()):
        padded[r, :v.size] = torch.from_numpy(v)
    again = rir.measure_t60(padded, lengths, FS)
    curve, at = host(curve), 0
    for r, (what, v) in enumerate(rows.items()):
        want = R.schroeder(v, FS, margin=1e-6)
        line = {key: float(got[key][r]) for key in rir.DECAY_KEYS}
        print(f"{what}: {line}; restatement t60 {want['t60']!r}, k {want['k_lo']} .. {want['k_hi']}")
        assert (line["k_lo"], line["k_hi"]) == (want["k_lo"], want["k_hi"]), what
        for key in ("t60", "slope", "intercept"):
            if math.isnan(want[key]):
                assert math.isnan(line[key]), (what, key)
            else:
                assert abs(line[key] - want[key]) <= 1e-9 * abs(want[key]), (what, key)
        assert line["db_last"] == pytest.approx(want["db_last"], rel=1e-9, abs=1e-9) or \
            (np.isinf(want["db_last"]) and line["db_last"] == want["db_last"])
        finite = np.isfinite(want["db"])
        assert np.allclose(curve[at:at + v.size][finite], want["db"][finite], rtol=1e-6, atol=1e-5), what
        assert all(np.array_equal(got[key][r], again[key][r], equal_nan=True) for key in rir.DECAY_KEYS), what
        at += v.size
    assert not math.isnan(got["t60"][1]) and abs(got["t60"][2] - 0.2) < 0.01 * 0.2
    assert math.isnan(got["t60"][3]) and got["k_hi"][3] == 257


# ---------------------------------------------------------------------------------------------------------- calibration
def test_calibration_follows_the_restatement(hip_device):
    beta, t60, h, path = rir.calibrate(ROOM, 0.15, FS, device=hip_device, return_path=True)
    want_beta, want_t60, want_path = R.calibrate(ROOM, 0.15, FS)
    for step, ((b, t), (wb, wt)) in enumerate(zip(path, want_path)):
        print(f"step {step}: beta {b!r} / {wb!r}, measured {t!r} / {wt!r} s, relative difference "
              f"{abs(t - wt) / abs(wt):.3e}")
    assert [b for b, _ in path] == [b for b, _ in want_path] and beta == want_beta
    assert all(abs(t - wt) <= 1e-9 * abs(wt) for (_, t), (_, wt) in zip(path, want_path))
    assert abs(t60 - 0.15) <= 0.02 * 0.15 and t60 == path[-1][1] and abs(t60 - want_t60) <= 1e-9 * want_t60
    assert h.numel() == math.ceil(1.5 * 0.15 * FS)
    assert_within_bound(host(h), dict(ROOM, beta=beta, n_samples=h.numel()), "the calibrated response")
    with pytest.raises(ValueError):
        rir.calibrate(ROOM, 0.15, FS, rtol=1e-9, max_iter=2, device=hip_device)


# ----------------------------------------------------------------------------------------------------------- end to end
def test_library_feeds_the_rir_condition(hip_device):
    rooms = {"booth": ROOM, "den": {"dims": (3.4, 2.8, 2.3), "source": (1.0, 1.9, 1.2), "mic": (2.5, 0.9, 1.5)}}
    lib = rir.room_library(FS, rooms, {"booth": (0.12,), "den": (0.15,)}, device=hip_device)
    print([{k: e[k] for k in ("room", "target_t60", "t60", "beta", "index")} for e in lib.entries])
    assert [(e["room"], e["target_t60"], e["index"]) for e in lib.entries] == [("booth", 0.12, 0), ("den", 0.15, 1)]
    assert all(abs(e["t60"] - e["target_t60"]) <= 0.02 * e["target_t60"] and 0.0 < e["beta"] < 0.9999
               for e in lib.entries)
    assert lib.lengths == [math.ceil(1.5 * 0.12 * FS), math.ceil(1.5 * 0.15 * FS)] and lib.h.numel() == sum(lib.lengths)
    rirs = lib.rir_set()
    assert rirs is lib.rir_set() and isinstance(rirs, stress.RirSet) and len(rirs) == 2
    arrays = np.split(host(lib.h), [lib.lengths[0]])
    by_hand = stress.RirSet([stress.prepare_rir(a) for a in arrays])
    rng = np.random.default_rng(5)
    lengths = [3000, 4097]
    x = torch.from_numpy(rng.uniform(-0.5, 0.5, sum(lengths)).astype(np.float32)).to(hip_device)
    for index in (0, 1, [1, 0]):
        y = stress.apply_rir(x, rirs, index, lengths)
        assert torch.equal(y, stress.apply_rir(x, by_hand, index, lengths)) and torch.count_nonzero(y) > 7000
    conds = lib.conditions()
    assert len(conds) == 2 * 14
    assert lib.select("booth", 1.5)["index"] == 0 and lib.select("den", 0.2)["index"] == 1
    for cond in (conds[0], conds[-1]):
        again = stress.Condition(cond.kind, cond.label, **cond.params)
        y, out_lengths = stress.apply_condition(again, x, int(FS), lengths)
        assert out_lengths == lengths
        assert torch.equal(y, stress.apply_rir(x, rirs, cond.params["rir_index"], lengths))
