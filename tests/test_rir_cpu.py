"""The room-response path without a GPU: the restatement in tests/rir_ref.py against a brute-force loop over the images
and against analytic answers, every refusal of ``pe_rir_plan``, the tile table, and the host side of the library
(``select``, ``conditions``), none of which reaches the device."""
import math

import numpy as np
import pytest

from pitchextractor_amd import _lib, rir, stress
from tests import rir_ref as R

ROOM = {"dims": (3.0, 2.5, 2.2), "source": (1.1, 0.9, 1.3), "mic": (2.2, 1.7, 1.0)}
ANECHOIC = {"dims": (5.0, 4.0, 3.0), "source": (1.0, 1.0, 1.0), "mic": (3.0, 1.0, 1.0), "beta": 0.0, "n_samples": 300}


@pytest.mark.parametrize("max_order", [0, 1, 2])
def test_restatement_equals_a_brute_force_loop(max_order):
    room = dict(ROOM, beta=[0.9, 0.7, 0.8, 0.6, 0.95, 0.5], n_samples=400)
    h, K, _ = R.image_source(room, 8000.0, max_order=max_order)
    brute = R.image_source_brute(room, 8000.0, max_order=max_order)
    print(f"max_order {max_order}: {int(np.count_nonzero(h))} non-zero samples, at most {int(K.max())} contributions")
    assert np.count_nonzero(h) > 40                        # the direct path arrives at sample 32: its first taps are cut
    assert np.array_equal(h.view(np.uint32), brute.view(np.uint32))


def test_anechoic_integer_delay_is_one_sample():
    """2 m at 320 m/s and 16 kHz is 100 samples exactly: one tap, 1 / (4 pi 2), and nothing else."""
    h, K, acc = R.image_source(ANECHOIC, 16000.0, c=320.0)
    assert h[100] == np.float32(1.0 / (8.0 * math.pi))
    assert acc[100] == int(np.rint(2.0 ** 44 / (8.0 * math.pi)))
    assert np.count_nonzero(h) == 1 and np.count_nonzero(acc) == 1
    assert K[100] == 1 and K[59] == 0 and K[60] == 1 and K[140] == 1 and K[141] == 0


@pytest.mark.parametrize("sign", ["+", "-"])
def test_schroeder_recovers_an_exponential(sign):
    """h[k] = (+-) exp(-a k): E[k] = (e^(-2 a k) - e^(-2 a N)) / (1 - e^(-2 a)), so the decay curve is the line
    -20 a k log10(e) dB but for the truncation term, which bends it by 10 log10(1 - e^(-2 a (N - k))) - 10 log10(1 -
    e^(-2 a N)); over the fitted range that is the discretisation error reported below."""
    fs, t60, N = 8000.0, 0.2, 1200
    a = 3.0 * math.log(10.0) / (t60 * fs)
    k = np.arange(N)
    h = np.exp(-a * k) * (np.where(k % 2, -1.0, 1.0) if sign == "-" else 1.0)
    m = R.schroeder(h, fs, margin=1e-6)
    bend = abs(10.0 * math.log10(1.0 - math.exp(-2.0 * a * (N - m["k_hi"]))))         # dB, at the end of the range
    # a monotone bend of B dB in all tilts a least-squares line over a 20 dB range by at most 1.5 B / 20 of its slope
    bound = 1.5 * bend / 20.0
    print(f"t60 {m['t60']!r} for {t60}: relative error {abs(m['t60'] - t60) / t60:.3e}, bound {bound:.3e}")
    assert m["k_lo"] == math.floor(5.0 / (20.0 * a * math.log10(math.e))) + 1
    assert abs(m["t60"] - t60) <= bound * t60 + 1e-12
    assert math.isnan(R.schroeder(np.ones(100), fs)["t60"])                            # never reaches -25 dB
    assert R.schroeder(np.ones(100), fs)["k_hi"] == 100


def test_bisection_reaches_the_target():
    beta, got, path = R.calibrate(ROOM, 0.15, 8000.0)
    print(f"beta {beta!r}: {got!r} s after {len(path)} steps; Eyring's {path[0][0]!r} measured {path[0][1]!r} s")
    assert abs(got - 0.15) <= 0.02 * 0.15 and len(path) <= 20
    assert path[0][0] == R.eyring_beta(ROOM["dims"], 0.15) == rir.eyring_beta(ROOM["dims"], 0.15)
    assert path[0][1] > 0.15                               # the shoebox model decays more slowly than Eyring's formula
    with pytest.raises(ValueError):
        R.calibrate(ROOM, 0.15, 8000.0, rtol=1e-9, max_iter=2)


# ------------------------------------------------------------------------------------------------------------ the plan
GOOD = dict(ROOM, beta=0.8, n_samples=1000)
BAD_ARG = {
    "zero dimension": dict(GOOD, dims=(3.0, 0.0, 2.2)),
    "negative dimension": dict(GOOD, dims=(-3.0, 2.5, 2.2)),
    "infinite dimension": dict(GOOD, dims=(3.0, 2.5, math.inf)),
    "nan dimension": dict(GOOD, dims=(3.0, math.nan, 2.2)),
    "source outside": dict(GOOD, source=(3.1, 0.9, 1.3)),
    "source on a wall": dict(GOOD, source=(0.0, 0.9, 1.3)),
    "mic outside": dict(GOOD, mic=(2.2, -0.1, 1.0)),
    "mic on a wall": dict(GOOD, mic=(2.2, 1.7, 2.2)),
    "less than 1 cm apart": dict(GOOD, mic=(1.105, 0.9, 1.3)),
    "beta above 1": dict(GOOD, beta=1.01),
    "beta below 0": dict(GOOD, beta=[0.5, 0.5, -0.1, 0.5, 0.5, 0.5]),
    "nan beta": dict(GOOD, beta=math.nan),
    "no samples": dict(GOOD, n_samples=0),
}


@pytest.mark.parametrize("name", sorted(BAD_ARG))
def test_plan_refuses_bad_rooms(name):
    lib = _lib.load()
    params = rir.room_params([GOOD, BAD_ARG[name]], 8000.0)
    off, consts, totals = np.zeros(2, np.int64), np.zeros(4, np.int64), np.zeros(2, np.int64)
    meta = np.zeros((2, lib.pe_rir_plan_fields()), np.int64)
    args = (params.ctypes.data, off.ctypes.data, consts.ctypes.data, meta.ctypes.data, None, 0, totals.ctypes.data)
    assert lib.pe_rir_plan(2, *args) == -1, name
    assert lib.pe_rir_plan(1, *args) == 0                                              # the good room alone passes
    with pytest.raises(ValueError):
        rir.plan_rooms([BAD_ARG[name]], 8000.0)


def test_plan_refuses_bad_rates_orders_and_offsets():
    for kw in (dict(fs=0.0), dict(fs=-8000.0), dict(fs=math.inf), dict(c=0.0), dict(c=math.nan), dict(max_order=-2),
               dict(max_order=1.5)):
        with pytest.raises(ValueError):
            rir.plan_rooms([GOOD], **{"fs": 8000.0, **kw})
    with pytest.raises(ValueError):
        rir.plan_rooms([GOOD], 8000.0, offsets=[-1])
    with pytest.raises(ValueError):
        rir.plan_rooms([GOOD], 8000.0, offsets=[0, 5])
    with pytest.raises(ValueError):
        rir.plan_rooms([dict(GOOD, n_samples=10.5)], 8000.0)
    with pytest.raises(ValueError):
        rir.plan_rooms([{"dims": (3, 2, 2)}], 8000.0)


def test_plan_refuses_what_the_kernel_cannot_serve():
    """PE_E_UNSUPPORTED: a row above 2^24 samples, and rooms whose bound on the sum of image amplitudes passes 2^18
    (a long response in a tiny room; a corridor whose diagonal dwarfs its volume)."""
    for room, fs in ((dict(GOOD, n_samples=(1 << 24) + 1), 8000.0),
                     ({"dims": (0.3, 0.3, 0.3), "source": (0.1, 0.1, 0.1), "mic": (0.2, 0.2, 0.2), "beta": 0.9,
                       "n_samples": 1 << 16}, 8000.0),
                     ({"dims": (100.0, 1.0, 1.0), "source": (10.0, 0.5, 0.5), "mic": (20.0, 0.5, 0.5), "beta": 0.9,
                       "n_samples": 100}, 8000.0)):
        with pytest.raises(_lib.HipLibraryError, match="unsupported"):
            rir.plan_rooms([room], fs)


def test_tile_table_covers_every_sample_once():
    T = rir.plan_rooms([], 8000.0)["tile"]
    lengths = [1, T - 1, T, T + 1, 2 * T + 77, 5 * T]
    rooms = [dict(ROOM, beta=0.5, n_samples=n) for n in lengths]
    rooms[2] = dict(rooms[2], dims=(6.0, 5.0, 4.0))
    offsets = [3, 2000, 9001, 20000, 40001, 60000]
    pl = rir.plan_rooms(rooms, 8000.0, offsets=offsets)
    assert pl["rows"] == len(rooms) and pl["n_samples"] == sum(lengths)
    assert pl["n_tiles"] == sum(-(-n // T) for n in lengths) == pl["tiles"].shape[0]
    assert pl["meta"][:, 0].tolist() == offsets and pl["meta"][:, 1].tolist() == lengths
    assert pl["meta"][:, 3].tolist() == np.concatenate([[0], np.cumsum(pl["meta"][:-1, 2])]).tolist()
    seen = [np.zeros(n, np.int64) for n in lengths]
    weights = []
    for row, k0 in pl["tiles"].tolist():
        assert k0 % T == 0 and 0 <= k0 < lengths[row]
        k1 = min(k0 + T, lengths[row])
        seen[row][k0:k1] += 1
        weights.append(k1 ** 2 / float(np.prod(rooms[row]["dims"])))
    assert all(np.all(s == 1) for s in seen)
    assert weights == sorted(weights, reverse=True)                                    # the heaviest tiles first
    packed = rir.plan_rooms(rooms, 8000.0)
    assert packed["offsets"].tolist() == (np.cumsum(lengths) - np.asarray(lengths)).tolist()


def test_synthesize_and_measure_refuse_the_cpu():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rir.synthesize([GOOD], 8000.0, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rir.measure_t60(torch.zeros(100), [100], 8000.0)


# --------------------------------------------------------------------------------------------------------- the library
def library(entries):
    lib = rir.RirLibrary(8000, [dict(e, index=i, beta=0.5) for i, e in enumerate(entries)], None, [])
    rng = np.random.default_rng(0)
    lib._rir_set = stress.RirSet([rng.standard_normal(50).astype(np.float32) for _ in entries])
    return lib


def test_select_is_the_nearest_and_the_first_on_a_tie():
    lib = library([dict(room="a", target_t60=0.3, t60=0.25), dict(room="a", target_t60=0.6, t60=0.75),
                   dict(room="b", target_t60=0.3, t60=0.5), dict(room="a", target_t60=0.9, t60=0.75)])
    assert lib.select("a", 0.5)["index"] == 0                                          # |0.25 - 0.5| == |0.75 - 0.5|
    assert lib.select("a", 0.51)["index"] == 1
    assert lib.select("a", 2.0)["index"] == 1                                          # entries 1 and 3 tie: the first
    assert lib.select("b", 2.0)["index"] == 2
    assert lib.select("c", 0.5) is None


def test_conditions_are_the_notebooks_sweep():
    names = list(rir.ROOMS)
    assert names == ["small_room", "office", "hall"] == list(rir.LIBRARY_T60S)
    lib = library([dict(room=n, target_t60=t, t60=t * 1.01) for n in names for t in rir.LIBRARY_T60S[n]])
    conds = lib.conditions()
    sweep = [round(float(x), 2) for x in np.linspace(0.2, 1.5, 14)]
    assert len(conds) == 3 * 14 and list(rir.T60_SWEEP) == sweep
    assert len({c.label for c in conds}) == len(conds)
    for c, (room, target) in zip(conds, [(n, t) for n in names for t in sweep]):
        e = lib.select(room, target)
        assert c.kind == "rir" and c.kind in stress.CONDITION_KINDS
        assert (c.params["room"], c.params["target_t60"], c.params["rir_t60"]) == (room, target, e["t60"])
        assert c.params["rirs"] is lib.rir_set() and c.params["rir_index"] == e["index"]
        assert room in c.label and f"{target:.2f}" in c.label and f"{e['t60']:.3f}" in c.label
    assert len(lib.conditions([0.5])) == 3
    assert stress.CONDITION_KINDS == ("rir", "microphone", "clipping", "agc", "resample", "additive_noise")


def test_presets_are_valid_rooms_at_the_notebooks_sizes():
    """Every library entry passes the plan at 24 kHz with the calibration's length (headroom and lattice limits)."""
    for name, room in rir.ROOMS.items():
        for t60 in rir.LIBRARY_T60S[name]:
            n = int(math.ceil(1.5 * t60 * 24000))
            pl = rir.plan_rooms([dict(room, beta=0.9999, n_samples=n)], 24000)
            assert pl["n_tiles"] == -(-n // pl["tile"])
