"""The noise kernels (``csrc/noise.hip`` through ``pitchextractor_amd.noise``) on the device against the float64
restatement in tests/noise_ref.py, the ``additive_noise`` stress condition and ``inference.noise_sweep``.

Shapes: with S = 2048 the scan piece, rows of n in {0, 1, 7, S - 1, S, S + 1, 3 S + 5} and warm-ups of {0, 5, S + 3}
samples, every length with every warm-up in one batch, and one row of 257 pieces (the per-row walks take 256 at a
time).  Each batch is made alone (one row per call), packed so that
every row starts at an odd offset, and padded; a row must come out bit-identical in the three.  Every figure is printed
before it is asserted."""
import math

import numpy as np
import pytest
import torch

from oracle import model_ref
from pitchextractor_amd import inference, noise as N, stress
from tests import noise_ref as R

pytestmark = pytest.mark.gpu

f32 = np.float32
LENGTHS = [0, 1, 7, R.PIECE - 1, R.PIECE, R.PIECE + 1, 3 * R.PIECE + 5]
WARMUPS = [0, 5, R.PIECE + 3]
ROWS = [(n, warm) for warm in WARMUPS for n in LENGTHS]                # (samples, warm-up) of every row of a batch
SEED = 100
CUSTOM = {"d0": 0.3, "d1": -0.2, "sections": [(0.999, 0.01), (0.9, 0.2), (-0.8, 0.1), (0.5, 0.3), (0.25, -0.4),
                                              (0.99, 0.02), (0.7, 0.05), (-0.3, 0.6)]}
COLOURS = {"pink": "pink", "brown": "brown", "white": "white", "custom": CUSTOM}
SNRS = [-5.0, 0.0, 20.0, 60.0]


def host(t):
    return t.detach().cpu().numpy()


def layouts(lengths):
    """name -> list of (row indices, offsets, output size)."""
    odd, at = [], 1
    for n in lengths:
        odd.append(at)
        at += n + n % 2 + 2                                            # keeps every start odd
    assert all(o % 2 == 1 for o in odd)
    width = max(lengths) + 3
    rows = list(range(len(lengths)))
    return {"alone": [([r], [0], lengths[r]) for r in rows], "packed": [(rows, odd, at)],
            "padded": [(rows, [r * width for r in rows], width * len(rows))]}


def run_layouts(lengths, device, make):
    """``make(rows, offsets, out)`` fills ``out`` in every layout; per layout the rows as arrays.  Nothing is written
    outside the rows."""
    got = {}
    for name, groups in layouts(lengths).items():
        got[name] = {}
        for rows, offsets, size in groups:
            out = torch.full((max(size, 1),), 7.0, dtype=torch.float32, device=device)
            make(rows, offsets, out)
            y = host(out)
            covered = np.zeros(y.size, bool)
            for r, o in zip(rows, offsets):
                got[name][r] = y[o:o + lengths[r]].copy()
                covered[o:o + lengths[r]] = True
            assert np.all(y[~covered] == 7.0), name
    return got


def assert_same_in_every_layout(got, what):
    for name in ("packed", "padded"):
        for r, row in got["alone"].items():
            assert np.array_equal(row.view(np.uint32), got[name][r].view(np.uint32)), (what, name, r)


# ---------------------------------------------------------------------------------------------------------- white noise
def test_white_noise(hip_device):
    lengths, warm = [n for n, _ in ROWS], [w for _, w in ROWS]
    got = run_layouts(lengths, hip_device, lambda rows, offsets, out: N.white(
        [lengths[r] for r in rows], [SEED + r for r in rows], offsets=offsets, warmup=[warm[r] for r in rows], out=out))
    assert_same_in_every_layout(got, "white")
    # an int seed is seed + r; a row is its stream from the warm-up on, whatever the batch around it
    packed = host(N.white(lengths, SEED, hip_device, warmup=warm))
    assert np.array_equal(packed, np.concatenate([got["alone"][r] for r in range(len(ROWS))]))
    stream = host(N.white([3 * R.PIECE + 5 + R.PIECE + 3], SEED + 20, hip_device))
    assert np.array_equal(got["alone"][20], stream[R.PIECE + 3:]) and ROWS[20] == (3 * R.PIECE + 5, R.PIECE + 3)
    # against the float64 Box-Muller, next to numpy's float32 evaluation of the same expression
    draws = 1 << 16
    for seed in (0, 1234):
        z64 = R.randn64(seed, np.arange(draws))
        dev = float(np.max(np.abs(host(N.white([draws], seed, hip_device)).astype(np.float64) - z64)))
        ref = float(np.max(np.abs(R.randn32_numpy(seed, np.arange(draws)).astype(np.float64) - z64)))
        print(f"seed {seed}: max |device - float64| {dev:.3e}, max |numpy float32 - float64| {ref:.3e} over {draws} draws")
        assert dev <= 4.0 * ref


# --------------------------------------------------------------------------------------------------------- colour stage
@pytest.fixture(scope="module")
def white_inputs():
    """Per input kind, the given white samples (warm-up + n float32) of every row."""
    rng = np.random.default_rng(5)
    random = [rng.standard_normal(n + w).astype(f32) for n, w in ROWS]
    impulse = []
    for n, w in ROWS:
        v = np.zeros(n + w, f32)
        if v.size:
            v[0] = 1.0
        impulse.append(v)
    return {"random": random, "impulse": impulse}


@pytest.mark.parametrize("name", list(COLOURS))
def test_colour_stage_given_white(hip_device, white_inputs, name):
    colour = COLOURS[name]
    d0, d1, sections = N.colour_sections(colour, 24000)
    lengths, warm = [n for n, _ in ROWS], [w for _, w in ROWS]
    for kind, given in white_inputs.items():
        want = [R.colour(given[r], d0, d1, sections, warm[r]) for r in range(len(ROWS))]

        def make(rows, offsets, out):
            white = torch.from_numpy(np.concatenate([given[r] for r in rows] + [np.zeros(1, f32)])).to(hip_device)
            N.coloured([lengths[r] for r in rows], colour, 24000, white=white, warmup=[warm[r] for r in rows],
                       offsets=offsets, out=out)

        got = run_layouts(lengths, hip_device, make)
        assert_same_in_every_layout(got, f"{name} {kind}")
        differing = 0
        for r, w in enumerate(want):
            g = got["alone"][r]
            assert g.shape == w.shape
            differing += int(np.count_nonzero(g != w))
            assert np.all(np.abs(g.astype(np.float64) - w.astype(np.float64)) <= 2.0 ** -23 * np.abs(w.astype(np.float64))), \
                (name, kind, r)
        print(f"{name}, {kind} white: {differing} of {sum(lengths)} float32 samples differ from the sequential recurrence")


def test_drawn_colours_are_the_filtered_drawn_white(hip_device):
    lengths, warm = [n for n, _ in ROWS], [w for _, w in ROWS]
    seeds = [SEED + r for r in range(len(ROWS))]
    white = N.white([n + w for n, w in ROWS], seeds, hip_device)
    for name in ("pink", "brown", "custom"):
        drawn = run_layouts(lengths, hip_device, lambda rows, offsets, out: N.coloured(
            [lengths[r] for r in rows], COLOURS[name], 24000, seeds=[seeds[r] for r in rows],
            warmup=[warm[r] for r in rows], offsets=offsets, out=out))
        assert_same_in_every_layout(drawn, f"drawn {name}")
        given = host(N.coloured(lengths, COLOURS[name], 24000, white=white, warmup=warm))
        assert np.array_equal(given.view(np.uint32), np.concatenate([drawn["alone"][r] for r in range(len(ROWS))]).view(np.uint32))
    # an int seed counts up over the rows, and the default warm-up is 4096 samples of the row's own stream
    a = host(N.coloured([100, 50], "pink", 24000, seeds=7, device=hip_device))
    b = host(N.coloured([50], "pink", 24000, seeds=8, device=hip_device))
    assert np.array_equal(a[100:], b)
    d0, d1, sections = N.colour_sections("pink", 24000)
    want = R.colour(host(N.white([4146], 8, hip_device)), d0, d1, sections, 4096)
    assert np.all(np.abs(b.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want))


def test_a_row_of_more_pieces_than_one_walk_holds(hip_device):
    """The per-row walks (the carries, the rms and the peak) take 256 pieces at a time: a row of 257 pieces and a
    remainder, alone and packed at an odd offset behind a short row, against the sequential recurrence and the mix."""
    n, warm = 257 * R.PIECE + 3, 5
    rng = np.random.default_rng(13)
    given = [rng.standard_normal(7 + warm).astype(f32), rng.standard_normal(n + warm).astype(f32)]
    slow = {"d0": 0.1, "sections": [(0.9999, 0.01), (-0.5, 0.2)]}
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)  # noqa: E731
    noise = None
    for name, colour in (("brown", "brown"), ("slow", slow)):
        d0, d1, sections = N.colour_sections(colour, 24000)
        want = R.colour(given[1], d0, d1, sections, warm)
        alone = host(N.coloured([n], colour, 24000, white=up(given[1]), warmup=warm))
        out = torch.zeros(n + 20, dtype=torch.float32, device=hip_device)
        N.coloured([7, n], colour, 24000, white=up(np.concatenate(given)), warmup=warm, offsets=[1, 11], out=out)
        packed = host(out)[11:11 + n]
        differing = int(np.count_nonzero(alone != want))
        print(f"{name}: {differing} of {n} float32 samples differ from the sequential recurrence")
        assert np.array_equal(alone.view(np.uint32), packed.view(np.uint32))
        # One float32 step, plus what the double states may differ by where the sections cancel to an output near
        # zero: a^2048 comes from 7 products and 8 squarings (a relative 2047 2^-53 at the most), the scan's own
        # products and sums stay below as much again, and a state is at most |b| max|w| / (1 - |a|); a carry's error
        # decays by |a|^2048 per piece.
        peak = float(np.max(np.abs(given[1])))
        slack = sum(4096 * 2.0 ** -53 * abs(b) * peak / ((1 - abs(a)) * (1 - abs(a) ** R.PIECE)) for a, b in sections)
        err = np.abs(alone.astype(np.float64) - want)
        print(f"{name}: worst |device - restatement| {err.max():.3e}, slack for the double states {slack:.3e}")
        assert np.all(err <= 2.0 ** -23 * np.abs(want.astype(np.float64)) + slack)
        noise = alone
    x = (0.2 * np.sin(np.arange(n) * 0.01)).astype(f32)
    y, st = N.mix_at_snr(up(x), up(noise), 5.0, return_stats=True)
    y, st = host(y), host(st)[0]
    lengths = [7, n]
    y2, st2 = N.mix_at_snr(up(np.concatenate([x[:7], x])), up(np.concatenate([noise[:7], noise])), 5.0, lengths,
                           return_stats=True)
    assert np.array_equal(y.view(np.uint32), host(y2)[7:].view(np.uint32)) and np.array_equal(st, host(st2)[1])
    want_y, want = R.mix(x, noise, 5.0, scale=st[3])
    print(f"mix of {n} samples: rms {st[1]:.17g} / {st[2]:.17g}, restatement {want[1]:.17g} / {want[2]:.17g}")
    assert abs(st[1] - want[1]) <= 1e-12 * want[1] and abs(st[2] - want[2]) <= 1e-12 * want[2] and st[0] == want[0]
    assert abs(st[3] - R.mix(x, noise, 5.0)[1][3]) <= float(np.spacing(f32(st[3])))
    assert np.array_equal(y.view(np.uint32), want_y.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ bed
def test_bed(hip_device):
    rng = np.random.default_rng(9)
    sizes = [1, 5, R.PIECE, 5000]
    beds = N.NoiseSet([rng.standard_normal(L).astype(f32) for L in sizes], hip_device)
    rows = [(n, k, s) for k, L in enumerate(sizes) for s in (0, L - 1) for n in LENGTHS]
    lengths = [n for n, _, _ in rows]
    got = run_layouts(lengths, hip_device, lambda idx, offsets, out: N.bed(
        beds, [lengths[r] for r in idx], [rows[r][1] for r in idx], [rows[r][2] for r in idx], offsets=offsets, out=out))
    assert_same_in_every_layout(got, "bed")
    for r, (n, k, s) in enumerate(rows):
        assert np.array_equal(got["alone"][r].view(np.uint32), R.bed(beds.recordings[k], n, s).view(np.uint32)), rows[r]
    assert max(lengths) > 5 * sizes[1] and min(n for n in lengths if n) < sizes[3]      # longer and shorter than a bed
    whole = host(N.bed(beds, [12], 1, 3))
    assert np.array_equal(whole, R.bed(beds.recordings[1], 12, 3))


# ------------------------------------------------------------------------------------------------------------------ mix
@pytest.fixture(scope="module")
def mix_rows():
    """(signal, noise, snr_db) per row: a quiet tone of every length, two loud ones that pass a peak of 0.99 once the
    noise is on, a silent signal and a zero noise."""
    rng = np.random.default_rng(21)
    rows = []

    def tone(n, amp):
        return (amp * np.sin(2 * np.pi * 220.0 * np.arange(n) / 24000.0 + 0.3)).astype(f32)

    for k, n in enumerate(LENGTHS):
        rows.append((tone(n, 0.05), rng.standard_normal(n).astype(f32), SNRS[k % 4]))
    rows.append((tone(R.PIECE + 1, 0.9), rng.standard_normal(R.PIECE + 1).astype(f32), 0.0))
    rows.append((tone(3 * R.PIECE + 5, 0.9), rng.standard_normal(3 * R.PIECE + 5).astype(f32), -5.0))
    rows.append((np.zeros(R.PIECE + 1, f32), rng.standard_normal(R.PIECE + 1).astype(f32), 20.0))
    rows.append((tone(R.PIECE + 1, 0.05), np.zeros(R.PIECE + 1, f32), 60.0))
    rows.append((tone(R.PIECE, 0.05), rng.standard_normal(R.PIECE).astype(f32), 60.0))
    rows.append((tone(7, 0.05), rng.standard_normal(7).astype(f32), 20.0))
    return rows


def _mix_layouts(rows, device, peak_normalize=True):
    """Per layout, per row ``(y, stats)``."""
    lengths = [x.size for x, _, _ in rows]
    snr = [s for _, _, s in rows]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    got = {"alone": {}, "packed": {}, "padded": {}}
    for r, (x, z, s) in enumerate(rows):
        y, st = N.mix_at_snr(up(x), up(z), s, peak_normalize=peak_normalize, return_stats=True)
        got["alone"][r] = (host(y), host(st)[0])
    cat = lambda k: up(np.concatenate([row[k] for row in rows] + [np.zeros(3, f32)]))  # noqa: E731
    y, st = N.mix_at_snr(cat(0), cat(1), snr, lengths, peak_normalize, return_stats=True)
    y, st, at = host(y), host(st), 0
    assert y.shape == (sum(lengths) + 3,) and np.all(y[sum(lengths):] == 0.0)
    for r, n in enumerate(lengths):
        got["packed"][r] = (y[at:at + n], st[r])
        at += n
    width = max(lengths) + 3

    def pad(k):
        a = np.full((len(rows), width), 3.0, f32)                      # the padding is not silence
        for r, row in enumerate(rows):
            a[r, :lengths[r]] = row[k]
        return up(a)

    y, st = N.mix_at_snr(pad(0), pad(1), snr, lengths, peak_normalize, return_stats=True)
    y, st = host(y), host(st)
    for r, n in enumerate(lengths):
        got["padded"][r] = (y[r, :n], st[r])
        assert np.all(y[r, n:] == 0.0)
    return got


def test_mix_at_snr(hip_device, mix_rows):
    got = _mix_layouts(mix_rows, hip_device)
    offsets = np.cumsum([0] + [x.size for x, _, _ in mix_rows])
    assert any(o % 2 == 1 for o in offsets[:-1])                       # packed rows start at odd offsets too
    for name in ("packed", "padded"):
        for r, (y, st) in got["alone"].items():
            assert np.array_equal(y.view(np.uint32), got[name][r][0].view(np.uint32)), (name, r)
            assert np.array_equal(st, got[name][r][1]), (name, r)
    worst_rms = worst_snr = 0.0
    for r, (x, z, snr) in enumerate(mix_rows):
        y, st = got["alone"][r]
        want_y, want = R.mix(x, z, snr)
        if x.size == 0:
            assert y.size == 0 and st.tolist() == [0.0, 0.0, 0.0, 0.0]
            continue
        for k in (1, 2):
            err = abs(st[k] - want[k]) / want[k] if want[k] else abs(st[k])
            worst_rms = max(worst_rms, err)
            assert err <= 1e-12, (r, k, st[k], want[k])
        assert st[3] == float(f32(st[3])) and abs(st[3] - want[3]) <= float(np.spacing(f32(want[3]))), (r, st[3], want[3])
        same_y, same = R.mix(x, z, snr, scale=st[3])
        assert st[0] == same[0] and np.array_equal(y.view(np.uint32), same_y.view(np.uint32)), r
        if st[3] != 0.0:
            achieved = 20.0 * math.log10(st[1] / (st[3] * st[2]))
            worst_snr = max(worst_snr, abs(achieved - snr))
            assert abs(achieved - snr) <= 1e-5, (r, achieved, snr)
    print(f"mix: worst relative rms error {worst_rms:.3e}, worst |achieved - requested SNR| {worst_snr:.3e} dB")
    # both sides of the peak rule, through stats: the quiet rows are the plain sum, the loud ones are divided
    quiet, loud = got["alone"][6], got["alone"][8]
    assert quiet[1][0] <= 0.99 and np.array_equal(quiet[0], mix_rows[6][0] + mix_rows[6][1] * f32(quiet[1][3]))
    for r in (7, 8):
        y, st = got["alone"][r]
        x, z, _ = mix_rows[r]
        assert st[0] > 0.99 and np.array_equal(y, (x + z * f32(st[3])) / f32(st[0] + 1e-6))
        assert float(np.max(np.abs(y))) <= 1.0
    # a silent signal and a zero noise are copies with a scale of 0
    for r, silent in ((9, 1), (10, 2)):
        y, st = got["alone"][r]
        assert st[3] == 0.0 and st[silent] == 0.0 and np.array_equal(y, mix_rows[r][0])
    # without the peak rule the loud rows stay the plain sum, and their stats do not change
    plain = _mix_layouts(mix_rows[7:9], hip_device, peak_normalize=False)
    for k, r in enumerate((7, 8)):
        y, st = plain["alone"][k]
        x, z, _ = mix_rows[r]
        assert np.array_equal(st, got["alone"][r][1]) and np.array_equal(y, x + z * f32(st[3]))
        assert np.array_equal(y, plain["packed"][k][0]) and np.array_equal(y, plain["padded"][k][0])


def test_refusals_on_the_device(hip_device):
    x = torch.zeros(100, dtype=torch.float32, device=hip_device)
    for bad in (math.nan, math.inf, [1.0, 2.0]):
        with pytest.raises(ValueError):
            N.mix_at_snr(x, x, bad)
    with pytest.raises(ValueError):
        N.mix_at_snr(x, x[:50], 10.0)
    with pytest.raises(ValueError):
        N.coloured([100], "pink", 24000, white=x)                      # 4096 + 100 samples are needed
    with pytest.raises(ValueError):
        N.white([100], 0, offsets=[50], out=x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        N.mix_at_snr(x, x.double(), 10.0)


# ---------------------------------------------------------------------------------------------- condition and the sweep
def test_additive_noise_condition(hip_device):
    rng = np.random.default_rng(2)
    lengths = [4800, 2049, 0, 7]
    x = torch.zeros((4, 4803), dtype=torch.float32, device=hip_device)
    for r, n in enumerate(lengths):
        x[r, :n] = torch.from_numpy((0.3 * np.sin(np.arange(n) * 0.06)).astype(f32)).to(hip_device)
    beds = N.NoiseSet([rng.standard_normal(1000).astype(f32), rng.standard_normal(333).astype(f32)], hip_device)
    for source in ("white", "pink", CUSTOM, beds):
        y, st = stress.apply_additive_noise(x, 24000, [20.0, 10.0, 0.0, -5.0], source, seed=4, bed_index=[0, 1, 0, 1],
                                            bed_start=[0, 332, 5, 7], lengths=lengths, return_stats=True)
        yh, sth = host(y), host(st)
        assert yh.shape == (4, 4803) and sth.shape == (4, 4) and sth[2].tolist() == [0.0, 0.0, 0.0, 0.0]
        for r, n in enumerate(lengths):
            assert np.all(yh[r, n:] == 0.0)
            if n:
                assert abs(20.0 * math.log10(sth[r, 1] / (sth[r, 3] * sth[r, 2])) - [20.0, 10.0, 0.0, -5.0][r]) <= 1e-5
            # the row alone, with its own seed, is the same row
            alone = host(stress.apply_additive_noise(x[r, :n].contiguous(), 24000, [20.0, 10.0, 0.0, -5.0][r], source,
                                                     seed=[4 + r], bed_index=[0, 1, 0, 1][r],
                                                     bed_start=[0, 332, 5, 7][r]))
            assert np.array_equal(alone.view(np.uint32), yh[r, :n].view(np.uint32)), (r, source if isinstance(source, str) else "")
        if isinstance(source, N.NoiseSet):
            want, _ = R.mix(host(x[1, :2049]), R.bed(beds.recordings[1], 2049, 332), 10.0, scale=sth[1, 3])
            assert np.array_equal(want, yh[1, :2049])
    cond = stress.Condition("additive_noise", "pink 10 dB", snr_db=10.0, source="pink", seed=4)
    a, row_lengths = stress.apply_condition(cond, x, 24000, lengths)
    b, _ = stress.apply_condition(cond, x, 24000, lengths)
    other, _ = stress.apply_condition(stress.Condition("additive_noise", "pink 10 dB", snr_db=10.0, source="pink", seed=5),
                                      x, 24000, lengths)
    assert row_lengths == lengths and torch.equal(a, b) and not torch.equal(a, other)
    assert int((other[0] != a[0]).sum()) > 4700


def test_noise_sweep(tmp_path, hip_device):
    torch.save({"model": model_ref.seeded_state(31, hidden_size=64, num_layers=2)}, tmp_path / "r.pth")
    net = inference.load_model(tmp_path / "r.pth", device=hip_device)
    rng = np.random.default_rng(8)
    t = np.arange(24000) / 24000.0
    items = []
    for f0 in (110.0, 220.0):
        audio = (0.5 * np.sin(2 * np.pi * f0 * t) + 0.01 * rng.standard_normal(t.size)).astype(f32)
        items.append({"audio": audio, "reference_f0": np.full(81, f0, f32)})
    keys = {"condition", "kind", "item", *stress.METRIC_KEYS}
    same = lambda a, b: a == b or (isinstance(a, float) and math.isnan(a) and math.isnan(b))  # noqa: E731
    conditions = [stress.Condition("additive_noise", "white 10 dB", snr_db=10.0, source="white", seed=3),
                  stress.Condition("additive_noise", "pink 0 dB", snr_db=0.0, source="pink", seed=3)]
    out = inference.stress_sweep(net, items, conditions, batched=True)
    assert len(out["baseline"]) == 2 and len(out["conditions"]) == 4
    assert all(set(rec) == keys for rec in out["baseline"] + out["conditions"])
    assert [(rec["condition"], rec["kind"], rec["item"]) for rec in out["conditions"]] == \
        [(c.label, "additive_noise", i) for c in conditions for i in range(2)]
    assert all(rec["n_frames"] == 81 for rec in out["conditions"])

    sweep = inference.noise_sweep(net, items, snrs_db=(20, 0), sources=("white", "pink"), seed=3)
    again = inference.noise_sweep(net, items, snrs_db=(20, 0), sources=("white", "pink"), seed=3)
    assert list(sweep) == ["baseline", "conditions", "summary"]
    assert len(sweep["baseline"]) == 2 and len(sweep["conditions"]) == 8 and len(sweep["summary"]) == 4
    assert all(set(rec) == keys | {"source", "snr_db"} for rec in sweep["conditions"])
    assert [(rec["source"], rec["snr_db"], rec["item"]) for rec in sweep["conditions"]] == \
        [(s, d, i) for s in ("white", "pink") for d in (20.0, 0.0) for i in range(2)]
    assert [rec["condition"] for rec in sweep["conditions"][:4:2]] == ["white 20 dB", "white 0 dB"]
    for a, b in zip(sweep["conditions"] + sweep["baseline"], again["conditions"] + again["baseline"]):
        assert all(same(a[k], b[k]) for k in a)                        # the same seed, the same records
    # the pink 0 dB records are those of the plain sweep's condition with the same seed
    for a, b in zip(sweep["conditions"][6:], out["conditions"][2:]):
        assert all(same(a[k], b[k]) for k in stress.METRIC_KEYS)
    want = inference.summarize_with_drop(sweep["conditions"], sweep["baseline"], ("source", "snr_db"))
    assert len(want) == 4 and [(g["source"], g["snr_db"]) for g in want] == [("white", 20.0), ("white", 0.0),
                                                                             ("pink", 20.0), ("pink", 0.0)]
    for g, w in zip(sweep["summary"], want):
        assert list(g) == list(w) and all(same(g[k], w[k]) for k in w)
    cols = [m + s for m in ("RPA", "RCA", "VUV", "OctaveError") for s in ("_mean", "_std", "_drop")]
    assert all(set(g) == {"source", "snr_db", *cols} for g in sweep["summary"])
    clean = float(np.mean([rec["VUV"] for rec in sweep["baseline"]]))
    for g in sweep["summary"]:
        rows = [rec["VUV"] for rec in sweep["conditions"] if (rec["source"], rec["snr_db"]) == (g["source"], g["snr_db"])]
        assert g["VUV_mean"] == float(np.mean(rows)) and g["VUV_drop"] == clean - float(np.mean(rows))
