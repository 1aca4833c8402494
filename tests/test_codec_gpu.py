"""The codec conditions on the GPU (``pitchextractor_amd/codec.py``, ``csrc/codec.hip``) against the restatement in
tests/codec_ref.py: the quantiser bit for bit, the transforms by the 4x rule (the kernel's largest deviation from the
float64 direct sums, relative to the frame's largest magnitude, is at most 4x that of float32 direct sums on the same
input), the fused call against the stage chain, row independence, mu-law bit for bit, and the sweep.

Measured on an MI355X (kernel deviation over float32 direct-sum deviation, worst frame of each row): mdct 0.12 .. 0.34
(1.28 on the one-sample row, where the direct sum is a single product), imdct 0.11 .. 0.33, the round trip 0.14 .. 0.40;
the table is in DESIGN.md section 28."""
import numpy as np
import pytest
import torch

from oracle import model_ref
from pitchextractor_amd import codec, inference, stress
from pitchextractor_amd.f0_tracker import PraatACTracker
from pitchextractor_amd.resample import RaggedResampler
from tests import codec_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32
ROWS = {256: (1, 255, 256, 257, 3 * 256 + 7), 1024: (1023, 1024, 1025, 3000)}


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ------------------------------------------------------------------------------------------------------------ quantiser
def quantiser_frames(M):
    """Band levels spread over 2^-40 .. 2^10 (three frames, one with zeroed bands), an all-zero frame, a frame below
    2^-100, a frame of plain noise."""
    rng = np.random.default_rng(100 + M)
    e = R.band_edges(M)
    X = rng.standard_normal((6, M))
    levels = np.linspace(-40, 10, len(e) - 1)
    for f in range(3):
        for b, lv in enumerate(rng.permutation(levels)):
            X[f, e[b]:e[b + 1]] *= 2.0 ** lv
    for b in (0, 3, 4, len(e) - 2):
        X[2, e[b]:e[b + 1]] = 0
    X[3] = 0
    X[4] *= 2.0 ** -108
    X[4, 5] = 2.0 ** -100                                   # the smallest maximum that still makes a band
    X[0, e[2]] = 1024.0 * 3.9                               # |q| in the millions at g = 0
    return X.astype(f32)


@pytest.mark.parametrize("M", [256, 1024])
@pytest.mark.parametrize("cut", ["17", "M/3", "M"])
def test_quantiser_bit_for_bit(M, cut, hip_device):
    k_c = {"17": 17, "M/3": M // 3, "M": M}[cut]
    X = quantiser_frames(M)
    c = codec.TransformCodec(24000, 64, M)
    floor = 8 + R.bands_below(M, k_c)
    for budget in (floor, floor + 9, 3 * floor, 20 * floor, c.budget, 100000):
        q, g, bits, deq = (t.cpu().numpy() for t in c.quantize(dev(X, hip_device), budget=budget, cutoff_bin=k_c))
        rq, rg, rbits, rdeq = R.quantize_frames(X, M, k_c, budget)
        print(f"M {M} K_c {k_c} budget {budget}: g {rg.tolist()} bits {rbits.tolist()} max |q| {np.abs(rq).max()}")
        assert np.array_equal(g, rg) and np.array_equal(bits, rbits)
        assert np.array_equal(q, rq)
        assert np.array_equal(deq.view(np.uint32), rdeq.view(np.uint32))
        if budget == floor:
            assert not q.any()
        if budget == 100000:
            assert not g.any() and np.abs(q).max() > 1000000


# ----------------------------------------------------------------------------------------------------------- transforms
def frame_deviation(got, ref, M):
    """Largest |got - ref| of a frame (M values) over the frame's largest |ref|, the worst frame."""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    worst = 0.0
    for s in range(0, ref.size, M):
        top = np.max(np.abs(ref[s:s + M]))
        if top > 0:
            worst = max(worst, float(np.max(np.abs(got[s:s + M] - ref[s:s + M])) / top))
    return worst


@pytest.fixture(scope="module")
def transform_rows():
    rng = np.random.default_rng(28)
    return {M: [rng.uniform(-1, 1, n).astype(f32) for n in ROWS[M]] for M in ROWS}


@pytest.mark.parametrize("M", [256, 1024])
def test_transform_accuracy(M, transform_rows, hip_device):
    c = codec.TransformCodec(24000, 64, M)
    for x in transform_rows[M]:
        n, xd = x.size, dev(x, hip_device)
        X, pl = c.mdct(xd)
        X = X.cpu().numpy()
        assert X.shape == (R.n_frames(n, M), M)
        X64 = R.mdct(x, M)
        k, y = frame_deviation(X, X64, M), frame_deviation(R.mdct(x, M, f32), X64, M)
        print(f"mdct  M {M} n {n}: kernel {k:.3e} float32 direct {y:.3e} ratio {k / y:.3f}")
        assert k <= 4 * y
        # the inverse on the kernel's own coefficients
        out = c.imdct(dev(X, hip_device), xd).cpu().numpy()
        y64 = R.imdct(X, n, M)
        k, y = frame_deviation(out, y64, M), frame_deviation(R.imdct(X, n, M, f32), y64, M)
        print(f"imdct M {M} n {n}: kernel {k:.3e} float32 direct {y:.3e} ratio {k / y:.3f}")
        assert out.shape == x.shape and k <= 4 * y
        # and the round trip against x
        chain32 = R.imdct(R.mdct(x, M, f32), n, M, f32)
        k, y = frame_deviation(out, x, M), frame_deviation(chain32, x, M)
        print(f"chain M {M} n {n}: kernel {k:.3e} float32 direct {y:.3e} ratio {k / y:.3f}")
        assert k <= 4 * y


# ------------------------------------------------------------------------------------------- fused call, row independence
def layouts(fn, rows, device):
    """``fn(x, lengths)`` on the rows packed behind a one-sample row (odd offsets) with trailing slack, in reversed
    order, padded with garbage past each row, and one by one: bit-identical rows, zeros outside.  Returns the rows."""
    rows = [np.ascontiguousarray(r, dtype=f32) for r in rows]
    lengths = [int(r.size) for r in rows]
    lead = f32([0.25])
    packed = dev(np.concatenate([lead] + rows + [np.full(3, 7.0, f32)]), device)
    yp = fn(packed, [1] + lengths).cpu().numpy()
    assert yp.shape == tuple(packed.shape) and np.all(yp[1 + sum(lengths):] == 0)
    out = np.split(yp[1:1 + sum(lengths)], np.cumsum(lengths)[:-1])
    rev = fn(dev(np.concatenate(rows[::-1]), device), lengths[::-1]).cpu().numpy()
    back = np.split(rev, np.cumsum(lengths[::-1])[:-1])[::-1]
    pad = torch.full((len(rows), max(lengths) + 5), 7.0, dtype=torch.float32, device=device)
    for r, row in enumerate(rows):
        pad[r, :row.size] = dev(row, device)
    yd = fn(pad, lengths).cpu().numpy()
    for r, n in enumerate(lengths):
        assert np.array_equal(back[r].view(np.uint32), out[r].view(np.uint32)), f"row {r}: reversed order differs"
        assert np.array_equal(yd[r, :n].view(np.uint32), out[r].view(np.uint32)), f"row {r}: padded differs"
        assert np.all(yd[r, n:] == 0)
        alone = fn(dev(rows[r], device), None).cpu().numpy()
        assert alone.shape == (n,) and np.array_equal(alone.view(np.uint32), out[r].view(np.uint32)), f"row {r}: alone"
    return out


def speechlike(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 24000.0
    x = sum(np.sin(2 * np.pi * 170.0 * h * t + rng.uniform(0, 6)) / h for h in range(1, 12))
    return (0.2 * x + 0.01 * rng.standard_normal(n)).astype(f32)


@pytest.mark.parametrize("M, kbps", [(256, 24), (512, 64), (1024, 16), (1024, 128)])
def test_fused_call_is_the_stage_chain(M, kbps, hip_device):
    c = codec.TransformCodec(24000, kbps, M)
    lengths = [0, 1, M - 1, M, M + 1, 3 * M + 7]
    x = dev(np.concatenate([speechlike(n, n) for n in lengths]), hip_device)
    y, stats = c(x, lengths, return_stats=True)
    X, pl = c.mdct(x, lengths)
    q, g, bits, deq = c.quantize(X)
    chain = c.imdct(deq, x, lengths)
    assert np.array_equal(y.cpu().numpy().view(np.uint32), chain.cpu().numpy().view(np.uint32))
    assert torch.equal(stats["g"], g) and torch.equal(stats["bits"], bits)
    assert stats["frames"].tolist() == [R.n_frames(n, M) for n in lengths]
    assert stats["frame_offsets"].tolist() == pl["frame_offsets"].tolist()
    assert int(bits.max()) <= c.budget and torch.equal(c(x, lengths), y)
    assert not torch.equal(y, x) and float((y - x).abs().max()) < 0.5


@pytest.mark.parametrize("M", [256, 1024])
def test_rows_do_not_depend_on_their_place(M, hip_device):
    rows = [speechlike(n, 7 + n) for n in (1, M - 1, M, M + 1, 3 * M + 7)]
    c = codec.TransformCodec(24000, 48, M)
    out = layouts(lambda x, lengths: c(x, lengths), rows, hip_device)
    assert all(o.size == r.size for o, r in zip(out, rows))
    empty = c(torch.zeros((2, 0), dtype=torch.float32, device=hip_device))
    assert empty.shape == (2, 0)
    assert c(torch.zeros(5, dtype=torch.float32, device=hip_device), [0, 0]).shape == (5,)


# --------------------------------------------------------------------------------------------------------------- mu-law
def test_mulaw_bit_for_bit(hip_device):
    p = np.arange(-32768, 32768)
    x = np.concatenate([(p / 32768.0).astype(f32), ((p + 0.5) / 32768.0).astype(f32),
                        f32([1.0, 1.5, -1.5, 100.0, -100.0, 1e-9, -1e-9, 0.0])])
    y = codec.apply_mulaw(dev(x, hip_device)).cpu().numpy()
    assert np.array_equal(y.view(np.uint32), R.mulaw(x).view(np.uint32))
    assert y[65536 + 65536] == f32(0.98034668)
    rng = np.random.default_rng(5)
    rows = [rng.uniform(-1.2, 1.2, n).astype(f32) for n in (1, 1023, 1024, 1025, 3000)]
    out = layouts(codec.apply_mulaw, rows, hip_device)
    for o, r in zip(out, rows):
        assert np.array_equal(o.view(np.uint32), R.mulaw(r).view(np.uint32))


def test_g711u_is_its_three_calls(hip_device):
    lengths = [24000, 7001, 1]
    rows = [speechlike(n, n) for n in lengths]
    pad = torch.zeros((3, 24000), dtype=torch.float32, device=hip_device)
    for r, row in enumerate(rows):
        pad[r, :row.size] = dev(row, hip_device)
    y, out_lengths = codec.apply_g711u(pad, 24000, lengths)
    down_rs, up_rs = RaggedResampler(8000), RaggedResampler(24000)
    down, _ = down_rs(pad, [24000] * 3, lengths)
    down_lengths = [down_rs.out_len(24000, n) for n in lengths]
    up, _ = up_rs(codec.apply_mulaw(down, down_lengths), [8000] * 3, down_lengths)
    assert out_lengths == [up_rs.out_len(8000, n) for n in down_lengths] and down_lengths[0] == 8000
    assert torch.equal(y, up)
    cond = codec.CodecCondition("phone", codec="g711u")
    y2, l2 = stress.apply_condition(cond, pad, 24000, lengths)
    assert torch.equal(y2, y) and l2 == out_lengths
    same, l3 = codec.apply_g711u(pad[:, :8000], 8000, [8000, 7001, 1])          # at 8 kHz: mu-law alone
    assert torch.equal(same, codec.apply_mulaw(pad[:, :8000], [8000, 7001, 1])) and l3 == [8000, 7001, 1]


# ---------------------------------------------------------------------------------------------------------------- sweep
def harmonic_complex(f0=220.0, seconds=1.0, sr=24000):
    t = np.arange(int(seconds * sr)) / sr
    x = sum(np.sin(2 * np.pi * f0 * h * t) / h for h in range(1, 9))
    return (0.4 * x / np.max(np.abs(x))).astype(f32)


def test_codec_sweep(tmp_path, hip_device):
    torch.save({"model": model_ref.seeded_state(31, hidden_size=64, num_layers=2)}, tmp_path / "r.pth")
    net = inference.load_model(tmp_path / "r.pth", device=hip_device)
    items = [{"audio": harmonic_complex(f0), "reference_f0": np.full(81, f0, f32)} for f0 in (110.0, 220.0)]
    out = inference.codec_sweep(net, items, bitrates_kbps=(16, 128), codecs=("transform", "g711u"))
    assert len(out["baseline"]) == 2 and len(out["conditions"]) == 6
    keys = {"condition", "kind", "item", "codec", "bitrate_kbps", *stress.METRIC_KEYS}
    assert all(set(rec) == keys and rec["kind"] == "codec" for rec in out["conditions"])
    assert [(rec["codec"], rec["bitrate_kbps"], rec["item"]) for rec in out["conditions"]] == \
        [(c, b, i) for c, b in (("transform", 16.0), ("transform", 128.0), ("g711u", 64.0)) for i in range(2)]
    assert [(row["codec"], row["bitrate_kbps"]) for row in out["summary"]] == \
        [("transform", 16.0), ("transform", 128.0), ("g711u", 64.0)]
    assert all({"RPA_mean", "RPA_std", "RPA_drop", "OctaveError_drop"} <= set(row) for row in out["summary"])
    with pytest.raises(ValueError):
        inference.codec_sweep(net, items, codecs=("opus",))


def test_a_tracker_survives_128_kbps(hip_device):
    """A 220 Hz harmonic complex through the 128 kbps condition, tracked by ``PraatACTracker``: every voiced frame of
    the clean track is found within the metric's 50 cents (tests/test_codec_cpu.py confirms the same of the
    restatement's output with tests/f0_track_ref.py)."""
    x = dev(harmonic_complex(), hip_device)
    cond = codec.CodecCondition("ptc 128", bitrate_kbps=128)
    y, lengths = stress.apply_condition(cond, x, 24000)
    assert lengths == [24000] and y.shape == x.shape
    tracker = PraatACTracker(24000, 300)
    clean, coded = tracker.track(x)[0], tracker.track(y)[0]
    m = inference.melody_metrics(coded, clean)
    print(f"128 kbps: RPA {m['RPA']} over {m['n_voiced']} voiced frames of {m['n_frames']}")
    assert m["n_voiced"] >= 40 and m["RPA"] == 1.0
    snr = 10 * torch.log10((x.double() ** 2).sum() / ((y.double() - x.double()) ** 2).sum())
    print(f"128 kbps: SNR {float(snr):.1f} dB")


# ------------------------------------------------------------------------------------------- end to end, reported only
@pytest.mark.parametrize("M, kbps", [(256, 32), (1024, 16), (1024, 64), (1024, 128)])
def test_end_to_end_is_reported(M, kbps, hip_device):
    """The kernel's output against the float64 chain around the same quantiser: a last-bit difference in a coefficient
    may move a q by one, so nothing is asserted but sanity; the figures are in DESIGN.md section 28."""
    x = R.vibrato_complex(seconds=0.5)
    c = codec.TransformCodec(24000, kbps, M)
    xd = dev(x, hip_device)
    y = c(xd).cpu().numpy().astype(np.float64)
    X, _ = c.mdct(xd)
    q = c.quantize(X)[0].cpu().numpy()
    X64 = R.mdct(x, M)
    rq, rg, rbits, rdeq = R.quantize_frames(X64.astype(f32), M, c.cutoff_bin, c.budget)
    y_ref = R.imdct(rdeq.astype(np.float64), x.size, M)
    rel = np.linalg.norm(y - y_ref) / np.linalg.norm(y_ref - x)
    share = float(np.mean(q != rq))
    print(f"M {M} {kbps} kbps: ||y_kernel - y_ref|| / ||y_ref - x|| = {rel:.3e}, share of differing q = {share:.3e}")
    assert np.all(np.isfinite(y)) and y.shape == x.shape
