"""The pitch shifter off the six default semitones: two octaves and fractional steps, the lengths where a frame count
changes, digital silence, output windows bit for bit against the full shift, ragged bookkeeping, and one row long
enough for every grid-stride loop to take a second pass.  Each stage is compared with the float64 restatement fed the
GPU's own input to that stage, at the bounds of ``test_pitch_shift_gpu.py``."""
import numpy as np
import pytest
import torch

from pitchextractor_amd import pitch_shift as ps
from tests import pitch_shift_ref as ref
from tests.test_pitch_shift_gpu import SR, _rows, _run

pytestmark = pytest.mark.gpu
N_, XOFF, FUSE, FOFF, CLO, CHI, COFF, M_, NOLA, SLO, SHI, SOFF, NRES, JLO, JCNT, JOFF, OOFF, NCOLS = range(18)
WIDE_STEPS = [-24, -12, -7.3, -0.5, 0.5, 7.3, 12, 24]
RES = ["kaiser_best", "kaiser_fast"]


def _close(got, want, bound, what):
    """|got - want| <= bound * max |want|, the stage criterion; an empty stage must be empty on both sides."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.size:
        err, top = np.abs(got - want).max(), np.abs(want).max()
        print(f"{what}: err {err:.3e}, max {top:.3e}, ratio {err / top if top else 0:.3e}")
        assert err <= bound * top, (what, err, top)


def _counts(m, n, s):
    """Frame counts, n_ola, M and int(M r) of a plan row against the restatement's."""
    F = 1 + n // ps.HOP
    rate = ps.stretch_rate(s)
    n_cols = len(np.arange(0, F, rate))
    M = int(round(n / rate))
    n_ola = min(n_cols, int(np.ceil((M + ps.N_FFT) / ps.HOP)))
    assert (m[N_], m[NCOLS], m[M_], m[NOLA], m[NRES]) == (n, n_cols, M, n_ola, int(M * ps.resample_ratio(s, SR)))
    assert m[FUSE] <= F
    return F, M


def _check_rows(waves, steps, plan, keep, out, res_type="kaiser_best", stages=("stft", "vocoder", "istft", "resample")):
    """Every whole-row stage of a ragged batch, row by row, against float64 on the GPU's own input to that stage."""
    spec = _rows(plan, keep["spec"], FOFF, lambda m: m[FUSE])
    cols = _rows(plan, keep["cols"], COFF, lambda m: m[CHI] - m[CLO])
    st = _rows(plan, keep["stretched"], SOFF, lambda m: m[SHI] - m[SLO])
    for r, (w, s) in enumerate(zip(waves, steps)):
        m, n = plan.meta[r], w.size
        F, M = _counts(m, n, s)
        assert m[CLO] == 0 and m[SLO] == 0 and (m[JLO], m[JCNT]) == (0, n)
        rate, ratio = plan.ratios[r]
        tag = f"n={n} s={s}"
        if "stft" in stages:
            _close(spec[r], ref.stft(w)[:m[FUSE]], 1e-5, f"stft {tag}")
        full = np.concatenate([spec[r].astype(np.complex128), np.zeros((F - m[FUSE], ps.N_BINS))])
        full[full == 0] = 0                                   # numpy's spectrum of silence is +0
        if "vocoder" in stages:
            _close(cols[r], ref.phase_vocoder(full, rate)[:m[CHI]], 1e-4, f"vocoder {tag}")
        if "istft" in stages and M == 0:
            assert st[r].size == 0 and cols[r].size == 0
        elif "istft" in stages:
            _close(st[r], ref.istft(cols[r].astype(np.complex128), M)[:m[SHI]], 1e-5, f"istft {tag}")
        if "resample" in stages:
            x = np.zeros(M)
            x[:m[SHI]] = st[r]
            y = ref.resample(x, ratio, res_type)
            assert y.size == m[NRES]
            want = np.zeros(n)
            want[:min(n, y.size)] = y[:n]
            _close(out[r, :n].astype(np.float64), want, 1e-5, f"resample {res_type} {tag}")
            assert (out[r, n:] == 0).all()


def _noise(rng, n, amp=0.3):
    return (amp * rng.standard_normal(n)).astype(np.float32)


# --------------------------------------------------------------------------- s = 0
def test_zero_semitones_every_stage_and_copy(hip_device):
    """n_steps = 0: rate and ratio are exactly 1, every stage holds its bound and the resampler copies the stretched
    signal (librosa's resample returns its input when the rates are equal)."""
    rng = np.random.default_rng(10)
    waves = [_noise(rng, n) + ref.three_sines(n) for n in (700, 20011)]
    for res_type in RES:
        plan, keep, out = _run(waves, [0, 0], hip_device, res_type=res_type)
        assert (plan.ratios == 1.0).all()
        _check_rows(waves, [0, 0], plan, keep, out, res_type)
        st = _rows(plan, keep["stretched"], SOFF, lambda m: m[SHI] - m[SLO])
        for r, w in enumerate(waves):
            assert st[r].size == w.size
            np.testing.assert_array_equal(out[r, :w.size], st[r])


# --------------------------------------------------------------------------- steps off the default list
@pytest.mark.parametrize("res_type", RES)
def test_resample_stage_wide_steps(hip_device, res_type):
    """Ratios 0.25 .. 4 (table stride 128 .. 512, up to 256 taps a side) and irrational ones, the zero tail from
    int(M r) to N at upward shifts included."""
    rng = np.random.default_rng(11)
    waves = [_noise(rng, 6000 + 997 * i) for i in range(len(WIDE_STEPS))]
    plan, keep, out = _run(waves, WIDE_STEPS, hip_device, res_type=res_type)
    _check_rows(waves, WIDE_STEPS, plan, keep, out, res_type, stages=("resample",))
    tails = [w.size - int(plan.meta[r, NRES]) for r, w in enumerate(waves)]
    assert max(tails) == 1                                    # int(M r) is within a sample or two of N: two rows end
    for r, t in enumerate(tails):                             # on one zero sample that the resampler does not make
        assert t <= 0 or (out[r, plan.meta[r, NRES]:waves[r].size] == 0).all()


def _vocoder_case(n_frames, s, dev, rng):
    """Well-conditioned random spectrum (|D| in [0.5, 2]) of n_frames frames through the GPU's vocoder stage and the
    float64 restatement: (got, want, plan)."""
    n = ps.HOP * (n_frames - 1)
    plan = ps.Plan([n], [s], sr=SR)
    F = plan.n_frames
    assert F <= n_frames == 1 + n // ps.HOP
    D = (rng.uniform(0.5, 2.0, (F, ps.N_BINS)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (F, ps.N_BINS))))
    D = D.astype(np.complex64)
    spec = torch.view_as_real(torch.from_numpy(D)).contiguous().to(dev)
    _, keep, _ = _run([np.zeros(n, np.float32)], [s], dev, spec=spec)
    got = keep["cols"].cpu().numpy()
    c_hi = int(plan.meta[0, CHI])
    assert got.shape[0] == c_hi and plan.meta[0, CLO] == 0
    full = np.concatenate([D.astype(np.complex128), np.zeros((n_frames - F, ps.N_BINS))])
    return got, ref.phase_vocoder(full, ps.stretch_rate(s))[:c_hi], plan


@pytest.mark.parametrize("s,n_frames", [(-24, 1210), (24, 80), (7.3, 200), (-0.5, 312)])
def test_phase_vocoder_stage_wide_steps(hip_device, s, n_frames):
    got, want, _ = _vocoder_case(n_frames, s, hip_device, np.random.default_rng(12))
    assert got.shape[0] >= 300
    _close(got, want, 1e-4, f"vocoder s={s}")


# --------------------------------------------------------------------------- length edges
EDGE_LENS = [2, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049]


@pytest.mark.parametrize("s", [-4, 4, -24, 24])
def test_length_edges(hip_device, s):
    """Rows of one and two frames and the lengths around 512, 1024 and 2048 where the frame count, n_ola and int(M r)
    change, in one ragged batch; at -24 the 2-sample row stretches to no sample at all."""
    rng = np.random.default_rng(13)
    lens = [n for n in EDGE_LENS if abs(s) < 24 or n <= 1025]
    waves = [_noise(rng, n) for n in lens]
    plan, keep, out = _run(waves, [s] * len(lens), hip_device)
    if s == -24:
        assert plan.meta[0, M_] == 0 and plan.meta[0, FUSE] == 0 and (out[0] == 0).all()
    _check_rows(waves, [s] * len(lens), plan, keep, out, stages=("stft", "istft", "resample"))


# --------------------------------------------------------------------------- digital silence
def test_all_zero_row_stays_zero(hip_device):
    waves = [np.zeros(20000, np.float32)] * 3
    _, keep, out = _run(waves, [-2, 4, 0], hip_device)
    assert (out == 0).all() and (keep["stretched"].cpu().numpy() == 0).all()


@pytest.mark.parametrize("s", [-2, 4])
def test_silence_then_signal_vocoder(hip_device, s):
    """8192 exact zeros, then three sines.  The transform of silence may hold -0; read as it stands, its phase pi would
    turn every column that fades in from silence.  Compared over the bins above 1e-3 of the largest magnitude (9.8 % /
    10.1 % of the cells from the onset column on at s = -2 / 4) and, because that is less than a fifth, also over the
    bins above 1e-4 (22.3 % / 24.9 %) at the same bound; test_pitch_shift_edges_cpu.py holds the shares."""
    y = ref.silence_then_signal()
    plan, keep, _ = _run([y], [s], hip_device)
    m = plan.meta[0]
    F = 1 + y.size // ps.HOP
    mask, onset, share = ref.loud_cells(ref.phase_vocoder(ref.stft(y), ps.stretch_rate(s)), ref.SILENCE_WIDE_FLOOR)
    assert share >= 0.2
    spec = keep["spec"].cpu().numpy()
    assert spec.shape[0] == m[FUSE] and (spec[:15] == 0).all()
    print(f"-0 in the silent frames: {np.signbit(spec[:15].real).sum()} real, {np.signbit(spec[:15].imag).sum()} imaginary")
    full = np.concatenate([spec.astype(np.complex128), np.zeros((F - m[FUSE], ps.N_BINS))])
    full[full == 0] = 0                                       # numpy's spectrum of silence is +0
    want = ref.phase_vocoder(full, ps.stretch_rate(s))[:m[CHI]]
    got = keep["cols"].cpu().numpy()
    assert got.shape == want.shape and (got[:onset] == 0).all()
    top = np.abs(want).max()
    for floor in (ref.SILENCE_FLOOR, ref.SILENCE_WIDE_FLOOR):
        keep_cells, onset_g, share_g = ref.loud_cells(want, floor)
        err = np.abs(got - want)[keep_cells].max()
        print(f"s={s} floor {floor}: onset {onset_g}, share {share_g:.3f}, err {err:.3e} of max {top:.3e}")
        assert onset_g == onset and err <= 1e-4 * top
    assert share_g >= 0.2


@pytest.mark.parametrize("s", [-2, 4])
def test_negative_zero_spectrum_reads_as_silence(hip_device, s):
    """Whether a transform of silence holds -0 is the transform's business (its sign flips); the vocoder must read
    -0 as +0 either way.  The silent frames are handed over as (-0, +0) and as (-0, -0), whose phases would be pi and
    -pi, against the float64 restatement of the spectrum with +0 there."""
    y = ref.silence_then_signal()
    D = ref.stft(y).astype(np.complex64)
    silent = np.abs(D).max(axis=1) == 0
    assert silent[:15].all() and not silent[15:].any()
    want = ref.phase_vocoder(D.astype(np.complex128), ps.stretch_rate(s))
    mask, onset, share = ref.loud_cells(want, ref.SILENCE_WIDE_FLOOR)
    assert share >= 0.2
    for im in (0.0, -0.0):
        Dn = D.copy()
        Dn[:15] = complex(-0.0, im)
        assert np.signbit(Dn[:15].real).all() and (np.signbit(Dn[:15].imag) == np.signbit(im)).all()
        spec = torch.view_as_real(torch.from_numpy(Dn)).contiguous().to(hip_device)
        plan, keep, _ = _run([y], [s], hip_device, spec=spec[:ps.Plan([y.size], [s], sr=SR).n_frames].contiguous())
        got = keep["cols"].cpu().numpy()
        c_hi = int(plan.meta[0, CHI])
        assert got.shape[0] == c_hi and (got[:onset] == 0).all()
        err = np.abs(got - want[:c_hi])[mask[:c_hi]].max()
        print(f"s={s} silent frames (-0, {im}): err {err:.3e} of max {np.abs(want).max():.3e}")
        assert err <= 1e-4 * np.abs(want).max()


# --------------------------------------------------------------------------- windows, bit for bit
@pytest.mark.parametrize("res_type", RES)
@pytest.mark.parametrize("s", [-12, -4, 0.5, 4, 12])
def test_windows_equal_the_full_shift_bit_for_bit(hip_device, s, res_type):
    """Every stage walks the same work in the same order whatever the window; the window only skips reads outside
    ranges that the plan proves sufficient (test_pitch_shift_edges_cpu.py), so equality is exact.  Gains are powers
    of two: gain and noise round once whether or not they are fused."""
    N = 60011
    rng = np.random.default_rng(14)
    w = _noise(rng, N, 0.05) + ref.three_sines(N)
    x = torch.from_numpy(w).to(hip_device)
    full = ps.pitch_shift(x, sr=SR, n_steps=s, res_type=res_type).cpu().numpy()
    wins = [(0, 1), (0, 5000), (29000, 2000), (N - 1, 1)]
    n_res = min(N, ps.resampled_len(N, s, SR))                 # int(M r) is N - 1 at 0.5 and 4, N at 12
    if s > 0:
        assert (full[n_res:] == 0).all() and np.abs(full[n_res - 100:n_res]).max() > 0
        wins.append((n_res - 100, N - (n_res - 100)))
    rows = [(lo, cnt, g) for g in (1.0, 0.5, 2.0) for lo, cnt in wins]
    R = len(rows)
    out = torch.zeros((R + 1, 5000), dtype=torch.float32, device=hip_device)
    noise = torch.randn(sum(c for _, c, _ in rows), device=hip_device) * 1e-3
    ps.pitch_shift_ragged(x, [0] * R, [N] * R, [s] * R, torch.tensor([g for _, _, g in rows]), out,
                          out_rows=list(range(R)), out_start=[lo for lo, _, _ in rows], out_len=[c for _, c, _ in rows],
                          sr=SR, res_type=res_type, noise=noise)
    plain = torch.zeros((len(wins), 5000), dtype=torch.float32, device=hip_device)
    ps.pitch_shift_ragged(x, [0] * len(wins), [N] * len(wins), [s] * len(wins), torch.ones(len(wins)), plain,
                          out_start=[lo for lo, _ in wins], out_len=[c for _, c in wins], sr=SR, res_type=res_type)
    torch.cuda.synchronize()
    o, p, nz = out.cpu().numpy(), plain.cpu().numpy(), noise.cpu().numpy()
    for i, (lo, cnt) in enumerate(wins):
        np.testing.assert_array_equal(p[i, :cnt], full[lo:lo + cnt], err_msg=f"window {lo}+{cnt}")
        assert (p[i, cnt:] == 0).all()
    at = 0
    for i, (lo, cnt, g) in enumerate(rows):
        np.testing.assert_array_equal(o[i, :cnt], np.float32(g) * full[lo:lo + cnt] + nz[at:at + cnt],
                                      err_msg=f"window {lo}+{cnt} gain {g}")
        assert (o[i, cnt:] == 0).all()
        at += cnt
    assert (o[R] == 0).all()


def test_ragged_rows_without_work_and_permuted_outputs(hip_device):
    """300 short rows at seeded steps, every 7th (the last included) with a window of no samples -- rows without work
    share their successor's offsets in every stage's row search -- written through a permutation of the output rows:
    each row equals the row alone bit for bit, what no row addresses stays zero."""
    rng = np.random.default_rng(15)
    R = 300
    lens = rng.integers(600, 3001, R)
    steps = rng.choice(WIDE_STEPS, R)
    waves = [_noise(rng, int(n)) for n in lens]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    empty = np.arange(R) % 7 == 5
    assert empty[R - 1] and empty.sum() == 43
    out_len = np.where(empty, 0, lens)
    out_rows = rng.permutation(R + 4)[:R]
    flat = torch.from_numpy(np.concatenate(waves)).to(hip_device)
    out = torch.zeros((R + 4, 3000), dtype=torch.float32, device=hip_device)
    ps.pitch_shift_ragged(flat, offs, lens, steps, torch.ones(R), out, out_rows=out_rows, out_len=out_len, sr=SR)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    alone = [None if empty[r] else ps.pitch_shift(flat[offs[r]:offs[r] + lens[r]], sr=SR, n_steps=float(steps[r]))
             for r in range(R)]
    torch.cuda.synchronize()
    used = np.zeros(R + 4, bool)
    for r in range(R):
        row = o[out_rows[r]]
        used[out_rows[r]] = True
        if empty[r]:
            assert (row == 0).all(), r
        else:
            np.testing.assert_array_equal(row[:lens[r]], alone[r].cpu().numpy(), err_msg=f"row {r}")
            assert np.abs(row[:lens[r]]).max() > 0 and (row[lens[r]:] == 0).all(), r
    assert (~used).sum() == 4 and (o[~used] == 0).all()


# --------------------------------------------------------------------------- second grid pass
def test_long_row_takes_a_second_grid_pass(hip_device):
    """4.3 M samples at s = -2: 8399 frames (the STFT grid holds 8192), 3.83 M stretched samples (the overlap-add grid
    1 Mi), 4.3 M outputs (the resampler grid 2 Mi).  The transforms are compared whole, the resampler on slices at the
    pass edges 2^21 and 2^22 and at the row's end."""
    N, s = 4_300_000, -2
    rng = np.random.default_rng(16)
    w = _noise(rng, N, 0.01) + (0.3 * np.sin(2 * np.pi * 220.0 * np.arange(N) / SR)).astype(np.float32)
    plan, keep, out = _run([w], [s], hip_device)
    m = plan.meta[0]
    F, M = _counts(m, N, s)
    assert F == 8399 == m[FUSE] > 8192 and m[SHI] == M > (1 << 20) and m[NRES] > (1 << 22)
    spec = keep["spec"].cpu().numpy()
    _close(spec, ref.stft(w), 1e-5, "stft long")
    del spec
    cols = keep["cols"].cpu().numpy()
    st = keep["stretched"].cpu().numpy()
    assert cols.shape[0] == m[CHI] and st.size == M
    _close(st, ref.istft(cols.astype(np.complex128), M), 1e-5, "istft long")
    del cols
    ratio = plan.ratios[0, 1]
    n_res = int(m[NRES])
    assert n_res <= N
    j = np.concatenate([np.arange((1 << 21) - 1000, (1 << 21) + 1000), np.arange((1 << 22) - 1000, (1 << 22) + 1000),
                        np.arange(n_res - 2000, n_res)])
    want = ref.resample_at(st.astype(np.float64), ratio, "kaiser_best", j)
    _close(out[0, j].astype(np.float64), want, 1e-5, "resample long")
    assert (out[0, n_res:] == 0).all()


def test_phase_vocoder_past_8192_columns(hip_device):
    """The vocoder's grid has no stride, but the inverse transform after it does: 8400 well-conditioned frames, the
    columns on both sides of 8192 and the last ones."""
    got, want, plan = _vocoder_case(8400, 1, hip_device, np.random.default_rng(17))
    C = got.shape[0]
    assert C > 8192 + 8
    for lo, hi in ((8184, 8192), (8192, 8200), (C - 8, C)):
        err = np.abs(got[lo:hi] - want[lo:hi]).max()
        print(f"vocoder columns {lo}..{hi}: err {err:.3e}")
        assert err <= 1e-4 * np.abs(want).max(), (lo, err)
