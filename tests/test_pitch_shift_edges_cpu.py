"""The pitch shifter's host side off the default semitones, without a GPU: the Python length helpers against the
plan at steps float32 does not represent, the plan's ranges against a restatement of what each kernel reads, and the
helpers the GPU edge tests stand on (``resample_at``, the s = 0 rule, the mask of the silence test)."""
import ctypes

import numpy as np
import pytest

from pitchextractor_amd import _lib, build
from pitchextractor_amd import pitch_shift as ps
from tests import pitch_shift_ref as ref

SR = 24000
# plan fields (csrc/pitch_shift.hip)
N_, XOFF, FUSE, FOFF, CLO, CHI, COFF, M_, NOLA, SLO, SHI, SOFF, NRES, JLO, JCNT, JOFF, OOFF, NCOLS = range(18)


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _lib.load()


def test_length_helpers_use_the_plans_float32_step(lib):
    """0.35, 7.3, ... are not float32 numbers: the plan sees the rounded step, and so must every helper."""
    lens = np.arange(1, 200000, 37)
    for s in (0.35, 7.3, -7.3, 0.1, -0.1, 3.3, 11.9, 0.5, -12, 24):
        plan = ps.Plan(lens, np.full(lens.size, s), sr=SR)
        assert (plan.ratios[:, 0] == ps.stretch_rate(s)).all() and (plan.ratios[:, 1] == ps.resample_ratio(s, SR)).all()
        assert ps.stretch_rate(s) == 2.0 ** (-float(np.float32(s)) / 12)
        np.testing.assert_array_equal(plan.meta[:, M_], [ps.stretched_len(n, s) for n in lens])
        np.testing.assert_array_equal(plan.meta[:, NRES], [ps.resampled_len(n, s, SR) for n in lens])
        np.testing.assert_array_equal(plan.meta[:, NCOLS], [ps.stretched_columns(n, s) for n in lens])


SWEEP_STEPS = (-24, -12, -7.3, -4, -1, -0.5, 0, 0.5, 1, 4, 7.3, 12, 24)
SWEEP_LENS = (1, 2, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 3000, 20011, 100000)


def _sweep_rows():
    rng = np.random.default_rng(7)
    rows = []
    for s in SWEEP_STEPS:
        for n in SWEEP_LENS:
            wins = [(0, n)]
            for _ in range(6):
                lo = int(rng.integers(0, n))
                wins.append((lo, int(rng.integers(0, n - lo + 1))))
            wins += [(0, 1), (n // 2, 1), (n - 1, 1), (n, 0)]
            rows += [(n, s, lo, cnt) for lo, cnt in wins]
    return rows


@pytest.mark.parametrize("res_type", ["kaiser_best", "kaiser_fast"])
def test_plan_ranges_cover_every_read(lib, res_type):
    """[s_lo, s_hi) holds every stretched sample the resampler's tap loops read for the kept outputs, [c_lo, c_hi)
    every frame the overlap-add sums into those samples, f_use every input frame the vocoder reads up to column
    c_hi - 1 (frames from F on are the two zero columns librosa appends)."""
    rows = _sweep_rows()
    assert len(rows) == len(SWEEP_STEPS) * len(SWEEP_LENS) * 11
    n, s, lo, cnt = (np.array(c) for c in zip(*rows))
    plan = ps.Plan(n, s, out_start=lo, out_len=cnt, sr=SR, res_type=res_type)
    meta = plan.meta
    gaps = []
    for r, m in enumerate(meta):
        rate, ratio = plan.ratios[r]
        N, M, n_res = int(n[r]), ps.stretched_len(n[r], s[r]), ps.resampled_len(n[r], s[r], SR)
        F, n_cols = ps.stft_frames(N), ps.stretched_columns(N, s[r])
        n_ola = min(n_cols, -(-(M + ps.N_FFT) // ps.HOP))
        assert (m[N_], m[M_], m[NRES], m[NCOLS], m[NOLA]) == (N, M, n_res, n_cols, n_ola), rows[r]
        assert (m[JLO], m[JCNT]) == (lo[r], cnt[r]) and m[OOFF] == r * plan.out_stride
        assert 0 <= m[SLO] <= m[SHI] <= M and 0 <= m[CLO] <= m[CHI] <= n_ola and 0 <= m[FUSE] <= F, rows[r]
        j = np.arange(lo[r], min(lo[r] + cnt[r], n_res))
        if j.size:
            r_lo, r_hi = ref.resampler_reads(j, ratio, M, res_type)
            some = r_lo <= r_hi
            assert r_lo[some].min(initial=0) >= 0 and r_hi[some].max(initial=0) < M
            if some.any() and not (m[SLO] <= r_lo[some].min() and r_hi[some].max() < m[SHI]):
                gaps.append(("resampler", rows[r]))
        if m[SHI] > m[SLO]:
            t_lo, t_hi = ref.ola_reads(np.arange(m[SLO], m[SHI]), n_ola)
            some = t_lo <= t_hi
            if some.any() and not (m[CLO] <= t_lo[some].min() and t_hi[some].max() < m[CHI]):
                gaps.append(("overlap-add", rows[r]))
        if m[CHI] > 0 and m[FUSE] < min(F, ref.vocoder_last_frame(int(m[CHI]), rate) + 1):
            gaps.append(("vocoder", rows[r]))
    assert not gaps, (len(gaps), gaps[:10])
    # prefix offsets and totals are the sums of the per-row extents
    ext = np.stack([meta[:, FUSE], meta[:, CHI] - meta[:, CLO], meta[:, SHI] - meta[:, SLO], meta[:, JCNT]], axis=1)
    np.testing.assert_array_equal(plan.totals, ext.sum(axis=0))
    off = np.concatenate([np.zeros((1, 4), np.int64), np.cumsum(ext, axis=0)[:-1]])
    np.testing.assert_array_equal(meta[:, [FOFF, COFF, SOFF, JOFF]], off)


def test_plan_accepts_two_octaves_and_no_more(lib):
    L = lambda *v: (ctypes.c_long * len(v))(*v)  # noqa: E731
    meta, rat, tot = (ctypes.c_long * 32)(), (ctypes.c_double * 2)(), (ctypes.c_long * 4)()

    def plan(s):
        return lib.pe_pitch_shift_plan(1, L(1000), (ctypes.c_float * 1)(s), L(0), L(0), L(1000), L(0), 1000, SR, 2048,
                                       512, 0, meta, rat, tot)
    assert plan(24.0) == 0 and rat[0] == 0.25 and rat[1] == 0.25
    assert plan(-24.0) == 0 and rat[0] == 4.0 and rat[1] == 4.0
    over = float(np.nextafter(np.float32(24), np.float32(np.inf)))
    assert over > 24.0 and plan(over) == -1 and plan(-over) == -1          # PE_E_ARG


# --------------------------------------------------------------------------- helpers of the GPU edge tests
@pytest.mark.parametrize("res_type", ["kaiser_best", "kaiser_fast"])
def test_resample_at_equals_resample(res_type):
    x = np.random.default_rng(0).standard_normal(3001)
    for s in (-24, -7.3, 0, 0.5, 12, 24):
        ratio = ps.resample_ratio(s, SR)
        y = ref.resample(x, ratio, res_type)
        j = np.concatenate([np.arange(40), np.arange(y.size // 2, y.size // 2 + 40), np.arange(y.size - 40, y.size)])
        got = ref.resample_at(x, ratio, res_type, j)
        assert np.abs(got - y[j]).max() <= 1e-13 * np.abs(y).max(), s


def test_zero_semitones_resamples_by_copy():
    """librosa.resample returns its input when orig_sr == target_sr: at n_steps = 0 no low-pass is applied."""
    assert ps.stretch_rate(0) == 1.0 and ps.resample_ratio(0, SR) == 1.0 and ps.resample_ratio(-0.0, SR) == 1.0
    x = np.random.default_rng(1).standard_normal(5000)
    np.testing.assert_array_equal(ref.resample(x, 1.0), x)
    np.testing.assert_array_equal(ref.resample(x, 1.0, "kaiser_fast"), x)


@pytest.mark.parametrize("s", [-2, 4])
def test_silence_masks_keep_a_fifth_of_the_cells(s):
    """The masks of the GPU silence test, from the float64 reference alone.  The cells compared must be at least 20 %
    of the (column, bin) cells from the onset column on, or the mask could hide a failure.  Bins above 1e-3 of the
    largest magnitude are 9.8 % (s = -2) and 10.1 % (s = 4) of them: three sines fill few bins.  The GPU test
    therefore also compares the bins down to 1e-4 of the largest, at the same bound: 22.3 % and 24.9 %.  What a -0
    in the silent frames does is restated here too: it turns the phase of the columns that fade in from silence by
    pi, an error of twice the magnitude in cells that both masks keep."""
    y = ref.silence_then_signal()
    D = ref.stft(y)
    assert (D[:15] == 0).all() and np.abs(D[15]).max() > 0
    want = ref.phase_vocoder(D, ps.stretch_rate(s))
    mask, onset, share = ref.loud_cells(want, ref.SILENCE_FLOOR)
    wide, onset_w, share_w = ref.loud_cells(want, ref.SILENCE_WIDE_FLOOR)
    print(f"s={s}: onset column {onset} of {want.shape[0]}, the masks keep {share:.3f} and {share_w:.3f} of the cells")
    assert onset == onset_w > 0 and (want[:onset] == 0).all() and (wide >= mask).all()
    assert 0.09 <= share < 0.2 <= share_w
    Dn = D.copy()
    Dn[:15] = complex(-0.0, 0.0)
    assert np.angle(Dn[0, 0]) == np.pi
    dev = np.abs(ref.phase_vocoder(Dn, ps.stretch_rate(s)) - want)
    hit = dev > 1e-4 * np.abs(want).max()
    assert (hit & mask).sum() >= 50 and (dev[hit & mask] >= np.abs(want[hit & mask])).all()
