"""The resampler's backward, host side (no GPU): the float64 restatement of its index form against the transpose of
the oracle, the adjoint identity, and the refusals that come before any device call."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import resample_ref as rr
from pitchextractor_amd import _lib, build, inference, ops
from pitchextractor_amd.resample import RaggedResampler, Resampler
from tests import resample_grad_ref as ref

RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 96000)
PAIRS = [(r, t) for t in (24000, 16000) for r in RATES if r != t]


def _sizes(rate, target):
    g = math.gcd(rate, target)
    orig, new = rate // g, target // g
    width = math.ceil(6 * orig / (min(orig, new) * 0.99))
    return orig, new, width


@pytest.mark.parametrize("rate,target", PAIRS)
def test_restatement_is_the_transpose_of_the_oracle(rate, target):
    """Column q of the forward matrix is the oracle's answer to the unit impulse at q; the restatement equals that
    matrix transposed times dy, with every output kept and with the last ones cut (n_out below out_len)."""
    orig, new, width = _sizes(rate, target)
    n_in = min(orig, 150) + 2 * width + 5                 # more than one phase period where that stays small
    rng = np.random.default_rng(rate + target)
    R = np.stack([rr.resample(np.eye(n_in)[q], rate, target) for q in range(n_in)], axis=1)     # (out_len, n_in)
    assert R.shape[0] == -(-n_in * new // orig)
    for n_out in (R.shape[0], R.shape[0] - min(new, R.shape[0] - 1) - 1):
        dy = rng.standard_normal(n_out)
        want = R[:n_out].T @ dy
        dx, T, K = ref.resample_backward(dy, rate, target, n_in)
        assert np.abs(dx - want).max() <= 1e-13 * np.abs(want).max()
        assert np.allclose(T, np.abs(R[:n_out]).T @ np.abs(dy), rtol=1e-12, atol=0)
        # every non-zero entry of a column is a term (a tap at the window's edge may itself be zero)
        assert (K >= (R[:n_out] != 0).sum(axis=0)).all() and K.max() <= new * -(-(2 * width + orig) // orig)


def test_largest_term_counts():
    """K_q of the common rates to 24 kHz: the length of the longest fmaf chain."""
    for rate, k_max in ((48000, 14), (16000, 24), (44100, 160), (22050, 320), (11025, 640)):
        orig, new, width = _sizes(rate, 24000)
        n_in = 3 * orig + 4 * width
        _, _, K = ref.resample_backward(np.ones(-(-n_in * new // orig)), rate, 24000, n_in)
        assert K.max() == k_max, rate


@pytest.mark.parametrize("rate,target", [(44100, 24000), (16000, 24000), (48000, 16000), (11025, 16000)])
def test_adjoint_identity(rate, target):
    rng = np.random.default_rng(5)
    n_in = 1777
    x = rng.standard_normal(n_in)
    y = rr.resample(x, rate, target)
    dy = rng.standard_normal(y.shape[0])
    dx, _, _ = ref.resample_backward(dy, rate, target, n_in)
    lhs, rhs = float(y @ dy), float(x @ dx)
    assert abs(lhs - rhs) <= 1e-12 * (np.abs(y) @ np.abs(dy))


def test_copied_rate_passes_the_gradient_through():
    dy = np.arange(5.0)
    dx, T, K = ref.resample_backward(dy, 24000, 24000, 7)
    assert np.array_equal(dx, [0, 1, 2, 3, 4, 0, 0]) and K.tolist() == [1] * 5 + [0] * 2


# --------------------------------------------------------------------------- refusals before any device call
def test_host_tensors_are_refused():
    g = torch.zeros(2, 80)
    with pytest.raises(RuntimeError, match=r"^resample_backward \(HIP\) needs a float32 device grad_out; no CPU"):
        ops.resample_backward(Resampler(44100, 24000), g, 147)
    with pytest.raises(RuntimeError, match=r"^resample_ragged_backward \(HIP\) needs a float32 device grad_out; no CPU"):
        ops.resample_ragged_backward(RaggedResampler(24000), g, [44100, 16000], [147, 40], packed=True)
    with pytest.raises(RuntimeError, match=r"\(HIP\) needs a float32 device grad_out"):
        ops.resample_backward(Resampler(44100, 24000), np.zeros((2, 80), np.float32), 147)
    x = torch.zeros(2, 147, requires_grad=True)
    with pytest.raises(RuntimeError, match=r"^Resampler \(HIP\) needs float32 device audio"):
        Resampler(44100, 24000)(x)
    with pytest.raises(RuntimeError, match=r"^RaggedResampler \(HIP\) needs contiguous-row float32 device audio"):
        RaggedResampler(24000)(x, [44100, 16000])


def test_f0_from_wave_rate_arguments_are_checked_first():
    x = torch.zeros(2, 4800)
    with pytest.raises(ValueError, match="not both"):
        inference.f0_from_wave(None, x, sample_rate=44100, rates=[44100, 16000])
    with pytest.raises(ValueError, match="whole rows"):
        inference.f0_from_wave(None, x, torch.tensor([4800, 100], dtype=torch.int32), sample_rate=44100)
    with pytest.raises(ValueError, match="host sequence"):
        inference.f0_from_wave(None, x, rates=[44100, 16000])


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _lib.load()


def test_backward_argument_checks(lib):
    """PE_E_ARG paths that return before any device call.  A single-rate plan owns a device table, so only its null
    check runs here; a ragged plan whose rates all equal the target allocates nothing, so every host-side check of
    pe_resample_ragged_backward does."""
    bad = -1
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.pe_resample_backward(None, p, 1, 8, 8, p, 16, 16, None) == bad
    plan = ctypes.c_void_p()
    rates = (ctypes.c_int * 2)(24000, 24000)
    assert lib.pe_resample_ragged_plan_create(ctypes.byref(plan), rates, 2, 24000, 6, 0.99) == 0
    try:
        off = ctypes.cast((ctypes.c_long * 2)(0, 16), ctypes.c_void_p)
        n_in = (ctypes.c_int * 2)(16, 10)
        idx = (ctypes.c_int * 2)(0, 1)
        p_n, p_i = ctypes.cast(n_in, ctypes.c_void_p), ctypes.cast(idx, ctypes.c_void_p)

        def bwd(**kw):
            a = dict(plan=plan, dy=p, stride=32, off=off, n=p_n, i=p_i, hn=p_n, hi=p_i, batch=2, dx=p, width=16)
            a.update(kw)
            return lib.pe_resample_ragged_backward(a["plan"], a["dy"], a["stride"], a["off"], a["n"], a["i"], a["hn"],
                                                   a["hi"], a["batch"], a["dx"], a["width"], None)
        for name in ("plan", "dy", "off", "n", "i", "hn", "hi", "dx"):
            assert bwd(**{name: None}) == bad, name
        assert bwd(stride=15) == bad                                   # row 0's 16 output gradients do not fit
        assert bwd(stride=-1) == bad
        assert bwd(width=15) == bad                                    # padded rows narrower than row 0
        assert bwd(width=-1) == bad
        assert bwd(batch=-1) == bad
        idx[1] = 2
        assert bwd() == bad                                            # rate index out of range
        idx[1] = -1
        assert bwd() == bad
        idx[1] = 1
        n_in[1] = -1
        assert bwd() == bad
        n_in[1] = 10
        assert bwd(batch=0) == 0                                       # nothing to do, nothing launched
    finally:
        assert lib.pe_resample_ragged_plan_destroy(plan) == 0
