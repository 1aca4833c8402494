"""The mel backward without a GPU: the float64 restatement (tests/mel_grad_ref.py) against torch autograd in float64
and against central finite differences of the oracle, and the host-side checks of the C-ABI entry points."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import mel_ref
from pitchextractor_amd import _lib, build
from tests import mel_grad_ref as ref


def _case(n, hop, seed=0):
    rng = np.random.default_rng(seed + 7 * n + hop)
    return 0.3 * rng.standard_normal(n), rng.standard_normal((80, 1 + n // hop))


@pytest.mark.parametrize("log", [True, False], ids=["log", "power"])
@pytest.mark.parametrize("hop", [300, 75, 1200])
@pytest.mark.parametrize("n", [513, 899, 900, 1025, 4801])
def test_restatement_matches_float64_autograd(n, hop, log):
    x, g = _case(n, hop)
    got = ref.mel_backward(x, g, log=log, hop_length=hop)
    want = ref.autograd_grad(x, g, torch.float64, log=log, hop_length=hop)
    assert ref.rel_err(got, want) <= 1e-10


def test_restatement_honours_crop_and_padding():
    """frame_start and out_frames: padded positions are never read (NaN there), a crop is the slice of the full map."""
    n, hop = 4801, 300
    x, g = _case(n, hop)
    padded = np.full((80, 24), np.nan)
    padded[:, :14] = g[:, 3:17]
    got = ref.mel_backward(x, padded, frame_start=3, hop_length=hop)
    full = np.zeros_like(g)
    full[:, 3:17] = g[:, 3:17]
    assert np.isfinite(got).all()
    assert ref.rel_err(got, ref.autograd_grad(x, full, torch.float64, hop_length=hop)) <= 1e-10
    assert ref.rel_err(ref.autograd_grad(x, padded, torch.float64, frame_start=3, hop_length=hop), got) <= 1e-10
    assert not ref.mel_backward(x[:300], g).any()


@pytest.mark.parametrize("log", [True, False], ids=["log", "power"])
def test_restatement_matches_finite_differences(log):
    """Central differences of the oracle's (log-)mel in float64 at a dozen samples, the ones the reflect fold lands on
    included: relative step error h^2 f''' / 6 f' is far below the 1e-6 asked, rounding ~1e-16 / h = 1e-10."""
    n, hop, h = 1500, 300, 1e-6
    x, g = _case(n, hop)
    fwd = mel_ref.log_mel if log else mel_ref.mel_spectrogram
    grad = ref.mel_backward(x, g, log=log, hop_length=hop)
    scale = np.abs(grad).max()
    for i in (0, 1, 2, 511, 512, 513, 700, n - 514, n - 513, n - 3, n - 2, n - 1):
        e = np.zeros(n)
        e[i] = h
        fd = ((fwd(x + e, hop_length=hop) - fwd(x - e, hop_length=hop)) * g).sum() / (2 * h)
        assert abs(fd - grad[i]) <= 1e-6 * scale, (i, fd, grad[i])


# ---- host-side checks of the entry points (no device call is reached)

@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _lib.load()


def _host_plan(hop=300, n_mels=80, n_pairs=162):
    """A plan header on the host (csrc/mel_plan.h: six ints, then device pointers, all null here): enough for the size
    function and for every check that precedes the first device call."""
    plan = (ctypes.c_int * 32)()
    plan[0:6] = [24000, 1024, hop, n_mels, 513, n_pairs]
    return plan


def _args(plan, p, batch=2, n=4801, stride=4801, frames=17, std=4.0, gw=None, gw_stride=4801, ws=None, ws_bytes=1 << 30,
          wave=None):
    ws = p if ws is None else ws
    return (plan, p if wave is None else wave, batch, n, stride, p, 80 * frames, frames, 1, frames, 1, 1e-5, -4.0, std,
            p if gw is None else gw, gw_stride, ws, ws_bytes, None)


def test_argument_checks_run_before_any_device_call(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    plan = ctypes.cast(_host_plan(), ctypes.c_void_p)
    arg, unsupported, workspace = -1, -2, -3              # PE_E_ARG, PE_E_UNSUPPORTED, PE_E_WORKSPACE
    fixed = lib.pe_mel_backward
    assert fixed(*_args(None, p)) == arg                                    # null plan
    for null in ("wave", "gw", "ws"):
        assert fixed(*_args(plan, p, **{null: ctypes.c_void_p(None)})) == arg
    assert fixed(plan, p, 2, 4801, 4801, None, 1360, 17, 1, 17, 1, 1e-5, -4.0, 4.0, p, 4801, p, 1 << 30, None) == arg
    assert fixed(*_args(plan, p, batch=0)) == arg
    assert fixed(*_args(plan, p, batch=-1)) == arg
    assert fixed(*_args(plan, p, n=0)) == arg
    assert fixed(*_args(plan, p, frames=0)) == arg
    assert fixed(*_args(plan, p, std=0.0)) == arg
    assert fixed(*_args(plan, p, n=512, stride=512, gw_stride=512)) == arg  # reflect padding needs more than 512
    assert fixed(*_args(plan, p, stride=4800)) == arg
    assert fixed(*_args(plan, p, gw_stride=4800)) == arg
    assert fixed(*_args(plan, p, batch=65536)) == unsupported
    big = (1 << 30) + 1
    assert fixed(*_args(plan, p, n=big, stride=big, gw_stride=big)) == unsupported
    assert fixed(*_args(ctypes.cast(_host_plan(hop=20000), ctypes.c_void_p), p)) == unsupported   # segment > LDS
    need = lib.pe_mel_backward_workspace_bytes(plan, 2, 4801, 17)
    assert fixed(*_args(plan, p, ws_bytes=need - 1)) == workspace
    assert fixed(*_args(plan, p, ws_bytes=0)) == workspace

    def ragged(plan_, lengths, **kw):
        a = _args(plan_, p, **kw)
        return lib.pe_mel_backward_ragged(*a[:5], lengths, None, *a[5:])

    assert ragged(None, p) == arg
    assert ragged(plan, None) == arg                                        # ragged without lengths
    assert ragged(plan, p, std=0.0) == arg
    assert ragged(plan, p, batch=0) == arg
    assert ragged(plan, p, batch=65536) == unsupported
    assert ragged(plan, p, n=300, stride=300, gw_stride=300, ws_bytes=0) == workspace   # short rows are valid here
    assert ragged(plan, p, ws_bytes=need - 1) == workspace


@pytest.mark.parametrize("hop", [300, 75, 1200])
def test_workspace_bytes_is_monotone_and_non_zero(lib, hop):
    plan = ctypes.cast(_host_plan(hop=hop), ctypes.c_void_p)
    size = lib.pe_mel_backward_workspace_bytes
    assert size(None, 2, 4801, 17) == 0
    assert size(plan, 0, 4801, 17) == size(plan, 2, 0, 17) == size(plan, 2, 4801, 0) == 0
    grid = [(b, n, t) for b in (1, 2, 7, 256) for n in (1, 513, 4801, 48000, 480000) for t in (1, 16, 17, 192, 2000)]
    sizes = {k: size(plan, *k) for k in grid}
    assert all(v > 0 for v in sizes.values())
    for (b, n, t), v in sizes.items():
        for (b2, n2, t2), v2 in sizes.items():
            if b2 >= b and n2 >= n and t2 >= t:
                assert v2 >= v, ((b, n, t), (b2, n2, t2))
    # one slab of (FB - 1) hop + 1024 floats per block of FB frames that a row of the batch can hold
    fb = max(4, -(-4800 // hop) + 3 & ~3)
    seg = ((fb - 1) * hop + 1024 + 3) & ~3
    assert size(plan, 256, 48000, 10 ** 6) == 256 * -(-(1 + 48000 // hop) // fb) * seg * 4
