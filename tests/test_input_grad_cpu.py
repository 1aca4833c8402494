"""d loss / d input of JDCNet: the functional oracle against the reference's golden, and the argument checks of the
first convolution's data-gradient entry point (no GPU needed).

tests/golden/input_grad_golden.npz holds the float64 input gradient of the reference model under torch autograd
(tests/golden/make_input_grad_golden.py).  The oracle must reproduce it to 1e-9 of its maximum, which pins
oracle/model_ref.py to the reference for this quantity; and on the T = 32 inputs the float32 oracle must stay within
1e-5 of the float64 one element by element: the network has max-pools and LeakyReLU kinks, a rounding-level change of
a near-tie moves a whole gradient path, and the GPU tests want inputs on which none moves.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import model_ref
from pitchextractor_amd import _lib, build
from tests.golden.make_golden import SEQ_CFG, TF_CFG, golden_input, golden_targets

SEED = 3
ENTRIES = [("bilstm", 32, "eval"), ("bilstm", 32, "train"), ("bilstm", 192, "eval"), ("tf", 32, "eval"),
           ("tf", 32, "train")]


def head_config(head):
    if head == "tf":
        return model_ref.seeded_state(11, num_class=1, model_type="transformer"), dict(TF_CFG)
    return model_ref.seeded_state(11, num_class=1, hidden_size=384), dict(SEQ_CFG, hidden_size=384)


@functools.lru_cache(maxsize=None)
def oracle_dx(head, T, mode, dtype):
    """Input gradient of the oracle's loss in ``dtype`` arithmetic, as a float64 array."""
    torch.set_num_threads(8)
    state, cfg = head_config(head)
    st = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in state.items()}
    x = golden_input(SEED, T=T).to(dtype).requires_grad_(True)
    f0, sil = (t.to(dtype) for t in golden_targets(SEED, T=T))
    cls, det = model_ref.jdcnet_forward(st, x, cfg, train=(mode == "train"))
    loss, _, _ = model_ref.jdc_loss(cls, det, f0, sil, 0.1)
    loss.backward()
    return x.grad.double().numpy()


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(golden_dir / "input_grad_golden.npz")


@pytest.mark.parametrize("head,T,mode", ENTRIES)
def test_float64_oracle_matches_reference_golden(G, head, T, mode):
    ref = G[f"{head}_T{T}_{mode}_dx"]
    assert ref.dtype == np.float64 and ref.shape == (2, 1, T, 80)
    got = oracle_dx(head, T, mode, torch.float64)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{head} T={T} {mode}: max |oracle64 - golden| / max|golden| = {err:.3e}")
    assert err <= 1e-9


@pytest.mark.parametrize("head,T,mode", [e for e in ENTRIES if e[1] == 32])
def test_float32_oracle_moves_no_gradient_path(head, T, mode):
    ref = oracle_dx(head, T, mode, torch.float64)
    got = oracle_dx(head, T, mode, torch.float32)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{head} T={T} {mode}: max |oracle32 - oracle64| / max|dx| = {err:.3e}")
    assert err <= 1e-5


def test_c1_dgrad_checks_its_arguments_before_any_device_call():
    """Null operands and bad sizes are refused on the host with the codes of pe_conv3x3_c1_fwd: PE_E_ARG (-1) for a
    null pointer or a non-positive size, PE_E_UNSUPPORTED (-2) for F % 4 != 0 or a pixel count the 32-bit indices
    cannot address."""
    build.build_library(verbose=False)
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)          # host memory: every call below returns before a launch
    for act16 in (0, 1, 2):
        assert lib.pe_conv3x3_c1_dgrad(act16, None, None, None, 1, 4, 8, None) == -1
        assert lib.pe_conv3x3_c1_dgrad(act16, None, p, p, 1, 4, 8, None) == -1
        assert lib.pe_conv3x3_c1_dgrad(act16, p, None, p, 1, 4, 8, None) == -1
        assert lib.pe_conv3x3_c1_dgrad(act16, p, p, None, 1, 4, 8, None) == -1
        assert lib.pe_conv3x3_c1_dgrad(act16, p, p, p, 0, 4, 8, None) == -1
        assert lib.pe_conv3x3_c1_dgrad(act16, p, p, p, 1, 0, 8, None) == -1
        assert lib.pe_conv3x3_c1_dgrad(act16, p, p, p, 1, 4, 6, None) == -2
        assert lib.pe_conv3x3_c1_dgrad(act16, p, p, p, 1 << 15, 1 << 10, 80, None) == -2     # 2.7e9 pixels
