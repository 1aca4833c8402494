"""The C-ABI library loads and exports every symbol include/*.h declares (no GPU needed)."""
import re
from pathlib import Path

import pytest

from pitchextractor_amd import _lib, build

ROOT = Path(__file__).resolve().parent.parent


def header_functions():
    text = (ROOT / "include" / "pitchextractor_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pe_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _lib.load()


def test_header_and_bindings_agree():
    assert header_functions() == sorted(_lib.PROTOTYPES)


def test_every_declared_symbol_is_exported(lib):
    for name in header_functions():
        assert hasattr(lib, name), name


def test_abi_version(lib):
    assert lib.pe_abi_version() >= 1


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", tmp_path / "nope.so")
    with pytest.raises(_lib.HipLibraryError):
        _lib.load()


def test_product_forms_agree_with_the_header():
    text = (ROOT / "include" / "pitchextractor_hip.h").read_text()
    enum = dict(re.findall(r"\b(PE_PROD_[A-Z0-9]+)\s*=\s*(\d+)", text))
    assert enum and {k: int(v) for k, v in enum.items()} == {k: getattr(_lib, k) for k in enum}


def test_argument_and_form_checks_run_before_any_device_call(lib):
    """The entry points validate their arguments on the host (no GPU in this test): a leading dimension the 32-bit
    buffer offsets of the operand loaders cannot address, a 3x3 convolution whose tensor passes 2 GiB, a missing
    operand-scale word, and a product form / activation type that no kernel of the entry point serves or that is not a
    form at all are refused with the documented codes instead of being launched."""
    import ctypes
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    word = ctypes.cast((ctypes.c_uint * 1)(), ctypes.c_void_p)
    unsupported, bad_arg = -2, -1
    codes = {c: getattr(_lib, c) for c in ("PE_E_UNSUPPORTED", "PE_E_ARG") if hasattr(_lib, c)}
    unsupported, bad_arg = codes.get("PE_E_UNSUPPORTED", unsupported), codes.get("PE_E_ARG", bad_arg)
    h2 = _lib.PE_PROD_H2
    # NT: lda = 2^21 floats; TN: ldb = 2^24
    assert lib.pe_gemm_nt(h2, 0, p, 1 << 21, p, 64, p, 64, 128, 64, 64, None, None, 0, word, word, None) == unsupported
    assert lib.pe_gemm_tn(h2, 0, p, 64, p, 1 << 24, p, 64, 64, 64, 64, 0, None, 0, word, word, None) == unsupported
    # h2 without the scale words
    assert lib.pe_gemm_nt(h2, 0, p, 64, p, 64, p, 64, 128, 64, 64, None, None, 0, None, None, None) == bad_arg
    # staged-window convolution: 2^31 bytes of input
    assert lib.pe_conv3x3_fwd_wf(h2, 0, p, p, p, 4096, 192, 80, 64, 64, 0, None, word, word, None) == unsupported
    # bf16 activation tensors with any form but bf16
    assert lib.pe_gemm_nt(h2, 1, p, 64, p, 64, p, 64, 128, 64, 64, None, None, 0, word, word, None) == unsupported
    # there is no native-fp32 persistent recurrence
    cells = (ctypes.c_void_p * 1)(p)
    rev = (ctypes.c_int * 1)(0)
    assert lib.pe_lstm_fwd_persistent(_lib.PE_PROD_NATIVE, 1, cells, cells, cells, cells, rev, 384, 64, 8, 384, p,
                                      None) == unsupported
    # not a product form
    assert lib.pe_gemm_nt(5, 0, p, 64, p, 64, p, 64, 128, 64, 64, None, None, 0, word, word, None) == bad_arg


# Status of each form-taking entry point called with null operands and positive sizes, for products = -1, 0 .. 4, 5:
# null operands return before any device call, so a served form answers its impl's null check (PE_E_ARG, -1), a valid
# form that no kernel of the entry point serves PE_E_UNSUPPORTED (-2), a value outside the enum PE_E_ARG.  Second row:
# the same with act16 = 1, which exists under PE_PROD_BF16 only.
_ALL = [-1, -1, -1, -1, -1, -1, -1]
_ACT16 = [-1, -2, -2, -2, -1, -2, -1]
_TERMS = [-1, -2, -1, -1, -1, -1, -1]              # no native-fp32 fragment form
_PERSISTENT = [-1, -2, -1, -2, -1, -1, -1]         # x3, bf16, f16
_ATTN = [-1, -1, -2, -2, -1, -2, -1]               # native, bf16
# name -> (arguments after `products` [and `act16`], expected with act16 = 0 / absent, expected with act16 = 1 or None)
_SERVED_FORMS = {
    "pe_gemm_nt": ((None, 64, None, 64, None, 64, 128, 64, 64, None, None, 0, None, None, None), _ALL, _ACT16),
    "pe_gemm_tn": ((None, 64, None, 64, None, 64, 64, 64, 64, 0, None, 0, None, None, None), _ALL, _ACT16),
    "pe_conv3x3_fwd": ((None, None, None, 1, 4, 8, 32, 32, 0, None, None, None), _ALL, _ACT16),
    "pe_conv3x3_wgrad": ((None, None, None, 1, 4, 8, 32, 32, None, 0, None, None, None), _ALL, _ACT16),
    "pe_conv3x3_fwd_wf": ((None, None, None, 1, 4, 8, 32, 32, 0, None, None, None, None), _TERMS, _ACT16),
    "pe_wfrag_pack": ((None, 32, 32, 32, None, None, None), _TERMS, None),
    "pe_lstm_whh_grad": ((None, None, 384, None, 1, 4, 384, 0, None, 0, None, None, None), _ALL, None),
    "pe_lstm_fwd_persistent": ((1, None, None, None, None, None, 384, 1, 4, 384, None, None), _PERSISTENT, None),
    "pe_lstm_bwd_persistent": ((1, None, None, None, None, None, 384, 1, 4, 384, None, None, None, None),
                               _PERSISTENT, None),
    "pe_attn_fwd": ((None, 192, None, 64, None, None, None, 1, 192, 1, 64, 0.125, 0.0, 0, 0, None), _ATTN, None),
    "pe_attn_bwd": ((None, 192, None, None, 64, None, None, None, 1, 192, 1, 64, 0.125, 0.0, None), _ATTN, None),
}


@pytest.mark.parametrize("name", sorted(_SERVED_FORMS))
def test_served_forms_of_every_entry_point(lib, name):
    args, plain, act16 = _SERVED_FORMS[name]
    fn = getattr(lib, name)
    forms = range(-1, 6)
    if act16 is None:
        assert [fn(f, *args) for f in forms] == plain
    else:
        assert [fn(f, 0, *args) for f in forms] == plain
        assert [fn(f, 1, *args) for f in forms] == act16


def test_fragment_bytes_of_every_form(lib):
    assert [lib.pe_wfrag_bytes(f, 32, 32) for f in range(-1, 6)] == [0, 0, 6144, 4096, 2048, 2048, 0]
