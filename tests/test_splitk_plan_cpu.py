"""The split-K plans of the weight-gradient products, seen through the only place they show outside the library: the
three workspace queries.  The byte counts below were read from the library as it stood before the plans moved into
csrc/splitk.h; the queries must return them unchanged, and tests/plan_ref.py -- the restatement the GPU tests use to
know a shape's tile and splits -- must explain every one of them (largest split count over the product forms times
one fp32 slab).  No device is needed: the queries are host arithmetic."""
import pytest

from pitchextractor_amd import _lib, build
from tests import plan_ref as P
from tests import test_ops_gpu
from tests.test_half_operands_gpu import TN_SHAPES
from tests.test_wgrad9_borders_gpu import BORDER_SHAPES

# (K, M, N): pe_gemm_tn_workspace_bytes(M, N, K) -- TN_SHAPES of tests/test_half_operands_gpu.py
TN_WS = {
    (5000, 64, 64): 147456,
    (3001, 192, 128): 491520,
    (777, 1536, 96): 0,
    (20000, 128, 64): 1212416,
    (64, 4, 8): 0,
    (600, 48, 132): 0,
    (2000, 32, 200): 76800,
    (900, 200, 40): 0,
    (3001, 260, 36): 187200,
    (333, 136, 260): 0,
}
# (B, T, H): pe_lstm_whh_grad_workspace_bytes(B, T, H) -- B T = 35, 1000, 49152
WHH_WS = {
    (5, 7, 32): 16384,
    (8, 125, 32): 16384,
    (64, 768, 32): 1572864,
    (5, 7, 64): 65536,
    (8, 125, 64): 65536,
    (64, 768, 64): 6291456,
    (5, 7, 96): 147456,
    (8, 125, 96): 147456,
    (64, 768, 96): 14155776,
    (5, 7, 128): 262144,
    (8, 125, 128): 262144,
    (64, 768, 128): 25165824,
    (5, 7, 384): 2359296,
    (8, 125, 384): 2359296,
    (64, 768, 384): 165150720,
}
# (B, T, F, Cin, Cout): pe_conv3x3_wgrad_workspace_bytes -- test_conv3x3_fwd_dgrad_wgrad, BORDER_SHAPES, Cin == 1
CONV_WS = {
    (2, 12, 10, 64, 64): 147456,
    (1, 9, 7, 64, 128): 294912,
    (2, 5, 20, 128, 192): 884736,
    (1, 6, 10, 192, 256): 1769472,
    (1, 4, 5, 256, 256): 2359296,
    (3, 16, 40, 128, 128): 589824,
    (1, 3, 80, 64, 64): 147456,
    (1, 5, 45, 64, 128): 294912,
    (1, 4, 50, 64, 128): 294912,
    (2, 1, 33, 96, 160): 552960,
    (2, 64, 40, 64, 64): 737280,
    (2, 48, 40, 128, 128): 1769472,
    (41, 5, 10, 64, 64): 294912,
    (103, 1, 20, 64, 128): 589824,
    (37, 3, 20, 128, 64): 589824,
    (70, 3, 10, 64, 192): 884736,
    (27, 2, 40, 64, 64): 294912,
    (2, 12, 10, 1, 64): 4718592,
    (3, 16, 40, 1, 64): 4718592,
}


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _lib.load()


def test_tables_cover_the_shape_lists_of_the_gpu_tests():
    assert set(TN_SHAPES) <= set(TN_WS)
    conv = [m.args[1] for m in test_ops_gpu.test_conv3x3_fwd_dgrad_wgrad.pytestmark if m.args[0].startswith("B,")]
    assert len(conv) == 1 and set(conv[0]) | set(BORDER_SHAPES) <= set(CONV_WS)
    assert any(Ci == 1 for _, _, _, Ci, _ in CONV_WS)
    assert {(B * T, H) for B, T, H in WHH_WS} == {(bt, H) for bt in (35, 1000, 49152) for H in (32, 64, 96, 128, 384)}


def test_gemm_tn_workspace_bytes(lib):
    for (K, M, N), want in TN_WS.items():
        assert lib.pe_gemm_tn_workspace_bytes(M, N, K) == want, (K, M, N)
        s = max(P.tn_tile_and_splits(M, N, K, multi)[1] for multi in (False, True))
        assert want == (s * M * N * 4 if s > 1 else 0), (K, M, N, s)     # one split stores to C: no slab


def test_lstm_whh_grad_workspace_bytes(lib):
    for (B, T, H), want in WHH_WS.items():
        assert lib.pe_lstm_whh_grad_workspace_bytes(B, T, H) == want, (B, T, H)
        assert want == max(P.whh_splits(B, T, H, multi) for multi in (False, True)) * 4 * H * H * 4, (B, T, H)


def test_conv3x3_wgrad_workspace_bytes(lib):
    for (B, T, F, Ci, Co), want in CONV_WS.items():
        assert lib.pe_conv3x3_wgrad_workspace_bytes(B, T, F, Ci, Co) == want, (B, T, F, Ci, Co)
        if Ci != 1:                                                    # (Cin == 1: the first layer's own kernel)
            assert want == P.wgrad_tile_and_splits(B * T * F, Co, Ci)[1] * 9 * Co * Ci * 4, (B, T, F, Ci, Co)
