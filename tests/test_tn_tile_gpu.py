"""The 192-wide tiles of the TN split-K engine (csrc/splitk.h): pe_gemm_tn and pe_lstm_whh_grad run the k-splits of the
128 x 128 plan on whatever tile they pick, so every result must have the same BYTES on every tiling.  The tile
override PE_TN_TILE is read once per process: the cases run here with each entry point's own choice and again in two
child processes, one kept on the 128-wide tiling (PE_TN_TILE=128) and one put on 192 x 192 wherever the form has it
(PE_TN_TILE=192), which hand their bytes back.  One case per form is also held against a float64 model at the
tolerances of tests/test_split_products_gpu.py / tests/test_half_operands_gpu.py, so that "identical" cannot mean
"identically wrong"."""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
from pitchextractor_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ("h2", "x3", "bf16")
# (M, N, K): one 192 x 192 tile, two splits; 2 x 3 tiles, ragged last k-tile (K % 32 != 0); M, N = 0 mod 4 but no
# multiples of 64 (edge quads fall outside the buffer descriptor); the training tiling of dW_ih at a short K; a shape
# of the 128 x 64 tile, which has no wide form; one split (stored to the destination directly)
SHAPES = [(192, 192, 2048), (384, 576, 1100), (200, 196, 1536), (1536, 768, 1024), (128, 64, 4096), (192, 192, 320)]
ACC_SHAPE, VIEW_SHAPES, REF_SHAPE = (384, 576, 1100), ((384, 576, 1100), (192, 192, 320)), (384, 576, 1100)
WHH = (384, 2, 40)                                   # H, B, T
SENTINEL = -7.25
GUARD = 8                                            # guard columns on either side of an ldc > N destination


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def operands(M, N, K):
    return rnd(K, M, seed=M + K, scale=1e-3), rnd(K, N, seed=N + 2 * K)


class product_mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = ops.FP32_MATMUL
        ops.FP32_MATMUL = self.mode if self.mode in ("h2", "x3") else "x3"
        self.cm = ops.matmul_bf16(self.mode == "bf16", "bf16")
        self.cm.__enter__()

    def __exit__(self, *exc):
        self.cm.__exit__(*exc)
        ops.FP32_MATMUL = self.prev
        return False


def run_all(dev):
    out = {}
    for mode in MODES:
        with product_mode(mode):
            for shape in SHAPES:
                M, N, K = shape
                A, B = (t.to(dev) for t in operands(M, N, K))
                out[("tn", mode, shape)] = ops.gemm_tn(A, B)
                if shape == ACC_SHAPE:
                    old = rnd(M, N, seed=5, scale=1e-2).to(dev)
                    out[("tn_acc", mode, shape)] = ops.gemm_tn(A, B, out=old, accumulate=True)
                if shape in VIEW_SHAPES:
                    # an aligned view (16-byte pieces) and one two floats off (scalar stores), guard columns around both
                    for name, off in (("tn_view", GUARD), ("tn_view_odd", GUARD + 2)):
                        buf = torch.full((M, N + 2 * GUARD + 4), SENTINEL, device=dev)
                        ops.gemm_tn(A, B, out=buf[:, off:off + N])
                        out[(name, mode, shape)] = buf
            H, Bn, T = WHH
            dg = rnd(Bn, T, 4 * H, seed=7, scale=1e-2).to(dev)
            ybuf = torch.tanh(rnd(Bn, T, 2 * H, seed=8)).to(dev)
            amax = (ops.absmax(dg), ops._unit_amax(dev)) if mode == "h2" else (None, None)
            for reverse in (0, 1):
                y = ybuf[:, :, reverse * H:(reverse + 1) * H]
                ysh = torch.zeros(Bn, T, H, device=dev)
                if reverse:
                    ysh[:, :-1] = y[:, 1:]
                else:
                    ysh[:, 1:] = y[:, :-1]
                out[("whh", mode, reverse)] = ops.lstm_whh_grad(
                    ops.Scaled(dg, amax[0]), ops.Scaled(y, amax[1]),
                    torch.full((4 * H, H), float("nan"), device=dev), reverse, Bn, T, H)
                out[("whh_as_tn", mode, reverse)] = ops.gemm_tn(ops.Scaled(dg.view(Bn * T, 4 * H), amax[0]),
                                                                ops.Scaled(ysh.view(Bn * T, H), amax[1]))
    return {k: v.cpu() for k, v in out.items()}


@pytest.fixture(scope="module")
def results(hip_device):
    assert "PE_TN_TILE" not in os.environ, "run the suite without PE_TN_TILE: the children set it"
    return run_all(hip_device)


def child(tmp_path_factory, tile):
    """every case again in a child process with PE_TN_TILE=tile (the override is read once per process)"""
    path = tmp_path_factory.mktemp("tn_tile") / f"tile_{tile}.pt"
    subprocess.run([sys.executable, str(Path(__file__).resolve()), str(path)], check=True, cwd=str(ROOT), timeout=120,
                   env=dict(os.environ, PE_TN_TILE=tile))
    return torch.load(path, weights_only=False)


@pytest.fixture(scope="module")
def results_128(hip_device, tmp_path_factory):
    return child(tmp_path_factory, "128")


@pytest.fixture(scope="module")
def results_192(hip_device, tmp_path_factory):
    return child(tmp_path_factory, "192")


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("mode", MODES)
def test_every_tiling_gives_the_same_bytes(results, results_128, results_192, mode):
    keys = [k for k in results if k[1] == mode]
    assert len(keys) == len(SHAPES) + 1 + 2 * len(VIEW_SHAPES) + 4
    assert set(results) == set(results_128) == set(results_192)
    for k in keys:
        assert same_bytes(results[k], results_128[k]), (k, "own choice against the 128-wide tiling")
        assert same_bytes(results_192[k], results_128[k]), (k, "192 x 192 against the 128-wide tiling")
        assert torch.isfinite(results[k]).all() and results[k].abs().max() > 0


@pytest.mark.parametrize("which", ["own", "128", "192"])
@pytest.mark.parametrize("mode", MODES)
def test_views_keep_their_guard_columns(results, results_128, results_192, mode, which):
    res = {"own": results, "128": results_128, "192": results_192}[which]
    for shape in VIEW_SHAPES:
        N = shape[1]
        for name, off in (("tn_view", GUARD), ("tn_view_odd", GUARD + 2)):
            buf = res[(name, mode, shape)]
            assert (buf[:, :off] == SENTINEL).all() and (buf[:, off + N:] == SENTINEL).all()
            assert same_bytes(buf[:, off:off + N].contiguous(), res[("tn", mode, shape)])


@pytest.mark.parametrize("which", ["own", "128", "192"])
@pytest.mark.parametrize("mode", MODES)
def test_accumulate_is_one_exact_add(results, results_128, results_192, mode, which):
    res = {"own": results, "128": results_128, "192": results_192}[which]
    M, N, _ = ACC_SHAPE
    old = rnd(M, N, seed=5, scale=1e-2)
    assert same_bytes(res[("tn_acc", mode, ACC_SHAPE)], res[("tn", mode, ACC_SHAPE)] + old)


@pytest.mark.parametrize("which", ["own", "128", "192"])
@pytest.mark.parametrize("mode", MODES)
def test_whh_grad_equals_gemm_tn_of_shifted_y(results, results_128, results_192, mode, which):
    res = {"own": results, "128": results_128, "192": results_192}[which]
    for reverse in (0, 1):
        assert same_bytes(res[("whh", mode, reverse)], res[("whh_as_tn", mode, reverse)])


@pytest.mark.parametrize("mode", MODES)
def test_against_float64(results_192, mode):
    """the 192 x 192 bytes (= all of them, above) against the float64 model of the form"""
    M, N, K = REF_SHAPE
    A, B = operands(M, N, K)
    got = results_192[("tn", mode, REF_SHAPE)]
    if mode == "bf16":
        from tests import half_ref as R
        from tests.test_half_operands_gpu import close, misses
        close(got, R.hr(A, "bf16").T @ R.hr(B, "bf16"))
        assert misses(got, A.double().T @ B.double())
    else:
        from tests import split_ref as S
        from tests.test_split_products_gpu import ACC_EXTRA, acc_tol, check, model
        check(got, model(mode, S.op_tn, A, B), acc_tol(K, mode, extra=ACC_EXTRA + 64))


if __name__ == "__main__":
    torch.save(run_all(torch.device("cuda:0")), sys.argv[1])
