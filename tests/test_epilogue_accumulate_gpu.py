"""Epilogues of the halo convolution and the transposed NT GEMM: the buffer-addressed form (old values of an
accumulate launch requested a block ahead, tile overhang dropped by the descriptor's range check) against exact
models, and against the pointer-addressed form of the same build (PE_EPILOGUE=pointer, read once per process: a
child process runs every case again and hands its bytes back).

Everything is compared with torch.equal: an fp32 ``v + old`` rounds once, and the order of the float64 column sums
is fixed, so no check here has a tolerance -- except the comparison with the implicit-GEMM kernel, which
sums the k blocks in another order (the bound of tests/test_ops_gpu.py)."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
from pitchextractor_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

# (B, T, F, Cin, Cout): one partial 128-pixel tile; the 192-wide variant over two pixel tiles; the 64-wide variant
# over five; Cout below the tile width (column bound); two column tiles
CONV_SHAPES = [(1, 3, 40, 32, 128), (2, 5, 20, 64, 192), (1, 7, 80, 32, 64), (1, 3, 40, 32, 96), (2, 3, 40, 64, 256)]
CONV_CASES = [(s, m) for s in CONV_SHAPES for m in ("h2", "x3", "bf16", "f16")] + [(CONV_SHAPES[1], "bf16_a16")]
# (M, N, K): the 128x192, 128x128 (N % 4 == 0, N % 32 != 0), 256x64 and 128x32 tiles
GEMM_SHAPES = [(200, 192, 64), (130, 100, 32), (300, 64, 32), (70, 20, 32)]
GEMM_CASES = [(s, m, b) for s in GEMM_SHAPES for m in ("h2", "x3", "bf16") for b in (False, True)]
SENTINEL = -7.25


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


class product_mode:
    """ops state of one of the test's modes: h2 / x3 fp32 products, bf16 / f16 mixed precision."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = ops.FP32_MATMUL
        ops.FP32_MATMUL = self.mode if self.mode in ("h2", "x3") else "x3"
        half = self.mode in ("bf16", "f16", "bf16_a16")
        self.cm = ops.matmul_bf16(half, "f16" if self.mode == "f16" else "bf16", act16=self.mode == "bf16_a16")
        self.cm.__enter__()

    def __exit__(self, *exc):
        self.cm.__exit__(*exc)
        ops.FP32_MATMUL = self.prev


def conv_inputs(shape, mode, dev):
    B, T, Fq, Ci, Co = shape
    x = rnd(B, T, Fq, Ci, seed=1)
    old = rnd(B, T, Fq, Co, seed=3)
    if mode == "bf16_a16":
        x, old = x.to(torch.bfloat16), old.to(torch.bfloat16)
    return x.to(dev), rnd(Co, Ci, 3, 3, seed=2, scale=0.1).to(dev), old.to(dev)


def run_conv(shape, mode, dev):
    """plain / accumulated outputs of the fragment-fed kernel with their BatchNorm partials, and the same two outputs
    without partials (the launches that must not differ for leaving the statistics out)."""
    x, w, old = conv_inputs(shape, mode, dev)
    with product_mode(mode):
        wf, _ = ops.conv3x3_repack(w, True, False)
        assert wf.frag is not None
        y, parts = ops.conv3x3_fwd(x, wf, bn_stats=True)
        ya, parts_a = ops.conv3x3_fwd(x, wf, out=old.clone(), accumulate=True, bn_stats=True)
        assert parts is not None and parts_a is not None
        y_ns = ops.conv3x3_fwd(x, wf)
        ya_ns = ops.conv3x3_fwd(x, wf, out=old.clone(), accumulate=True)
    return {"y": y, "parts": parts, "ya": ya, "parts_a": parts_a, "y_ns": y_ns, "ya_ns": ya_ns}


def gemm_inputs(shape, bias, dev):
    M, N, K = shape
    b0, b1 = (rnd(N, seed=14).to(dev), rnd(N, seed=15).to(dev)) if bias else (None, None)
    return rnd(M, K, seed=11).to(dev), rnd(N, K, seed=12, scale=0.2).to(dev), rnd(M, N, seed=13).to(dev), b0, b1


def run_gemm(shape, mode, bias, dev):
    a, b, old, b0, b1 = gemm_inputs(shape, bias, dev)
    with product_mode(mode):
        c = ops.gemm_nt(a, b, bias0=b0, bias1=b1)
        ca = ops.gemm_nt(a, b, bias0=b0, bias1=b1, out=old.clone(), accumulate=True)
    return {"c": c, "ca": ca}


def run_gemm_view(dev):
    """accumulate into an ldc = N + 8 column view of a sentinel-filled buffer with three rows behind M"""
    (M, N, K), mode = GEMM_SHAPES[0], "h2"
    a, b, old, _, _ = gemm_inputs(GEMM_SHAPES[0], False, dev)
    buf = torch.full((M + 3, N + 8), SENTINEL, device=dev)
    buf[:M, :N] = old
    with product_mode(mode):
        ops.gemm_nt(a, b, out=buf[:M, :N], accumulate=True)
    return {"buf": buf}


def run_all(dev):
    out = {}
    for shape, mode in CONV_CASES:
        out[("conv", shape, mode)] = run_conv(shape, mode, dev)
    for shape, mode, bias in GEMM_CASES:
        out[("gemm", shape, mode, bias)] = run_gemm(shape, mode, bias, dev)
    out[("gemm_view",)] = run_gemm_view(dev)
    return {k: {n: t.cpu() for n, t in v.items()} for k, v in out.items()}


@pytest.fixture(scope="module")
def results(hip_device):
    assert os.environ.get("PE_EPILOGUE") != "pointer", "run the suite without PE_EPILOGUE: the child sets it"
    return run_all(hip_device)


@pytest.fixture(scope="module")
def pointer_results(hip_device, tmp_path_factory):
    """every case again in a child process with PE_EPILOGUE=pointer (the switch is read once per process)"""
    path = tmp_path_factory.mktemp("epilogue") / "pointer.pt"
    env = dict(os.environ, PE_EPILOGUE="pointer")
    subprocess.run([sys.executable, str(Path(__file__).resolve()), str(path)], check=True, env=env, cwd=str(ROOT),
                   timeout=120)
    return torch.load(path, weights_only=False)


def ids(case):
    return "-".join("x".join(map(str, c)) if isinstance(c, tuple) else str(c) for c in case)


# ------------------------------------------------------------------ convolution
@pytest.mark.parametrize("case", CONV_CASES, ids=ids)
def test_conv_accumulate_is_one_exact_add(results, hip_device, case):
    """accumulate=True onto a random `out` == out_before + the same launch without accumulate, bit for bit.  With
    bf16 activation storage the kernel adds in fp32 and rounds once, so the model is
    bf16(conv in fp32 storage + widened old) with the same bf16 products (operands already bf16 values)."""
    shape, mode = case
    r = results[("conv",) + case]
    _, _, old = conv_inputs(shape, mode, "cpu")
    if mode == "bf16_a16":
        x, w, _ = conv_inputs(shape, mode, hip_device)
        with product_mode("bf16"):
            wf, _ = ops.conv3x3_repack(w, True, False)
            y32 = ops.conv3x3_fwd(x.float(), wf).cpu()
        assert torch.equal(r["y"], y32.to(torch.bfloat16))
        want = torch.add(y32, old.float()).to(torch.bfloat16)
    else:
        want = torch.add(old, r["y"])
    assert torch.equal(r["ya"], want)
    assert torch.equal(r["ya_ns"], r["ya"]) and torch.equal(r["y_ns"], r["y"])


def partials_model(y):
    """[tiles, 2, N] float64: per 128-pixel tile and column, sum and sum of squares of the STORED outputs in the
    kernel's order: a lane (wave row wm, lane half h) adds its rows 64 wm + 4 h + 32 i + (g & 3) + 8 (g >> 2) for
    i = 0, 1 and g = 0 .. 15 in that order; then half 0 + half 1; then wm 0 + wm 1.  v * v is exact in double."""
    v = y.reshape(-1, y.shape[-1]).double().numpy()
    P, N = v.shape
    tiles = (P + 127) // 128
    pad = np.zeros((tiles * 128, N))
    pad[:P] = v
    pad = pad.reshape(tiles, 128, N)
    s1 = np.zeros((tiles, 2, 2, N))
    s2 = np.zeros((tiles, 2, 2, N))
    for wm in range(2):
        for h in range(2):
            for i in range(2):
                for g in range(16):
                    e = pad[:, 64 * wm + 4 * h + 32 * i + (g & 3) + 8 * (g >> 2)]
                    s1[:, wm, h] = s1[:, wm, h] + e
                    s2[:, wm, h] = s2[:, wm, h] + e * e
    s1 = s1[:, :, 0] + s1[:, :, 1]
    s2 = s2[:, :, 0] + s2[:, :, 1]
    return np.stack([s1[:, 0] + s1[:, 1], s2[:, 0] + s2[:, 1]], axis=1)


@pytest.mark.parametrize("case", CONV_CASES, ids=ids)
def test_conv_partials_equal_the_float64_model(results, case):
    r = results[("conv",) + case]
    for y, parts in ((r["y"], r["parts"]), (r["ya"], r["parts_a"])):
        want = partials_model(y)
        assert parts.shape == want.shape
        assert np.array_equal(parts.numpy(), want)


@pytest.mark.parametrize("case", CONV_CASES, ids=ids)
def test_conv_pointer_form_gives_identical_bytes(results, pointer_results, case):
    a, b = results[("conv",) + case], pointer_results[("conv",) + case]
    for name in a:
        assert torch.equal(a[name], b[name]), name


# (not with bf16 activation storage: both kernels serve it, but the outputs are then rounded to 8 bits, and the
# different order of the k blocks, an fp32-level difference, can flip such a rounding: 2^-8 against a bound of 2e-6.
# The bf16 case with fp32 storage runs the same products; the storage form is covered exactly by the other checks.)
@pytest.mark.parametrize("case", [c for c in CONV_CASES if c[1] != "bf16_a16"], ids=ids)
def test_conv_fragment_fed_matches_implicit_gemm(results, hip_device, case, monkeypatch):
    """as tests/test_ops_gpu.py asserts at its shapes: same operand terms, another order of the k blocks"""
    shape, mode = case
    x, w, _ = conv_inputs(shape, mode, hip_device)
    monkeypatch.setattr(ops, "CONV_WFRAG", False)
    with product_mode(mode):
        wf, _ = ops.conv3x3_repack(w, True, False)
        assert wf.frag is None
        ref = ops.conv3x3_fwd(x, wf).cpu()
    got = results[("conv",) + case]["y"]
    assert (got - ref).abs().max().item() <= 2e-6 * ref.abs().max().item()


# ------------------------------------------------------------------ GEMM NT
@pytest.mark.parametrize("case", GEMM_CASES, ids=ids)
def test_gemm_nt_accumulate_is_one_exact_add(results, case):
    """((acc + bias0) + bias1) + old: the accumulated result == old + the result without accumulate, bit for bit"""
    shape, mode, bias = case
    r = results[("gemm",) + case]
    _, _, old, _, _ = gemm_inputs(shape, bias, "cpu")
    assert torch.equal(r["ca"], torch.add(old, r["c"]))


def test_gemm_nt_column_view_keeps_its_guard(results):
    """ldc = N + 8: the 8 guard columns of every row and the rows behind M keep the sentinel"""
    M, N, _ = GEMM_SHAPES[0]
    buf = results[("gemm_view",)]["buf"]
    _, _, old, _, _ = gemm_inputs(GEMM_SHAPES[0], False, "cpu")
    assert torch.equal(buf[:M, :N], torch.add(old, results[("gemm", GEMM_SHAPES[0], "h2", False)]["c"]))
    assert torch.equal(buf[:, N:], torch.full((M + 3, 8), SENTINEL))
    assert torch.equal(buf[M:], torch.full((3, N + 8), SENTINEL))


@pytest.mark.parametrize("case", GEMM_CASES + [("view",)], ids=ids)
def test_gemm_nt_pointer_form_gives_identical_bytes(results, pointer_results, case):
    key = ("gemm_view",) if case == ("view",) else ("gemm",) + case
    for name in results[key]:
        assert torch.equal(results[key][name], pointer_results[key][name]), name


if __name__ == "__main__":
    torch.save(run_all(torch.device("cuda:0")), sys.argv[1])
