"""The single-term 16-bit operand kernels (mixed precision, ``ops.matmul_bf16(True, half)``: operands rounded to
bf16 or fp16, fp32 accumulation) against float64 computed on operands rounded exactly as the kernel rounds them
(tests/half_ref.py), at the shapes that select every tile and kernel instance, for both operand types.

Every check also shows that it can tell a wrong rounding model apart where that is cheap: the same reference with
unrounded operands, or with the other half type, misses the GPU result by more than the tolerance.
"""
import pytest
import torch
import torch.nn.functional as F

from pitchextractor_amd import _lib, ops
from tests import half_ref as R
from tests.plan_ref import tn_tile_and_splits
from tests.test_ops_gpu import close, nchw, nhwc, rnd

pytestmark = pytest.mark.gpu

HALVES = ("bf16", "f16")
OTHER = {"bf16": "f16", "f16": "bf16"}


def err_scale(got, ref):
    got = got.detach().cpu().double()
    return (got - ref).abs().max().item(), ref.abs().max().item() + 1e-30


def misses(got, ref, tol=1e-5):
    """the reference `ref` does NOT reproduce `got` within close()'s bound"""
    e, s = err_scale(got, ref)
    return e > tol * s


# ------------------------------------------------------------------ GEMM NT
# gemm_nt_impl (csrc/gemm.hip) picks the tile from N: N <= 32 -> 128x32, N <= 64 -> 256x64, N % 192 == 0 -> 128x192
# (16-bit modes), else 128x128; the transposed-store kernel runs when N % 4 == 0 (and C is aligned), else the scalar one.
NT_SHAPES = [
    (300, 1536, 384),    # 128x192
    (1000, 64, 576),     # 256x64
    (257, 192, 96),      # 128x192, M ragged
    (130, 20, 64),       # 128x32
    (64, 128, 32),       # 128x128
    (5, 360, 768),       # 128x128
    (1024, 256, 640),    # 128x128
    (33, 1, 4),          # 128x32, scalar-store kernel
    (77, 33, 100),       # 256x64, scalar-store kernel, K not a multiple of 32
    (70, 62, 20),        # 256x64, scalar-store kernel, K < 32
    (1000, 256, 384),    # 128x128
    (259, 360, 52),      # 128x128, M / K ragged
    (100, 190, 68),      # 128x128, scalar-store kernel
    (129, 768, 36),      # 128x192 (768 % 128 == 0 too: the 16-bit modes still take the 192 tile)
]


@pytest.mark.parametrize("M,N,K", NT_SHAPES)
@pytest.mark.parametrize("half", HALVES)
def test_gemm_nt_half(hip_device, M, N, K, half):
    A, B = rnd(M, K, seed=1), rnd(N, K, seed=2)
    b0, b1 = rnd(N, seed=3), rnd(N, seed=4)
    dev = hip_device
    ref = R.hr(A, half) @ R.hr(B, half).T
    with ops.matmul_bf16(True, half):
        got = ops.gemm_nt(A.to(dev), B.to(dev))
        got_b = ops.gemm_nt(A.to(dev), B.to(dev), bias0=b0.to(dev), bias1=b1.to(dev))
        out = rnd(M, N, seed=5).to(dev)
        acc_ref = ref + out.cpu().double()
        got_acc = ops.gemm_nt(A.to(dev), B.to(dev), out=out, accumulate=True)
    close(got, ref)
    close(got_b, ref + b0.double() + b1.double())
    close(got_acc, acc_ref)
    if K >= 32:       # (tiny K: too few products for the roundings to show reliably)
        assert misses(got, A.double() @ B.double().T) and misses(got, R.hr(A, OTHER[half]) @ R.hr(B, OTHER[half]).T)


@pytest.mark.parametrize("half", HALVES)
def test_gemm_nt_half_strided_rows(hip_device, half):
    big = rnd(300, 7, 96, seed=6).to(hip_device)             # rows taken at a fixed time step: ld = 7*96
    A = big[:, 3, 32:96]
    for N in (50, 256):                                      # 256x64 and 128x128 tiles
        B = rnd(N, 64, seed=7).to(hip_device)
        out = torch.zeros(300, N + 30, device=hip_device)
        with ops.matmul_bf16(True, half):
            ops.gemm_nt(A, B, out=out[:, 10:10 + N])
        close(out[:, 10:10 + N], R.hr(A, half) @ R.hr(B, half).T)
        assert (out[:, :10] == 0).all() and (out[:, 10 + N:] == 0).all()


# ------------------------------------------------------------------ GEMM TN
TN_SHAPES = [   # (K, M, N): tile, splits
    (5000, 64, 64),      # 64x64, split
    (3001, 192, 128),    # 128x128, split, K ragged
    (777, 1536, 96),     # 128x128, one split
    (20000, 128, 64),    # 128x64, split
    (64, 4, 8),          # 64x64, one split
    (600, 48, 132),      # 64x128, one split, N ragged
    (2000, 32, 200),     # 64x128, split
    (900, 200, 40),      # 128x64, one split
    (3001, 260, 36),     # 128x64, split, M ragged
    (333, 136, 260),     # 128x128, one split, M / N / K ragged
]
TN_EXPECT = {(5000, 64, 64): ((64, 64), True), (3001, 192, 128): ((128, 128), True), (777, 1536, 96): ((128, 128), False),
             (20000, 128, 64): ((128, 64), True), (64, 4, 8): ((64, 64), False), (600, 48, 132): ((64, 128), False),
             (2000, 32, 200): ((64, 128), True), (900, 200, 40): ((128, 64), False), (3001, 260, 36): ((128, 64), True),
             (333, 136, 260): ((128, 128), False)}


def test_tn_shape_list_covers_every_tile_and_both_split_forms():
    seen = set()
    for K, M, N in TN_SHAPES:
        tile, splits = tn_tile_and_splits(M, N, K)
        assert (tile, splits > 1) == TN_EXPECT[(K, M, N)], (K, M, N, tile, splits)
        seen.add((tile, splits > 1))
    assert {t for t, _ in seen} == {(64, 64), (64, 128), (128, 64), (128, 128)} and {s for _, s in seen} == {True, False}


@pytest.mark.parametrize("K,M,N", TN_SHAPES)
@pytest.mark.parametrize("half", HALVES)
def test_gemm_tn_half(hip_device, K, M, N, half):
    A, B = rnd(K, M, seed=1), rnd(K, N, seed=2)
    ref = R.hr(A, half).T @ R.hr(B, half)
    out = rnd(M, N, seed=3).to(hip_device)
    acc_ref = ref + out.cpu().double()
    with ops.matmul_bf16(True, half):
        got = ops.gemm_tn(A.to(hip_device), B.to(hip_device))
        got_acc = ops.gemm_tn(A.to(hip_device), B.to(hip_device), out=out, accumulate=True)
    close(got, ref)
    close(got_acc, acc_ref)
    assert misses(got, A.double().T @ B.double()) and misses(got, R.hr(A, OTHER[half]).T @ R.hr(B, OTHER[half]))


# ------------------------------------------------------------------ conv 3x3
def halo_kernel(F_, N):
    """which fragment-fed kernel conv3x3_fwd_wf_impl runs (csrc/conv.hip conv_halo_passes), None: implicit GEMM"""
    wr = 128 + 2 * F_ + 2
    if wr <= 7 * 32 and N >= 96:
        return "7-pass/192" if (N % 192 == 0 and N % 128 != 0) else "7-pass/128"
    if wr <= 10 * 32 and N <= 64:
        return "10-pass"
    return None


CONV_SHAPES = [(2, 12, 10, 64, 64), (1, 9, 7, 64, 128), (2, 5, 20, 128, 192), (1, 6, 10, 192, 256), (1, 4, 5, 256, 256),
               (3, 16, 40, 128, 128), (1, 3, 80, 64, 64), (1, 5, 45, 64, 128), (1, 4, 50, 64, 128), (2, 1, 33, 96, 160),
               (2, 64, 40, 64, 64), (2, 48, 40, 128, 128)]        # as test_ops_gpu.test_conv3x3_fwd_dgrad_wgrad


def test_conv_shape_list_reaches_every_halo_kernel_and_the_implicit_gemm():
    kinds = set()
    for B, T, Fq, Ci, Co in CONV_SHAPES:
        kinds.add(halo_kernel(Fq, Co))          # forward
        kinds.add(halo_kernel(Fq, Ci))          # data gradient: N = Ci
    assert kinds == {"10-pass", "7-pass/128", "7-pass/192", None}


@pytest.mark.parametrize("B,T,Fq,Ci,Co", CONV_SHAPES)
@pytest.mark.parametrize("half", HALVES)
def test_conv3x3_half(hip_device, B, T, Fq, Ci, Co, half, monkeypatch):
    """forward with the fragment-fed (halo) kernel and with the implicit GEMM, the data gradient (the `wdg` pack),
    the weight gradient and the residual accumulate, each against float64 of the rounded operands.  The weight gradient
    rounds its operands only in the nine-tap kernel (channel counts that are multiples of 64, every layer of the
    model); the per-tap fallback computes the fp32 product in every mode, and that is what is pinned for it."""
    dev = hip_device
    x, w, dy = rnd(B, Ci, T, Fq, seed=1), rnd(Co, Ci, 3, 3, seed=2, scale=0.1), rnd(B, Co, T, Fq, seed=3)
    xr, wr, dyr = R.hr(x, half), R.hr(w, half), R.hr(dy, half)
    y_ref = F.conv2d(xr, wr, padding=1)
    dx_ref = torch.nn.grad.conv2d_input(xr.shape, wr, dyr, padding=1)
    dw_ref = torch.nn.grad.conv2d_weight(xr, wr.shape, dyr, padding=1)
    xd, dyd, wd_ = nhwc(x).to(dev), nhwc(dy).to(dev), w.to(dev)
    for frag in (True, False):
        monkeypatch.setattr(ops, "CONV_WFRAG", frag)
        with ops.matmul_bf16(True, half):
            wf, wdg = ops.conv3x3_repack(wd_)
            assert (wf.frag is not None) == frag
            y = ops.conv3x3_fwd(xd, wf)
            dx = ops.conv3x3_fwd(dyd, wdg)
            acc = rnd(B, T, Fq, Co, seed=4).to(dev)
            acc_ref = y_ref + nchw(acc.cpu()).double()
            ya = ops.conv3x3_fwd(xd, wf, out=acc, accumulate=True)
        close(nchw(y), y_ref)
        close(nchw(dx), dx_ref)
        close(nchw(ya), acc_ref)
        assert misses(nchw(y), F.conv2d(x.double(), w.double(), padding=1))
    dw = torch.empty_like(wd_)
    with ops.matmul_bf16(True, half):
        ops.conv3x3_wgrad(xd, dyd, dw)
    if Ci % 64 == 0 and Co % 64 == 0:                                    # the nine-tap kernel: rounded operands
        close(dw, dw_ref)
        assert misses(dw, torch.nn.grad.conv2d_weight(R.hr(x, OTHER[half]), wr.shape, R.hr(dy, OTHER[half]), padding=1))
    else:   # other channel counts take the per-tap kernels, which run on the native fp32 MFMA in every mode
        close(dw, torch.nn.grad.conv2d_weight(x.double(), w.shape, dy.double(), padding=1))   # (conv3x3_wgrad_impl)


@pytest.mark.parametrize("B,T,Fq,Ci,Co,acc", [(3, 16, 40, 128, 128, False), (2, 5, 20, 128, 192, True),
                                              (1, 3, 80, 64, 64, False), (2, 9, 10, 192, 256, True)])
@pytest.mark.parametrize("half", HALVES)
def test_conv3x3_epilogue_bn_statistics_half(hip_device, B, T, Fq, Ci, Co, acc, half):
    """test_ops_gpu.test_conv3x3_epilogue_bn_statistics under mixed precision: the fragment-fed kernel's BatchNorm
    partials (column sums of the final outputs) == the separate statistics pass over the stored activation"""
    dev = hip_device
    x = nhwc(rnd(B, Ci, T, Fq, seed=1)).to(dev)
    w = rnd(Co, Ci, 3, 3, seed=2, scale=0.1).to(dev)
    out = rnd(B, T, Fq, Co, seed=3).to(dev) if acc else None
    with ops.matmul_bf16(True, half):
        wf, _ = ops.conv3x3_repack(w, True, False)
        y, parts = ops.conv3x3_fwd(x, wf, out=out, accumulate=acc, bn_stats=True)
    assert parts is not None and parts.shape[1:] == (2, Co)
    gamma, beta = (rnd(Co, seed=4).abs() + 0.5).to(dev), rnd(Co, seed=5).to(dev)
    rm_a, rv_a = rnd(Co, seed=6).to(dev), (rnd(Co, seed=7).abs() + 0.5).to(dev)
    rm_b, rv_b = rm_a.clone(), rv_a.clone()
    st_a = ops.bn_train_stats(y, gamma, beta, rm_a, rv_a)
    st_b = ops.bn_train_stats(y, gamma, beta, rm_b, rv_b, partials=parts)
    for u, v in ((st_a.mean, st_b.mean), (st_a.invstd, st_b.invstd), (st_a.scale, st_b.scale), (st_a.shift, st_b.shift),
                 (rm_a, rm_b), (rv_a, rv_b)):
        close(v, u.cpu(), 1e-6)


def test_wfrag_pack_products_f16_is_rne_fp16_in_fragment_layout(hip_device):
    """pe_wfrag_pack (f16): fragment (kb, nb), lane 32 h + r  <->  w[32 nb + r][16 kb + 8 h .. + 7], bit-equal to the
    RNE fp16 of w (tail rows zero), including values that round to 65504, overflow, and fp16 subnormals"""
    N, K = 70, 96
    w = rnd(N, K, seed=3) * torch.exp(rnd(N, K, seed=4) * 2)
    w[0, :4] = torch.tensor([65519.0, 65520.0, -1e5, 3 * 2.0 ** -26])
    w[1, :3] = torch.tensor([2.0 ** -20, -(2.0 ** -24), 1 + 2.0 ** -11])
    raw = ops.wfrag_pack(w.to(hip_device), _lib.PE_PROD_F16).cpu()
    frag = raw.view(torch.int16).view(K // 16, 3, 1, 64, 8)[:, :, 0]                      # [kb][nb][lane][8]
    wpad = torch.zeros(96, K, dtype=torch.float16)
    wpad[:N] = w.to(torch.float16)
    ref = wpad.view(3, 32, K // 16, 2, 8).permute(2, 0, 3, 1, 4).reshape(K // 16, 3, 64, 8)
    assert torch.equal(frag, ref.view(torch.int16))


def test_products_bf16_packed_weight_used_under_f16_falls_back_to_the_implicit_gemm(hip_device):
    """A weight packed under bf16 carries bf16 fragments; used inside an f16 scope ops.conv3x3_fwd must not feed them
    to the f16 kernel (the `pw.products` guard) and gives the f16 result of the implicit GEMM"""
    B, T, Fq, Ci, Co = 2, 12, 10, 64, 128
    x, w = rnd(B, Ci, T, Fq, seed=1), rnd(Co, Ci, 3, 3, seed=2, scale=0.1)
    with ops.matmul_bf16(True, "bf16"):
        wf, _ = ops.conv3x3_repack(w.to(hip_device))
    assert wf.frag is not None and wf.products == _lib.PE_PROD_BF16
    with ops.matmul_bf16(True, "f16"):
        got = ops.conv3x3_fwd(nhwc(x).to(hip_device), wf)
    ref = F.conv2d(R.hr(x, "f16"), R.hr(w, "f16"), padding=1)
    close(nchw(got), ref)
    assert misses(nchw(got), F.conv2d(R.hr(x, "bf16"), R.hr(w, "bf16"), padding=1))


# ------------------------------------------------------------------ persistent LSTM (H = 384), teacher forcing
H_P = 384


def _init_cells(n, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    k = H_P ** -0.5
    whh = [(torch.rand(4 * H_P, H_P, generator=g) * 2 - 1) * k for _ in range(n)]
    xg = [torch.randn(B, T, 4 * H_P, generator=g) for _ in range(n)]
    dy = [torch.randn(B, T, 2 * H_P, generator=g) for _ in range((n + 1) // 2)]
    return whh, xg, dy


@pytest.mark.parametrize("B,reverse", [(1, (0,)), (1, (1,)), (65, (0,)), (65, (1,)), (130, (0,)), (130, (1,)),
                                       (256, (0, 1, 0, 1))])
@pytest.mark.parametrize("half", HALVES)
def test_persistent_lstm_half_step_by_step(hip_device, B, reverse, half, T=None):
    """pe_lstm_fwd_persistent_{bf16,f16} and pe_lstm_bwd_persistent_{bf16,f16}, one float64 step at a time from the
    kernel's own stored state.

    Forward, step t: gates_in[t] + r(W_hh) r(y[t-+1]) -> i, f, g, o -> c = f cbuf[t-+1] + i g, h = o tanh(c), against
    y[t], cbuf[t] and the activated gates the kernel leaves in the gates buffer.  gates_in is a copy of the buffer
    taken before the call (the kernel overwrites it), y[t-+1] / cbuf[t-+1] are read from the y slice and cbuf after
    the call; r(W_hh) is the kernel's register operand (round8<TH> of W_hh), r(y) its h operand.
    Backward, step t: dh = dY[t] + sum over the H/32 producer workgroups of bf16(partial), partial = r(dgates[t+-1])
    restricted to the producer's 128 gate columns times the matching rows of r(W_hh^T).  r(dgates[t+-1]) is the GPU's
    in-place output (the gates buffer after the call; the kernel rounds the same fp32 values with round4<TH> into its
    LDS operand), W_hh^T is the transposed weight the call reads; the partials travel as bf16 in both half modes
    (store_sc1_h).  The activated gates (copied after the forward) and cbuf give the gate gradients; dc is carried in
    float64.  A partial within fp32 accumulation noise of a bf16 rounding midpoint may round either way: its bf16 ulp
    is allowed (propagated to the gate gradients), and such partials must be rare.
    Also: the per-batch-tile bias-gradient rows (the ragged last tile at B = 65, 130), the gate-gradient absmax word,
    and controls -- unrounded operands and the other half type miss the GPU result (from T = 2 on: a single step has
    no recurrent product, so nothing is rounded and every model agrees).  ``T``: another sequence length
    (test_persistent_lstm_half_one_cell_edges)."""
    dev = hip_device
    n = len(reverse)
    T = T if T is not None else (6 if B < 256 else 4)
    whh, xg, dyb = _init_cells(n, B, T, seed=B + n)
    ybuf = [torch.zeros(B, T, 2 * H_P, device=dev) for _ in range((n + 1) // 2)]
    col = lambda i: slice((i % 2) * H_P, (i % 2 + 1) * H_P) if n > 1 else \
        slice(reverse[0] * H_P, (reverse[0] + 1) * H_P)                                  # noqa: E731
    ysl = [ybuf[i // 2][:, :, col(i)] for i in range(n)]
    dsl = [dyb[i // 2].to(dev)[:, :, col(i)] for i in range(n)]
    wd = [w.to(dev) for w in whh]
    gates = [x.to(dev) for x in xg]
    cbuf = [torch.empty(B, T, H_P, device=dev) for _ in range(n)]
    ops.clear_persistent_lstm_error(dev)
    with ops.matmul_bf16(True, half):
        assert ops._persistent_ok(n, B, H_P, dev, "fwd") and ops._persistent_ok(n, B, H_P, dev, "bwd")
        ops.lstm_fwd(wd, gates, ysl, cbuf, list(reverse), B, T, H_P)
        acts = [g.cpu() for g in gates]
        nrows = ops.lstm_bwd_dbias_rows(n, B, T, H_P, dsl[0].stride(1), dev)
        assert nrows == (B + 63) // 64
        rows = [torch.full((nrows, 4 * H_P), float("nan"), device=dev) for _ in range(n)]
        amx = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(n)]
        assert ops.lstm_bwd([ops.transpose2d(w) for w in wd], gates, cbuf, dsl, [torch.empty(B, H_P, device=dev)] * n,
                            list(reverse), B, T, H_P, dbias_rows=rows, amax_out=amx)
    torch.cuda.synchronize()
    assert not ops.persistent_lstm_error(dev)
    for i in range(n):
        y, c, dgt = ysl[i].cpu(), cbuf[i].cpu(), gates[i].cpu()
        # forward
        G, C, Y = R.lstm_fwd_teacher(xg[i], y, c, whh[i], reverse[i], half)
        for got, ref in ((y, Y), (c, C), (acts[i], G)):
            close(got, ref)
        for wrong in (None, OTHER[half]) if T > 1 else ():
            assert misses(y, R.lstm_fwd_teacher(xg[i], y, c, whh[i], reverse[i], wrong)[2])
        # backward
        dy = dsl[i].cpu()
        D, E, n_amb = R.lstm_bwd_teacher(dy, acts[i], c, whh[i], reverse[i], half, dgates_src=dgt)
        scale = D.abs().max().item()
        tol = 1e-5 * scale + E
        err = (dgt.double() - D).abs()
        assert (err <= tol).all(), (err.max().item(), scale, (err > tol).sum().item())
        parts = max(T - 1, 0) * (H_P // 32) * B * H_P
        assert n_amb <= 0.02 * parts, (n_amb, parts)
        print(f"cell {i}: dgates err {err.max().item():.2e} of {scale:.2e}; {n_amb} of {parts} partials at a "
              f"rounding boundary")
        for wrong, xh in ((None, None), (OTHER[half], R.XCHG_HALF)) if T > 1 else ():
            Dw, _, _ = R.lstm_bwd_teacher(dy, acts[i], c, whh[i], reverse[i], wrong, dgates_src=dgt, xhalf=xh)
            assert not ((dgt.double() - Dw).abs() <= tol).all(), wrong
        # bias-gradient rows: column sums of this cell's gate gradients over each 64-sample batch tile
        got_rows = rows[i].cpu().double()
        d64 = dgt.double()
        for bt in range(nrows):
            blk = d64[64 * bt:64 * bt + 64]
            ref_row, mag = blk.sum((0, 1)), blk.abs().sum((0, 1))
            assert ((got_rows[bt] - ref_row).abs() <= 1e-5 * mag + 1e-30).all(), bt
        assert amx[i].item() == dgt.abs().max().view(torch.int32).item()


@pytest.mark.parametrize("B,T", [(65, 1), (65, 2), (32, 3), (33, 3), (64, 3)])
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("half", HALVES)
def test_persistent_lstm_half_one_cell_edges(hip_device, B, T, reverse, half):
    """test_persistent_lstm_half_step_by_step (its models and its bounds) on one cell at the edges of the recurrence:
    T = 1 is the peeled step 0 alone and T = 2 adds the trailing cell update with no step between them; B = 32, 33
    and 64 leave the second half of the 64-sample batch tile empty, with one row and full."""
    test_persistent_lstm_half_step_by_step(hip_device, B, (reverse,), half, T=T)


@pytest.mark.parametrize("H", [64, 384])
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("half", HALVES)
def test_lstm_whh_grad_half(hip_device, H, reverse, half):
    """pe_lstm_whh_grad_{bf16,f16}: dW_hh = sum over (b, t) of r(dgates[b, t])^T r(h_{t-+1}[b]), y a strided slice of
    a [B, T, 2H] buffer; a long product (B T = 5200) takes the split-K form"""
    dev = hip_device
    for B, T in ((37, 9), (130, 40)):
        dg = rnd(B, T, 4 * H, seed=1)
        ybuf = torch.tanh(rnd(B, T, 2 * H, seed=2))
        ysl = ybuf.to(dev)[:, :, reverse * H:(reverse + 1) * H]
        dw = torch.empty(4 * H, H, device=dev)
        with ops.matmul_bf16(True, half):
            ops.lstm_whh_grad(dg.to(dev), ysl, dw, reverse, B, T, H)
        close(dw, R.whh_grad_ref(dg, ysl, reverse, half))
        assert misses(dw, R.whh_grad_ref(dg, ysl, reverse, None))
        assert misses(dw, R.whh_grad_ref(dg, ysl, reverse, OTHER[half]))


def test_lstm_recurrence_mixed_precision_f16(hip_device):
    from tests import test_ops_gpu
    for B, T, H in ((130, 9, 384), (5, 7, 64), (66, 6, 128)):
        test_ops_gpu.test_lstm_recurrence_mixed_precision(hip_device, B, T, H, half="f16")


def test_mixed_precision_recurrences_are_exactly_batch_invariant_f16(hip_device):
    from tests import test_ops_gpu
    test_ops_gpu.test_mixed_precision_recurrences_are_exactly_batch_and_scale_invariant(hip_device, half="f16")


# ------------------------------------------------------------------ fp16 range edges
def _product(op, a, b, dev, monkeypatch):
    """(GPU result, float64 reference of the rounded operands, |.| reference) of one product in the current half
    mode; ``a`` is the operand the edge values go into"""
    half = ops.HALF_DTYPE
    if op == "gemm_nt":
        got = ops.gemm_nt(a.to(dev), b.to(dev))
        f = lambda p, q: p @ q.T                                                          # noqa: E731
    elif op == "gemm_tn":
        got = ops.gemm_tn(a.to(dev), b.to(dev))
        f = lambda p, q: p.T @ q                                                          # noqa: E731
    elif op in ("conv_wf", "conv_igemm"):
        monkeypatch.setattr(ops, "CONV_WFRAG", op == "conv_wf")
        wf, _ = ops.conv3x3_repack(b.to(dev), True, False)
        assert (wf.frag is not None) == (op == "conv_wf")
        got = nchw(ops.conv3x3_fwd(a.to(dev), wf))
        f = lambda p, q: F.conv2d(nchw(p), q, padding=1)                                  # noqa: E731
    elif op == "conv_wgrad":
        got = torch.empty(b.shape[3], a.shape[3], 3, 3, device=dev)
        ops.conv3x3_wgrad(a.to(dev), b.to(dev), got)
        f = lambda p, q: torch.nn.grad.conv2d_weight(nchw(p), (q.shape[3], p.shape[3], 3, 3), nchw(q),  # noqa: E731
                                                     padding=1)
    elif op == "whh_grad":                                      # a = dgates [B, T, 4H], b = y [B, T, H]
        Bn, T, H = b.shape
        got = torch.empty(4 * H, H, device=dev)
        ops.lstm_whh_grad(a.to(dev), b.to(dev), got, 0, Bn, T, H)
        f = lambda p, q: p.reshape(-1, 4 * H).T @ R.shifted_y(q, 0).reshape(-1, H)       # noqa: E731
    ra, rb = R.hr(a, half), R.hr(b, half)
    return got.cpu().double(), f(ra, rb), f(ra.abs(), rb.abs())


def _operands(op, g):
    """operands of a small product of each kind, and one interior element of ``a`` with the mask of the outputs that
    read it"""
    r = lambda *s: torch.randn(*s, generator=g)                                          # noqa: E731
    if op == "gemm_nt":
        a, b, idx = r(100, 64), r(72, 64), (37, 11)
        reads = lambda o: torch.zeros_like(o, dtype=torch.bool).index_fill_(0, torch.tensor([37]), True)  # noqa: E731
    elif op == "gemm_tn":
        a, b, idx = r(300, 64), r(300, 72), (123, 9)
        reads = lambda o: torch.zeros_like(o, dtype=torch.bool).index_fill_(0, torch.tensor([9]), True)   # noqa: E731
    elif op in ("conv_wf", "conv_igemm"):
        a, b, idx = r(1, 6, 10, 64), r(128, 64, 3, 3) * 0.1, (0, 3, 4, 17)

        def reads(o):
            m = torch.zeros_like(o, dtype=torch.bool)
            m[0, :, 2:5, 3:6] = True
            return m
    elif op == "conv_wgrad":
        a, b, idx = r(1, 6, 10, 64), r(1, 6, 10, 128), (0, 3, 4, 17)
        reads = lambda o: torch.zeros_like(o, dtype=torch.bool).index_fill_(1, torch.tensor([17]), True)  # noqa: E731
    else:
        a, b, idx = r(5, 7, 4 * 64), torch.tanh(r(5, 7, 64)), (2, 3, 77)
        reads = lambda o: torch.zeros_like(o, dtype=torch.bool).index_fill_(0, torch.tensor([77]), True)  # noqa: E731
    return a, b, idx, reads


RANGE_OPS = ["gemm_nt", "gemm_tn", "conv_wf", "conv_igemm", "conv_wgrad", "whh_grad"]


@pytest.mark.parametrize("op", RANGE_OPS)
def test_fp16_operand_overflow_reaches_the_output(hip_device, op, monkeypatch):
    """f16 mode: an operand of 65504 or 65519 (RNE -> 65504) gives the finite product with 65504; 65520 or 1e5 rounds
    to Inf (RNE, no saturation to 65504) and makes exactly the outputs that read it non-finite, which
    ops.nonfinite_flag reports -- the GradScaler's overflow signal"""
    g = torch.Generator().manual_seed(7)
    a, b, idx, reads = _operands(op, g)
    with ops.matmul_bf16(True, "f16"):
        for v in (65504.0, 65519.0):
            a[idx] = v
            got, ref, mag = _product(op, a, b, hip_device, monkeypatch)
            assert torch.isfinite(got).all()
            assert ((got - ref).abs() <= 1e-5 * mag + 1e-30).all()
            assert int(ops.nonfinite_flag(got.float().to(hip_device)).item()) == 0
        for v in (65520.0, 1e5):
            a[idx] = v
            got, _, _ = _product(op, a, b, hip_device, monkeypatch)
            assert torch.equal(~torch.isfinite(got), reads(got)), op
            assert int(ops.nonfinite_flag(got.float().to(hip_device)).item()) == 1


@pytest.mark.parametrize("op", RANGE_OPS)
def test_fp16_subnormal_operands_are_kept(hip_device, op, monkeypatch):
    """f16 mode: operands scaled into the fp16 subnormal range (|a| ~ 2^-18, below 2^-14) are kept as torch's
    .to(torch.float16) keeps them: the product equals float64 of the rounded operands, bounded relative to
    |r(a)| |r(b)|; flushing them would leave zeros"""
    g = torch.Generator().manual_seed(8)
    a, b, _, _ = _operands(op, g)
    a = a * 2.0 ** -18
    assert R.hr(a, "f16").abs().max() < 2.0 ** -14 and (R.hr(a, "f16") != 0).float().mean() > 0.99
    with ops.matmul_bf16(True, "f16"):
        got, ref, mag = _product(op, a, b, hip_device, monkeypatch)
    assert ((got - ref).abs() <= 1e-5 * mag + 1e-40).all(), ((got - ref).abs() / mag).max()
    assert (got != 0).float().mean() > 0.99


@pytest.mark.parametrize("op", RANGE_OPS)
def test_bf16_operands_keep_the_fp32_exponent_range(hip_device, op, monkeypatch):
    """bf16 mode: operands of 1e30 and 1e-30 stay finite and accurate (an fp16 type leaking into a bf16 entry point
    would overflow / flush them)"""
    g = torch.Generator().manual_seed(9)
    a, b, _, _ = _operands(op, g)
    for sa, sb in ((1e30, 1e-30), (1e-30, 1e30)):
        with ops.matmul_bf16(True, "bf16"):
            got, ref, mag = _product(op, a * sa, b * sb, hip_device, monkeypatch)
        assert torch.isfinite(got).all()
        assert ((got - ref).abs() <= 1e-5 * mag).all()
