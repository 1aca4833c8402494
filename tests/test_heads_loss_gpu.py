"""The kernels of csrc/heads_loss.hip off the one shape each ran at: the output heads, the two losses, the fused AdamW
step and the non-finite test, against the float64 references of tests/small_ops_ref.py.

Every bound is per element and scaled by the magnitude of the terms that were added (u = 2^-24); every test prints
its worst error / bound ratio (``-s``).  Each capped launcher's cap is restated here and the size that is meant to
cross it is asserted to, so a later change of a cap cannot make the case vacuous:

    pe_head_fwd            4096 blocks x 4 waves, one row per wave
    pe_head_bwd (dx)       16384 blocks x 256 threads, one float4 of dx per thread
    pe_f0_bins_ce_loss     4096 x 4 row waves;  gradient: 8192 blocks x 256 elements
    pe_adamw_step          8192 blocks x 256 float4
    pe_nonfinite_flag      8192 blocks x 256 float4
    pe_f0_sil_loss         one block of 1024 threads (a loop over R, no grid cap)
"""
import functools

import numpy as np
import pytest
import torch

from oracle import model_ref
from pitchextractor_amd import _lib, ops
from tests import small_ops_ref as S
from tests.test_ops_gpu import rnd

pytestmark = pytest.mark.gpu

U = S.U
FLT_MIN = 2.0 ** -126
REFUSED = (ValueError, _lib.HipLibraryError)

HEAD_FWD_WAVES_CAP = 4096 * 4
HEAD_BWD_DX_QUADS_CAP = 16384 * 256
BINS_ROW_WAVES_CAP = 4096 * 4
BINS_GRAD_ELEMS_CAP = 8192 * 256
ADAMW_ELEMS_CAP = 8192 * 256 * 4
NONFINITE_ELEMS_CAP = 8192 * 256 * 4
BIG_N = 8388608 + 1027


def f64(t):
    return t.detach().cpu().double().numpy()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (inf where the bound is 0 and the error is not)."""
    got = f64(got) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref, bound = np.asarray(ref, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(ref))
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    assert np.isfinite(got).all(), "non-finite result"
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max())


def misses(got, ref, bound):
    return ratio(got, ref, bound) > 1.0


def report(what, **ratios):
    print(f"[ratio] {what}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


# ------------------------------------------------------------------ heads
HEAD_CASES = [(1, 4, 1), (3, 8, 2), (255, 260, 8), (256, 64, 1), (257, 768, 2), (16389, 1028, 2)]


@functools.lru_cache(maxsize=None)
def head_case(R, D, n_out):
    x, w, b, dy = rnd(R, D, seed=1), rnd(n_out, D, seed=2, scale=0.05), rnd(n_out, seed=3), rnd(R, seed=4)
    return x, w, b, dy, S.head_ref(x, w, b, dy)


def head_bounds(D, n_out, ref):
    """y: one fma chain of ceil(D / 64) per lane, six shuffle adds, the bias and output adds; dx: n_out - 1 adds of
    the weight rows and one product; dw: the product rounded in fp32, the sum in double, one final rounding; db: the
    final rounding."""
    return dict(y=(-(-D // 64) + 8 + 2 * n_out) * U * ref["y"][1], dx=(n_out + 1) * U * ref["dx"][1],
                dw=2 * U * ref["dw"][1], db=U * ref["db"][1])


def test_head_cases_cross_the_grid_caps():
    R, D, _ = HEAD_CASES[-1]
    assert R > HEAD_FWD_WAVES_CAP and R * (D // 4) > HEAD_BWD_DX_QUADS_CAP
    assert all(r * (d // 4) <= HEAD_BWD_DX_QUADS_CAP and r <= HEAD_FWD_WAVES_CAP for r, d, _ in HEAD_CASES[:-1])
    assert D % 256 == 4 and 260 % 256 == 4             # lane 0 takes one more k pass than its neighbours


@pytest.mark.parametrize("R,D,n_out", HEAD_CASES)
def test_heads_against_float64(hip_device, R, D, n_out):
    dev = hip_device
    x, w, b, dy, ref = head_case(R, D, n_out)
    bound = head_bounds(D, n_out, ref)
    xd, wd, bd, dyd = (t.to(dev) for t in (x, w, b, dy))
    y = ops.head_fwd(xd, wd, bd)
    dw, db = torch.full((n_out, D), float("nan"), device=dev), torch.full((n_out,), float("nan"), device=dev)
    dx = ops.head_bwd(xd, wd, dyd, dw, db)
    r = dict(y=ratio(y, ref["y"][0], bound["y"]), dx=ratio(dx, ref["dx"][0], bound["dx"]),
             dw=ratio(dw[0], ref["dw"][0], bound["dw"]), db=ratio(db[0], ref["db"][0], bound["db"]))
    report(f"heads R={R} D={D} n_out={n_out}", **r)
    assert max(r.values()) <= 1.0, r
    # one sum is written to every row of dw and db
    for o in range(1, n_out):
        assert torch.equal(bits(dw[o]), bits(dw[0])) and torch.equal(bits(db[o]), bits(db[0]))
    # the data gradient alone: same bits
    dx2 = ops.head_bwd(xd, wd, dyd, None, None)
    assert torch.equal(bits(dx2), bits(dx))
    # controls at the same bounds: a weight row left out, dy shifted by one row
    assert misses(y, S.head_ref(x, w[:-1], b[:-1], dy)["y"][0], bound["y"])
    if R > 1:
        assert misses(dw[0], S.head_ref(x, w, b, torch.roll(dy, 1))["dw"][0], bound["dw"])


@pytest.mark.parametrize("fill", [0.0, float("nan")])
@pytest.mark.parametrize("R,D,n_out", HEAD_CASES[:3])
def test_heads_on_column_slices_of_wider_buffers(hip_device, R, D, n_out, fill):
    """ldx, lddx > D (offsets multiples of 4 floats): the dense call's bits, and nothing outside the slice is touched."""
    dev = hip_device
    x, w, b, dy, _ = head_case(R, D, n_out)
    xd, wd, bd, dyd = (t.to(dev) for t in (x, w, b, dy))
    y0 = ops.head_fwd(xd, wd, bd)
    dw0, db0 = torch.empty(n_out, D, device=dev), torch.empty(n_out, device=dev)
    dx0 = ops.head_bwd(xd, wd, dyd, dw0, db0)
    xbuf = torch.full((R, D + 12), fill, device=dev)
    xv = xbuf[:, 4:4 + D]
    xv.copy_(xd)
    dxbuf = torch.full((R, D + 16), fill, device=dev)
    before = bits(dxbuf).clone()
    dxv = dxbuf[:, 8:8 + D]
    assert xv.data_ptr() % 16 == 0 and dxv.data_ptr() % 16 == 0
    assert torch.equal(bits(ops.head_fwd(xv, wd, bd)), bits(y0))
    dw1, db1 = torch.empty(n_out, D, device=dev), torch.empty(n_out, device=dev)
    ops.head_bwd(xv, wd, dyd, dw1, db1, dx=dxv)
    assert torch.equal(bits(dxv), bits(dx0)) and torch.equal(bits(dw1), bits(dw0)) and torch.equal(bits(db1), bits(db0))
    after = bits(dxbuf)
    assert torch.equal(after[:, :8], before[:, :8]) and torch.equal(after[:, 8 + D:], before[:, 8 + D:])


def test_heads_refuse_what_they_cannot_run(hip_device):
    dev = hip_device
    z = lambda *s: torch.zeros(*s, device=dev)                                 # noqa: E731
    with pytest.raises(REFUSED):
        ops.head_fwd(z(3, 8), z(9, 8), z(9))                                   # n_out = 9
    with pytest.raises(REFUSED):
        ops.head_bwd(z(3, 8), z(9, 8), z(3), z(9, 8), z(9))
    with pytest.raises(REFUSED):
        ops.head_fwd(z(3, 6), z(2, 6), z(2))                                   # D = 6
    with pytest.raises(REFUSED):
        ops.head_bwd(z(3, 6), z(2, 6), z(3), z(2, 6), z(2))
    with pytest.raises(REFUSED):
        ops.head_fwd(z(3, 10)[:, :8], z(2, 8), z(2))                           # ldx = D + 2
    with pytest.raises(REFUSED):
        ops.head_bwd(z(3, 8), z(2, 8), z(3), z(2, 8), z(2), dx=z(3, 10)[:, :8])


# ------------------------------------------------------------------ SmoothL1 + BCE loss
D_EDGES = [0.75, 1.0, -1.0, 1 - 2.0 ** -24, -(1 - 2.0 ** -24), 1 + 2.0 ** -23, -(1 + 2.0 ** -23), 0.0, -0.75]
Z_EDGES = [100.0, -100.0, 1e4, -1e4, 0.0]


def loss_inputs(R):
    """The inputs of test_loss_matches_torch_criteria at R frames, with |f0_pred - f0| planted at 0, 1 - 2^-24, 1 and
    1 + 2^-23 in both signs (against f0 = 0, so the float32 difference is exact) and sil_pred at +-100, +-1e4 and 0,
    once on silent frames (target 1) and, where R allows, once on voiced ones (target 0).  |d| = 0.75 is planted too:
    the loss is continuous at |d| = 1, so only a point well inside the quadratic branch tells a wrong threshold."""
    f0p = rnd(R, seed=1) * 150 + 100
    f0 = torch.where(rnd(R, seed=2) > -0.5, rnd(R, seed=3).abs() * 200 + 80, torch.zeros(R))
    silp = rnd(R, seed=4) * 3
    n = min(R, len(D_EDGES))
    f0[:n], f0p[:n] = 0.0, torch.tensor(D_EDGES[:n])
    n = min(R, len(Z_EDGES))
    silp[:n] = torch.tensor(Z_EDGES[:n])
    if R >= 17:
        f0[12:17], silp[12:17] = 100.0, torch.tensor(Z_EDGES)
    return f0p, f0, silp, (f0 == 0).float()


def loss_check(out3, d_f0, d_sil, ref, R, gs):
    """Scalars within 2e-6 of sum |terms| / R, plus FLT_MIN: a mean below the normal range of float32 (R = 1 at z =
    100, y = 1: the loss is log1p(e^-100) = 3.7e-44) is a denormal or 0.
    d_f0 within 4 u |ref| + 1e-45: three fp32 multiplies and 1 / (float)R.
    d_sil = k (sigma - y), k = grad_scale / R, within 4 u |ref| + k (4 u sigma + FLT_MIN) + 1e-45: the same four
    roundings, plus those of sigma itself -- expf, 1 + e, the reciprocal (4 u sigma in all) -- which the subtraction of
    y = 1 does not scale down with the result, and the underflow of sigma where expf(-z) overflows (sigma < 1 /
    FLT_MAX comes out as 0: an absolute k FLT_MIN at most).  Measured on the MI355X: d_f0 at most 0.36 of its bound
    and d_sil 0.40 of this one; over 4 u |ref| + 1e-45 alone d_sil's error reaches 11 000 (z = 100 on a silent frame at
    grad_scale 65536: sigma rounds to 1 and the true 3.7e-44 k is lost), printed as d_sil_over_4u_ref."""
    k = float(S.F32(gs)) / R
    o = f64(out3)
    assert np.isfinite(o).all()
    lam0 = ref["abs_l1"] == 0.0                                          # lambda = 0: an exact zero, no floor
    r = dict(total=ratio(o[0], ref["total"], 2e-6 * (ref["abs_l1"] + ref["abs_bce"]) + FLT_MIN),
             l1=ratio(o[1], ref["l1"], 2e-6 * ref["abs_l1"] + (0.0 if lam0 else FLT_MIN)),
             bce=ratio(o[2], ref["bce"], 2e-6 * ref["abs_bce"] + FLT_MIN))
    if d_f0 is not None:
        r["d_f0"] = ratio(d_f0, ref["d_f0"], 4 * U * np.abs(ref["d_f0"]) + 1e-45)
        r["d_sil"] = ratio(d_sil, ref["d_sil"],
                           4 * U * np.abs(ref["d_sil"]) + k * (4 * U * ref["sigma"] + FLT_MIN) + 1e-45)
        # for the record (printed, not asserted): the same errors over 4 u |ref| + 1e-45 alone
        r["d_sil_over_4u_ref"] = ratio(d_sil, ref["d_sil"], 4 * U * np.abs(ref["d_sil"]) + 1e-45)
    return r


def asserted(r):
    return max(v for key, v in r.items() if key != "d_sil_over_4u_ref")


@pytest.mark.parametrize("R", [1, 3, 1023, 1024, 1025, 5000])
def test_f0_sil_loss_against_float64(hip_device, R):
    dev = hip_device
    f0p, f0, silp, sil = loss_inputs(R)
    args = [t.to(dev) for t in (f0p, f0, silp, sil)]
    big = (silp.abs() >= 100).numpy()
    worst = {}
    for lam in (0.1, 0.0):
        for gs in (1.0, 65536.0, 0.125):
            ref = S.f0_sil_loss_ref(f0p, f0, silp, sil, lam, gs)
            out3, d_f0, d_sil = ops.f0_sil_loss(*args, lam, grad_scale=gs)
            r = loss_check(out3, d_f0, d_sil, ref, R, gs)
            assert asserted(r) <= 1.0, (lam, gs, r)
            for key, v in r.items():
                worst[key] = max(worst.get(key, 0.0), v)
            # saturated logits: no NaN out of expf's overflow, and still grad_scale / R (sigma - y)
            got = f64(d_sil)[big]
            assert np.isfinite(got).all() and np.isfinite(f64(d_f0)).all()
            assert (np.abs(got - ref["d_sil"][big]) <= 4 * U * np.abs(ref["d_sil"][big]) + gs / R * FLT_MIN + 1e-45).all()
            # the evaluation pass: no gradients, the same scalar bits
            o2, g1, g2 = ops.f0_sil_loss(*args, lam, grad_scale=gs, want_grads=False)
            assert g1 is None and g2 is None and torch.equal(bits(o2), bits(out3))
            # |d| <= 1 is the same loss; beta = 0.5 is another one
            incl = S.f0_sil_loss_ref(f0p, f0, silp, sil, lam, gs, inclusive=True)
            assert asserted(loss_check(out3, d_f0, d_sil, incl, R, gs)) <= 1.0
            if lam != 0.0:
                half = S.f0_sil_loss_ref(f0p, f0, silp, sil, lam, gs, beta=0.5)
                assert loss_check(out3, None, None, half, R, gs)["l1"] > 1.0
            else:
                assert f64(out3)[1] == 0.0 and (f64(d_f0) == 0.0).all()
    report(f"f0_sil_loss R={R}", **worst)


# ------------------------------------------------------------------ 360-bin cross-entropy loss
BINS_CASES = [(1, 2), (5, 63), (5, 64), (5, 65), (517, 361), (16390, 130)]
LAM = float(np.float32(0.1))


@functools.lru_cache(maxsize=None)
def bins_case(R, C, voicing):
    """Inputs and the float64 oracle.  voicing: "mixed" (30 % unvoiced), "one" (exactly one voiced frame in the batch),
    "all".  Planted rows where R >= 5: 0 = one logit at +1e4 on the target bin, the rest at -1e4; 1 = the same off the
    target; 2 = a constant row; 3 = -inf everywhere except three finite logits, one of them the target."""
    g = torch.Generator().manual_seed(5 + R + C)
    logits = torch.randn(R, C, generator=g) * 3
    f0 = torch.rand(R, generator=g) * 600 + 40
    if voicing == "mixed":
        f0[torch.rand(R, generator=g) < 0.3] = 0.0
        f0[:min(R, 4)] = torch.tensor([55.0, 5.0, 31.7, 3000.0])[:min(R, 4)]    # on / below / on / above the grid
    elif voicing == "one":
        keep = f0[min(3, R - 1)].item()
        f0[:] = 0.0
        f0[min(3, R - 1)] = keep
    silp, sil = torch.randn(R, generator=g), (f0 == 0).float()
    if R >= 5:
        tgt = model_ref.f0_to_bins(f0.numpy()[:4], C)
        tgt = [int(t) if t >= 0 else 0 for t in tgt]
        logits[0], logits[1] = -1e4, -1e4
        logits[0, tgt[0]] = 1e4
        logits[1, (tgt[1] + 1) % C] = 1e4
        logits[2] = 3.0
        logits[3] = float("-inf")
        logits[3, [tgt[3], (tgt[3] + 1) % C, (tgt[3] + 7) % C]] = torch.tensor([0.5, -1.0, 2.0])
    lg, sp = logits.double().requires_grad_(True), silp.double().requires_grad_(True)
    tot, lf0, bce = model_ref.jdc_bins_loss(lg, sp, f0.double(), sil.double(), LAM)
    tot.backward()
    ref = dict(scalars=[tot.item(), lf0.item(), bce.item()], d_logits=lg.grad.numpy(), d_sil=sp.grad.numpy(),
               bins=model_ref.f0_to_bins(f0.numpy(), C), n_voiced=int((f0 > 0).sum()))
    return logits, f0, silp, sil, ref


def bins_check(out4, d_logits, d_sil, ref, R, gs):
    """Scalars: 2e-6 relative (every term of either mean is >= 0, so the value is its own sum of magnitudes).
    d_logits within 2e-6 k, k = grad_scale lambda / n_voiced the row's largest possible entry; d_sil within 2e-6
    grad_scale / R."""
    o = f64(out4)
    assert int(o[3]) == ref["n_voiced"]
    s = ref["scalars"]
    r = dict(total=ratio(o[0], s[0], 2e-6 * (abs(s[1]) + abs(s[2]))), ce=ratio(o[1], s[1], 2e-6 * abs(s[1])),
             bce=ratio(o[2], s[2], 2e-6 * abs(s[2])))
    if d_logits is not None:
        k = gs * LAM / max(ref["n_voiced"], 1)
        r["d_logits"] = ratio(d_logits, gs * ref["d_logits"], 2e-6 * k)
        r["d_sil"] = ratio(d_sil, gs * ref["d_sil"], 2e-6 * gs / R)
        # index work: the one-hot column is f0_to_bins' (wherever the softmax leaves it visible), unvoiced rows vanish
        got = f64(d_logits)
        voiced = ref["bins"] >= 0
        rows = np.nonzero(voiced)[0]
        seen = ref["d_logits"][rows, ref["bins"][rows]] < -1e-3 * LAM / max(ref["n_voiced"], 1)
        assert np.array_equal((got[rows] < 0).argmax(1)[seen], ref["bins"][rows][seen])
        assert seen.sum() >= len(rows) - 1
        assert (got[~voiced] == 0).all()
    return r


def test_bins_cases_cross_the_grid_caps():
    R, C = BINS_CASES[-1]
    assert R > BINS_ROW_WAVES_CAP and R * C > BINS_GRAD_ELEMS_CAP
    assert all(r <= BINS_ROW_WAVES_CAP and r * c <= BINS_GRAD_ELEMS_CAP for r, c in BINS_CASES[:-1])


@pytest.mark.parametrize("voicing", ["mixed", "one", "all"])
@pytest.mark.parametrize("R,C", BINS_CASES)
def test_f0_bins_ce_loss_against_float64(hip_device, R, C, voicing):
    dev = hip_device
    logits, f0, silp, sil, ref = bins_case(R, C, voicing)
    if voicing == "one":
        assert ref["n_voiced"] == 1
    args = [t.to(dev) for t in (logits, f0, silp, sil)]
    worst = {}
    for gs in (1.0, 65536.0):
        out4, d_logits, d_sil = ops.f0_bins_ce_loss(*args, LAM, grad_scale=gs)
        r = bins_check(out4, d_logits, d_sil, ref, R, gs)
        assert max(r.values()) <= 1.0, (gs, r)
        for key, v in r.items():
            worst[key] = max(worst.get(key, 0.0), v)
        o2, g1, g2 = ops.f0_bins_ce_loss(*args, LAM, grad_scale=gs, want_grads=False)
        assert g1 is None and g2 is None and torch.equal(bits(o2), bits(out4))
    report(f"f0_bins_ce_loss R={R} C={C} {voicing}", **worst)


def test_f0_bins_ce_loss_strided_through_the_c_abi(hip_device):
    """ldl = C + 8, ldd = C + 4: the dense call's bits, and the padding columns of d_logits keep theirs."""
    dev = hip_device
    R, C, gs = 517, 361, 65536.0
    logits, f0, silp, sil, _ = bins_case(R, C, "mixed")
    ld, f0d, spd, sd = (t.to(dev) for t in (logits, f0, silp, sil))
    out4, d_logits, d_sil = ops.f0_bins_ce_loss(ld, f0d, spd, sd, LAM, grad_scale=gs)
    lbuf = torch.full((R, C + 8), float("nan"), device=dev)
    lbuf[:, :C] = ld
    dbuf = torch.full((R, C + 4), float("nan"), device=dev)
    o2, ds2 = torch.empty(4, device=dev), torch.empty(R, device=dev)
    ws = ops.workspace(_lib.load().pe_f0_bins_ce_workspace_bytes(R), dev)
    ops._call("pe_f0_bins_ce_loss", lbuf.data_ptr(), C + 8, C, f0d.data_ptr(), spd.data_ptr(), sd.data_ptr(), LAM, R,
              gs, o2.data_ptr(), dbuf.data_ptr(), C + 4, ds2.data_ptr(), ws.data_ptr(), ws.numel(), ops._s())
    assert torch.equal(bits(o2), bits(out4)) and torch.equal(bits(ds2), bits(d_sil))
    assert torch.equal(bits(dbuf[:, :C]), bits(d_logits))
    assert torch.equal(bits(dbuf[:, C:]), bits(torch.full((R, 4), float("nan"), device=dev)))
    # a row stride below the row is refused before any launch
    with pytest.raises(REFUSED):
        ops._call("pe_f0_bins_ce_loss", lbuf.data_ptr(), C - 1, C, f0d.data_ptr(), spd.data_ptr(), sd.data_ptr(), LAM,
                  R, gs, o2.data_ptr(), dbuf.data_ptr(), C + 4, ds2.data_ptr(), ws.data_ptr(), ws.numel(), ops._s())


# ------------------------------------------------------------------ AdamW
LR, BETA1, BETA2 = 3e-4, 0.9, 0.98
ADAMW_COMBOS = [(step, wd, eps, gs) for step in (1, 2, 1000, 10 ** 6) for wd in (0.0, 5e-4, 0.1)
                for eps in (1e-9, 1e-3) for gs in (1.0, 0.125, 2.0 ** -16)]


def adamw_check(before, after, g, hyper):
    """|m' - ref| <= 4 u mag_m, |v' - ref| <= 4 u mag_v, |p' - ref_p(m'_gpu, v'_gpu)| <= 8 u mag_p: the fp32 roundings
    are 3 for m, 4 for v and 7 for p (sqrtf and the two divisions included).  Returns the three worst ratios and the
    reference pieces."""
    p0, m0, v0 = before
    p1, m1, v1 = after
    mr, vr, mag_m, mag_v, param = S.adamw_step_ref(p0, g, m0, v0, *hyper)
    pr, mag_p = param(m1, v1)
    assert np.isfinite(f64(p1)).all() and np.isfinite(f64(m1)).all() and np.isfinite(f64(v1)).all()
    return dict(m=ratio(m1, mr, 4 * U * mag_m), v=ratio(v1, vr, 4 * U * mag_v), p=ratio(p1, pr, 8 * U * mag_p))


def adamw_controls_miss(before, after, g, hyper):
    """double 1 - beta2 (the unrounded beta2) must miss v'; coupled (L2) weight decay must miss m' where wd > 0."""
    p0, m0, v0 = before
    _, m1, v1 = after
    _, vr, _, mag_v, _ = S.adamw_step_ref(p0, g, m0, v0, *hyper)
    _, vc, _, _, _ = S.adamw_step_ref(p0, g, m0, v0, *hyper, w2_double=True)
    assert misses(v1, vc, 4 * U * mag_v)
    if hyper[4] > 0:
        mc, _, mag_m, _, _ = S.adamw_step_ref(p0, g, m0, v0, *hyper, coupled=True)
        assert misses(m1, mc, 4 * U * mag_m)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1003])
def test_adamw_step_against_float64(hip_device, n):
    """Three consecutive steps per combination of step, weight decay, eps and grad_scale (gradients scaled up by its
    inverse), each checked from the kernel's own previous p, m, v.  Element 0 (n >= 2) has g = 0 and v = 0: the
    denominator is eps alone."""
    dev = hip_device
    worst = dict(m=0.0, v=0.0, p=0.0)
    for ci, (step, wd, eps, gs) in enumerate(ADAMW_COMBOS):
        p = rnd(n, seed=100 + ci)
        m = torch.zeros(n) if step == 1 else rnd(n, seed=200 + ci) * 0.1
        v = torch.zeros(n) if step == 1 else (rnd(n, seed=300 + ci) * 0.1) ** 2
        if n >= 2:
            v[0] = 0.0
            m[0] = 0.0 if step == 1 else 0.01
        pd, md, vd = p.to(dev), m.to(dev), v.to(dev)
        for s in range(3):
            g = rnd(n, seed=400 + 3 * ci + s) * (1.0 / gs)
            if n >= 2:
                g[0] = 0.0
            before = (pd.cpu(), md.cpu(), vd.cpu())
            hyper = (LR, BETA1, BETA2, eps, wd, step + s, gs)
            ops.adamw_step(pd, g.to(dev), md, vd, *hyper)
            after = (pd.cpu(), md.cpu(), vd.cpu())
            r = adamw_check(before, after, g, hyper)
            assert max(r.values()) <= 1.0, (step + s, wd, eps, gs, r)
            for key in worst:
                worst[key] = max(worst[key], r[key])
            if n == 1003:
                adamw_controls_miss(before, after, g, hyper)
    report(f"adamw n={n}", **worst)


def test_adamw_step_second_grid_pass_and_tail(hip_device):
    """n = 8 388 608 + 1027: the float4 loop runs a second pass (elements 8 388 608 .. 8 389 631) and the tail holds 3.
    Two steps on data drawn on the device; the reference on every 997th element plus the last 2048."""
    dev, n = hip_device, BIG_N
    assert n > ADAMW_ELEMS_CAP and n & 3 == 3 and n - 2048 < ADAMW_ELEMS_CAP
    gen = torch.Generator(device=dev).manual_seed(7)
    pd = torch.randn(n, generator=gen, device=dev)
    md = torch.randn(n, generator=gen, device=dev) * 0.1
    vd = (torch.randn(n, generator=gen, device=dev) * 0.1) ** 2
    idx = torch.unique(torch.cat([torch.arange(0, n, 997), torch.arange(n - 2048, n)])).to(dev)
    take = lambda *ts: tuple(t[idx].cpu() for t in ts)                         # noqa: E731
    worst = dict(m=0.0, v=0.0, p=0.0)
    for s in range(2):
        gd = torch.randn(n, generator=gen, device=dev) * 8.0
        hyper = (LR, BETA1, BETA2, 1e-9, 5e-4, 5 + s, 0.125)
        before = take(pd, md, vd)
        ops.adamw_step(pd, gd, md, vd, *hyper)
        after = take(pd, md, vd)
        r = adamw_check(before, after, gd[idx].cpu(), hyper)
        assert max(r.values()) <= 1.0, (s, r)
        adamw_controls_miss(before, after, gd[idx].cpu(), hyper)
        for key in worst:
            worst[key] = max(worst[key], r[key])
    report(f"adamw n={n}", **worst)
    # a non-zero skip word: nothing moves
    keep = [t.clone() for t in (pd, md, vd)]
    ops.adamw_step(pd, gd, md, vd, LR, BETA1, BETA2, 1e-9, 5e-4, 7, 0.125, skip_flag=torch.ones(1, device=dev))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((pd, md, vd), keep))
    # and a zero one lets the step through
    ops.adamw_step(pd, gd, md, vd, LR, BETA1, BETA2, 1e-9, 5e-4, 7, 0.125, skip_flag=torch.zeros(1, device=dev))
    assert not torch.equal(pd[-1024:], keep[0][-1024:])


def test_adamw_step_skip_word_and_refusals(hip_device):
    dev, n = hip_device, 5
    p, g, m, v = (rnd(n, seed=i).abs().to(dev) for i in range(4))
    keep = [t.clone() for t in (p, m, v)]
    ops.adamw_step(p, g, m, v, LR, BETA1, BETA2, 1e-9, 5e-4, 3, skip_flag=torch.full((1,), 2.0, device=dev))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((p, m, v), keep))
    # a parameter view that starts one element into its buffer is not 16-byte aligned
    buf = torch.zeros(n + 3, device=dev)
    with pytest.raises(REFUSED):
        ops.adamw_step(buf[1:n + 1], g, m, v, LR, BETA1, BETA2, 1e-9, 5e-4, 3)
    # step 0: bias_correction1 = 0, an infinite step size -- refused by the wrapper and by the C ABI, nothing launched
    with pytest.raises(ValueError):
        ops.adamw_step(p, g, m, v, LR, BETA1, BETA2, 1e-9, 5e-4, 0)
    for bc1, bc2 in ((0.0, 0.5), (0.5, 0.0), (1.5, 0.5), (-0.1, 0.5), (float("nan"), 0.5), (0.5, float("nan"))):
        with pytest.raises(_lib.HipLibraryError):
            ops._call("pe_adamw_step", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, BETA1, BETA2,
                      1e-9, 5e-4, bc1, bc2, 1.0, 0, ops._s())
    torch.cuda.synchronize()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((p, m, v), keep))


# ------------------------------------------------------------------ non-finite test
FLT_MAX = float(np.finfo(np.float32).max)
NEG_NAN = float(np.array([0xFFC00000], np.uint32).view(np.float32)[0])


def flag_of(x, flag=None):
    return int(ops.nonfinite_flag(x, flag).item())


def test_nonfinite_flag_small_sizes_and_values(hip_device):
    dev = hip_device
    assert flag_of(torch.empty(0, device=dev)) == 0                 # an empty tensor has no pointer: the wrapper's word
    live, word = torch.ones(4, device=dev), torch.ones(1, dtype=torch.int32, device=dev)
    ops._call("pe_nonfinite_flag", live.data_ptr(), 0, word.data_ptr(), ops._s())      # n = 0 through the C ABI
    assert word.item() == 0
    for n in (1, 2, 3, 5):
        x = torch.ones(n, device=dev)
        assert flag_of(x) == 0
        for bad in (float("nan"), NEG_NAN, float("inf"), float("-inf")):
            y = x.clone()
            y[n - 1] = bad                                          # the last element: the n & 3 tail
            assert flag_of(y) == 1, (n, bad)
        for fine in (FLT_MAX, -FLT_MAX, 2.0 ** -149, -0.0):
            y = x.clone()
            y[n - 1] = fine
            assert flag_of(y) == 0, (n, fine)
    # the sign bit of a NaN survives the trip to the device
    y = torch.from_numpy(np.array([0xFFC00000, 0xFF800000], np.uint32).view(np.float32).copy()).to(dev)
    assert bits(y).tolist() == [-4194304, -8388608] and flag_of(y[:1].clone()) == 1
    # a word that holds 1 from an earlier call is cleared by a clean one
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    assert flag_of(torch.full((5,), float("inf"), device=dev), word) == 1 and word.item() == 1
    assert flag_of(torch.ones(5, device=dev), word) == 0 and word.item() == 0


def test_nonfinite_flag_second_grid_pass_and_tail(hip_device):
    dev, n = hip_device, BIG_N
    assert n > NONFINITE_ELEMS_CAP and n & 3 == 3
    x = torch.ones(n, device=dev)
    assert flag_of(x) == 0
    for pos in (NONFINITE_ELEMS_CAP + 5, n - 1, 0):          # only the second pass / only the tail reaches these
        x[pos] = float("nan")
        assert flag_of(x) == 1, pos
        x[pos] = 1.0
    assert flag_of(x) == 0
