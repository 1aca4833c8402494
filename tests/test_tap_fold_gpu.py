"""Detector taps folded into the BatchNorm passes (pe_bn_act_pool_tap_fwd / pe_bn_act_pool_tap_bwd).

The fused passes must leave exactly the bits of the two passes they replace: ``bn_act_pool_fwd`` + ``maxpool_fwd`` and
``bn_act_pool_bwd`` + ``maxpool_bwd_add`` (outputs, tap slice, positions of the maxima, absmax words, BatchNorm
parameter gradients), at the three geometries of the network, with a partial last workgroup, in both storage types.  The
first-maximum rule is also held to torch's CPU max_pool2d in float64, and a whole model step must not change with the
fold on or off."""
import pytest
import torch
import torch.nn.functional as F

from pitchextractor_amd import _lib, ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
POOL = 2
# F, C, tap_pool, channel offset of the tap in the 640-wide concat
GEOMETRIES = [(80, 64, 40, 0), (40, 128, 20, 64), (20, 192, 10, 192)]      # C = 192: 5 pixel lanes, 16 idle threads


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def r16(t):                      # bf16-representable, so the same values serve both storage types
    return t.to(BF).float()


def word(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


def bn_state(x, C, dev):
    gamma, beta = rnd(C, seed=2).to(dev) + 1.5, rnd(C, seed=3).to(dev)
    return ops.bn_train_stats(x, gamma, beta, None, None)


def served(x, tap_pool, with_arg=True):
    B, T, Fq, C = x.shape
    return _lib.load().pe_bn_act_pool_tap_supported(B * T, Fq, C, POOL, tap_pool, int(with_arg)) == 1


def two_passes_fwd(x, st, tap_pool, coff, wide):
    w = word(x.device)
    y = ops.bn_act_pool_fwd(x, st, pool=POOL, amax_out=w)
    _, arg = ops.maxpool_fwd(x, tap_pool, out=wide, coff=coff, want_argmax=True)
    return y, arg, w


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows", [3, 5])
@pytest.mark.parametrize("Fq,C,tap_pool,coff", GEOMETRIES)
def test_fused_passes_equal_the_two_passes(hip_device, Fq, C, tap_pool, coff, rows, dt):
    dev = hip_device
    x = r16(rnd(1, rows, Fq, C, seed=1) * 3).to(dev).to(dt)
    assert served(x, tap_pool)
    st = bn_state(x, C, dev)
    Ft = Fq // tap_pool
    wide_ref = torch.full((1, rows, Ft, 640), 7.0, device=dev, dtype=dt)
    wide = wide_ref.clone()
    y_ref, arg_ref, w_ref = two_passes_fwd(x, st, tap_pool, coff, wide_ref)

    tap = ops.Tap(wide, tap_pool, coff, want_argmax=True)
    w = word(dev)
    y = ops.bn_act_pool_fwd(x, st, pool=POOL, amax_out=w, tap=tap)
    assert torch.equal(y, y_ref) and torch.equal(w, w_ref)
    assert torch.equal(wide, wide_ref)                              # the slice, and nothing outside it
    assert (wide[..., :coff] == 7.0).all() and (wide[..., coff + C:] == 7.0).all()
    assert tap.argmax.dtype == torch.uint8 and torch.equal(tap.argmax, arg_ref)

    # without positions (eval / inference): same outputs, no byte array
    wide2 = torch.full_like(wide, 7.0)
    tap2 = ops.Tap(wide2, tap_pool, coff)
    y2 = ops.bn_act_pool_fwd(x, st, pool=POOL, tap=tap2)
    assert tap2.argmax is None and torch.equal(y2, y_ref) and torch.equal(wide2, wide_ref)

    dy = r16(rnd(1, rows, Fq // POOL, C, seed=4)).to(dev).to(dt)
    dwide = r16(rnd(1, rows, Ft, 640, seed=5)).to(dev).to(dt)
    g_ref = [torch.empty(C, device=dev) for _ in range(2)]
    wb_ref = word(dev)
    dx_ref = ops.bn_act_pool_bwd(x, dy, st, g_ref[0], g_ref[1], pool=POOL, amax_out=wb_ref)
    ops.maxpool_bwd_add(x, dwide, dx_ref, tap_pool, coff=coff, amax_out=wb_ref, argmax=arg_ref)
    g = [torch.empty(C, device=dev) for _ in range(2)]
    wb = word(dev)
    tap.grad = dwide
    dx = ops.bn_act_pool_bwd(x, dy, st, g[0], g[1], pool=POOL, amax_out=wb, tap=tap)
    assert dx.dtype == dt and torch.equal(dx, dx_ref)
    assert torch.equal(g[0], g_ref[0]) and torch.equal(g[1], g_ref[1])
    assert torch.equal(wb, wb_ref)


@pytest.mark.parametrize("Fq,C,tap_pool,coff", GEOMETRIES)
def test_ties_go_to_the_first_maximum_like_torch(hip_device, Fq, C, tap_pool, coff):
    """Three distinct values only, so every tap window holds its maximum many times: in one BN window, in several windows
    of one pixel lane and in the segments of different lanes.  Channels 0..7 of the first row are constant (the maximum
    is everywhere: position 0), channels 8..15 put the only maximum last.  Reference: torch CPU max_pool2d in float64."""
    dev, rows = hip_device, 5
    g = torch.Generator().manual_seed(11)
    x = torch.randint(0, 3, (1, rows, Fq, C), generator=g).float() - 1.0
    x[0, 0, :, 0:8] = 1.0
    x[0, 0, :, 8:16] = -1.0
    x[0, 0, tap_pool - 1, 8:16] = 0.0
    x[0, 0, Fq - 1, 8:16] = 0.0
    ref_v, ref_i = F.max_pool2d(x.double().permute(0, 3, 1, 2), (1, tap_pool), return_indices=True)   # [1, C, rows, Ft]
    Ft = Fq // tap_pool
    ref_pos = (ref_i % Fq) - torch.arange(Ft).view(1, 1, 1, Ft) * tap_pool
    ref_v, ref_pos = ref_v.permute(0, 2, 3, 1), ref_pos.permute(0, 2, 3, 1)
    assert (ref_pos[0, 0, :, 0:8] == 0).all() and (ref_pos[0, 0, :, 8:16] == tap_pool - 1).all()
    for dt in (torch.float32, BF):
        xd = x.to(dev).to(dt)
        assert served(xd, tap_pool)
        wide = torch.zeros(1, rows, Ft, 640, device=dev, dtype=dt)
        tap = ops.Tap(wide, tap_pool, coff, want_argmax=True)
        ops.bn_act_pool_fwd(xd, bn_state(xd, C, dev), pool=POOL, tap=tap)
        assert torch.equal(wide[..., coff:coff + C].double().cpu(), ref_v)
        assert torch.equal(tap.argmax.cpu().long(), ref_pos)


def test_unserved_geometry_falls_back_to_the_two_passes(hip_device):
    """tap_pool % pool != 0: the library refuses the fused pass and ops runs the BN pass and the tap pass."""
    dev, rows, Fq, C, tap_pool, coff = hip_device, 3, 80, 64, 5, 64
    x = r16(rnd(1, rows, Fq, C, seed=1)).to(dev)
    assert not served(x, tap_pool)
    lib = _lib.load()
    assert lib.pe_bn_act_pool_tap_supported(rows, Fq, C, POOL, 40, 1) == 1
    assert lib.pe_bn_act_pool_tap_supported(rows, Fq, C, POOL, 30, 1) == 0        # Fin % tap_pool != 0
    assert lib.pe_bn_act_pool_tap_supported(rows, 512, C, POOL, 256, 1) == 0      # positions do not fit a byte
    assert lib.pe_bn_act_pool_tap_supported(rows, 512, C, POOL, 256, 0) == 1
    st = bn_state(x, C, dev)
    Ft = Fq // tap_pool
    wide_ref = torch.zeros(1, rows, Ft, 640, device=dev)
    y_ref, arg_ref, w_ref = two_passes_fwd(x, st, tap_pool, coff, wide_ref)
    wide = torch.zeros_like(wide_ref)
    tap, w = ops.Tap(wide, tap_pool, coff, want_argmax=True), word(dev)
    y = ops.bn_act_pool_fwd(x, st, pool=POOL, amax_out=w, tap=tap)
    assert torch.equal(y, y_ref) and torch.equal(wide, wide_ref) and torch.equal(tap.argmax, arg_ref)
    assert torch.equal(w, w_ref)
    dy, dwide = rnd(1, rows, Fq // POOL, C, seed=4).to(dev), rnd(1, rows, Ft, 640, seed=5).to(dev)
    g_ref, g = [torch.empty(C, device=dev) for _ in range(2)], [torch.empty(C, device=dev) for _ in range(2)]
    wb_ref, wb = word(dev), word(dev)
    dx_ref = ops.bn_act_pool_bwd(x, dy, st, g_ref[0], g_ref[1], pool=POOL, amax_out=wb_ref)
    ops.maxpool_bwd_add(x, dwide, dx_ref, tap_pool, coff=coff, amax_out=wb_ref, argmax=arg_ref)
    tap.grad = dwide
    dx = ops.bn_act_pool_bwd(x, dy, st, g[0], g[1], pool=POOL, amax_out=wb, tap=tap)
    assert torch.equal(dx, dx_ref) and torch.equal(wb, wb_ref)
    assert torch.equal(g[0], g_ref[0]) and torch.equal(g[1], g_ref[1])


def _model_step(state, x, d_cls, d_det, dev, calls):
    from tests.test_model_gpu import build
    net = build(state, 360, 64, dev, dropout=0.2).train()
    calls.clear()
    cls, det = net(x)
    torch.autograd.backward([cls, det], [d_cls, d_det])
    out = {"cls": cls.detach().clone(), "det": det.detach().clone()}
    out.update({"grad " + n: p.grad.detach().clone() for n, p in net.named_parameters()})
    out.update({"buffer " + n: b.detach().clone() for n, b in net.named_buffers()})
    net.eval()
    with torch.no_grad():
        ecls, edet = net(x)
    out["eval cls"], out["eval det"] = ecls.clone(), edet.clone()
    return out


@pytest.mark.parametrize("mode", ["h2", "bf16_act16"])
def test_model_step_is_the_same_with_the_fold_on_and_off(hip_device, mode, monkeypatch):
    """One train forward + backward and one eval forward at B = 2: outputs, every parameter gradient and the BatchNorm
    running statistics are bit-identical with FOLD_TAPS on and off (fresh, equally seeded networks: same dropout)."""
    import contextlib
    from oracle import model_ref
    from pitchextractor_amd import model as pe_model
    dev = hip_device
    state = model_ref.seeded_state(5, num_class=360, hidden_size=64)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 1, 64, 80, generator=g).to(dev)
    d_cls, d_det = torch.randn(2, 64, 360, generator=g).to(dev), torch.randn(2, 64, generator=g).to(dev)
    calls, orig_call = [], ops._call

    def spy(name, *a, **k):
        calls.append(name)
        return orig_call(name, *a, **k)

    monkeypatch.setattr(ops, "_call", spy)
    if mode == "h2":
        monkeypatch.setattr(ops, "FP32_MATMUL", "h2")
        ctx = contextlib.nullcontext()
    else:
        ctx = ops.matmul_bf16(True, "bf16", act16=True)
    runs = {}
    with ctx:
        for fold in (False, True):
            monkeypatch.setattr(pe_model, "FOLD_TAPS", fold)
            runs[fold] = _model_step(state, x, d_cls, d_det, dev, calls)
            n = {k: calls.count(k) for k in ("pe_maxpool_fwd", "pe_maxpool_bwd_add", "pe_bn_act_pool_tap_fwd",
                                             "pe_bn_act_pool_tap_bwd")}
            # train forward + eval forward, one backward
            assert list(n.values()) == ([0, 0, 6, 3] if fold else [6, 3, 0, 0]), n
    assert not ops.persistent_lstm_error(dev)
    assert runs[False].keys() == runs[True].keys()
    for name, ref in runs[False].items():
        assert torch.equal(runs[True][name], ref), name
