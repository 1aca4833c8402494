"""The mel front end's backward on the GPU (csrc/mel_grad.hip, ops.mel_backward, the autograd wrapper of mel.py).

Parity: for each case the kernel's gradient g is compared with the float64 restatement g64 of tests/mel_grad_ref.py,
e = max|g - g64| / max|g64| per row.  The yardstick y is the same figure for the float32 CPU autograd of the
reference's own arithmetic, and the bound is e <= 4 max(y, 2^-24): the 4x this project gives a float32 kernel over a
float32 restatement, and half an ulp of the largest element, below which no float32 result can be asked to go.  The
bound is relative to y because 1 / (log_eps + M) amplifies the bins near the log floor (tone: y ~ 5e-5).
"""
import functools

import numpy as np
import pytest
import torch

from pitchextractor_amd import _lib, inference, ops
from pitchextractor_amd.mel import DEFAULT_MEL_PARAMS, LOG_EPS, MEL_MEAN, MEL_STD, MelSpectrogram
from tests import mel_grad_ref as ref
from tests.mel_plan_ref import PARAM_SETS, mel_kwargs

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -24
SETS = {"default": dict(DEFAULT_MEL_PARAMS), **{k: mel_kwargs(p) for k, p, _ in PARAM_SETS}}
# a block segment of 3 * 4000 + 1024 floats: the frames kernel needs more than the default 64 KB of dynamic LDS
SETS["hop4000"] = dict(DEFAULT_MEL_PARAMS, hop_length=4000)


@functools.lru_cache(maxsize=None)
def transform(name):
    return MelSpectrogram(**SETS[name])


def wave_of(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        x = 0.3 * rng.standard_normal(n)
    elif kind == "tone":
        x = 0.5 * np.sin(2 * np.pi * 220.0 * np.arange(n) / 24000.0) + 1e-3 * rng.standard_normal(n)
    else:
        x = 1e-4 * rng.standard_normal(n)
    return x.astype(np.float32)


def grad_map(n_mels, frames, seed=1):
    return np.random.default_rng(seed).standard_normal((n_mels, frames)).astype(np.float32)


def dev(a, device):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device)


def run_row(mel, x, g, log, device):
    """One row through ops.mel_backward: x (n,), g (n_mels, T) -> (n,) float32 numpy."""
    gt = dev(g, device)[None, None] if log else dev(g, device)[None]
    return ops.mel_backward(mel, dev(x, device)[None], gt, log=log)[0].cpu().numpy()


def check_parity(got, x, g, what, **kw):
    g64 = ref.mel_backward(x, g, **kw)
    e, y = ref.rel_err(got, g64), ref.rel_err(ref.yardstick32(x, g, **kw), g64)
    print(f"{what}: e = {e:.3e}, yardstick y = {y:.3e}, e / y = {e / y:.2f}")
    assert e <= 4 * max(y, FLOOR), (what, e, y)


CASES = [("default", kind, n) for kind, n in (("noise", 513), ("noise", 1500), ("noise", 4801), ("tone", 4801),
                                               ("quiet", 4801))]
CASES += [(name, "noise", 4801) for name in ("hop75", "hop1200", "sr16k", "mels128")] + [("hop4000", "noise", 9000)]


@pytest.mark.parametrize("log", [True, False], ids=["log", "power"])
@pytest.mark.parametrize("name,kind,n", CASES, ids=[f"{c[0]}-{c[1]}{c[2]}" for c in CASES])
def test_parity_with_the_float64_restatement(hip_device, name, kind, n, log):
    """Worst e / y measured on the MI355X: see DESIGN section 22."""
    mel, params = transform(name), SETS[name]
    x, g = wave_of(kind, n), grad_map(mel.n_mels, mel.num_frames(n))
    got = run_row(mel, x, g, log, hip_device)
    assert np.isfinite(got).all()
    check_parity(got, x, g, f"{name} {kind} n={n} log={log}", log=log, **params)


def test_samples_no_frame_covers_get_exactly_zero(hip_device):
    """hop 1200: frame t covers padded positions [1200 t, 1200 t + 1024), so 176 of every 1200 have no frame."""
    mel, n = transform("hop1200"), 4801
    x, g = wave_of("noise", n), grad_map(80, 5)
    got = run_row(mel, x, g, True, hip_device)
    pos = np.arange(n + 1024)
    covered = np.zeros(n + 1024, bool)
    covered[pos[(pos % 1200 < 1024) & (pos // 1200 < 5)]] = True
    from oracle import mel_ref
    hit = np.zeros(n, bool)
    np.logical_or.at(hit, mel_ref.reflect_index(pos - 512, n), covered)
    assert (~hit).sum() > 500 and not got[~hit].any()
    assert np.count_nonzero(got[hit]) > 0.99 * hit.sum()


# ---- ragged batch with a crop, padding poisoned with NaN

LENGTHS, STARTS, T_OUT = (513, 2000, 4801, 300), (0, 1, 3, 0), 20


@functools.lru_cache(maxsize=None)
def ragged_case():
    n_max = max(LENGTHS)
    waves = np.zeros((len(LENGTHS), n_max), np.float32)
    g = np.full((len(LENGTHS), 1, 80, T_OUT), np.nan, np.float32)
    for b, (n, fs) in enumerate(zip(LENGTHS, STARTS)):
        waves[b, :n] = wave_of("noise", n, seed=10 + b)
        t_out, _ = ref.valid_frames(n, 300, fs, T_OUT)
        g[b, 0][:, t_out] = grad_map(80, t_out.size, seed=20 + b)
    return waves, g


def ragged_run(device, waves=None):
    w, g = ragged_case()
    wd = dev(w, device) if waves is None else waves
    out = ops.mel_backward(transform("default"), wd, dev(g, device),
                           lengths=torch.tensor(LENGTHS, dtype=torch.int32, device=device),
                           frame_start=torch.tensor(STARTS, dtype=torch.int32, device=device))
    return out.cpu().numpy()


def test_padding_never_leaks(hip_device):
    """out_frames past the valid frames, a crop, a row too short for the reflect padding; grad_out is NaN wherever
    the forward wrote padding."""
    w, g = ragged_case()
    got = ragged_run(hip_device)
    assert np.isfinite(got).all()
    for b, (n, fs) in enumerate(zip(LENGTHS, STARTS)):
        assert not got[b, n:].any()
        if n <= 512:
            assert not got[b].any()
            continue
        assert got[b, :n].any()
        check_parity(got[b, :n], w[b, :n], g[b, 0], f"ragged row {b} n={n} start={fs}", frame_start=fs)


def alone(device, b, stride_pad=0, replicas=1):
    """Row b of the ragged case through the fixed-batch entry point: its grad_out shifted to the source frames, zero
    where the crop shows nothing."""
    w, g = ragged_case()
    n, fs = LENGTHS[b], STARTS[b]
    t_out, t_src = ref.valid_frames(n, 300, fs, T_OUT)
    full = np.zeros((1, 1, 80, 1 + n // 300), np.float32)
    full[0, 0][:, t_src] = g[b, 0][:, t_out]
    mel = transform("default")
    wave = torch.zeros((replicas, n + stride_pad), device=device)
    wave[:, :n] = dev(w[b, :n], device)
    out = torch.full((replicas, n + stride_pad), 7.0, device=device)
    gt = dev(full, device).expand(replicas, 1, 80, full.shape[3])
    ws = ops.workspace(_lib.load().pe_mel_backward_workspace_bytes(mel._get_plan(device), replicas, n, full.shape[3]),
                       device)
    ops._call("pe_mel_backward", mel._get_plan(device), wave.data_ptr(), replicas, n, wave.stride(0), gt.data_ptr(),
              0 if replicas > 1 else gt.stride(0), gt.stride(2), gt.stride(3), full.shape[3], 1, LOG_EPS, MEL_MEAN,
              MEL_STD, out.data_ptr(), out.stride(0), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    assert (out[:, n:] == 7.0).all()                     # nothing is written past a row
    return out[:, :n].cpu().numpy()


def test_a_row_is_the_same_bits_alone_strided_and_in_any_batch(hip_device):
    got = ragged_run(hip_device)
    for b in (0, 1, 2):
        n = LENGTHS[b]
        assert np.array_equal(alone(hip_device, b)[0], got[b, :n]), b
        assert np.array_equal(alone(hip_device, b, stride_pad=37)[0], got[b, :n]), b     # odd stride: unaligned rows
    many = alone(hip_device, 2, replicas=300)              # a batch size at which the forward splits rows differently
    assert all(np.array_equal(many[r], got[2, :LENGTHS[2]]) for r in (0, 1, 150, 299))
    wide = torch.zeros((len(LENGTHS), max(LENGTHS) + 11), device=hip_device)
    wide[:, :max(LENGTHS)] = dev(ragged_case()[0], hip_device)
    assert np.array_equal(ragged_run(hip_device, wide[:, :max(LENGTHS)]), got)


def test_grad_out_layouts_give_the_same_bits(hip_device):
    mel, n = transform("default"), 4801
    x = dev(np.stack([wave_of("noise", n, seed=s) for s in (0, 1)]), hip_device)
    g = dev(np.stack([grad_map(80, 24, seed=s) for s in (2, 3)])[:, None], hip_device)       # (B, 1, n_mels, T)
    a = ops.mel_backward(mel, x, g)
    gt = g.transpose(-1, -2).contiguous()                                                    # (B, 1, T, n_mels)
    assert torch.equal(ops.mel_backward(mel, x, gt, frames_last=False), a)
    assert torch.equal(ops.mel_backward(mel, x, gt.transpose(-1, -2)), a)
    assert torch.equal(ops.mel_backward(mel, x, g.transpose(-1, -2), frames_last=False), a)


def test_linearity_is_exact_for_powers_of_two(hip_device):
    mel, n = transform("default"), 4801
    x, g = dev(wave_of("noise", n), hip_device)[None], dev(grad_map(80, 17), hip_device)[None]
    for log in (True, False):
        gg = g[None] if log else g
        base = ops.mel_backward(mel, x, gg, log=log)
        assert torch.equal(ops.mel_backward(mel, x, 2 * gg, log=log), 2 * base)
    assert torch.equal(ops.mel_backward(mel, 2 * x, g, log=False), 2 * ops.mel_backward(mel, x, g, log=False))


def test_shape_checks(hip_device):
    mel = transform("default")
    x = torch.zeros((2, 4801), device=hip_device)
    with pytest.raises(ValueError):
        ops.mel_backward(mel, x, torch.zeros((2, 1, 79, 17), device=hip_device))
    with pytest.raises(ValueError):
        ops.mel_backward(mel, x, torch.zeros((3, 1, 80, 17), device=hip_device))
    with pytest.raises(ValueError):
        ops.mel_backward(mel, x[:, :512], torch.zeros((2, 1, 80, 2), device=hip_device))
    with pytest.raises(ValueError):
        ops.mel_backward(mel, x.cpu(), torch.zeros((2, 1, 80, 17)))


# ---- autograd

def test_autograd_plumbing(hip_device):
    mel, n = transform("default"), 4801
    x = dev(np.stack([wave_of("noise", n, seed=s) for s in (0, 1)]), hip_device)
    g = dev(np.stack([grad_map(80, 24, seed=s) for s in (2, 3)])[:, None], hip_device)

    plain = mel.log_mel_batch(x, max_frames=24)
    assert plain.grad_fn is None
    xr = x.clone().requires_grad_()
    with torch.no_grad():
        assert mel.log_mel_batch(xr, max_frames=24).grad_fn is None
    out = mel.log_mel_batch(xr, max_frames=24)
    assert out.grad_fn is not None and torch.equal(out.detach(), plain)
    (out * g).sum().backward()
    assert torch.equal(xr.grad, ops.mel_backward(mel, x, g))
    with pytest.raises(ValueError):
        mel.log_mel_batch(xr, max_frames=24, out=torch.empty_like(plain))
    mel.log_mel_batch(xr.detach(), max_frames=24, out=torch.empty_like(plain))          # a plain wave keeps out=

    lengths = torch.tensor([4801, 2000], dtype=torch.int32, device=hip_device)
    starts = torch.tensor([2, 0], dtype=torch.int32, device=hip_device)
    plain = mel.log_mel_ragged(x, lengths, starts, max_frames=24)
    xr = x.clone().requires_grad_()
    out = mel.log_mel_ragged(xr, lengths, starts, max_frames=24)
    assert plain.grad_fn is None and out.grad_fn is not None and torch.equal(out.detach(), plain)
    gz = torch.nan_to_num(g)
    (out * gz).sum().backward()
    assert torch.equal(xr.grad, ops.mel_backward(mel, x, gz, lengths=lengths, frame_start=starts))
    assert xr.grad[1, :2000].any() and not xr.grad[1, 2000:].any()
    with pytest.raises(ValueError):
        mel.log_mel_ragged(xr, lengths, starts, max_frames=24, out=torch.empty_like(plain))

    x1 = x[0].clone().requires_grad_()
    out = mel(x1)
    assert out.grad_fn is not None and out.shape == (80, 17) and torch.equal(out.detach(), mel(x[0]))
    assert mel(x[0]).grad_fn is None
    (out * g[0, 0, :, :17]).sum().backward()
    assert x1.grad.shape == (n,)
    assert torch.equal(x1.grad, ops.mel_backward(mel, x[:1], g[:1, 0, :, :17], log=False)[0])
    x2 = x.clone().requires_grad_()
    (mel(x2) * g[:, 0, :, :17]).sum().backward()
    assert torch.equal(x2.grad[0], x1.grad)


def test_f0_loss_reaches_the_waveform(hip_device, monkeypatch):
    """The chain of INTEGRATION.md: audio -> log-mel -> frozen JDCNet -> loss, and back.  wave.grad is the mel backward
    of the network's own input gradient, bit for bit; the numbers of each link are checked above and in
    tests/test_input_grad_gpu.py."""
    from tests.test_input_grad_gpu import build
    monkeypatch.setattr(ops, "FP32_MATMUL", "h2")
    mel, T = transform("default"), 32
    net = build("bilstm", hip_device).eval().requires_grad_(False)
    assert net.is_frozen()
    x = dev(np.stack([wave_of("noise", 4801, seed=s) for s in (0, 1)]), hip_device)
    target = torch.linspace(80.0, 300.0, 2 * T, device=hip_device)

    wave = x.clone().requires_grad_()
    cls, _ = inference.f0_from_wave(net, wave, mel_transform=mel, max_frames=T)
    torch.nn.functional.smooth_l1_loss(cls.reshape(-1), target).backward()

    xin = mel.log_mel_batch(x, max_frames=T).requires_grad_()          # the detached mel, (B, 1, n_mels, T)
    cls2, _ = net(xin.transpose(-1, -2))
    assert torch.equal(cls2, cls.detach())
    torch.nn.functional.smooth_l1_loss(cls2.reshape(-1), target).backward()
    assert xin.grad.shape == (2, 1, 80, T)
    assert torch.equal(wave.grad, ops.mel_backward(mel, x, xin.grad))
    assert torch.isfinite(wave.grad).all() and wave.grad.any()
