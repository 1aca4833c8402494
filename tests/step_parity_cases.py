"""One train forward and backward of JDCNet per head and product mode, reduced to the sequence of C-ABI launches and to
digests of what the step leaves behind.

Shared by tests/golden/make_step_parity_golden.py, which recorded both with the build BEFORE a scale word travelled with
its tensor (``ops.Scaled``), and tests/test_step_parity_gpu.py, which holds today's build to them launch for launch and
bit for bit.  The cases use only what both builds have: ``JDCNet``, ``ops.FP32_MATMUL``, ``ops.matmul_bf16`` and
``ops._call``, which the recorder wraps to note (entry point, products, act16) in call order.

Shapes are the smallest that reach every branch of the word plumbing: input randn(B, 1, T, 80) (80 mel bins are the
network's geometry) with B = 2, T = 64; the BiLSTM head at num_class 1, H = 384 (persistent recurrences, bias rows and
gate-gradient words from the kernel) and at num_class 360, H = 64 (per-step kernels, the classifier as a GEMM); the
Transformer head at T = 64 (unfused attention) and at B = 1, T = 192 (fused attention); each in the modes h2, x3, native,
bf16 with bf16 activation storage, and f16.  Two more h2 steps: a frozen network with ``x.requires_grad`` (the
input-gradient chain) and an eval forward under ``no_grad``.  Temporal-head dropout is 0.2, the block dropout the
network's own 0.5; the masks are Philox streams of seed 0, so a step is a pure function of its case.
"""
import hashlib
from contextlib import contextmanager
from functools import lru_cache

import torch

from oracle import model_ref
from pitchextractor_amd import ops
from pitchextractor_amd.model import JDCNet
from tests.golden.make_golden import SEQ_CFG, TF_CFG

DROPOUT = 0.2
# head -> (model type, num_class, hidden size, B, T)
HEADS = {"lstm_nc1_h384": ("bilstm", 1, 384, 2, 64), "lstm_nc360_h64": ("bilstm", 360, 64, 2, 64),
         "tf_t64": ("transformer", 1, 384, 2, 64), "tf_b1_t192": ("transformer", 1, 384, 1, 192)}
MODES = ("h2", "x3", "native", "bf16_act16", "f16")
EXTRA = {"lstm_nc1_h384/h2/frozen_dx": ("lstm_nc1_h384", "h2", "frozen"),
         "lstm_nc1_h384/h2/eval": ("lstm_nc1_h384", "h2", "eval")}
CASES = {**{f"{h}/{m}": (h, m, "train") for h in HEADS for m in MODES}, **EXTRA}


def digest(*tensors) -> str:
    """sha256 of the tensors' bytes, one after the other."""
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


@contextmanager
def mode(name):
    """The product mode ``name`` for the ops called inside."""
    prev = ops.FP32_MATMUL
    try:
        if name in ("h2", "x3", "native"):
            ops.FP32_MATMUL = name
            yield
        else:
            with ops.matmul_bf16(True, "bf16" if name == "bf16_act16" else "f16", act16=(name == "bf16_act16")):
                yield
    finally:
        ops.FP32_MATMUL = prev


@contextmanager
def recorded(calls):
    """Append (entry point, products, act16) of every C-ABI launch made inside to ``calls``."""
    orig = ops._call

    def call(name, *args, products=None, act16=None, **kw):
        calls.append((name, products, None if act16 is None else int(act16)))
        return orig(name, *args, products=products, act16=act16, **kw)

    ops._call = call
    try:
        yield
    finally:
        ops._call = orig


def run_length(calls):
    """[[entry point, products, act16, repeats], ...] of a call list."""
    out = []
    for c in calls:
        if out and tuple(out[-1][:3]) == c:
            out[-1][3] += 1
        else:
            out.append([*c, 1])
    return out


def counts(calls):
    out = {}
    for name, _, _ in calls:
        out[name] = out.get(name, 0) + 1
    return out


@lru_cache(maxsize=None)
def _state(head):
    kind, nc, hidden, _, _ = HEADS[head]
    return model_ref.seeded_state(11, num_class=nc, hidden_size=hidden, model_type=kind)


@lru_cache(maxsize=None)
def _net(head, device):
    """One network per head, built as tests/test_model_gpu.build and tests/test_transformer_gpu.build do; ``run_case``
    puts its state back before every step."""
    kind, nc, hidden, _, _ = HEADS[head]
    cfg = dict(TF_CFG, dropout=DROPOUT) if kind == "transformer" else dict(SEQ_CFG, hidden_size=hidden, dropout=DROPOUT)
    return JDCNet(num_class=nc, sequence_model_config=cfg).to(device)


def inputs(head, device):
    """(x, d_cls, d_det) of a head: seeded normal draws made on the host."""
    _, nc, _, B, T = HEADS[head]
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(B, 1, T, 80, generator=g)
    d_cls = torch.randn(B, T, nc, generator=g) / (B * T)
    d_det = torch.randn(B, T, generator=g) / (B * T)
    return x.to(device), d_cls.to(device), d_det.to(device)


def run_case(name, device):
    """One step of case ``name``: {"calls": run-length call sequence, "counts": launches per entry point, and the
    digests "cls", "det", then "grads" and "bn" (train), "dx" (frozen)}."""
    head, m, kind = CASES[name]
    net = _net(head, device)
    net.load_state_dict(_state(head), strict=True)          # parameters, running statistics, batch counters
    net.requires_grad_(kind != "frozen")
    net.train(kind != "eval")
    net.dropout_cfg.offset = 0
    if kind == "train":
        net.flat_gradients().zero_()
    x, d_cls, d_det = inputs(head, device)
    calls, out = [], {}
    with mode(m), recorded(calls):
        if kind == "eval":
            with torch.no_grad():
                cls, det = net(x)
        else:
            x.requires_grad_(kind == "frozen")
            cls, det = net(x)
            torch.autograd.backward([cls, det], [d_cls, d_det])
    torch.cuda.synchronize(device)
    out["calls"], out["counts"] = run_length(calls), counts(calls)
    out["cls"], out["det"] = digest(cls), digest(det)
    if kind == "train":
        out["grads"] = digest(net.flat_gradients())
        out["bn"] = digest(*[b for n, b in net.named_buffers() if "running_" in n])
    if kind == "frozen":
        out["dx"] = digest(x.grad)
    net.requires_grad_(True)
    return out


def run_cases(device, names=None):
    return {name: run_case(name, device) for name in (sorted(CASES) if names is None else names)}
