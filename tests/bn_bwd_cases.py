"""Train-mode BatchNorm + LeakyReLU + max-pool backward on fixed inputs, reduced to digests of the output bits.

Shared by tests/golden/make_bn_bwd_train_golden.py, which recorded the digests with the build BEFORE the backward passes
took an eval mode, and tests/test_bn_eval_bwd_gpu.py, which holds today's train-mode passes to them: the calls below
use only the arguments the passes had then, so the same code runs on both builds.  Inputs come from numpy's PCG64
streams by seed (as tests/golden/make_golden.py::golden_input), values representable in bf16 so that both storage types
see the same numbers.
"""
import hashlib

import numpy as np
import torch

# name -> (rows, F, C, pool, tap (tap_pool, coff) or None, storage dtype)
CASES = {
    "pool1_fp32": (3, 80, 64, 1, None, torch.float32),
    "pool2_fp32": (3, 40, 128, 2, None, torch.float32),
    "pool4_fp32": (5, 10, 256, 4, None, torch.float32),          # 10 % 4: floor-mode remainder pixels
    "pool1_bf16": (3, 80, 64, 1, None, torch.bfloat16),
    "tap40_fp32": (3, 80, 64, 2, (40, 0), torch.float32),
    "tap20_fp32": (5, 40, 128, 2, (20, 64), torch.float32),
    "tap10_bf16": (5, 20, 192, 2, (10, 192), torch.bfloat16),
}


def bf16_values(seed, *shape, scale=1.0, shift=0.0):
    v = np.random.default_rng(seed).standard_normal(shape).astype(np.float32) * scale + shift
    return torch.from_numpy(v).to(torch.bfloat16).float()


def case_inputs(name):
    rows, Fq, C, pool, tap, dt = CASES[name]
    seed = sorted(CASES).index(name) * 10
    return dict(x=bf16_values(seed, 1, rows, Fq, C, scale=2.0, shift=0.5).to(dt),
                dy=bf16_values(seed + 1, 1, rows, Fq // pool, C).to(dt),
                gamma=bf16_values(seed + 2, C).abs() + 0.5, beta=bf16_values(seed + 3, C),
                dwide=None if tap is None else bf16_values(seed + 4, 1, rows, Fq // tap[0], 640).to(dt))


def run_train_case(ops, name, dev):
    """Batch statistics, forward (for the tap's positions) and backward of one case: {output name: tensor}."""
    rows, Fq, C, pool, tap, dt = CASES[name]
    t = {k: (None if v is None else v.to(dev)) for k, v in case_inputs(name).items()}
    st = ops.bn_train_stats(t["x"], t["gamma"], t["beta"], None, None)
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    tp = None
    if tap is not None:
        wide = torch.zeros(1, rows, Fq // tap[0], 640, device=dev, dtype=dt)
        tp = ops.Tap(wide, tap[0], tap[1], want_argmax=True)
        ops.bn_act_pool_fwd(t["x"], st, pool=pool, tap=tp)
        tp.grad = t["dwide"]
    dx = ops.bn_act_pool_bwd(t["x"], t["dy"], st, dg, db, pool=pool, amax_out=word, tap=tp)
    return {"dx": dx, "dgamma": dg, "dbeta": db, "amax": word}


def digest(t: torch.Tensor) -> str:
    """sha256 of the tensor's bytes (bf16 viewed as int16)."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()
