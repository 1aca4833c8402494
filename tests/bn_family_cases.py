"""The BatchNorm / LeakyReLU / max-pool passes on fixed inputs, reduced to digests of the output bits.

Shared by tests/golden/make_bn_family_golden.py, which recorded the digests with the build BEFORE these passes were
rewritten around shared helpers (one first-maximum scan, one BN + LeakyReLU quad, one input-gradient quad, one apply
body), and tests/test_bn_family_bits_gpu.py, which holds every later build to them.  tests/bn_bwd_cases.py pins the
train-mode backward at seven cases; this module covers what it leaves out: the forward passes, the tap's values and
positions, bf16 tensors at pool 2 / 4, eval mode, taps at pool 1 / 4 and the plain max-pools at every shape of their
scan (tail only, one group of four, group plus tail, the model's widths).  Only public ``ops`` functions are called.

Inputs are numpy PCG64 draws by seed, representable in bf16 so that both storage types see the same numbers.  Where a
maximum is searched in the raw x (taps, max-pools) x comes from a handful of integer levels, half as many as the window
has elements and five at the least: ties inside a window are the rule, the first-maximum rule decides the positions,
and about one window in eight has a maximum below the top level, so the values are not all alike.
"""
import zlib

import numpy as np
import torch

from tests.bn_bwd_cases import bf16_values, digest  # noqa: F401  (digest: re-exported for the recorder and the test)

F32, BF = torch.float32, torch.bfloat16
WIDE = 640                    # channels of the detector's concatenated buffer
FILL = 7.0                    # what a tap's target buffer holds before the pass


def _c(kind, rows, Fq, C, pool, dt, **kw):
    return dict(kind=kind, rows=rows, F=Fq, C=C, pool=pool, dt=dt, **kw)


def _tag(dt):
    return "fp32" if dt == F32 else "bf16"


CASES = {}
# forward: y and its absmax word
for rows, Fq, C, pool in [(3, 80, 64, 1), (3, 40, 128, 2), (5, 20, 192, 2), (5, 10, 256, 4)]:
    for dt in (F32, BF):
        CASES[f"fwd_F{Fq}_C{C}_pool{pool}_{_tag(dt)}"] = _c("fwd", rows, Fq, C, pool, dt)
# forward with a folded tap: y, the word, the tap's slice, the positions
for rows, Fq, C, pool, tp, coff, dts in [(3, 80, 64, 2, 40, 0, (F32, BF)), (5, 40, 128, 2, 20, 64, (F32, BF)),
                                         (5, 20, 192, 2, 10, 192, (F32, BF)), (3, 20, 64, 1, 10, 0, (F32,)),
                                         (3, 40, 64, 4, 20, 0, (F32,))]:
    for dt in dts:
        for arg in (True, False):
            CASES[f"fwdtap{tp}_pool{pool}_{_tag(dt)}_{'arg' if arg else 'noarg'}"] = _c(
                "fwd_tap", rows, Fq, C, pool, dt, tap=(tp, coff), want_argmax=arg)
# backward, batch statistics
CASES["bwd_pool2_bf16"] = _c("bwd", 3, 40, 128, 2, BF, tap=None, eval=False, sums=True)
CASES["bwd_pool4_bf16"] = _c("bwd", 5, 10, 256, 4, BF, tap=None, eval=False, sums=True)
CASES["bwd_tap10_pool1_fp32"] = _c("bwd", 3, 20, 64, 1, F32, tap=(10, 0), eval=False, sums=True)
CASES["bwd_tap20_pool4_fp32"] = _c("bwd", 3, 40, 64, 4, F32, tap=(20, 0), eval=False, sums=True)
# backward, running statistics
for rows, Fq, C, pool in [(3, 80, 64, 1), (3, 40, 128, 2), (5, 10, 256, 4)]:
    for dt in (F32, BF):
        for sums in (True, False):
            CASES[f"bwdeval_pool{pool}_{_tag(dt)}_{'sums' if sums else 'dxonly'}"] = _c(
                "bwd", rows, Fq, C, pool, dt, tap=None, eval=True, sums=sums)
CASES["bwdeval_tap20_pool2_bf16"] = _c("bwd", 5, 40, 128, 2, BF, tap=(20, 64), eval=True, sums=True)
# plain max-pools: the model's three taps, then the shapes of the scan (tail only / one group of four / group + tail)
for rows, Fq, C, pool, coff in [(3, 80, 64, 40, 0), (5, 40, 128, 20, 64), (5, 20, 192, 10, 192), (3, 12, 64, 3, 0),
                                (3, 20, 64, 5, 0), (3, 14, 64, 7, 0)]:
    for dt in (F32, BF):
        CASES[f"maxpool{pool}_{_tag(dt)}"] = _c("maxpool", rows, Fq, C, pool, dt, coff=coff)


def levels(seed, window, *shape):
    """Integer draws from max(5, window // 2) levels centred on zero."""
    n = max(5, window // 2)
    return torch.from_numpy((np.random.default_rng(seed).integers(0, n, size=shape) - n // 2).astype(np.float32))


def _seed(name):
    return zlib.crc32(name.encode()) % (1 << 30)


def _state(ops, c, seed, x, dev):
    C = c["C"]
    gamma, beta = (bf16_values(seed + 2, C).abs() + 0.5).to(dev), bf16_values(seed + 3, C).to(dev)
    if c.get("eval"):
        rm, rv = bf16_values(seed + 5, C, scale=1.5, shift=2.0), bf16_values(seed + 6, C).abs() * 3.0 + 0.3
        return ops.bn_eval_affine(gamma, beta, rm.to(dev), rv.to(dev))
    return ops.bn_train_stats(x, gamma, beta, None, None)


def _word(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


def _wide(rows, Fo, dt, dev):
    return torch.full((1, rows, Fo, WIDE), FILL, device=dev, dtype=dt)


def _run_bn(ops, c, seed, dev):
    rows, Fq, C, pool, dt, tap = c["rows"], c["F"], c["C"], c["pool"], c["dt"], c.get("tap")
    x = (bf16_values(seed, 1, rows, Fq, C, scale=2.0, shift=0.5) if tap is None
         else levels(seed, tap[0], 1, rows, Fq, C)).to(dt).to(dev)
    st = _state(ops, c, seed, x, dev)
    tp = None
    if tap is not None:
        wide = _wide(rows, Fq // tap[0], dt, dev)
        tp = ops.Tap(wide, tap[0], tap[1], want_argmax=c.get("want_argmax", True))
    if c["kind"] != "bwd":
        word = _word(dev)
        out = {"y": ops.bn_act_pool_fwd(x, st, pool=pool, amax_out=word, tap=tp), "amax": word}
        if tp is not None:
            out["wide"] = wide
            out["tap"] = wide[..., tap[1]:tap[1] + C]
            if tp.want_argmax:
                out["argmax"] = tp.argmax
        return out
    if tp is not None:
        ops.bn_act_pool_fwd(x, st, pool=pool, tap=tp)
        tp.grad = bf16_values(seed + 4, 1, rows, Fq // tap[0], WIDE).to(dt).to(dev)
    dy = bf16_values(seed + 1, 1, rows, Fq // pool, C).to(dt).to(dev)
    word = _word(dev)
    out = {"amax": word}
    dg = db = None
    if c["sums"]:
        out["dgamma"], out["dbeta"] = dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    out["dx"] = ops.bn_act_pool_bwd(x, dy, st, dg, db, pool=pool, amax_out=word, tap=tp)
    return out


def _run_maxpool(ops, c, seed, dev):
    rows, Fq, C, pool, dt, coff = c["rows"], c["F"], c["C"], c["pool"], c["dt"], c["coff"]
    x = levels(seed, pool, 1, rows, Fq, C).to(dt).to(dev)
    wide = _wide(rows, Fq // pool, dt, dev)
    _, arg = ops.maxpool_fwd(x, pool, out=wide, coff=coff, want_argmax=True)
    out = {"wide": wide, "y": wide[..., coff:coff + C], "argmax": arg}
    dwide = bf16_values(seed + 1, 1, rows, Fq // pool, WIDE).to(dt).to(dev)
    dx0 = bf16_values(seed + 2, 1, rows, Fq, C).to(dt).to(dev)
    for key, a in (("arg", arg), ("scan", None)):
        word = _word(dev)
        out[f"dx_{key}"] = ops.maxpool_bwd_add(x, dwide, dx0.clone(), pool, coff=coff, amax_out=word, argmax=a)
        out[f"amax_{key}"] = word
    return out


def run_case(ops, name, dev):
    """One case on ``dev``: {output name: tensor}."""
    c = CASES[name]
    return (_run_maxpool if c["kind"] == "maxpool" else _run_bn)(ops, c, _seed(name), dev)
