"""Accumulate launches of the training step at their real shapes, `accumulate` off and on (h2 products by default).

The step's launches that read their output back before writing it:
  conv   the second 3x3 convolution of each res block (model.py::_res_forward, out=out, accumulate=True, BatchNorm
         partials on) -- also timed without the partials and without the add, which is what a dgrad launch runs;
  dx     the second direction's dX product of an LSTM layer (M 49 152, N 768, K 1 536);
  sc     the three 1x1-shortcut dgrad products added onto d_p.
Per shape and setting: the median of --iters launches (HIP events around each launch) after --warmup launches.
on - off is what the accumulate read costs; PE_EPILOGUE=pointer selects the pointer-addressed epilogue of the same
build, PITCHEXTRACTOR_HIP_LIB another build.  One JSON line per shape.

Usage: python tools/bench_epilogue.py [--mode h2|x3|bf16] [--iters 30] [--warmup 5] [--batch 256] [--tag BUILD]"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pitchextractor_amd import ops  # noqa: E402

T = 192
CONVS = [(40, 128), (20, 192), (10, 256)]                      # (F, C = N) of the accumulate forward convolutions
SHORTCUTS = [(40, 64, 128), (20, 128, 192), (10, 192, 256)]    # (F, N = Cin, K = Cout) of the shortcut dgrad products
DX = (T, 768, 1536)                                            # (rows per utterance, N, K)


def median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def bench_conv(B, F, C, args, dev):
    x = torch.randn(B, T, F, C, device=dev)
    w = torch.randn(C, C, 3, 3, device=dev) * 0.05
    out = torch.randn(B, T, F, C, device=dev)
    sx = ops.Scaled.measured(x)
    wf, _ = ops.conv3x3_repack(w, True, False)
    res = {}
    for name, acc, stats in (("off", False, True), ("on", True, True), ("off_nostats", False, False),
                             ("on_nostats", True, False)):
        res[name] = median_ms(lambda: ops.conv3x3_fwd(sx, wf, out=out, accumulate=acc, bn_stats=stats),
                              args.iters, args.warmup)
    return res


def bench_gemm(M, N, K, args, dev):
    a = torch.randn(M, K, device=dev)
    b = torch.randn(N, K, device=dev) * 0.05
    out = torch.randn(M, N, device=dev)
    sa, sb = ops.Scaled.measured(a), ops.Scaled.measured(b)
    return {name: median_ms(lambda: ops.gemm_nt(sa, sb, out=out, accumulate=acc), args.iters, args.warmup)
            for name, acc in (("off", False), ("on", True))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["h2", "x3", "bf16"], default="h2")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--tag", default="", help="name of the build under test, copied into every line")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ops.FP32_MATMUL = "x3" if args.mode == "x3" else "h2"
    head = {"build": args.tag, "mode": args.mode, "PE_EPILOGUE": os.environ.get("PE_EPILOGUE", "")}
    B = args.batch
    with ops.matmul_bf16(args.mode == "bf16"):
        rows = []
        for F, C in CONVS:
            rows.append(({"op": "conv", "P": B * T * F, "C": C, "N": C}, bench_conv(B, F, C, args, dev)))
        rows.append(({"op": "dx", "M": B * DX[0], "N": DX[1], "K": DX[2]}, bench_gemm(B * DX[0], DX[1], DX[2], args, dev)))
        for F, N, K in SHORTCUTS:
            rows.append(({"op": "sc", "M": B * T * F, "N": N, "K": K}, bench_gemm(B * T * F, N, K, args, dev)))
    total = 0.0
    for shape, ms in rows:
        gap = ms["on"] - ms["off"]
        total += gap
        print(json.dumps({**head, **shape, "ms": {k: round(v, 4) for k, v in ms.items()}, "on_minus_off": round(gap, 4)}),
              flush=True)
    # launches per step: each conv and shortcut shape once, the dX shape 8 times
    dx_gap = rows[len(CONVS)][1]["on"] - rows[len(CONVS)][1]["off"]
    print(json.dumps({**head, "sum_on_minus_off": round(total, 4), "per_step": round(total + 7 * dx_gap, 4)}), flush=True)


if __name__ == "__main__":
    main()
