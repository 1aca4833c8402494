"""Time the TN weight-gradient products of the training step on the tiling the environment selects.

The tile override PE_TN_TILE (128, 192, 128x192, 192x128; unset = each entry point's own choice) is read once per
process, so one run measures one tiling; run it once per tiling, taking turns, and compare the lines:

  for t in 128 192 192x128 128x192 default; do PE_TN_TILE=$t python3 tools/bench_tn_tile.py; done     ("default": unset)

Per shape and product form: median ms over the launches of one call (main kernel + slab reduce) between device
events, and the main kernel's h2 TFLOP/s equivalent.  A kernel trace of the same run (rocprofv3 --kernel-trace --stats)
separates tn_splitk_kernel from splitk_reduce_kernel; --only IDX restricts the run to one shape for that.
One JSON line per (shape, form) and a summary line.
"""
import argparse
import json
import os
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pitchextractor_amd import ops  # noqa: E402

R = 256 * 192                                   # batch x time of the default step
# (name, M, N, K): dW_ih of LSTM layer 0 and layers 1-3, the four 1x1 / detector products, and dW_hh (H = 384)
SHAPES = [("dW_ih_l0", 1536, 512, R), ("dW_ih_l1-3", 1536, 768, R), ("tn_128x64", 128, 64, R * 40),
          ("tn_192x128", 192, 128, R * 20), ("tn_256x192", 256, 192, R * 10), ("tn_256x640", 256, 640, R * 2),
          ("dW_hh", 1536, 384, R)]


def median_ms(fn, launches):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=31)
    ap.add_argument("--forms", default="h2,bf16")
    ap.add_argument("--only", type=int, default=None, help="index into the shape list")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    tile = os.environ.get("PE_TN_TILE", "default")
    total = {}
    for idx, (name, M, N, K) in enumerate(SHAPES):
        if args.only is not None and idx != args.only:
            continue
        g = torch.Generator(device=dev).manual_seed(idx)
        if name == "dW_hh":
            B, T, H = 256, 192, N
            dg = torch.randn(B, T, M, device=dev, generator=g) * 1e-4
            y = torch.tanh(torch.randn(B, T, 2 * H, device=dev, generator=g))
            out = torch.empty(M, N, device=dev)
            sa, sb = ops.Scaled(dg, ops.absmax(dg)), ops.Scaled(y[:, :, :H], None)
            call = lambda: ops.lstm_whh_grad(sa, sb, out, False, B, T, H)          # noqa: E731
        else:
            A = torch.randn(K, M, device=dev, generator=g) * 1e-4
            Bm = torch.randn(K, N, device=dev, generator=g)
            out = torch.empty(M, N, device=dev)
            sa, sb = ops.Scaled(A, ops.absmax(A)), ops.Scaled(Bm, ops.absmax(Bm))
            call = lambda: ops.gemm_tn(sa, sb, out=out)                             # noqa: E731
        for form in args.forms.split(","):
            if form in ("bf16", "f16"):
                ctx = ops.matmul_bf16(True, form)
            else:
                ops.FP32_MATMUL = form
                ctx = ops.matmul_bf16(False)
            with ctx:
                med, best = median_ms(call, args.launches)
            total[form] = total.get(form, 0.0) + med
            print(json.dumps({"tile": tile, "shape": name, "M": M, "N": N, "K": K, "form": form,
                              "median_ms": round(med, 4), "min_ms": round(best, 4),
                              "tflops": round(2.0 * M * N * K / med / 1e9, 1)}), flush=True)
        del out, sa, sb
    print(json.dumps({"tile": tile, "total_median_ms": {k: round(v, 3) for k, v in total.items()}}), flush=True)


if __name__ == "__main__":
    main()
